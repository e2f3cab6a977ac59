"""The rasteriser library and robir_amd/meshrender.py as far as they go without a GPU: loading, the export list, argument errors before any
launch, the host build of csrc/raster/raster_math.h against the restatement bit for bit (tools/check_raster_host.py), and the rule itself
on the restatement (tests/meshrender_restatement.py): coverage and depth of an icosphere against the two balls that bound it, no
back-facing winner, perspective-correct positions on the pixels' rays, and the projection against the oracle's camera_rays."""
import ctypes
import functools
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import meshrender_restatement as mr
from conftest import ROOT

c_long, c_int, c_float = ctypes.c_long, ctypes.c_int, ctypes.c_float
NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(4096)                    # never read: every call below is refused, or has nothing to do, before a launch
OTHER_HEADERS = ("robir_hip.h", "robir_hip_legacy.h", "robir_hip_train.h", "robir_hip_vistrain.h", "robir_hip_illumtrain.h",
                 "robir_hip_cesrtrain.h", "robir_hip_lightfit.h", "robir_hip_texbake.h", "robir_hip_observe.h", "robir_hip_photoloss.h",
                 "robir_hip_metrics.h")
H = W = 64


def _header_symbols(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return sorted(set(re.findall(r"^(?:int|long|const char\*) (rb_[a-z0-9_]+)\s*\(", hdr, re.M)))


def _rs_lib():
    from robir_amd import _lib
    if not os.path.exists(_lib.RASTER_PATH):
        _lib.build(legacy=False)
    return _lib.raster()


def test_raster_library_exports_its_header():
    """librobir_hip_raster.so loads without a GPU and exports exactly what include/robir_hip_raster.h declares, every name rb_rs_*; no rb_
    name is shared with the other eleven headers, and none of them names this one."""
    from robir_amd import _lib
    L = _rs_lib()
    assert L.rb_rs_abi_version() == _lib.RASTER_ABI_VERSION == 1
    syms = _header_symbols("robir_hip_raster.h")
    assert syms == ["rb_rs_abi_version", "rb_rs_bin_count", "rb_rs_bin_emit", "rb_rs_gbuffer", "rb_rs_last_error", "rb_rs_project",
                    "rb_rs_raster"]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.RASTER_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[-1] for l in out.splitlines() if " T rb_" in l) == syms
    others = set()
    for h in OTHER_HEADERS:
        text = open(os.path.join(ROOT, "include", h)).read()
        others |= set(_header_symbols(h))
        assert "rb_rs_" not in text and "robir_hip_raster" not in text
    assert len(OTHER_HEADERS) == 11 and not set(syms) & others
    assert "#define RB_RS_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "robir_hip_raster.h")).read()


def test_raster_argument_errors_before_any_launch():
    L = _rs_lib()
    err = L.rb_rs_last_error
    big = c_long(1 << 31)
    assert L.rb_rs_project(NULL, c_long(4), FAKE, FAKE, FAKE, NULL) != 0 and b"null pointer" in err()
    assert L.rb_rs_project(FAKE, c_long(4), FAKE, FAKE, NULL, NULL) != 0 and b"null pointer" in err()
    assert L.rb_rs_project(FAKE, c_long(-1), FAKE, FAKE, FAKE, NULL) != 0 and b"negative" in err()
    assert L.rb_rs_project(NULL, c_long(0), NULL, NULL, NULL, NULL) == 0

    def count(screen=FAKE, V=6, faces=FAKE, F=4, Hh=64, Ww=64, near=1e-4, cull=0, counts=FAKE):
        return L.rb_rs_bin_count(screen, c_long(V), faces, c_long(F), c_int(Hh), c_int(Ww), c_float(near), c_int(cull), counts, NULL)
    assert count(Hh=0) != 0 and b"empty image" in err()
    assert count(Hh=16385) != 0 and b"16384" in err()
    assert count(Ww=16385) != 0 and b"16384" in err()
    assert count(faces=NULL) != 0 and b"null pointer" in err()
    assert count(screen=NULL) != 0 and b"null pointer" in err()
    assert count(near=0.0) != 0 and b"near" in err()
    assert count(near=float("nan")) != 0 and b"near" in err()
    assert count(cull=3) != 0 and b"cull" in err()
    assert count(F=1 << 31) != 0 and b"32 bits" in err()
    assert count(F=0, screen=NULL, faces=NULL, counts=NULL) == 0          # nothing to do: no launch

    def emit(screen=FAKE, faces=FAKE, F=4, Hh=64, base=FAKE, P=9, pt=FAKE, pf=FAKE):
        return L.rb_rs_bin_emit(screen, c_long(6), faces, c_long(F), c_int(Hh), c_int(64), c_float(1e-4), c_int(0), base, c_long(P), pt, pf, NULL)
    assert emit(P=-1) != 0 and b"negative" in err()
    assert emit(P=1 << 31) != 0 and b"2^31" in err()
    assert emit(Hh=0) != 0 and b"empty image" in err()
    assert emit(base=NULL) != 0 and b"null pointer" in err()
    assert emit(F=0) != 0 and b"no face" in err()
    assert emit(P=0, screen=NULL, faces=NULL, base=NULL, pt=NULL, pf=NULL) == 0
    assert emit(P=0, F=0, screen=NULL, faces=NULL, base=NULL, pt=NULL, pf=NULL) == 0

    def raster(screen=FAKE, F=4, Hh=64, Ww=64, ts=FAKE, pf=FAKE, P=4, fid=FAKE, bary=FAKE, depth=FAKE):
        return L.rb_rs_raster(screen, c_long(6), FAKE, c_long(F), c_int(Hh), c_int(Ww), c_float(1e-4), c_int(0), ts, pf, c_long(P), fid, bary,
                              depth, NULL)
    assert raster(Hh=16385) != 0 and b"16384" in err()
    assert raster(Ww=0) != 0 and b"empty image" in err()
    assert raster(P=1 << 31) != 0 and b"2^31" in err()
    assert raster(P=-2) != 0 and b"negative" in err()
    assert raster(fid=NULL) != 0 and b"null pointer" in err()
    assert raster(depth=NULL) != 0 and b"null pointer" in err()
    assert raster(ts=NULL) != 0 and b"null pointer" in err()
    assert raster(pf=NULL) != 0 and b"null pointer" in err()

    def gbuf(fid=FAKE, Hh=8, Ww=8, index=NULL, n=64, faces=FAKE, F=4, V=6, vn=NULL, planes=FAKE, R=16, C=8, filt=1, pos=FAKE, tex=FAKE,
             nrm=NULL):
        return L.rb_rs_gbuffer(fid, FAKE, c_int(Hh), c_int(Ww), index, c_long(n), faces, c_long(F), FAKE, c_long(V), FAKE, vn, FAKE, planes,
                               c_int(R), c_int(C), c_int(filt), pos, FAKE, FAKE, tex, nrm, NULL)
    assert gbuf(C=17) != 0 and b"C = 17" in err()
    assert gbuf(C=0) != 0 and b"C = 0" in err()
    assert gbuf(R=16385) != 0 and b"R = 16385" in err()
    assert gbuf(Hh=0) != 0 and b"empty image" in err()
    assert gbuf(Hh=16385) != 0 and b"16384" in err()
    assert gbuf(n=32) != 0 and b"image form" in err()
    assert gbuf(n=-1) != 0 and b"negative" in err()
    assert gbuf(index=FAKE, n=65) != 0 and b"65 rows" in err()
    assert gbuf(filt=2) != 0 and b"filter" in err()
    assert gbuf(tex=NULL) != 0 and b"both or neither" in err()
    assert gbuf(vn=FAKE) != 0 and b"both or neither" in err()
    assert gbuf(pos=NULL) != 0 and b"null pointer" in err()
    assert gbuf(fid=NULL) != 0 and b"null pointer" in err()
    assert gbuf(faces=NULL) != 0 and b"null pointer" in err()
    assert gbuf(index=FAKE, n=0, fid=NULL, pos=NULL) == 0


def test_python_wrappers_refuse_before_the_library():
    from robir_amd import meshrender, ops
    with pytest.raises(ValueError, match="16384"):
        ops._rs_image(16385, 8)
    with pytest.raises(ValueError, match="vis"):
        meshrender.render_mesh("nowhere", torch.eye(4), torch.eye(3), 8, 8, light=torch.zeros(4, 7), vis="traced")
    with pytest.raises(ValueError, match="needs the model"):
        meshrender.render_mesh("nowhere", torch.eye(4), torch.eye(3), 8, 8, light=torch.zeros(4, 7), vis="network")
    with pytest.raises(ValueError, match="model or a light"):
        meshrender.render_mesh("nowhere", torch.eye(4), torch.eye(3), 8, 8)


def test_host_build_equals_the_restatement_bit_for_bit():
    spec = importlib.util.spec_from_file_location("check_raster_host", os.path.join(ROOT, "tools", "check_raster_host.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if mod.compiler() is None:
        pytest.skip("no host C++ compiler")
    rows = mod.check()
    assert len(rows) >= 70
    assert not [what for what, ok in rows if not ok]


# ----------------------------------------------------------------------------------------- the rule, on the restatement
def _camera():
    from robir_amd import synth
    _, _, K = synth.synth_camera(H, W)
    pose = mr.rotated_pose()
    assert np.abs(pose[:3, :3]).max() < 0.999 and np.abs(pose[:3, :3]).min() > 0.05          # not axis-aligned
    return pose, mr.pose_inverse(pose), K


@functools.lru_cache(maxsize=None)
def _ball(subdivisions):
    """An icosphere of radius 0.25 seen by the rotated camera at 64 x 64: everything the property tests share, computed once."""
    pose, pinv, K = _camera()
    v, f = mr.icosphere(subdivisions)
    assert f.shape[0] == 20 * 4 ** subdivisions
    screen = mr.project(v, pinv, K)
    face_id, bary, depth = mr.raster(screen, f, H, W)
    v64 = v.astype(np.float64)
    tri = v64[f]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    r_in = float(np.abs((nrm * tri[:, 0]).sum(-1)).min())
    r_out = float(np.linalg.norm(v64, axis=-1).max())
    cam, rays = mr.pixel_rays(pose, K, H, W)
    return dict(pose=pose, pinv=pinv, K=K, v=v, f=f, screen=screen, face_id=face_id, bary=bary, depth=depth, nrm=nrm, tri=tri, r_in=r_in,
                r_out=r_out, cam=cam, rays=rays)


@pytest.fixture(scope="module", params=(1, 3), ids=("80", "1280"))
def ball(request):
    return _ball(request.param)


def test_coverage_lies_between_the_two_balls(ball):
    """Every pixel whose ray hits the inscribed ball is covered, none whose ray misses the circumscribed one; the band between is free."""
    covered = ball["face_id"] >= 0
    hit_in, _ = mr.ray_ball(ball["cam"], ball["rays"], ball["r_in"])
    hit_out, _ = mr.ray_ball(ball["cam"], ball["rays"], ball["r_out"])
    assert 0.23 < ball["r_in"] < ball["r_out"] <= 0.2501
    assert hit_in.sum() > 300 and (~hit_out).sum() > 1000          # the object is on the image and leaves background
    assert covered[hit_in].all()
    assert not covered[~hit_out].any()


def test_depth_lies_between_the_two_balls(ball):
    """Nested convex bodies: along a covered pixel's ray the mesh is met after the outer ball and, where the ray meets the inner ball, before
    it; 1e-5 for fp32 rounding.  depth is measured along the viewing axis and the rays have unit axis component: same parameter."""
    covered = ball["face_id"] >= 0
    hit_in, t_in = mr.ray_ball(ball["cam"], ball["rays"], ball["r_in"])
    hit_out, t_out = mr.ray_ball(ball["cam"], ball["rays"], ball["r_out"])
    assert hit_out[covered].all()
    length = np.linalg.norm(ball["rays"], axis=-1)
    t = ball["depth"].astype(np.float64) * length
    assert (t_out[covered] * length[covered] * (1 - 1e-5) <= t[covered]).all()
    both = covered & hit_in
    assert (t[both] <= t_in[both] * length[both] * (1 + 1e-5)).all()
    assert (ball["depth"][~covered] == 0).all()


def test_no_winning_face_is_back_facing(ball):
    fid = ball["face_id"][ball["face_id"] >= 0]
    centroid = ball["tri"].mean(1)
    facing = (ball["nrm"] * (ball["cam"][None, :] - centroid)).sum(-1)
    assert (facing[fid] > 0).all()
    # and culling the back faces (positive screen area for this outward winding: v points down) changes no pixel
    area = np.array([mr.Face(ball["screen"][t], H, W).area for t in ball["f"]])
    assert (area[facing > 1e-3] < 0).all() and (area[facing < -1e-3] > 0).all()
    culled = mr.raster(ball["screen"], ball["f"], H, W, cull=2)
    assert np.array_equal(culled[0], ball["face_id"]) and np.array_equal(culled[1], ball["bary"])
    assert (mr.raster(ball["screen"], ball["f"], H, W, cull=1)[0][ball["face_id"] >= 0] != ball["face_id"][ball["face_id"] >= 0]).all()


def test_perspective_correct_position_lies_on_the_pixels_ray():
    """On the 80-face mesh (large faces, strong perspective inside a face) the interpolated position is on the pixel's ray within 1e-6
    (a numpy fp32 prototype of the rule measured 1.0e-7; the cap is 10 x that for other poses).  Interpolating with the SCREEN weights
    instead is 5.6e-3 off on the same input: that is what this catches."""
    ball = _ball(1)
    idx = np.nonzero(ball["face_id"].reshape(-1) >= 0)[0]
    uv = np.zeros((80, 3, 2), dtype=np.float32)
    g = mr.gbuffer(ball["face_id"], ball["bary"], ball["f"], ball["v"], uv, ball["cam"], index=idx)

    def off_ray(p):
        d = ball["rays"].reshape(-1, 3)[idx]
        d = d / np.linalg.norm(d, axis=-1, keepdims=True)
        rel = p.astype(np.float64) - ball["cam"][None, :]
        return np.linalg.norm(rel - (rel * d).sum(-1, keepdims=True) * d, axis=-1).max()

    err = off_ray(g["position"])
    print("perspective-correct position off its ray:", err)
    assert err <= 1e-6
    # the screen-space weights on the same faces, for contrast
    pos = np.zeros((idx.size, 3))
    for i, t in enumerate(idx):
        r, c = divmod(int(t), W)
        face = mr.Face(ball["screen"][ball["f"][ball["face_id"][r, c]]], H, W)
        l0, l1 = face.edge(0, np.float32(c), np.float32(r)) / face.area, face.edge(1, np.float32(c), np.float32(r)) / face.area
        tri = ball["tri"][ball["face_id"][r, c]]
        pos[i] = l0 * tri[0] + l1 * tri[1] + (1 - l0 - l1) * tri[2]
    assert off_ray(pos) > 1e-3
    # view_dir is the unit vector from the point back to the camera: minus the pixel's ray
    d = ball["rays"].reshape(-1, 3)[idx]
    assert np.abs(g["view_dir"] + d / np.linalg.norm(d, axis=-1, keepdims=True)).max() < 1e-5


def test_float64_path_agrees_with_the_float32_rule(ball):
    """The same rule in double precision (the end-to-end test's reference path): the two masks differ on silhouette pixels at most, and the
    weights agree to fp32 accuracy elsewhere."""
    s64 = mr.project(ball["v"], ball["pinv"], ball["K"], dtype=np.float64)
    fid, bary, depth = mr.raster(s64, ball["f"], H, W, dtype=np.float64)
    same = fid == ball["face_id"]
    assert (~same).sum() <= 8
    inner = same & (fid >= 0)
    assert np.abs(depth[inner] - ball["depth"][inner]).max() < 2e-6
    assert np.abs(bary[inner] - ball["bary"][inner]).max() < 5e-4          # weights of a 1.5-pixel face: conditioned by its size


@pytest.mark.parametrize("form", ("matrix", "quaternion"))
def test_projection_recovers_the_pixels_of_the_oracles_rays(form):
    """Points cam + t dirs of the oracle's camera_rays project back onto their pixel within 1e-3 px at W = 1024, for both pose forms."""
    from robir_amd import synth
    from robir_oracle import renderer as orend
    Wd = Hd = 1024
    _, _, K = synth.synth_camera(Hd, Wd)
    pose = mr.rotated_pose()
    if form == "quaternion":
        q = torch.tensor([[0.8, 0.3, -0.4, 0.2]])
        Rm = orend.quat_to_rot(q)[0].numpy()
        pose = pose.copy()
        pose[:3, :3] = Rm
        pose[:3, 3] = Rm @ np.array([0.02, -0.01, 0.9], dtype=np.float32)
        pose_t = torch.cat([q, torch.from_numpy(pose[:3, 3])[None]], 1)
    else:
        pose_t = torch.from_numpy(pose)[None]
    cols, rows = np.meshgrid(np.arange(0, Wd, 31, dtype=np.float32), np.arange(0, Hd, 37, dtype=np.float32))
    uv = np.stack([cols, rows], -1).reshape(-1, 2)
    dirs, cam = orend.camera_rays(torch.from_numpy(uv)[None], pose_t, torch.from_numpy(K)[None])
    pinv = mr.pose_inverse(pose)
    worst = 0.0
    for t in (0.4, 0.9, 2.5):
        x = (cam[0][None, :] + t * dirs[0]).numpy().astype(np.float32)
        s = mr.project(x, pinv, K)
        worst = max(worst, float(np.abs(s[:, :2] - uv).max()))
        axis = -(pose[:3, :3].astype(np.float64)[:, 2])
        zc = ((x.astype(np.float64) - cam[0].numpy()[None, :]) * axis[None, :]).sum(-1)
        assert np.abs(s[:, 3] - zc).max() < 1e-5 and np.abs(s[:, 2] * s[:, 3] - 1).max() < 1e-6
    print("pixel error of the projection:", worst)
    assert worst <= 1e-3


# ----------------------------------------------------------------------------------------- the cases of the GPU test, on the restatement
def test_raster_cases_say_what_they_are_meant_to():
    cases = mr.raster_cases()
    screen, faces, Hc, Wc = cases["tile200"]
    pt, pf = mr.bin_pairs(screen, faces, Hc, Wc)
    ntx = (Wc + 7) // 8
    assert Hc % 8 and Wc % 8 and Hc != Wc
    assert (pt == 1 * ntx + 1).sum() > 128                      # more than two batches of 64 in one tile
    fid, _, depth = mr.raster(screen, faces, Hc, Wc)
    win = np.unique(fid[fid >= 0])
    assert win.size > 10 and (win < 64).any() and (win >= 128).any()          # winners from the first and from a later batch
    fid, _, _ = mr.raster(*cases["coincident"])
    assert (fid == 0).sum() > 10 and not (fid == 1).any() and (fid == 2).sum() > 5
    for name in ("shared_edge", "shared_edge_mixed"):
        screen, faces, Hc, Wc = cases[name]
        fid, _, _ = mr.raster(screen, faces, Hc, Wc)
        assert (fid[1:12, 2:13] >= 0).all()                     # no hole in the quad, the diagonal's pixel centres included
        owners = sum(not mr.Face(screen[t], Hc, Wc).empty for t in faces)
        assert owners == 2 and {int(fid[r, 2 + r - 1]) for r in range(1, 12)} <= {0, 1}
    screen, faces, Hc, Wc = cases["edge_cases"]
    fid, _, _ = mr.raster(screen, faces, Hc, Wc)
    assert set(np.unique(fid)) == {-1, 0, 6, 8}                 # partly off-screen, the ordinary face, the zc = inf corner
    assert list(mr.bin_counts(screen, faces, Hc, Wc)[[1, 2, 3, 4, 5, 7, 9]]) == [0] * 7
    screen, faces, Hc, Wc = cases["windings"]
    ids = [set(np.unique(mr.raster(screen, faces, Hc, Wc, cull=c)[0])) for c in (0, 1, 2)]
    assert ids[0] == {-1, 0, 1} and ids[1] | ids[2] == {-1, 0, 1} and ids[1] != ids[2] and len(ids[1]) == len(ids[2]) == 2


def test_filters_return_a_texel_centre_bit_for_bit():
    verts, faces, uv, planes, vn = mr.gbuffer_case()
    R = planes.shape[0]
    u = np.array([(c + 0.5) / R for c in (0, 3, 7)], dtype=np.float32)
    v = np.array([1.0 - (r + 0.5) / R for r in (0, 5, 7)], dtype=np.float32)
    want = planes[[0, 5, 7], [0, 3, 7]]
    assert np.array_equal(mr.fetch_nearest(planes, u, v).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(mr.fetch_bilinear(planes, u, v).view(np.uint32), want.view(np.uint32))
    # out of the texture: the nearest filter clamps, the bilinear one pads with zeros
    far = np.array([2.0], dtype=np.float32)
    assert np.array_equal(mr.fetch_nearest(planes, far, far), planes[0:1, R - 1])
    assert (mr.fetch_bilinear(planes, far, far) == 0).all()
