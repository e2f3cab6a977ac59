"""The observation library and robir_amd/observe.py as far as they go without a GPU: loading, the export list, argument errors before any
launch, the host build of csrc/observe/observe_math.h against the numpy fp32 restatement bit for bit (tools/check_observe_host.py), the
restatement against the reference's own lines on PyTorch-CPU and against its float64 form, what the seeded cases claim to contain, and
the export of the observed planes."""
import ctypes
import importlib.util
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import observe_restatement as obr
from conftest import ROOT, rel_err

c_long, c_int = ctypes.c_long, ctypes.c_int
NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(4096)                    # never read: every call below is refused, or has nothing to do, before a launch
OTHER_HEADERS = ("robir_hip.h", "robir_hip_legacy.h", "robir_hip_train.h", "robir_hip_vistrain.h", "robir_hip_illumtrain.h",
                 "robir_hip_cesrtrain.h", "robir_hip_lightfit.h", "robir_hip_texbake.h")
CASES = obr.cases()
BIG = sorted(n for n, c in CASES.items() if c.N == 300)


def _header_symbols(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return sorted(set(re.findall(r"^(?:int|long|const char\*) (rb_[a-z0-9_]+)\s*\(", hdr, re.M)))


def _ob_lib():
    from robir_amd import _lib
    if not os.path.exists(_lib.OBSERVE_PATH):
        _lib.build(legacy=False)
    return _lib.observe()


def test_observe_library_exports_its_header():
    """librobir_hip_observe.so loads without a GPU and exports exactly what include/robir_hip_observe.h declares, every name rb_ob_*; no rb_
    name is shared with the other eight headers, and none of them names this one."""
    from robir_amd import _lib
    L = _ob_lib()
    assert L.rb_ob_abi_version() == _lib.OBSERVE_ABI_VERSION == 1
    syms = _header_symbols("robir_hip_observe.h")
    assert syms == ["rb_ob_abi_version", "rb_ob_accumulate", "rb_ob_fetch", "rb_ob_gather", "rb_ob_last_error", "rb_ob_scatter", "rb_ob_select"]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.OBSERVE_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[-1] for l in out.splitlines() if " T rb_" in l) == syms
    others = set()
    for h in OTHER_HEADERS:
        text = open(os.path.join(ROOT, "include", h)).read()
        others |= set(_header_symbols(h))
        assert "rb_ob_" not in text and "observe" not in text
    assert not set(syms) & others
    assert "#define RB_OB_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "robir_hip_observe.h")).read()


def test_missing_observe_library_has_its_own_message(monkeypatch, tmp_path):
    from robir_amd import _lib
    monkeypatch.setattr(_lib, "_observe", None)
    monkeypatch.setattr(_lib, "OBSERVE_PATH", str(tmp_path / "nope_observe.so"))
    with pytest.raises(_lib.RobirHipError, match="OBSERVATION library") as e:
        _lib.call_observe("rb_ob_scatter")
    msg = str(e.value)
    assert "make -C robir_amd/csrc observe" in msg and "librobir_hip_observe.so" in msg and "LEGACY" not in msg


def test_observe_argument_errors_before_any_launch():
    L = _ob_lib()
    err = L.rb_ob_last_error

    def scatter(x=FAKE, N=8, M=2, images=FAKE, masks=FAKE, H=8, W=8, C=3, uv=FAKE, valid=FAKE):
        return L.rb_ob_scatter(x, c_long(N), FAKE, FAKE, FAKE, c_int(M), images, masks, c_int(H), c_int(W), c_int(C), uv, FAKE, FAKE, valid, NULL)
    assert scatter(M=0) != 0 and b"M = 0" in err()
    assert scatter(M=4097) != 0 and b"4096" in err()
    assert scatter(H=1) != 0 and b"at least 2" in err()
    assert scatter(W=1) != 0 and b"at least 2" in err()
    assert scatter(C=2) != 0 and b"C = 2" in err()
    assert scatter(C=4) != 0 and b"C = 4" in err()
    assert scatter(N=-1) != 0 and b"negative" in err()
    assert scatter(N=1 << 31) != 0 and b"2^31" in err()
    assert scatter(x=NULL) != 0 and b"null pointer" in err()
    assert scatter(images=NULL) != 0 and b"null pointer" in err()
    assert scatter(uv=NULL) != 0 and b"null pointer" in err()
    assert scatter(valid=NULL) != 0 and b"null pointer" in err()
    assert scatter(N=0, x=NULL, uv=NULL, valid=NULL) == 0              # nothing to do; a null masks pointer is a valid argument

    def fetch(images=FAKE, M=2, H=8, W=8, C=1, uv=FAKE, N=8, out=FAKE):
        return L.rb_ob_fetch(images, c_int(M), c_int(H), c_int(W), c_int(C), uv, c_long(N), out, NULL)
    assert fetch(M=0) != 0 and b"M = 0" in err()
    assert fetch(H=0) != 0 and b"at least 2" in err()
    assert fetch(C=0) != 0 and b"C = 0" in err()
    assert fetch(out=NULL) != 0 and b"null pointer" in err()
    assert fetch(N=0, uv=NULL, out=NULL) == 0

    def select(vis=FAKE, draws=FAKE, M=3, N=8, n_obs=1, index=FAKE, count=FAKE):
        return L.rb_ob_select(vis, draws, c_int(M), c_long(N), c_int(n_obs), index, count, NULL)
    assert select(n_obs=0) != 0 and b"n_obs = 0" in err()
    assert select(n_obs=9) != 0 and b"n_obs = 9" in err()
    assert select(M=0) != 0 and b"M = 0" in err()
    assert select(M=4097) != 0 and b"4096" in err()
    assert select(N=-2) != 0 and b"negative" in err()
    assert select(vis=NULL) != 0 and b"null pointer" in err()
    assert select(draws=NULL) != 0 and b"null pointer" in err()
    assert select(count=NULL) != 0 and b"null pointer" in err()
    assert select(N=0, vis=NULL, draws=NULL, index=NULL, count=NULL) == 0

    def gather(index=FAKE, n_obs=2, x=FAKE, N=8, M=3, H=8, W=8, C=3, rgb=FAKE):
        return L.rb_ob_gather(index, c_int(n_obs), x, c_long(N), FAKE, FAKE, FAKE, c_int(M), FAKE, NULL, c_int(H), c_int(W), c_int(C), FAKE, FAKE,
                              rgb, FAKE, NULL)
    assert gather(n_obs=0) != 0 and b"n_obs = 0" in err()
    assert gather(n_obs=9) != 0 and b"n_obs = 9" in err()
    assert gather(M=0) != 0 and b"M = 0" in err()
    assert gather(C=2) != 0 and b"C = 2" in err()
    assert gather(W=1) != 0 and b"at least 2" in err()
    assert gather(index=NULL) != 0 and b"null pointer" in err()
    assert gather(rgb=NULL) != 0 and b"null pointer" in err()
    assert gather(N=0, index=NULL, x=NULL, rgb=NULL) == 0

    def acc(x=FAKE, normals=FAKE, N=8, M=3, H=8, W=8, C=3, vis=FAKE, weight=FAKE, count=FAKE):
        return L.rb_ob_accumulate(x, normals, c_long(N), FAKE, FAKE, FAKE, c_int(M), FAKE, c_int(H), c_int(W), c_int(C), vis, weight, FAKE, FAKE,
                                  count, NULL)
    assert acc(M=0) != 0 and b"M = 0" in err()
    assert acc(M=4097) != 0 and b"4096" in err()
    assert acc(H=1) != 0 and b"at least 2" in err()
    assert acc(C=2) != 0 and b"C = 2" in err()
    assert acc(N=-1) != 0 and b"negative" in err()
    assert acc(normals=NULL) != 0 and b"null pointer" in err()
    assert acc(vis=NULL) != 0 and b"null pointer" in err()
    assert acc(weight=NULL) != 0 and b"null pointer" in err()
    assert acc(count=NULL) != 0 and b"null pointer" in err()
    assert acc(N=0, x=NULL, normals=NULL, vis=NULL, weight=NULL, count=NULL) == 0


def _host_tool():
    spec = importlib.util.spec_from_file_location("check_observe_host", os.path.join(ROOT, "tools", "check_observe_host.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_host_build_of_the_math_equals_the_restatement():
    """tools/check_observe_host.py: observe_math.h compiled with the host C++ compiler as a stand-alone program (tools/observe_host.cpp
    supplies main and the loops) against the numpy restatement, bit for bit, on every case and both n_obs; and on a case whose draws are
    all equal, where only the tie rule decides the selection."""
    tool = _host_tool()
    if tool.compiler() is None:
        pytest.skip("no host C++ compiler")
    prog = tool.build()
    rows = tool.check(prog)
    assert len(rows) == 14 * (len(CASES) * len(obr.N_OBS) + 1)
    assert [what for what, ok in rows if not ok] == []
    tied = obr.Case(5, 300, 24, 40, "random")
    tied.draws = np.zeros_like(tied.draws)
    rows = tool.check_case(prog, tied, 3)
    assert [what for what, ok in rows if not ok] == []
    index, _ = obr.select(tied.vis(), tied.draws, 3)
    assert (np.diff(index.astype(np.int64), axis=0)[:, tied.vis().sum(0) == 0] > 0).all()      # no view visible: cameras 0, 1, 2


def test_cases_say_what_they_claim():
    assert len(CASES) == 24 and {c.N for c in CASES.values()} == {0, 1, 300} and {c.M for c in CASES.values()} == {1, 5}
    assert {(c.H, c.W) for c in CASES.values()} == {(32, 32), (24, 40)}
    for name in BIG:
        c = CASES[name]
        s = c.scatter()
        valid = s["valid"].astype(bool)
        frac = valid.mean(1)
        if c.M == 5:
            behind = s["z"][obr.BEHIND] <= 0
            assert 10 <= int(behind.sum()) <= 290, name                  # some points behind camera 3, some in front
            assert not valid[obr.BEHIND][behind].any()
            assert (s["z"][[0, 1, 2, 4]] > 0).all()
            frac = frac[[0, 1, 2, 4]]
        assert (frac > 0.3).all() and (frac < 0.95).all(), (name, frac)      # the image border and the mask both cut
        u, v = s["uv"][..., 0], s["uv"][..., 1]
        inside = (u >= 0) & (u < c.W) & (v >= 0) & (v < c.H)
        assert int((inside & (s["z"] > 0) & ~valid).sum()) > 10 and int((~inside).sum()) > 10, name
        seen = c.vis().sum(0)
        assert (np.unique(c.draws).size == c.draws.size) and (seen < 3).any() and (seen >= 1).any()
        if c.M == 5:
            assert (seen >= 3).any() and (seen == 0).any()
        keys = c.vis().astype(np.float32) + np.float32(0.01) * c.draws
        assert np.unique(keys).size == keys.size                         # all keys differ in fp32


@pytest.mark.parametrize("name", sorted(CASES))
def test_excluded_pairs_and_valid_against_float64(name):
    """valid of the fp32 restatement equals that of the float64 form outside the pairs whose float64 uv lies within 1e-3 pixels of an image
    border or whose float64 mask sample lies within 1e-4 of 0.5; at most 1 % of a case's pairs are such."""
    c = CASES[name]
    ex = c.excluded()
    assert ex.sum() <= 0.01 * max(ex.size, 1), (name, int(ex.sum()))
    assert np.array_equal(c.scatter()["valid"][~ex], c.scatter(np.float64)["valid"][~ex])
    nomask = c.scatter(np.float32, False)
    assert np.array_equal(nomask["uv"].view(np.uint32), c.scatter()["uv"].view(np.uint32)) and (nomask["valid"] >= c.scatter()["valid"]).all()


@pytest.mark.parametrize("name", [n for n in BIG if "32x32" in n])
def test_restatement_against_the_reference_lines_on_square_images(name):
    """The fp32 restatement against the reference's lines (F.normalize, matmul, grid_sample(align_corners=True)) on PyTorch-CPU: the two
    float64 forms agree to 1e-9, and the fp32 restatement is within max(2 e_torch, 1e-5) of float64, e_torch being the distance of the
    reference's lines in float32.  valid agrees with the reference's wherever the point is in front of the camera."""
    c = CASES[name]
    s32, s64, t32, t64 = c.scatter(), c.scatter(np.float64), c.scatter_torch(), c.scatter_torch(torch.float64)
    for k in ("uv", "view_dir", "rgb", "mask_value"):
        assert s32[k].dtype == np.float32
        assert rel_err(t64[k], s64[k]) <= 1e-9, k
        e, e_torch = rel_err(s32[k], s64[k]), rel_err(t32[k], s64[k])
        assert e <= max(2 * e_torch, 1e-5), (k, e, e_torch)
    front, ex = s64["z"] > 0, c.excluded()
    assert np.array_equal(s32["valid"][front & ~ex], t64["valid"][front & ~ex])
    if c.M == 5:
        assert int(t64["valid"][~front].sum()) > 0          # the reference takes mirrored projections of points behind the camera
    for n_obs in obr.N_OBS:
        index, count = obr.select(c.vis(), c.draws, n_obs)
        rows = min(c.M, n_obs)                               # the sort of M cameras has M rows: the rest of the index is -1
        assert np.array_equal(index[:rows], obr.select_torch(c.vis(), c.draws, n_obs)) and (index[rows:] == -1).all()
        assert np.array_equal(count, c.vis().sum(0))


@pytest.mark.parametrize("name", [n for n in BIG if "24x40" in n])
def test_non_square_images_take_width_for_u(name):
    """On 24 x 40 images the pair (W, H) is not (H, W): the restatement agrees with grid_sample fed u / W, v / H, points with 24 <= u < 40
    are valid, and none with 24 <= v is."""
    c = CASES[name]
    s32, s64, t32 = c.scatter(), c.scatter(np.float64), c.scatter_torch()
    for k in ("uv", "rgb"):
        e, e_torch = rel_err(s32[k], s64[k]), rel_err(t32[k], s64[k])
        assert e <= max(2 * e_torch, 1e-5), (k, e, e_torch)
    u, v, valid = s32["uv"][..., 0], s32["uv"][..., 1], s32["valid"].astype(bool)
    assert int((valid & (u >= 24)).sum()) > 0 and not (valid & (v >= 24)).any()


@pytest.mark.parametrize("name", [n for n in BIG if "affine" in n])
def test_bilinear_reproduces_the_affine_image(name):
    c = CASES[name]
    s = c.scatter()
    valid = s["valid"].astype(bool)
    ix, iy = obr.pixel_position(s["uv"].astype(np.float64), c.H, c.W, np.float64)
    want = np.stack([ix / c.W, iy / c.H, np.broadcast_to(np.arange(c.M)[:, None] / c.M, ix.shape)], -1)
    assert int(valid.sum()) > 100 and float(np.abs(s["rgb"][valid] - want[valid]).max()) <= 1e-5


@pytest.mark.parametrize("name", BIG)
def test_statistics_restatement_against_float64(name):
    """rb_ob_accumulate's restatement against its float64 form under the parity rule, e_torch being the same statistics written with
    torch sums over the camera axis in float32.  With one camera the exact variance is zero: the fp32 one is at most 8 ulp of the second
    moment (three roundings in s2 / w, three in mean^2)."""
    c = CASES[name]
    v = c.vis()
    a32 = obr.accumulate(c.x, c.normals, *c.cams(), c.images, v)
    a64 = obr.accumulate(c.x, c.normals, *c.cams(), c.images, v, np.float64)
    t32 = obr.accumulate_torch(c.scatter_torch(), c.normals, v)
    t64 = obr.accumulate_torch(c.scatter_torch(torch.float64), c.normals, v, torch.float64)
    assert np.array_equal(a32["count"], a64["count"]) and np.array_equal(a32["count"], t64["count"])
    assert (a32["count"] <= v.sum(0)).all() and (a32["count"] < v.sum(0)).any()          # back-facing views do not count
    none = a32["count"] == 0
    assert none.any() and all((a32[k][none] == 0).all() for k in ("weight", "mean", "var"))
    for k in ("weight", "mean", "var"):
        if c.M > 1 or k != "var":
            assert rel_err(t64[k], a64[k]) <= 1e-9, k
        e, e_torch = rel_err(a32[k], a64[k]), rel_err(t32[k], a64[k])
        assert e <= max(2 * e_torch, 1e-5), (k, e, e_torch)
    if c.M == 1:
        assert (a32["var"] <= 8 * 2.0 ** -24 * a32["mean"] ** 2 + 1e-30).all()


def test_recasting_on_the_restatement():
    """The reference's own test_inv_sampler on the CPU: get_camera_params of the returned uv reproduces view_dir at the valid pairs."""
    c = CASES["M5_N300_24x40_random"]
    s = c.scatter()
    valid = s["valid"].astype(bool)
    d = obr.recast_torch(s["uv"], c.pose, c.K)
    assert float(np.abs(d - s["view_dir"])[valid].max()) <= 1e-5


def test_focus_sampler_and_tex_space_sampler_construction():
    from robir_amd import observe
    c = CASES["M5_N1_24x40_random"]
    t = torch.from_numpy
    fs = observe.FocusSampler(t(c.images).reshape(5, 24 * 40, 3), t(c.masks).reshape(5, 24 * 40), t(c.pose), t(c.K), img_res=(24, 40))
    assert fs.n_cameras == 5 and tuple(fs.images.shape) == (5, 24, 40, 3) and tuple(fs.masks.shape) == (5, 24, 40)
    assert fs.images.dtype == torch.float32 and fs.img_size.tolist() == [24.0, 40.0]
    assert torch.equal(fs.cam_loc, t(c.cam_loc)) and rel_err(fs.pose_inv, c.pose_inv) <= 1e-6
    assert tuple(fs.cameras(slice(2, 3))[3].shape) == (1, 24, 40, 3)
    bare = observe.FocusSampler(t(c.images), torch.zeros(0), t(c.pose)[:, :3, :4], t(c.K))
    assert bare.masks is None and tuple(bare.images.shape) == (5, 24, 40, 3) and torch.equal(bare.pose_inv, fs.pose_inv)
    with pytest.raises(ValueError, match="3 channels"):
        observe.FocusSampler(t(c.images)[..., :2], None, t(c.pose), t(c.K))
    trainer = types.SimpleNamespace(model="m", tex_sampler="t", focus_sampler=fs)
    s = observe.TexSpaceSampler(trainer)
    assert (s.model, s.tex_sampler, s.focus_sampler) == ("m", "t", fs)
    s = observe.TexSpaceSampler("m", "t", fs)
    assert s.focus_sampler is fs
    with pytest.raises(TypeError):
        observe.TexSpaceSampler("m")
    with pytest.raises(ValueError, match="n_obs"):
        s.sample_observations_sorted(torch.zeros(2, 3), torch.ones(2, dtype=torch.bool), n_obs=9, normals=torch.zeros(2, 3))
    assert observe._chunk_points(100) % 256 == 0 and observe._chunk_points(100) * 100 * observe.PAIR_BYTES <= observe.SCATTER_BYTES
    assert observe._chunk_points(4096) >= 256 and observe._chunk_points(5, chunk=7) == 7


def test_export_with_and_without_observed_planes(tmp_path):
    """export writes observed.png and the three planes into maps.npz only when they exist; every other file keeps its bytes."""
    import texbake_restatement as tr
    from robir_amd import mesh, texture
    from test_texbake_cpu import _decode_png
    rng = np.random.default_rng(9)
    V, F, R = 7, 6, 32
    verts = torch.from_numpy(rng.normal(size=(V, 3)).astype(np.float32))
    faces = torch.from_numpy(rng.integers(0, V, (F, 3)).astype(np.int32))
    uv = torch.from_numpy(tr.atlas_uv(F, R))
    fid, bary = tr.raster(uv.numpy(), R)
    planes = {k: torch.from_numpy(rng.uniform(0, 1, (R, R, 3) if k in ("albedo", "normal", "position") else (R, R)).astype(np.float32))
              for k in ("albedo", "roughness", "metallic", "normal", "position", "mask")}
    ts = texture.TextureSet(mesh.Mesh(verts, faces, verts.clone()), uv, torch.from_numpy(fid), torch.from_numpy(bary), **planes)
    assert ts.observed_planes() == {}
    plain = ts.export(str(tmp_path / "plain"))
    assert sorted(os.path.basename(p) for p in plain) == sorted(texture.FILES) and not os.path.exists(str(tmp_path / "plain" / "observed.png"))
    assert sorted(np.load(str(tmp_path / "plain" / "maps.npz")).files) == sorted(["face_id", "uv", *planes])
    ts.observed = torch.from_numpy(rng.uniform(0, 1, (R, R, 3)).astype(np.float32))
    ts.observed_var = torch.from_numpy(rng.uniform(0, 0.1, (R, R, 3)).astype(np.float32))
    ts.observed_count = torch.from_numpy(rng.integers(0, 5, (R, R)).astype(np.float32))
    full = ts.export(str(tmp_path / "full"))
    assert sorted(os.path.basename(p) for p in full) == sorted(texture.FILES + ("observed.png",))
    for n in texture.FILES:
        if n != "maps.npz":          # a zip archive stores its members' time stamps: compared array by array below
            assert open(str(tmp_path / "plain" / n), "rb").read() == open(str(tmp_path / "full" / n), "rb").read(), n
    a, b = np.load(str(tmp_path / "plain" / "maps.npz")), np.load(str(tmp_path / "full" / "maps.npz"))
    assert sorted(b.files) == sorted(a.files + ["observed", "observed_var", "observed_count"])
    assert all(a[k].tobytes() == b[k].tobytes() and a[k].dtype == b[k].dtype for k in a.files)
    for k in ("observed", "observed_var", "observed_count"):
        assert b[k].tobytes() == getattr(ts, k).numpy().tobytes()
    rgb = _decode_png(open(str(tmp_path / "full" / "observed.png"), "rb").read())
    assert np.array_equal(rgb, np.round(mesh._srgb(ts.observed.numpy().astype(np.float64)) * 255).astype(np.uint8))
