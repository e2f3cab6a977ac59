"""The camera-space rasteriser on the device (robir_amd/csrc/raster/raster.hip, robir_amd/meshrender.py) against the numpy fp32 restatement
of its conventions (tests/meshrender_restatement.py): every kernel bit for bit; then the view of the baked synthetic scene end to end
against the neural view it was baked from (tests/meshrender_scene.py), and the command line into robir_amd.evaluate."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshrender_restatement as mr  # noqa: E402
import meshrender_scene as ms  # noqa: E402
from conftest import GOLD, record_metric  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = mr.raster_cases()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def reference(name, cull=0):
    """The restatement's (face_id, bary, depth) of a raster case -- computed once, shared, never modified."""
    screen, faces, H, W = CASES[name]
    return mr.raster(screen, faces, H, W, cull=cull)


def device_raster(screen, faces, H, W, cull=0):
    from robir_amd import meshrender
    fid, bary, depth = meshrender.rasterize_screen(dev(screen), dev(faces), H, W, cull=cull)
    assert fid.dtype == torch.int32 and tuple(fid.shape) == (H, W) and tuple(bary.shape) == (H, W, 2) and tuple(depth.shape) == (H, W)
    return fid.cpu().numpy(), bary.cpu().numpy(), depth.cpu().numpy()


def _camera(H, W):
    from robir_amd import synth
    _, _, K = synth.synth_camera(H, W)
    pose = mr.rotated_pose()
    return pose, mr.pose_inverse(pose), K


# ----------------------------------------------------------------------------------------- kernels against the restatement
@pytest.mark.parametrize("cull", (0, 1, 2))
@pytest.mark.parametrize("name", sorted(CASES))
def test_raster_equals_restatement(name, cull):
    """13 x 21 images (H != W, neither a multiple of 8): 200 faces in one tile (four batches, depth order across them), coincident faces, a
    shared edge through pixel centres, faces off-screen / behind the camera / NaN / zero area / out-of-range indices, every cull value."""
    screen, faces, H, W = CASES[name]
    ref_id, ref_bary, ref_depth = reference(name, cull)
    fid, bary, depth = device_raster(screen, faces, H, W, cull)
    assert np.array_equal(fid, ref_id)
    assert same_bits(bary, ref_bary) and same_bits(depth, ref_depth)


def test_binning_equals_restatement():
    from robir_amd import ops
    for name in ("tile200", "edge_cases", "windings"):
        screen, faces, H, W = CASES[name]
        for cull in (0, 1, 2):
            counts = ops.rs_bin_count(dev(screen), dev(faces), H, W, mr.NEAR, cull)
            assert np.array_equal(counts.cpu().numpy(), mr.bin_counts(screen, faces, H, W, cull=cull)), (name, cull)
            incl = torch.cumsum(counts.to(torch.int64), 0)
            P = int(incl[-1])
            pt, pf = ops.rs_bin_emit(dev(screen), dev(faces), H, W, mr.NEAR, cull, (incl - counts).contiguous(), P)
            ref_t, ref_f = mr.bin_pairs(screen, faces, H, W, cull=cull)
            assert np.array_equal(pt.cpu().numpy(), ref_t) and np.array_equal(pf.cpu().numpy(), ref_f), (name, cull)


def test_raster_properties():
    fid, _, _ = device_raster(*CASES["coincident"])
    assert (fid == 0).sum() > 10 and not (fid == 1).any()                     # the lower index of two coincident faces wins
    for name in ("shared_edge", "shared_edge_mixed"):
        fid, _, _ = device_raster(*CASES[name])
        assert (fid[1:12, 2:13] >= 0).all()                                   # no hole along the shared edge
    screen, faces, H, W = CASES["edge_cases"]
    fid, bary, depth = device_raster(screen, faces[:0], H, W)                 # no face at all
    assert (fid == -1).all() and not bary.any() and not depth.any()
    fid, _, _ = device_raster(screen, faces[1:6], H, W)                       # only skipped faces: no pair
    assert (fid == -1).all()


@pytest.mark.parametrize("size", ((64, 64), (13, 21)))
def test_projected_icosphere_equals_restatement(size):
    """Projection and rasteriser on a rotated camera: 1280 faces, several faces per pixel at 13 x 21, both culls."""
    from robir_amd import meshrender, ops
    H, W = size
    pose, pinv, K = _camera(H, W)
    v, f = mr.icosphere(3)
    screen = ops.rs_project(dev(v), dev(pinv), dev(K))
    ref_screen = mr.project(v, pinv, K)
    assert same_bits(screen, ref_screen)
    for cull in (0, 2):
        fid, bary, depth = meshrender.rasterize_screen(screen, dev(f), H, W, cull=cull)
        ref_id, ref_bary, ref_depth = mr.raster(ref_screen, f, H, W, cull=cull)
        assert np.array_equal(fid.cpu().numpy(), ref_id) and same_bits(bary, ref_bary) and same_bits(depth, ref_depth)
    assert (ref_id >= 0).sum() > (40 if H == 13 else 900)
    # the public entry point forms the inverse pose itself (torch.inverse): same mask, depth to rounding
    fid2, _, depth2 = meshrender.rasterize(dev(v), dev(f), dev(pose), dev(K), H, W)
    assert (fid2.cpu().numpy() != ref_id).sum() <= 2 and np.abs(depth2.cpu().numpy() - ref_depth)[(fid2.cpu().numpy() == ref_id)].max() < 1e-5


@pytest.mark.parametrize("filt", (0, 1))
def test_gbuffer_equals_restatement(filt):
    """Image form and list form (hit rows; and rows out of range, which give zeros), both filters, vertex normals."""
    from robir_amd import meshrender
    verts, faces, uv, planes, vn = mr.gbuffer_case()
    H, W = 13, 21
    pose, pinv, K = _camera(H, W)
    screen = mr.project(verts, pinv, K)
    face_id, bary, _ = mr.raster(screen, faces, H, W)
    hit = np.nonzero(face_id.reshape(-1) >= 0)[0]
    assert hit.size > 60 and len(np.unique(face_id)) == 3
    for index in (None, hit, np.array([0, 5, -1, H * W, hit[0]], dtype=np.int64)):
        got = meshrender.gbuffer(dev(face_id), dev(bary), dev(verts), dev(faces), dev(uv), dev(pose[:3, 3].copy()), dev(planes), filt, dev(vn),
                                 None if index is None else dev(index))
        want = mr.gbuffer(face_id, bary, faces, verts, uv, pose[:3, 3], planes, filt, vn, index)
        assert set(got) == set(want) == {"position", "uv", "view_dir", "tex", "normal"}
        for k in want:
            assert same_bits(got[k], want[k]), (k, filt, None if index is None else len(index))
    # without planes and normals only the geometry comes back
    got = meshrender.gbuffer(dev(face_id), dev(bary), dev(verts), dev(faces), dev(uv), dev(pose[:3, 3].copy()), index=dev(hit))
    assert set(got) == {"position", "uv", "view_dir"} and same_bits(got["position"], want_position(face_id, bary, faces, verts, uv, pose, hit))


def want_position(face_id, bary, faces, verts, uv, pose, hit):
    return mr.gbuffer(face_id, bary, faces, verts, uv, pose[:3, 3], index=hit)["position"]


@pytest.mark.parametrize("filt", (0, 1))
def test_filters_return_a_texel_centre_bit_for_bit(filt):
    """Pixels whose weights are exactly (1, 0), (0, 1) and (0, 0) get a corner's uv exactly; the corners sit on texel centres (R = 8: exact
    in fp32), so either filter returns that texel bit for bit -- the bilinear one with weights 1, 0, 0, 0."""
    from robir_amd import meshrender
    verts, faces, _, planes, _ = mr.gbuffer_case()
    R = planes.shape[0]
    texels = ((5, 3), (0, 7), (7, 0))
    uv = np.zeros((2, 3, 2), dtype=np.float32)
    uv[0] = [((c + 0.5) / R, 1.0 - (r + 0.5) / R) for r, c in texels]
    face_id = np.array([[0, 0, 0], [0, -1, 0]], dtype=np.int32)
    bary = np.array([[(1, 0), (0, 1), (0, 0)], [(0.25, 0.5), (0, 0), (1, 0)]], dtype=np.float32)
    g = meshrender.gbuffer(dev(face_id), dev(bary), dev(verts), dev(faces), dev(uv), dev(np.zeros(3, dtype=np.float32)), dev(planes), filt)
    tex = g["tex"].cpu().numpy()
    want = mr.gbuffer(face_id, bary, faces, verts, uv, np.zeros(3), planes, filt)["tex"]
    assert same_bits(tex, want)
    for row, (r, c) in zip((0, 1, 2, 5), texels + (texels[0],)):
        assert np.array_equal(bits(tex[row]), bits(planes[r, c])), (row, filt)
    assert not tex[4].any()


def test_two_runs_are_byte_equal():
    from robir_amd import meshrender
    screen, faces, H, W = CASES["tile200"]
    a, b = device_raster(screen, faces, H, W), device_raster(screen, faces, H, W)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    pose, pinv, K = _camera(64, 64)
    v, f = mr.icosphere(3)
    runs = [meshrender.rasterize(dev(v), dev(f), dev(pose), dev(K), 64, 64) for _ in range(2)]
    assert all(torch.equal(x, y) for x, y in zip(*runs))


# ----------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def scene():
    return ms.build(DEV)


@pytest.fixture(scope="module")
def mesh_view(scene):
    from robir_amd import meshrender
    return meshrender.render_mesh(scene["ts"], torch.from_numpy(scene["pose"]), torch.from_numpy(scene["K"]), ms.H, ms.W, model=scene["model"],
                                  vis="network", draws=scene["draws"])


def test_hit_mask_differs_from_the_neural_one_on_its_boundary_only(scene, mesh_view):
    """The mesh's chord error (~1e-3) is a tenth of a pixel's footprint (~1e-2): the two hit masks may differ only where the neural mask's
    8-neighbourhood holds both a hit and a miss."""
    neural = scene["neural"]["network_object_mask"].reshape(ms.H, ms.W).cpu().numpy()
    mine = mesh_view["network_object_mask"].reshape(ms.H, ms.W).cpu().numpy()
    differ = mine != neural
    record_metric("meshrender_mask", differ=int(differ.sum()), off_boundary=int((differ & ~ms.boundary(neural)).sum()), hit=int(neural.sum()))
    print("hit pixels", int(neural.sum()), "differ", int(differ.sum()), "off the boundary", int((differ & ~ms.boundary(neural)).sum()))
    assert neural.sum() > 500
    assert not (differ & ~ms.boundary(neural)).any()


def test_fields_stay_within_twice_the_float64_paths_distance(scene, mesh_view):
    """diffuse_albedo, roughness, normals and sg_rgb (vis='network') on the interior pixels against forward('Material'): the distance is
    discretisation (mesh, atlas, dilation; for sg_rgb also the baked normal in place of the normal network's), which cannot be derived, so
    it was measured with the float64 path of tests/meshrender_restatement.py -- independent of the new kernels -- by
    tools/measure_meshrender_caps.py into tests/golden/meshrender_caps.json; the cap is twice that, without a floor."""
    caps = json.load(open(os.path.join(GOLD, "meshrender_caps.json")))["caps"]
    neural = scene["neural"]
    inner = ms.interior(neural["network_object_mask"].reshape(ms.H, ms.W).cpu().numpy())
    got = ms.distances(mesh_view, neural, inner)
    record_metric("meshrender_fields", **got)
    print("measured", got, "caps", caps)
    assert inner.sum() > 400
    for k in ms.FIELDS:
        assert got[k] <= 2.0 * caps[k], (k, got[k], caps[k])


def test_result_layout_and_direct_shading(scene, mesh_view):
    """render.py's keys with one row per pixel; vis='none' is direct SG shading: no indirect term, no shadow, and needs no model."""
    from robir_amd import meshrender
    N = ms.H * ms.W
    for k in meshrender.KEYS:
        assert k in mesh_view and mesh_view[k].shape[0] == N, k
    hit = mesh_view["network_object_mask"]
    assert (mesh_view["depth"][~hit] == 0).all() and (mesh_view["depth"][hit] > 0.5).all() and (mesh_view["depth"][hit] < 0.9).all()
    assert float(mesh_view["indir_rgb"][hit].abs().max()) > 0
    lgt = scene["model"].envmap_material_network.lgtSGs.detach()
    pose, K = torch.from_numpy(scene["pose"]), torch.from_numpy(scene["K"])
    direct = meshrender.render_mesh(scene["ts"], pose, K, ms.H, ms.W, light=lgt, vis="none")
    with_model = meshrender.render_mesh(scene["ts"], pose, K, ms.H, ms.W, model=scene["model"], vis="none")
    assert torch.equal(direct["network_object_mask"], hit) and torch.equal(direct["diffuse_albedo"], mesh_view["diffuse_albedo"])
    assert not direct["indir_rgb"].any() and torch.isfinite(direct["sg_rgb"]).all()
    assert not with_model["indir_rgb"].any() and torch.isfinite(with_model["sg_rgb"]).all() and "pred_rgb" in with_model
    assert float((with_model["sg_rgb"][hit] - mesh_view["sg_rgb"][hit]).abs().max()) > 0          # the visibility is gone
    nearest = meshrender.render_mesh(scene["ts"], pose, K, ms.H, ms.W, light=lgt, vis="none", filter=0)
    assert float((nearest["diffuse_albedo"] - direct["diffuse_albedo"]).abs().max()) < 0.05


def test_command_line_writes_a_view_that_evaluate_accepts(scene, tmp_path):
    from robir_amd import evaluate, meshrender
    asset = str(tmp_path / "asset")
    scene["ts"].export(asset)
    out = str(tmp_path / "meshview.npz")
    meshrender.main(["--asset", asset, "--synthetic", "--size", str(ms.H), "--vis", "none", "--out", out])
    with np.load(out) as z:
        for k in meshrender.KEYS:
            assert k in z.files and z[k].shape[:2] == (ms.H, ms.W), k
        assert z["network_object_mask"].sum() > 500
    gt = str(tmp_path / "neuralview.npz")
    keep = ("sg_rgb", "indir_rgb", "diffuse_albedo", "roughness", "normals", "normal_map", "network_object_mask")
    np.savez(gt, **{k: scene["neural"][k].cpu().numpy().reshape(ms.H, ms.W, -1) for k in keep})
    report = str(tmp_path / "metrics.json")
    evaluate.main(["--pred", out, "--gt", gt, "--out", report])
    doc = json.load(open(report))
    assert len(doc["views"]) == 1 and all(k in doc["mean"] for k in ("psnr", "ssim", "albedo_psnr", "roughness_mse", "normal_mae_deg"))
    print("round trip, direct shading against the neural view:", doc["mean"])
