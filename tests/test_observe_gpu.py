"""Multi-view observations on the device (robir_amd/csrc/observe/observe.hip, robir_amd/observe.py) against the numpy fp32 restatement of
their arithmetic (tests/observe_restatement.py): every kernel bit for bit, the scatter and the statistics also against float64 under the
parity rule, and the Python layers on the synthetic scene: visibility, the texture-space sampler, a rendered batch and the export."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import observe_restatement as obr  # noqa: E402
from conftest import record_metric, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = obr.cases()
BIG = sorted(n for n, c in CASES.items() if c.N == 300)


def same_bits(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_scatter(c, masks=True):
    from robir_amd import ops
    uv, view_dir, rgb, valid = ops.ob_scatter(dev(c.x), dev(c.cam_loc), dev(c.pose_inv), dev(c.K), dev(c.images), dev(c.masks) if masks else None)
    assert tuple(uv.shape) == (c.M, c.N, 2) and tuple(view_dir.shape) == (c.M, c.N, 3) and tuple(rgb.shape) == (c.M, c.N, 3)
    assert tuple(valid.shape) == (c.M, c.N) and valid.dtype == torch.uint8
    return {"uv": uv, "view_dir": view_dir, "rgb": rgb, "valid": valid}


# ----------------------------------------------------------------------------------------- the kernels, bit for bit
@pytest.mark.parametrize("name", sorted(CASES))
def test_scatter_equals_restatement(name):
    c = CASES[name]
    got, ref = device_scatter(c), c.scatter()
    for k in ("uv", "view_dir", "rgb", "valid"):
        assert same_bits(got[k], ref[k]), k
    if name == "M5_N300_24x40_random":                               # a null masks pointer: the mask term is left out
        got, ref = device_scatter(c, masks=False), c.scatter(np.float32, False)
        assert all(same_bits(got[k], ref[k]) for k in ("uv", "view_dir", "rgb", "valid"))
        assert int(got["valid"].sum()) > int(c.scatter()["valid"].sum())


@pytest.mark.parametrize("name", sorted(CASES))
def test_select_gather_and_fetch_equal_restatement(name):
    from robir_amd import ops
    c = CASES[name]
    sc = c.scatter()
    for n_obs in obr.N_OBS:
        index, count = ops.ob_select(dev(c.vis()), dev(c.draws), n_obs)
        ref_index, ref_count = obr.select(c.vis(), c.draws, n_obs)
        assert index.dtype == torch.int32 and np.array_equal(index.cpu().numpy(), ref_index) and np.array_equal(count.cpu().numpy(), ref_count)
        uv, view_dir, rgb, valid = ops.ob_gather(index, dev(c.x), dev(c.cam_loc), dev(c.pose_inv), dev(c.K), dev(c.images), dev(c.masks))
        ref = obr.gather(ref_index, sc)
        assert same_bits(uv, ref["uv"]) and same_bits(view_dir, ref["view_dir"]) and same_bits(rgb, ref["rgb"]) and same_bits(valid, ref["valid"])
    assert same_bits(ops.ob_fetch(dev(c.images), dev(sc["uv"])), sc["rgb"])
    assert same_bits(ops.ob_fetch(dev(c.masks[..., None]), dev(sc["uv"]))[..., 0], sc["mask_value"])


def test_select_ties_go_to_the_lower_camera():
    """Equal draws: only the tie rule decides.  Points with fewer visible views than n_obs take invisible cameras, lowest first."""
    from robir_amd import ops
    c = CASES["M5_N300_24x40_random"]
    zeros = np.zeros_like(c.draws)
    index, count = ops.ob_select(dev(c.vis()), dev(zeros), 3)
    ref_index, _ = obr.select(c.vis(), zeros, 3)
    assert np.array_equal(index.cpu().numpy(), ref_index)
    few = c.vis().sum(0) < 3
    assert few.any() and np.array_equal(count.cpu().numpy()[few], c.vis().sum(0)[few])
    none = c.vis().sum(0) == 0
    assert (index.cpu().numpy()[:, none] == np.array([[0], [1], [2]])).all()
    one = ops.ob_select(dev(c.vis()[:1]), dev(zeros[:1]), 3)[0].cpu().numpy()          # M < n_obs: -1 beyond the cameras
    assert (one[0] == 0).all() and (one[1:] == -1).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_accumulate_equals_restatement(name):
    from robir_amd import ops
    c = CASES[name]
    weight, mean, var, count = ops.ob_accumulate(dev(c.x), dev(c.normals), dev(c.cam_loc), dev(c.pose_inv), dev(c.K), dev(c.images), dev(c.vis()))
    ref = obr.accumulate(c.x, c.normals, *c.cams(), c.images, c.vis())
    assert same_bits(weight, ref["weight"]) and same_bits(mean, ref["mean"]) and same_bits(var, ref["var"])
    assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), ref["count"])


# ----------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("name", BIG)
def test_scatter_and_statistics_against_float64(name):
    """e <= max(2 e_torch, 1e-5) against the float64 restatement, e_torch being the distance of the reference's lines on fp32 PyTorch-CPU
    from the same float64 form; valid equals the float64 one outside the pairs on an image border or on the mask's 0.5 level."""
    from robir_amd import ops
    c = CASES[name]
    got, s64, t32 = device_scatter(c), c.scatter(np.float64), c.scatter_torch()
    for k in ("uv", "view_dir", "rgb"):
        e, e_torch = rel_err(got[k], s64[k]), rel_err(t32[k], s64[k])
        record_metric(f"observe/scatter/{name}/{k}", e=e, e_torch=e_torch)
        print(name, k, e, e_torch)
        assert e <= max(2 * e_torch, 1e-5), (k, e, e_torch)
    ex = c.excluded()
    assert ex.sum() <= 0.01 * ex.size
    assert np.array_equal(got["valid"].cpu().numpy()[~ex], s64["valid"][~ex])
    weight, mean, var, count = ops.ob_accumulate(dev(c.x), dev(c.normals), dev(c.cam_loc), dev(c.pose_inv), dev(c.K), dev(c.images), dev(c.vis()))
    a64 = obr.accumulate(c.x, c.normals, *c.cams(), c.images, c.vis(), np.float64)
    a_t = obr.accumulate_torch(t32, c.normals, c.vis())
    for k, a in (("mean", mean), ("var", var)):
        e, e_torch = rel_err(a, a64[k]), rel_err(a_t[k], a64[k])
        record_metric(f"observe/accumulate/{name}/{k}", e=e, e_torch=e_torch)
        print(name, k, e, e_torch)
        assert e <= max(2 * e_torch, 1e-5), (k, e, e_torch)
    assert np.array_equal(count.cpu().numpy(), a64["count"])


@pytest.mark.parametrize("name", BIG)
def test_recasting_reproduces_view_dir(name):
    """The reference's test_inv_sampler: camera rays cast through the returned uv are the returned view_dir at the valid pairs, to
    max(2 x, 1e-5) of what the reference's two steps (inv_camera_params, get_camera_params) achieve on fp32 PyTorch-CPU."""
    from robir_amd import ops
    c = CASES[name]
    got, t32 = device_scatter(c), c.scatter_torch()
    valid = got["valid"].bool().cpu().numpy()
    assert valid.any()
    d = torch.stack([ops.camera_rays(dev(c.pose[m]), dev(c.K[m]), got["uv"][m].contiguous()) for m in range(c.M)])
    e = float(np.abs(d.cpu().numpy() - got["view_dir"].cpu().numpy())[valid].max())
    e_torch = float(np.abs(obr.recast_torch(t32["uv"], c.pose, c.K) - t32["view_dir"])[valid].max())
    record_metric(f"observe/recast/{name}", e=e, e_torch=e_torch)
    print(name, e, e_torch)
    assert e <= max(2 * e_torch, 1e-5), (e, e_torch)


@pytest.mark.parametrize("name", [n for n in BIG if "affine" in n])
def test_bilinear_reproduces_the_affine_image(name):
    c = CASES[name]
    got = device_scatter(c)
    valid = got["valid"].bool().cpu().numpy()
    ix, iy = obr.pixel_position(got["uv"].cpu().numpy().astype(np.float64), c.H, c.W, np.float64)
    want = np.stack([ix / c.W, iy / c.H, np.broadcast_to(np.arange(c.M)[:, None] / c.M, ix.shape)], -1)
    assert int(valid.sum()) > 100 and float(np.abs(got["rgb"].cpu().numpy() - want)[valid].max()) <= 1e-5


# ----------------------------------------------------------------------------------------- the Python layers on the synthetic scene
@functools.lru_cache(maxsize=None)
def _scene():
    """(model with its octrees, mesh of the 33^3 lattice, FocusSampler of five views of 32 x 32 around it, 300 surface points, normals) --
    built once, shared, never modified.  Camera 1 looks past the object, so that part of it leaves the image."""
    from robir_amd import mesh, observe, renderer
    model = renderer.build_synthetic_model(DEV, scene="sphere")
    m = mesh.extract_mesh(model, resolution=33)
    c = CASES["M5_N300_32x32_random"]
    K = c.K.copy()
    K[1, 0, 2] += 14.0
    fs = observe.FocusSampler(dev(c.images), dev(c.masks), dev(c.pose), dev(K))
    pick = torch.linspace(0, m.vertices.shape[0] - 1, 300, device=DEV).long()
    x = m.vertices[pick].contiguous()
    n = m.normals[pick]
    return model, m, fs, x, (n / n.norm(dim=-1, keepdim=True)).contiguous()


class _CountRays:
    """Counts the rays that go through model.octree_ray_tracer while it is in force."""

    def __init__(self, model):
        self.tracer, self.rays, self.calls = model.octree_ray_tracer, 0, 0

    def __enter__(self):
        inner = self.tracer.forward

        def forward(sdf, cam_loc, object_mask, ray_directions):
            self.rays += ray_directions.shape[0] * ray_directions.shape[1]
            self.calls += 1
            return inner(sdf=sdf, cam_loc=cam_loc, object_mask=object_mask, ray_directions=ray_directions)
        self.tracer.forward = forward
        return self

    def __exit__(self, *exc):
        del self.tracer.forward


def test_focus_sampler_scatter_sample():
    """scatter_sample's keys, shapes and dtypes; its numbers are the restatement's on the sampler's own inverse poses."""
    model, m, fs, x, n = _scene()
    sample, gt = fs.scatter_sample(x)
    assert sorted(sample) == ["object_mask", "uv", "view_dir"] and sorted(gt) == ["rgb"]
    assert sample["object_mask"].dtype == torch.bool and tuple(sample["object_mask"].shape) == (5, 300) and tuple(gt["rgb"].shape) == (5, 300, 3)
    ref = obr.scatter(x.cpu().numpy(), fs.cam_loc.cpu().numpy(), fs.pose_inv.cpu().numpy(), fs.intrinsics.cpu().numpy(), fs.images.cpu().numpy(),
                      fs.masks.cpu().numpy())
    assert same_bits(sample["uv"], ref["uv"]) and same_bits(sample["view_dir"], ref["view_dir"]) and same_bits(gt["rgb"], ref["rgb"])
    assert np.array_equal(sample["object_mask"].cpu().numpy(), ref["valid"].astype(bool))
    assert rel_err(fs.pose_inv, CASES["M5_N300_32x32_random"].pose_inv) <= 1e-5
    from robir_amd import observe
    uv, dirs = observe.inv_camera_params(x[None].expand(5, -1, -1), fs.pose_inv, fs.cam_loc, fs.intrinsics)
    assert same_bits(uv, ref["uv"]) and same_bits(dirs, ref["view_dir"])
    assert same_bits(fs.sample_images(uv), ref["rgb"]) and np.array_equal(fs.sample_masks(uv)[..., 0].cpu().numpy(), ref["mask_value"] > 0.5)


def test_visible_views_equals_a_dense_cast():
    """visible_views casts the valid pairs only, as one batch, and scatters the answers back: at the valid entries it equals a cast of all
    M N pairs through the same tracer, and it is False elsewhere."""
    from robir_amd import observe
    model, m, fs, x, n = _scene()
    sample, _ = fs.scatter_sample(x)
    valid = sample["object_mask"]
    assert 0 < int(valid.sum()) < valid.numel() and bool((~valid[1]).any())
    with _CountRays(model) as counter:
        vis = observe.visible_views(model, fs, x, n)
    assert counter.calls == 1 and counter.rays == int(valid.sum())
    assert vis.dtype == torch.bool and tuple(vis.shape) == (5, 300)
    origins = (x + n * 0.005)[None].expand(5, -1, -1).reshape(-1, 3).contiguous()
    dirs = (-sample["view_dir"]).reshape(-1, 1, 3).contiguous()
    _, hit, _ = model.octree_ray_tracer(sdf=None, cam_loc=origins, object_mask=None, ray_directions=dirs)
    dense = ~hit.reshape(5, 300)
    assert torch.equal(vis[valid], dense[valid]) and not bool(vis[~valid].any())
    assert 0 < int(vis.sum()) < int(valid.sum())                      # the far side of the object is occluded
    one = observe.visible_views(model, fs, x, n, cameras=slice(2, 3))
    assert tuple(one.shape) == (1, 300) and torch.equal(one[0], vis[2])
    with _CountRays(model) as counter:                                # every point behind the camera: no valid pair, no cast at all
        behind = observe.visible_views(model, fs, (x + 2.0 * fs.cam_loc[0]).contiguous(), n, cameras=slice(0, 1))
    assert counter.calls == 0 and not bool(behind.any())


def test_observed_color_is_reproducible():
    """The same bytes twice and for two chunk sizes; the numbers are the restatement's statistics fed the same visibility."""
    from robir_amd import observe
    model, m, fs, x, n = _scene()
    a = observe.observed_color(model, fs, x, n)
    b = observe.observed_color(model, fs, x, n)
    small = observe.observed_color(model, fs, x, n, chunk=64)
    odd = observe.observed_color(model, fs, x, n, chunk=77)
    for other in (b, small, odd):
        assert all(same_bits(p, q) for p, q in zip(a, other))
    mean, var, weight, count = a
    assert tuple(mean.shape) == (300, 3) and tuple(var.shape) == (300, 3) and tuple(weight.shape) == (300,) and count.dtype == torch.int32
    vis = observe.visible_views(model, fs, x, n).to(torch.uint8)
    ref = obr.accumulate(x.cpu().numpy(), n.cpu().numpy(), fs.cam_loc.cpu().numpy(), fs.pose_inv.cpu().numpy(), fs.intrinsics.cpu().numpy(),
                         fs.images.cpu().numpy(), vis.cpu().numpy())
    assert same_bits(mean, ref["mean"]) and same_bits(var, ref["var"]) and same_bits(weight, ref["weight"])
    assert np.array_equal(count.cpu().numpy(), ref["count"]) and 0 < int((count > 0).sum())


def test_tex_space_sampler_equals_the_reference_lines():
    """With the camera and the draws pinned, sample_observations_sorted equals tex_module.py's lines (PyTorch-CPU) fed what
    sample_observations returns; with all_views it takes the restatement's choice among the five cameras."""
    from robir_amd import observe
    model, m, fs, x, n = _scene()
    tss = observe.TexSpaceSampler(model, types.SimpleNamespace(), fs)
    surface = torch.ones(300, dtype=torch.bool, device=DEV)
    surface[::7] = False
    xs, ns = x[surface].contiguous(), n[surface].contiguous()
    with _CountRays(model) as counter:
        rgb, dirs, vis, pos = tss.sample_observations(xs, ns, camera=2)
    sc = fs.scatter(xs, slice(2, 3))
    assert counter.rays == int(sc[3].sum())                          # the cast is that camera's alone
    assert tuple(rgb.shape) == (1, xs.shape[0], 3) and tuple(vis.shape) == (1, xs.shape[0]) and tuple(pos.shape) == (1, 3)
    assert same_bits(rgb, sc[2]) and same_bits(dirs, sc[1]) and torch.equal(pos, fs.cam_loc[2:3]) and 0 < int(vis.sum()) < vis.numel()
    draws = torch.rand(1, xs.shape[0], device=DEV)
    mask = surface.clone()
    got = tss.sample_observations_sorted(x, mask, normals=n, camera=2, draws=draws)
    ref = obr.sorted_torch(x.cpu(), surface.cpu(), rgb.cpu(), dirs.cpu(), vis.cpu(), pos.cpu(), 1, draws.cpu())
    for g, r in zip(got, ref[:4]):
        assert same_bits(g, r)
    assert np.array_equal(mask.cpu().numpy(), ref[4]) and 0 < int(mask.sum()) < int(surface.sum())      # narrowed in place
    # all five cameras, three observations per point
    vis_all = observe.visible_views(model, fs, xs, ns).to(torch.uint8)
    draws = dev(((np.random.default_rng(3).permutation(5 * xs.shape[0]).reshape(5, -1) + 0.5) / (5 * xs.shape[0])).astype(np.float32))
    mask = surface.clone()
    rgb3, dirs3, m3, pos3 = tss.sample_observations_sorted(x, mask, n_obs=3, normals=n, all_views=True, draws=draws)
    index, count = obr.select(vis_all.cpu().numpy(), draws.cpu().numpy(), 3)
    keep = count >= 3
    assert 0 < int(keep.sum()) < keep.size and np.array_equal(mask.cpu().numpy()[surface.cpu().numpy()], keep)
    full = fs.scatter(xs)
    cols = np.arange(xs.shape[0])[keep]
    assert tuple(rgb3.shape) == (3, 300, 3) and same_bits(rgb3[:, mask], full[2].cpu().numpy()[index[:, keep], cols])
    assert same_bits(dirs3[:, mask], full[1].cpu().numpy()[index[:, keep], cols])
    assert same_bits(pos3[:, mask], fs.cam_loc.cpu().numpy()[index[:, keep]])
    assert bool((rgb3[:, ~mask] == 1).all()) and bool((pos3[:, ~mask] == 0).all()) and torch.equal(m3, mask.float())
    assert bool(vis_all.bool()[torch.from_numpy(index[:, keep]).to(DEV).long(), torch.from_numpy(cols).to(DEV)].all())   # every chosen view sees its point


@pytest.fixture(scope="module")
def baked():
    """(model, FocusSampler of four 32 x 32 views from distance 0.9, TextureSet of a 256^2 bake of the 33^3 mesh) -- made once, shared."""
    from robir_amd import observe, texture
    model, m, _, _, _ = _scene()
    rng = np.random.default_rng(21)
    pose = np.stack([obr.look_at(np.array(p) / np.linalg.norm(p) * 0.9) for p in ((1, 0.2, 0.3), (-1, 0.5, 0.2), (0.2, 1, -0.4), (0.1, -1, 0.5))])
    K = np.tile(np.array([[44.0, 0, 16.0], [0, 44.0, 16.0], [0, 0, 1]]), (4, 1, 1))
    fs = observe.FocusSampler(dev(rng.uniform(size=(4, 32, 32, 3)).astype(np.float32)), None, dev(pose.astype(np.float32)), dev(K.astype(np.float32)))
    return model, fs, texture.bake(model, m, resolution=256)


def test_data_batch_renders(baked):
    """data_batch(64) of the baked scene goes through model(new_inputs, trainstage="Material"): finite outputs, and the hook sees one
    tex_uv row per hit."""
    from robir_amd import observe
    model, fs, ts = baked
    tss = observe.TexSpaceSampler(model, ts.sampler(), fs)
    torch.manual_seed(5)
    new_inputs, normal, obs_rgb = tss.data_batch(64)
    assert sorted(new_inputs) == ["dirs", "object_mask", "points", "tex_uv"]
    assert tuple(new_inputs["points"].shape) == (1, 64, 3) and tuple(new_inputs["dirs"].shape) == (1, 64, 3)
    assert new_inputs["object_mask"].dtype == torch.bool and tuple(new_inputs["object_mask"].shape) == (1, 64)
    assert tuple(new_inputs["tex_uv"].shape) == (1, 64, 2) and tuple(normal.shape) == (64, 3) and tuple(obs_rgb.shape) == (64, 3)
    assert int(new_inputs["object_mask"].sum()) > 0
    seen, orig = {}, model.get_sg_render

    def hook(*a, **k):
        seen["tex_uv"] = k.get("tex_uv")
        return orig(*a, **k)
    hook.robir_native = True
    model.get_sg_render = hook
    try:
        out = model(new_inputs, trainstage="Material")
    finally:
        del model.get_sg_render
    hit = out["network_object_mask"]
    assert int(hit.sum()) > 0 and seen["tex_uv"].shape[1] == int(hit.sum()) and torch.equal(seen["tex_uv"], new_inputs["tex_uv"][:, hit])
    assert not bool(hit[~new_inputs["object_mask"][0]].any())          # rays outside the mask are not traced
    for k in ("sg_rgb", "diffuse_albedo", "roughness", "normals", "points"):
        assert bool(torch.isfinite(out[k]).all()), k
    simple = tss.simple_data_batch({"uv": torch.zeros(1, 16, 2)})
    assert sorted(simple) == ["normals", "object_mask", "points"] and tuple(simple["points"].shape) == (16, 3)


def test_bake_observations_and_export(baked, tmp_path):
    """bake_observations adds the three planes (the covered texels hold observed_color's numbers), export then writes observed.png and
    leaves every other file as an export without the planes writes it."""
    from robir_amd import observe, texture
    model, fs, ts = baked
    assert ts.observed is None
    before = ts.export(str(tmp_path / "before"))
    assert sorted(os.path.basename(p) for p in before) == sorted(texture.FILES)
    ts.bake_observations(model, fs)
    try:
        R, cov = ts.resolution, ts.mask > 0
        assert tuple(ts.observed.shape) == (R, R, 3) and tuple(ts.observed_var.shape) == (R, R, 3) and tuple(ts.observed_count.shape) == (R, R)
        mean, var, weight, count = observe.observed_color(model, fs, ts.position[cov].contiguous(), ts.normal[cov].contiguous())
        assert same_bits(ts.observed[cov], mean) and same_bits(ts.observed_var[cov], var) and same_bits(ts.observed_count[cov], count.float())
        assert 0 < int((count > 0).sum()) and all(bool(torch.isfinite(v).all()) for v in ts.observed_planes().values())
        after = ts.export(str(tmp_path / "after"))
        assert sorted(os.path.basename(p) for p in after) == sorted(texture.FILES + ("observed.png",))
        assert os.path.getsize(str(tmp_path / "after" / "observed.png")) > 0
        for name in texture.FILES:
            if name != "maps.npz":                                   # a zip archive stores time stamps: compared array by array
                assert open(str(tmp_path / "before" / name), "rb").read() == open(str(tmp_path / "after" / name), "rb").read(), name
        a, b = np.load(str(tmp_path / "before" / "maps.npz")), np.load(str(tmp_path / "after" / "maps.npz"))
        assert sorted(b.files) == sorted(a.files + list(texture.OBSERVED_PLANES)) and all(a[k].tobytes() == b[k].tobytes() for k in a.files)
        assert same_bits(b["observed"], ts.observed)
    finally:
        ts.observed = ts.observed_var = ts.observed_count = None        # the fixture is shared
