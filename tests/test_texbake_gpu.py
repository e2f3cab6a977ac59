"""Texture-space baking on the device (robir_amd/csrc/texbake/texbake.hip, robir_amd/texture.py) against the numpy fp32 restatement of its
conventions (tests/texbake_restatement.py): every kernel bit for bit, the sampler also against float64 under the parity rule, and the bake
of the synthetic scenes end to end."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import texbake_restatement as tr  # noqa: E402
from conftest import record_metric, rel_err  # noqa: E402
from test_texbake_cpu import dilate_case, sampler_case  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = tr.raster_cases()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's (face_id, bary) of a raster case -- computed once, shared, never modified."""
    uv, R = CASES[name]
    return tr.raster(uv, R)


def device_raster(uv, R, faces_vt=None):
    from robir_amd import texture
    fid, bary = texture.rasterize_uv(dev(uv), R, None if faces_vt is None else dev(faces_vt))
    assert fid.dtype == torch.int32 and tuple(fid.shape) == (R, R) and bary.dtype == torch.float32 and tuple(bary.shape) == (R, R, 2)
    return fid.cpu().numpy(), bary.cpu().numpy()


@pytest.mark.parametrize("name", sorted(CASES))
def test_raster_equals_restatement(name):
    uv, R = CASES[name]
    ref_id, ref_bary = reference(name)
    fid, bary = device_raster(uv, R)
    assert np.array_equal(fid, ref_id)
    assert same_bits(bary, ref_bary)


def test_binning_equals_restatement():
    """Counts, the emitted pairs in face order and their order after the stable sort, on the case whose tile size does not divide R."""
    from robir_amd import ops
    for name in ("tiles_r20", "overlap", "degenerate_first", "slivers"):
        uv, R = CASES[name]
        counts = ops.tb_bin_count(dev(uv), R)
        assert np.array_equal(counts.cpu().numpy(), tr.bin_counts(uv, R)), name
        incl = torch.cumsum(counts.to(torch.int64), 0)
        P = int(incl[-1])
        pt, pf = ops.tb_bin_emit(dev(uv), R, (incl - counts).contiguous(), P)
        ref_t, ref_f = tr.bin_pairs(uv, R)
        assert np.array_equal(pt.cpu().numpy(), ref_t) and np.array_equal(pf.cpu().numpy(), ref_f), name


def test_raster_properties():
    fid, _ = device_raster(*CASES["quad_diagonal"])
    assert (fid >= 0).all() and all(fid[15 - c, c] == 0 for c in range(16))          # covered once, the tie goes to face 0
    assert (device_raster(*CASES["no_faces"])[0] == -1).all()
    assert (device_raster(*CASES["slivers"])[0] == -1).all()
    fid, bary = device_raster(*CASES["degenerate_first"])
    alone, bary_alone = device_raster(*CASES["good_alone"])
    assert np.array_equal(fid, np.where(alone >= 0, 3, -1)) and same_bits(bary, bary_alone)
    uv, R = CASES["overlap"]
    n = tr.owners(uv, R)
    assert (device_raster(uv, R)[0][n == 3] == 0).all()


@pytest.mark.parametrize("variant", ["irrational", "half_texel"])
def test_fan_has_no_holes(variant):
    """Nine triangles around a hub, every spoke named in opposite order by its two faces, in the indexed (vt, faces_vt) form: every texel
    centre that float64 puts inside the union and more than 1e-2 texel from the outer boundary has a face; which one is the restatement's."""
    vt, faces, R = tr.fan(variant)
    for k in range(9):
        assert faces[k][2] == faces[(k + 1) % 9][1] and faces[k][0] == faces[(k + 1) % 9][0] == 0
    fid, bary = device_raster(vt, R, faces)
    inner = tr.fan_interior(vt, R, 1e-2)
    assert int(inner.sum()) > 1500 and (fid[inner] >= 0).all()
    ref_id, ref_bary = reference("fan_" + variant)
    assert np.array_equal(fid, ref_id) and same_bits(bary, ref_bary)


@pytest.mark.parametrize("F,R", tr.ATLAS_CASES)
def test_atlas_equals_restatement(F, R):
    from robir_amd import texture
    uv = texture.atlas_uv(F, R, DEV)
    ref = tr.atlas_uv(F, R)
    assert tuple(uv.shape) == (F, 3, 2) and same_bits(uv, ref)
    fid, bary = texture.rasterize_uv(uv, R)
    ref_id, ref_bary = tr.raster(ref, R)
    assert np.array_equal(fid.cpu().numpy(), ref_id) and same_bits(bary, ref_bary)
    with pytest.raises(ValueError, match=str(6 * tr.atlas_ncols(F))):
        texture.atlas_uv(F, 6 * tr.atlas_ncols(F) - 1, DEV)


@pytest.mark.parametrize("C", [1, 3, 5])
def test_interp_equals_restatement(C):
    from robir_amd import texture
    rng = np.random.default_rng(C)
    vt, fv, R = tr.fan("irrational")
    fid, bary = reference("fan_irrational")
    attr = rng.normal(size=(10, C)).astype(np.float32)
    img = texture.interpolate(dev(fid), dev(bary), dev(fv), dev(attr))
    ref = tr.interp(fid, bary, fv, attr)
    assert tuple(img.shape) == (R, R, C) and same_bits(img, ref)
    assert (img.cpu().numpy()[fid < 0] == 0).all() and np.signbit(img.cpu().numpy()[fid < 0]).sum() == 0
    idx = np.concatenate([np.flatnonzero(fid.reshape(-1) >= 0)[::3], np.flatnonzero(fid.reshape(-1) < 0)[:7]]).astype(np.int64)
    lst = texture.interpolate(dev(fid), dev(bary), dev(fv), dev(attr), dev(idx))
    assert tuple(lst.shape) == (idx.size, C) and same_bits(lst, ref.reshape(-1, C)[idx]) and same_bits(lst, tr.interp(fid, bary, fv, attr, idx))


def test_dilate_equals_restatement():
    from robir_amd import texture
    img, mask = dilate_case()
    ref, mref = tr.dilate(img, mask)
    out, mo = texture.dilate(dev(img), dev(mask), 1)
    assert same_bits(out, ref) and np.array_equal(mo.cpu().numpy(), mref) and mo.dtype == torch.uint8
    # rings = 3 equals three single rings
    a, am, ref, mref = dev(img), dev(mask), img, mask
    for _ in range(3):
        ref, mref = tr.dilate(ref, mref)
        a, am = texture.dilate(a, am, 1)
    out3, mo3 = texture.dilate(dev(img), dev(mask), 3)
    assert same_bits(out3, a) and torch.equal(mo3, am) and same_bits(out3, ref) and np.array_equal(mo3.cpu().numpy(), mref)
    # an empty mask: no NaN, nothing moves; a full mask: unchanged bytes
    zeros = np.zeros_like(img)
    e, em = texture.dilate(dev(zeros), dev(np.zeros_like(mask)), 2)
    assert same_bits(e, zeros) and int(em.sum()) == 0 and not bool(torch.isnan(e).any())
    f, fm = texture.dilate(dev(img), dev(np.ones_like(mask)), 2)
    assert same_bits(f, img) and int(fm.sum()) == mask.size
    g, _ = texture.dilate(dev(img[..., 0]), dev(mask), 1)               # a [H,W] plane
    assert tuple(g.shape) == img.shape[:2] and same_bits(g, tr.dilate(img[..., :1], mask)[0][..., 0])


def test_sampler_returns_texel_centres_bit_for_bit():
    """R = 64: u R is exact, so the centre of a covered texel fetches that texel with weight 1 and its neighbours with weight 0."""
    from robir_amd import texture
    pos, nrm, mask, _ = sampler_case()
    rows, cols = np.nonzero(mask)
    centres = np.stack([(cols + 0.5) / 64, 1.0 - (rows + 0.5) / 64], -1).astype(np.float32)
    s = texture.TexSampler(dev(pos), dev(nrm), dev(mask)).sample(0, dev(centres))
    assert same_bits(s["x"], pos[rows, cols] + np.float32(0)) and bool(s["object_mask"].all()) and s["object_mask"].dtype == torch.bool
    assert same_bits(s["uv"], centres)


def test_sampler_against_restatement_and_float64():
    """Random UVs, UVs within a texel of the border and over empty regions: the kernel equals the fp32 restatement bit for bit and holds
    e <= max(2 e_torch, 1e-5) against the float64 restatement, e_torch being the reference's lines on fp32 PyTorch-CPU grid_sample."""
    from robir_amd import texture
    pos, nrm, mask, uv = sampler_case()
    s = texture.TexSampler(dev(pos), dev(nrm), dev(mask), scale=0.5).sample(0, dev(uv))
    assert sorted(s) == ["normal", "object_mask", "tangent_u", "tangent_v", "uv", "x"]
    r32 = tr.sample(pos, nrm, mask, uv, scale=0.5)
    r64 = tr.sample(pos, nrm, mask, uv, scale=0.5, dt=np.float64)
    t32 = tr.sample_torch(pos, nrm, mask, uv, scale=0.5)
    for k in ("x", "normal", "tangent_u", "tangent_v"):
        e, e_torch = rel_err(s[k], r64[k]), rel_err(t32[k], r64[k])
        record_metric("texbake/sampler/" + k, e=e, e_torch=e_torch)
        print(k, e, e_torch)
        assert e <= max(2 * e_torch, 1e-5), (k, e, e_torch)
        assert same_bits(s[k], r32[k]), k
    sure = np.abs(r64["mask_value"] - 0.1) > 1e-5
    got = s["object_mask"].cpu().numpy()
    assert np.array_equal(got, r32["object_mask"]) and np.array_equal(got[sure], r64["object_mask"][sure])
    assert 0 < int(got.sum()) < uv.shape[0]
    # n uniform draws: the keys, the shapes, UVs in [0,1)
    d = texture.TexSampler(dev(pos), dev(nrm), dev(mask)).sample(33)
    assert tuple(d["uv"].shape) == (33, 2) and tuple(d["x"].shape) == (33, 3) and float(d["uv"].min()) >= 0 and float(d["uv"].max()) < 1


# ----------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _model(name):
    from robir_amd import renderer
    return renderer.build_synthetic_model(DEV, build_octrees=False, scene=name)


@pytest.fixture(scope="module", params=["sphere", "nonconvex"])
def baked(request):
    """(scene, model, mesh, TextureSet at R = 512 with project = 1) -- baked once, shared, never modified."""
    from robir_amd import mesh, texture
    model = _model(request.param)
    m = mesh.extract_mesh(model, resolution=33)
    return request.param, model, m, texture.bake(model, m, resolution=512)


def test_bake_atlas_and_planes(baked):
    from robir_amd import mesh
    name, model, m, ts = baked
    R, F = 512, m.faces.shape[0]
    fid = ts.face_id.cpu().numpy()
    # (a) every face owns a texel and the gutter is clean on the device's face_id
    assert int(np.bincount(fid[fid >= 0], minlength=F).min()) >= 1 and tr.gutter_is_clean(fid)
    assert np.array_equal(fid, tr.raster(tr.atlas_uv(F, R), R)[0])
    cov = ts.face_id >= 0
    assert torch.equal(ts.mask, cov.float()) and abs(ts.stats["covered_fraction"] - float(cov.float().mean())) < 1e-12
    for k, shape in (("albedo", (R, R, 3)), ("roughness", (R, R)), ("metallic", (R, R)), ("normal", (R, R, 3)), ("position", (R, R, 3)), ("mask", (R, R))):
        assert tuple(getattr(ts, k).shape) == shape and getattr(ts, k).dtype == torch.float32 and bool(torch.isfinite(getattr(ts, k)).all()), k
    # (b) the materials at the covered texels equal ONE direct call at the baked positions; if the bytes differ, the distance is held against
    # that between two direct calls that chunk the same points differently
    x = ts.position[cov].contiguous()
    src = mesh._Source(model)
    direct = mesh.bake_materials(src.materials_net, x)
    half = x.shape[0] // 2 + 1
    parts = [mesh.bake_materials(src.materials_net, x[:half].contiguous()), mesh.bake_materials(src.materials_net, x[half:].contiguous())]
    for k, plane in (("albedo", ts.albedo), ("roughness", ts.roughness), ("metallic", ts.metallic)):
        got, ref = plane[cov].reshape(x.shape[0], -1), direct[k]
        rechunk = rel_err(torch.cat([p[k] for p in parts]), ref)
        e = rel_err(got, ref)
        record_metric(f"texbake/bake/{name}/{k}", e=e, rechunk=rechunk, equal=float(torch.equal(got, ref)))
        print(name, k, "bake vs direct", e, "rechunked direct vs direct", rechunk)
        assert torch.equal(got, ref) or e <= rechunk, (k, e, rechunk)
    # (d) unit normals to fp32
    n = ts.normal[cov]
    assert float((n.norm(dim=-1) - 1).abs().max()) <= 4 * 2.0 ** -24 * 3


def test_bake_projection_reduces_the_sdf(baked):
    """(c) with project = 1 the largest |sdf| over the covered texels is strictly smaller than with project = 0."""
    from robir_amd import mesh, texture
    name, model, m, ts = baked
    src = mesh._Source(model)
    cov = ts.face_id >= 0
    flat = texture.bake(model, m, resolution=512, project=0)
    assert torch.equal(flat.face_id, ts.face_id)
    d0 = float(src.value(flat.position[cov].contiguous()).abs().max())
    d1 = float(src.value(ts.position[cov].contiguous()).abs().max())
    record_metric(f"texbake/project/{name}", max_abs_sdf_project0=d0, max_abs_sdf_project1=d1)
    print(name, "max |sdf| project 0 / 1:", d0, d1)
    assert d1 < d0
    # project = 0 keeps the interpolated points: the plane is the list form of the interpolation, scattered
    ref = texture.interpolate(ts.face_id, ts.bary, m.faces, m.vertices)
    assert torch.equal(flat.position[cov], ref[cov])


def test_bake_is_deterministic_and_takes_user_uvs(baked):
    """(e) two bakes give identical bytes in every plane; (g) the atlas' own UVs passed as a user UV set give the default bake."""
    from robir_amd import texture
    name, model, m, ts = baked
    again = texture.bake(model, m, resolution=512, uv=ts.uv.clone())
    assert torch.equal(again.face_id, ts.face_id) and same_bits(again.bary, ts.bary)
    for k, v in ts.planes().items():
        assert same_bits(again.planes()[k], v), k
    if name == "sphere":
        once_more = texture.bake(model, m, resolution=512)
        for k, v in ts.planes().items():
            assert same_bits(once_more.planes()[k], v), k


def test_export_and_read_back(baked, tmp_path):
    """(f) the six files (and maps.npz); maps.npz and mesh.obj reproduce the device tensors."""
    from robir_amd import texture
    name, model, m, ts = baked
    paths = ts.export(str(tmp_path / name))
    assert sorted(os.path.basename(p) for p in paths) == sorted(texture.FILES) and all(os.path.getsize(p) > 0 for p in paths)
    z = np.load(str(tmp_path / name / "maps.npz"))
    for k, v in ts.planes().items():
        assert same_bits(z[k], v), k
    assert np.array_equal(z["face_id"], ts.face_id.cpu().numpy()) and same_bits(z["uv"], ts.uv)
    o = texture.load_obj(str(tmp_path / name / "mesh.obj"))
    assert same_bits(o["vertices"], m.vertices) and same_bits(o["vn"], m.normals)
    assert np.array_equal(o["faces"], m.faces.cpu().numpy()) and same_bits(o["vt"][o["faces_vt"]], ts.uv)
    # the read-back mesh rasterises to the same ownership through the indexed form
    fid, _ = texture.rasterize_uv(dev(o["vt"]), 512, dev(o["faces_vt"]))
    assert torch.equal(fid, ts.face_id)
    s = ts.sampler().sample(64)
    assert bool(s["object_mask"].any()) and bool(torch.isfinite(s["x"]).all())
