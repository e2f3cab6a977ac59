"""Isosurface extraction on the device (robir_amd/csrc/mesh.hip, robir_amd/mesh.py) against the numpy restatement of its conventions
(tests/mesh_restatement.py): exact equality of canonicalised meshes, topological properties, determinism, the block culling and the
network scenes end to end."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_restatement as mr  # noqa: E402
from conftest import record_metric  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# an anisotropic box that is not centred: axis mix-ups and spacing mix-ups change the mesh
BOX = ((-1.0, 1.0), (-0.95, 1.05), (-1.1, 0.9))


def axes(shape, box=BOX):
    return tuple(np.linspace(box[i][0], box[i][1], shape[i], dtype=np.float32) for i in range(3))


@functools.lru_cache(maxsize=None)
def case(name, shape, iso, symmetric=False):
    """(axes, field, restatement vertices, restatement faces, canonical form) -- computed once, shared, never modified."""
    xs, ys, zs = axes(shape, ((-1.0, 1.0),) * 3 if symmetric else BOX)
    f = mr.field(name, xs, ys, zs)
    v, fc = mr.marching_tets(f, xs, ys, zs, iso)
    return (xs, ys, zs), f, v, fc, mr.canonical(v, fc)


def device_mesh(f, ax, iso):
    from robir_amd import mesh
    v, fc = mesh.marching_tets(torch.from_numpy(f).to(DEV), *(torch.from_numpy(a).to(DEV) for a in ax), threshold=iso)
    assert v.dtype == torch.float32 and fc.dtype == torch.int32 and v.shape[1:] == (3,) and fc.shape[1:] == (3,)
    return v.cpu().numpy(), fc.cpu().numpy()


def assert_same_mesh(v, fc, v_ref, fc_ref, canon_ref=None):
    assert v.shape == v_ref.shape and fc.shape == fc_ref.shape, (v.shape, v_ref.shape, fc.shape, fc_ref.shape)
    if fc.shape[0]:
        assert int(fc.min()) >= 0 and int(fc.max()) < v.shape[0]
    canon_ref = mr.canonical(v_ref, fc_ref) if canon_ref is None else canon_ref
    assert np.array_equal(mr.canonical(v, fc), canon_ref)        # triangles as coordinate triples, bit for bit


@pytest.mark.parametrize("iso", [0.0, 0.05])
@pytest.mark.parametrize("shape", [(17, 17, 17), (9, 12, 20), (20, 27, 33), (2, 2, 2)])
@pytest.mark.parametrize("name", ["sphere", "torus", "union", "sines"])
def test_kernel_equals_restatement(name, shape, iso):
    ax, f, v_ref, fc_ref, canon = case(name, shape, iso)
    v, fc = device_mesh(f, ax, iso)
    assert_same_mesh(v, fc, v_ref, fc_ref, canon)
    if shape != (2, 2, 2):
        assert fc.shape[0] > 0
    # the documented order: vertices by owner then slot, faces by cell, tetrahedron, triangle -- the restatement emits the same
    assert np.array_equal(v.view(np.uint32), v_ref.view(np.uint32)) and np.array_equal(fc, fc_ref)


@pytest.mark.parametrize("shape,iso", [((9, 9, 9), 0.0), ((17, 9, 13), 0.0), ((9, 9, 9), 0.25)])
def test_lattice_values_equal_to_the_threshold(shape, iso):
    """A Chebyshev box of half width 0.5 on lattices that contain +-0.5 (and, at 0.25, +-0.75): lattice values EQUAL to the threshold
    count as outside, mesh vertices then coincide with lattice vertices and triangles of zero area appear -- the combinatorics must
    still match."""
    ax, f, v_ref, fc_ref, canon = case("box", shape, iso, True)
    assert int((f == np.float32(iso)).sum()) > 0
    v, fc = device_mesh(f, ax, iso)
    assert_same_mesh(v, fc, v_ref, fc_ref, canon)
    area = np.linalg.norm(np.cross(v[fc[:, 1]] - v[fc[:, 0]], v[fc[:, 2]] - v[fc[:, 0]]), axis=1)
    assert int((area == 0).sum()) > 0
    once, paired, _ = mr.edge_report(fc)
    assert once and paired and mr.euler(len(v), fc) == 2


@pytest.fixture(scope="module")
def property_meshes():
    out = {}
    for name in ("sphere", "torus"):
        for n in (17, 33):
            ax, f, *_ = case(name, (n, n, n), 0.0, True)
            out[name, n] = device_mesh(f, ax, 0.0)
    return out


@pytest.mark.parametrize("name,chi", [("sphere", 2), ("torus", 0)])
def test_mesh_properties(property_meshes, name, chi):
    exact = 4 * math.pi * 0.7 ** 2 if name == "sphere" else 4 * math.pi ** 2 * 0.55 * 0.25
    err = {}
    for n in (17, 33):
        v, fc = property_meshes[name, n]
        once, paired, _ = mr.edge_report(fc)
        assert once and paired                                     # closed, consistently oriented
        assert mr.euler(len(v), fc) == chi
        assert np.unique(fc).shape[0] == len(v)                    # every vertex is referenced
        area, vol = mr.area_volume(v, fc)
        assert vol > 0                                             # outward
        err[n] = abs(area / exact - 1)
        record_metric(f"mesh/area_error/{name}/{n}", rel=err[n], V=len(v), F=len(fc))
    assert err[33] < err[17] / 3, err                              # second order gives a quarter


def test_open_surface_and_empty_field():
    ax, f, v_ref, fc_ref, canon = case("plane", (17, 17, 17), 0.0, True)
    v, fc = device_mesh(f, ax, 0.0)
    assert_same_mesh(v, fc, v_ref, fc_ref, canon)
    once, paired, _ = mr.edge_report(fc)
    assert once and not paired and mr.euler(len(v), fc) == 1       # a disc: open, chi = 1
    ax, f, *_ = case("outside", (9, 12, 20), 0.0)
    v, fc = device_mesh(f, ax, 0.0)
    assert v.shape == (0, 3) and fc.shape == (0, 3)
    v, fc = device_mesh(-f, ax, 0.0)                               # all inside
    assert v.shape == (0, 3) and fc.shape == (0, 3)


def test_non_finite_field_is_refused():
    from robir_amd import mesh
    ax, f, *_ = case("sphere", (9, 12, 20), 0.0)
    g = torch.from_numpy(f).to(DEV).clone()
    g[3, 4, 5] = float("nan")
    with pytest.raises(ValueError):
        mesh.marching_tets(g, *(torch.from_numpy(a).to(DEV) for a in ax))
    with pytest.raises(ValueError):
        mesh.marching_tets(g[:, :1], *(torch.from_numpy(a).to(DEV) for a in ax))


@pytest.mark.parametrize("where", ["first", "last", "all"])
def test_determinism_and_scan_bases(where):
    """Two calls give the same bytes.  On a (200,2,2) lattice (four workgroups of 256 lattice vertices) a field that changes side
    between ix = 0 and 1 has all its crossings owned by the first workgroup's vertices, one that changes between ix = 198 and 199 by
    the last workgroup's: a wrong scan base shows against the restatement."""
    from robir_amd import mesh
    if where == "all":
        ax, f, v_ref, fc_ref, _ = case("union", (20, 27, 33), 0.0)
    else:
        ax = axes((200, 2, 2))
        cut = 0.5 if where == "first" else 198.5
        f = np.ascontiguousarray(np.broadcast_to((cut - np.arange(200, dtype=np.float32))[:, None, None], (200, 2, 2)))
        v_ref, fc_ref = mr.marching_tets(f, *ax, 0.0)
        assert len(v_ref) == 4 + 2 + 2 + 1 and len(fc_ref) == 2 + 4 + 2       # one layer of cells: a disc
    ft, at = torch.from_numpy(f).to(DEV), [torch.from_numpy(a).to(DEV) for a in ax]
    v1, f1 = mesh.marching_tets(ft, *at)
    v2, f2 = mesh.marching_tets(ft.clone(), *at)
    assert torch.equal(v1, v2) and torch.equal(f1, f2)
    assert np.array_equal(v1.cpu().numpy().view(np.uint32), v_ref.view(np.uint32)) and np.array_equal(f1.cpu().numpy(), fc_ref)


# ------------------------------------------------------------------------------------------------- block culling
def _torch_field(name):
    n3 = lambda x, y, z: torch.sqrt(x * x + y * y + z * z)

    def fn(p):
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        if name == "sphere":
            return n3(x, y, z) - 0.7
        if name == "torus":
            q = torch.sqrt(x * x + y * y) - 0.55
            return torch.sqrt(q * q + z * z) - 0.25
        s1 = n3(x - 0.35, y, z) - 0.4
        s2 = n3(x + 0.4, y - 0.1, z) - 0.3
        q = torch.sqrt(y * y + z * z) - 0.6
        return torch.minimum(torch.minimum(s1, s2), torch.sqrt(q * q + x * x) - 0.12)
    return fn


@pytest.mark.parametrize("shape", [(33, 33, 33), (20, 27, 33)])
@pytest.mark.parametrize("name", ["sphere", "torus", "union"])
def test_culled_fill_gives_the_dense_mesh(name, shape):
    from robir_amd import mesh
    at = [torch.from_numpy(a).to(DEV) for a in axes(shape)]
    fn = _torch_field(name)
    dense, one = mesh.fill_lattice(fn, *at, lip=None)
    assert one == 1.0
    pts = torch.stack(torch.meshgrid(*at, indexing="ij"), -1).reshape(-1, 3)
    assert torch.equal(dense.reshape(-1), fn(pts))                 # block points / store put every value where it belongs
    culled, frac = mesh.fill_lattice(fn, *at, lip=1.0)
    record_metric(f"mesh/cull/{name}/{shape[0]}x{shape[1]}x{shape[2]}", evaluated_fraction=frac)
    assert 0.0 < frac < 1.0                                         # both branches ran
    assert not torch.equal(dense, culled)
    vd, fd = mesh.marching_tets(dense, *at)
    vc, fc = mesh.marching_tets(culled, *at)
    assert vd.shape[0] > 0 and torch.equal(vd, vc) and torch.equal(fd, fc)


# ------------------------------------------------------------------------------------------------- network scenes
@functools.lru_cache(maxsize=None)
def synthetic_model(name):
    from robir_amd import renderer
    return renderer.build_synthetic_model(DEV, build_octrees=False, scene=name)


@pytest.fixture(scope="module", params=[("sphere", 33), ("nonconvex", 49)], ids=["sphere33", "nonconvex49"])
def scene(request):
    from robir_amd import mesh
    name, res = request.param
    model = synthetic_model(name)
    src = mesh._Source(model)
    at = [torch.linspace(-1.0, 1.0, res, dtype=torch.float32, device=DEV) for _ in range(3)]
    dense, _ = mesh.fill_lattice(src.value, *at, lip=None)
    return name, res, model, src, at, dense


def test_network_culling(scene):
    """lip = 1.5 x the largest |grad sdf| measured on the dense lattice (a lattice maximum underestimates the supremum)."""
    from robir_amd import mesh
    name, res, model, src, at, dense = scene
    pts = torch.stack(torch.meshgrid(*at, indexing="ij"), -1).reshape(-1, 3).contiguous()
    gmax = float(src.value_grad(pts)[1].norm(dim=-1).max())
    culled, frac = mesh.fill_lattice(src.value, *at, lip=1.5 * gmax)
    record_metric(f"mesh/cull/network/{name}/{res}", evaluated_fraction=frac, max_grad_norm=gmax, lip=1.5 * gmax)
    print(f"{name} {res}^3: max |grad sdf| on the lattice {gmax:.4f}, evaluated fraction {frac:.4f}")
    vd, fd = mesh.marching_tets(dense, *at)
    vc, fc = mesh.marching_tets(culled, *at)
    assert vd.shape[0] > 0 and torch.equal(vd, vc) and torch.equal(fd, fc)


def test_network_scene_end_to_end(scene, tmp_path):
    from robir_amd import mesh
    name, res, model, src, at, dense = scene
    m = mesh.extract_mesh(model, resolution=res, materials=True)
    V, F = m.vertices.shape[0], m.faces.shape[0]
    assert V > 0 and F > 0 and m.normals.shape == (V, 3)
    v, fc = m.vertices.cpu().numpy(), m.faces.cpu().numpy()
    # the restatement on the same device field: same mesh (the default box of an IDRNetwork is the bounding sphere's cube,
    # [-1,1]^3 here, and refine = 0 leaves the vertices where the kernel put them)
    ax = [a.cpu().numpy() for a in at]
    v_ref, fc_ref = mr.marching_tets(dense.cpu().numpy(), *ax, 0.0)
    assert_same_mesh(v, fc, v_ref, fc_ref)
    once, paired, _ = mr.edge_report(fc)
    once_r, paired_r, _ = mr.edge_report(fc_ref)
    assert (once, paired, mr.euler(V, fc)) == (once_r, paired_r, mr.euler(len(v_ref), fc_ref))
    if name == "sphere":
        assert once and paired and mr.euler(V, fc) == 2
    # normals: outward, along the faces' own
    n = m.normals.cpu().numpy().astype(np.float64)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-5)
    fn = np.cross(v[fc[:, 1]].astype(np.float64) - v[fc[:, 0]], v[fc[:, 2]].astype(np.float64) - v[fc[:, 0]])
    agree = float((fn * n[fc].mean(1)).sum() / np.linalg.norm(fn, axis=1).sum())
    record_metric(f"mesh/normal_agreement/{name}", area_weighted_cosine=agree)
    assert agree > 0
    # one Newton step does not move the vertices away from the surface
    r1 = mesh.extract_mesh(model, resolution=res, refine=1)
    assert torch.equal(r1.faces, m.faces) and r1.albedo is None and r1.roughness is None and r1.metallic is None
    d0, d1 = float(src.value(m.vertices).abs().mean()), float(src.value(r1.vertices).abs().mean())
    record_metric(f"mesh/refine/{name}", mean_abs_sdf_refine0=d0, mean_abs_sdf_refine1=d1)
    print(f"{name}: mean |sdf(vertex)| {d0:.3e} -> {d1:.3e} after one Newton step")
    assert d1 <= d0
    # materials = the material network called on the vertices directly
    assert m.albedo.shape == (V, 3) and m.roughness.shape == (V, 1) and m.metallic.shape == (V, 1)
    assert bool(torch.isfinite(m.albedo).all()) and bool(torch.isfinite(m.roughness).all())
    direct = model.envmap_material_network(m.vertices, train_spec=True)
    assert torch.equal(direct["sg_diffuse_albedo"].reshape(V, 3), m.albedo)
    assert torch.equal(direct["sg_roughness"].reshape(V, 1), m.roughness)
    assert torch.equal(direct["sg_metallic"].reshape(V, 1), m.metallic)
    assert mesh.extract_mesh(model, resolution=res, normals=False).normals is None
    # the exported file loads back equal
    got = mesh.load_ply(m.export(str(tmp_path / "scene.ply")))
    assert np.array_equal(got["vertices"], v) and np.array_equal(got["faces"], fc)
    assert np.array_equal(got["normals"], m.normals.cpu().numpy()) and np.array_equal(got["albedo"], m.albedo.cpu().numpy())
    assert np.array_equal(got["roughness"], m.roughness.cpu().numpy()) and np.array_equal(got["metallic"], m.metallic.cpu().numpy())


def test_callables_and_sdf_network():
    """extract_geometry with the reference's parameter order: a plain callable and the NeuS-unit SDFNetwork (stage-2 sdf(x) =
    net(2x)/2: the NeuS-unit surface is the stage-2 surface scaled by two)."""
    from robir_amd import mesh
    model, res = synthetic_model("sphere"), 33
    lo, hi = torch.tensor([-1.0, -1.0, -1.0], device=DEV), torch.tensor([1.0, 1.0, 1.0], device=DEV)
    v, fc = mesh.extract_geometry(lo, hi, 17, 0.0, lambda p: p.norm(dim=-1) - 0.7)
    ax, f, v_ref, fc_ref, _ = case("sphere", (17, 17, 17), 0.0, True)
    assert isinstance(v, np.ndarray) and v.shape == v_ref.shape and fc.shape == fc_ref.shape and mr.euler(len(v), fc) == 2
    net = model.implicit_network.neus_model.sdf_network
    big = mesh.extract_mesh(net, bbox=2.0, resolution=res, normals=False)
    small = mesh.extract_mesh(model, resolution=res, normals=False)
    assert torch.equal(big.faces, small.faces)
    assert float((big.vertices - 2 * small.vertices).abs().max()) < 1e-4
