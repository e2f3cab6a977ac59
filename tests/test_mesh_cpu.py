"""Isosurface extraction, the parts that need no GPU: the entry points' argument validation (before any launch), the generated
marching-tetrahedra table against the restatement (tests/mesh_restatement.py), the PLY writer / reader and the command line."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_restatement as mr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("rb_mesh_groups", "rb_mesh_table", "rb_mesh_count", "rb_mesh_emit_vertices", "rb_mesh_emit_faces", "rb_mesh_block_points",
         "rb_mesh_block_store", "rb_mesh_block_fill")
NULL, P = ctypes.c_void_p(0), ctypes.c_void_p(4096)      # P: a non-null pointer that a refused call never touches
ci, cl, cf = ctypes.c_int, ctypes.c_long, ctypes.c_float


@pytest.fixture(scope="module")
def L():
    from robir_amd import _lib
    return _lib.lib()


def test_entry_points_exist_and_are_declared(L):
    hdr = open(os.path.join(ROOT, "include", "robir_hip.h")).read()
    declared = set(re.findall(r"^(?:int|long|const char\*) (rb_[a-z0-9_]+)\s*\(", hdr, re.M))
    for name in ENTRY:
        assert hasattr(L, name) and name in declared, name
    assert L.rb_mesh_groups(ci(17), ci(17), ci(17)) == (17 ** 3 + 255) // 256
    assert L.rb_mesh_groups(ci(512), ci(512), ci(512)) == 512 ** 3 // 256


def _refused(L, rc, text):
    assert rc != 0 and text in L.rb_last_error(), (rc, L.rb_last_error())


def test_entry_points_refuse_bad_arguments_before_launching(L):
    n = (ci(4), ci(4), ci(4))
    G = (64 + 255) // 256
    for bad in ((ci(1), ci(4), ci(4)), (ci(4), ci(1), ci(4)), (ci(4), ci(4), ci(0))):
        assert L.rb_mesh_groups(*bad) == -1 and b">= 2" in L.rb_last_error()
        _refused(L, L.rb_mesh_count(P, *bad, cf(0), P, cl(2 * G), NULL), b">= 2")
        _refused(L, L.rb_mesh_emit_vertices(P, P, P, P, *bad, cf(0), P, cl(5), P, P, NULL), b">= 2")
        _refused(L, L.rb_mesh_emit_faces(P, *bad, cf(0), P, P, cl(5), cl(5), P, NULL), b">= 2")
        _refused(L, L.rb_mesh_block_points(P, cl(1), ci(8), P, P, P, *bad, P, cl(512), NULL), b">= 2")
        _refused(L, L.rb_mesh_block_store(P, cl(1), ci(8), P, cl(512), *bad, P, NULL), b">= 2")
        _refused(L, L.rb_mesh_block_fill(P, cl(1), ci(8), P, *bad, P, NULL), b">= 2")
    # null pointers, one at a time
    _refused(L, L.rb_mesh_table(NULL), b"null pointer")
    for args in ((NULL, P), (P, NULL)):
        _refused(L, L.rb_mesh_count(args[0], *n, cf(0), args[1], cl(2 * G), NULL), b"null pointer")
    for k in range(7):
        a = [P] * 7
        a[k] = NULL
        _refused(L, L.rb_mesh_emit_vertices(a[0], a[1], a[2], a[3], *n, cf(0), a[4], cl(5), a[5], a[6], NULL), b"null pointer")
    for k in range(4):
        a = [P] * 4
        a[k] = NULL
        _refused(L, L.rb_mesh_emit_faces(a[0], *n, cf(0), a[1], a[2], cl(5), cl(5), a[3], NULL), b"null pointer")
    for k in range(5):
        a = [P] * 5
        a[k] = NULL
        _refused(L, L.rb_mesh_block_points(a[0], cl(1), ci(8), a[1], a[2], a[3], *n, a[4], cl(512), NULL), b"null pointer")
    for k in range(3):
        a = [P] * 3
        a[k] = NULL
        _refused(L, L.rb_mesh_block_store(a[0], cl(1), ci(8), a[1], cl(512), *n, a[2], NULL), b"null pointer")
        _refused(L, L.rb_mesh_block_fill(a[0], cl(1), ci(8), a[1], *n, a[2], NULL), b"null pointer")
    # buffers too small for the totals passed in; totals that do not fit 32-bit indices
    _refused(L, L.rb_mesh_count(P, *n, cf(0), P, cl(2 * G - 1), NULL), b"too small")
    _refused(L, L.rb_mesh_block_points(P, cl(2), ci(8), P, P, P, *n, P, cl(1023), NULL), b"too small")
    _refused(L, L.rb_mesh_block_store(P, cl(2), ci(8), P, cl(1023), *n, P, NULL), b"too small")
    _refused(L, L.rb_mesh_emit_vertices(P, P, P, P, *n, cf(0), P, cl(2 ** 31), P, P, NULL), b"2^31")
    _refused(L, L.rb_mesh_emit_faces(P, *n, cf(0), P, P, cl(5), cl(2 ** 31), P, NULL), b"2^31")
    _refused(L, L.rb_mesh_emit_faces(P, *n, cf(0), P, P, cl(2 ** 31), cl(5), P, NULL), b"2^31")
    _refused(L, L.rb_mesh_emit_faces(P, *n, cf(0), P, P, cl(-1), cl(5), P, NULL), b"2^31")
    for B in (1, 17):
        _refused(L, L.rb_mesh_block_points(P, cl(1), ci(B), P, P, P, *n, P, cl(1 << 20), NULL), b"block size")
        _refused(L, L.rb_mesh_block_store(P, cl(1), ci(B), P, cl(1 << 20), *n, P, NULL), b"block size")
        _refused(L, L.rb_mesh_block_fill(P, cl(1), ci(B), P, *n, P, NULL), b"block size")
    _refused(L, L.rb_mesh_count(P, ci(2048), ci(2048), ci(2048), cf(0), P, cl(1 << 40), NULL), b"too large")


def test_zero_work_returns_without_a_launch(L):
    n = (ci(4), ci(4), ci(4))
    assert L.rb_mesh_emit_vertices(NULL, NULL, NULL, NULL, *n, cf(0), NULL, cl(0), NULL, NULL, NULL) == 0
    assert L.rb_mesh_emit_faces(NULL, *n, cf(0), NULL, NULL, cl(0), cl(0), NULL, NULL) == 0
    assert L.rb_mesh_block_points(NULL, cl(0), ci(8), NULL, NULL, NULL, *n, NULL, cl(0), NULL) == 0
    assert L.rb_mesh_block_store(NULL, cl(0), ci(8), NULL, cl(0), *n, NULL, NULL) == 0
    assert L.rb_mesh_block_fill(NULL, cl(0), ci(8), NULL, *n, NULL, NULL) == 0


def test_generated_table_equals_the_restatement():
    """All 6 x 16 (tetrahedron, inside mask) cases: triangle count, the tet edges of every triangle, in order (winding included)."""
    from robir_amd import ops
    got, want = ops.mesh_table(), mr.table()
    assert len(got) == 6 and all(len(r) == 16 for r in got)
    for t in range(6):
        for m in range(16):
            assert got[t][m] == want[t][m], (t, m, got[t][m], want[t][m])
    assert sum(want[t][m][0] for t in range(6) for m in range(16)) == 6 * (8 * 1 + 6 * 2)


def test_restatement_meshes_are_closed_and_oriented():
    """The restatement itself (it is the GPU tests' reference): closed, chi = 2 / 0, positive volume, second-order area."""
    errs = {}
    for n in (9, 17):
        xs, ys, zs = mr.lattice((n, n, n))
        v, f = mr.marching_tets(mr.field("sphere", xs, ys, zs), xs, ys, zs)
        once, paired, _ = mr.edge_report(f)
        area, vol = mr.area_volume(v, f)
        assert once and paired and mr.euler(len(v), f) == 2 and vol > 0
        assert np.unique(f).shape[0] == len(v)
        errs[n] = abs(area / (4 * np.pi * 0.49) - 1)
    assert errs[17] < errs[9] / 3
    xs, ys, zs = mr.lattice((12, 13, 9))
    v, f = mr.marching_tets(mr.field("torus", xs, ys, zs), xs, ys, zs, 0.05)
    once, paired, _ = mr.edge_report(f)
    assert once and paired and mr.euler(len(v), f) == 0 and mr.area_volume(v, f)[1] > 0


def _mesh(with_faces=True):
    rng = np.random.default_rng(3)
    V = 7
    v = rng.standard_normal((V, 3)).astype(np.float32)
    f = rng.integers(0, V, (5, 3)).astype(np.int32) if with_faces else np.zeros((0, 3), np.int32)
    nrm = rng.standard_normal((V, 3)).astype(np.float32)
    alb = rng.random((V, 3)).astype(np.float32)
    alb[0] = (0.0, 0.002, 1.5)                      # below the sRGB knee, and clipped
    return v, f, nrm, alb, rng.random((V, 1)).astype(np.float32), rng.random((V, 1)).astype(np.float32)


@pytest.mark.parametrize("normals,materials,with_faces", [(False, False, True), (True, False, True), (True, True, True),
                                                          (False, True, True), (True, True, False)])
def test_ply_round_trip(tmp_path, normals, materials, with_faces):
    from robir_amd import mesh
    v, f, nrm, alb, rough, metal = _mesh(with_faces)
    path = str(tmp_path / "m.ply")
    mesh.save_ply(path, v, f, nrm if normals else None, *((alb, rough, metal) if materials else (None, None, None)))
    header, vdt, fdt = mesh.ply_layout(len(v), len(f), normals, materials)
    assert vdt.itemsize == 12 + (12 if normals else 0) + (23 if materials else 0) and fdt.itemsize == 13
    assert os.path.getsize(path) == len(header) + len(v) * vdt.itemsize + len(f) * fdt.itemsize
    blob = open(path, "rb").read()
    assert blob.startswith(b"ply\nformat binary_little_endian 1.0\n") and blob[:len(header)] == header
    got = mesh.load_ply(path)
    assert np.array_equal(got["vertices"], v) and np.array_equal(got["faces"], f) and got["faces"].dtype == np.int32
    assert ("normals" in got) == normals and ("albedo" in got) == materials
    if normals:
        assert np.array_equal(got["normals"], nrm)
    if materials:
        assert np.array_equal(got["albedo"], alb) and np.array_equal(got["roughness"], rough) and np.array_equal(got["metallic"], metal)
        assert got["rgb"].dtype == np.uint8 and got["rgb"][0].tolist() == [0, round(12.92 * 0.002 * 255), 255]
        x = float(alb[1, 0])
        assert int(got["rgb"][1, 0]) == round((1.055 * x ** (1 / 2.4) - 0.055) * 255 if x > 0.0031308 else 12.92 * x * 255)
    with open(path, "ab") as fh:
        fh.write(b"\0")
    with pytest.raises(ValueError, match="header predicts"):
        mesh.load_ply(path)


def test_mesh_export_uses_the_writer(tmp_path):
    import torch
    from robir_amd import mesh
    v, f, nrm, *_ = _mesh()
    m = mesh.Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(nrm))
    assert m.albedo is None and m.roughness is None and m.metallic is None
    got = mesh.load_ply(m.export(str(tmp_path / "e.ply")))
    assert np.array_equal(got["vertices"], v) and np.array_equal(got["normals"], nrm) and "albedo" not in got


def test_command_line_help():
    r = subprocess.run([sys.executable, "-m", "robir_amd.mesh", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "--resolution" in r.stdout and "--materials" in r.stdout
