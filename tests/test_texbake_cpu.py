"""The texture-baking library and robir_amd/texture.py as far as they go without a GPU: loading, the export list, argument errors before
any launch, the atlas' properties on the restatement (tests/texbake_restatement.py), the host build of csrc/texbake/texbake_math.h against
the restatement bit for bit (tools/check_texbake_host.py), the PNG and OBJ writers, and the restatements of the dilation and the sampler
against independently written float64 forms."""
import ctypes
import importlib.util
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

import texbake_restatement as tr
from conftest import ROOT, rel_err

c_long, c_int, c_float = ctypes.c_long, ctypes.c_int, ctypes.c_float
NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(4096)                    # never read: every call below is refused, or has nothing to do, before a launch
OTHER_HEADERS = ("robir_hip.h", "robir_hip_legacy.h", "robir_hip_train.h", "robir_hip_vistrain.h", "robir_hip_illumtrain.h",
                 "robir_hip_cesrtrain.h", "robir_hip_lightfit.h")


def _header_symbols(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return sorted(set(re.findall(r"^(?:int|long|const char\*) (rb_[a-z0-9_]+)\s*\(", hdr, re.M)))


def _tb_lib():
    from robir_amd import _lib
    if not os.path.exists(_lib.TEXBAKE_PATH):
        _lib.build(legacy=False)
    return _lib.texbake()


def test_texbake_library_exports_its_header():
    """librobir_hip_texbake.so loads without a GPU and exports exactly what include/robir_hip_texbake.h declares, every name rb_tb_*; no rb_
    name is shared with the other seven headers, and none of them names this one."""
    from robir_amd import _lib
    L = _tb_lib()
    assert L.rb_tb_abi_version() == _lib.TEXBAKE_ABI_VERSION == 1
    syms = _header_symbols("robir_hip_texbake.h")
    assert syms == ["rb_tb_abi_version", "rb_tb_atlas_cell", "rb_tb_atlas_uv", "rb_tb_bin_count", "rb_tb_bin_emit", "rb_tb_dilate",
                    "rb_tb_interp", "rb_tb_last_error", "rb_tb_raster", "rb_tb_sample"]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.TEXBAKE_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[-1] for l in out.splitlines() if " T rb_" in l) == syms
    others = set()
    for h in OTHER_HEADERS:
        text = open(os.path.join(ROOT, "include", h)).read()
        others |= set(_header_symbols(h))
        assert "rb_tb_" not in text and "texbake" not in text
    assert not set(syms) & others
    assert "#define RB_TB_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "robir_hip_texbake.h")).read()


def test_atlas_cell_query_and_refusal():
    L = _tb_lib()
    q = lambda F, R: L.rb_tb_atlas_cell(c_long(F), c_int(R))
    for F, R in tr.ATLAS_CASES + ((5000, 512), (277000, 4096), (554000, 4096)):
        assert q(F, R) == tr.atlas_cell(F, R) == R // tr.atlas_ncols(F), (F, R)
    assert [tr.atlas_ncols(F) for F in (1, 2, 3, 7, 8, 9, 200, 5000)] == [1, 1, 2, 2, 2, 3, 10, 50]
    # below six texels per cell: refused, naming the smallest resolution that works (6 ncols)
    assert q(200, 59) == -1 and b"60" in L.rb_tb_last_error()
    assert q(200, 60) == 6
    with pytest.raises(ValueError, match="60"):
        tr.atlas_uv(200, 59)
    from robir_amd import ops
    with pytest.raises(ValueError, match="smallest resolution at which every face owns a texel is 60"):
        ops.tb_atlas_cell(200, 59)
    assert q(0, 64) == -1 and b"at least one face" in L.rb_tb_last_error()
    assert q(1 << 31, 64) == -1 and b"32 bits" in L.rb_tb_last_error()
    assert q(4, 16385) == -1 and b"16384" in L.rb_tb_last_error()
    assert q(4, 0) == -1 and b"empty texture" in L.rb_tb_last_error()


def test_texbake_argument_errors_before_any_launch():
    L = _tb_lib()
    err = L.rb_tb_last_error
    big = c_long(1 << 31)
    assert L.rb_tb_atlas_uv(c_long(8), c_int(64), NULL, NULL) != 0 and b"null pointer" in err()
    assert L.rb_tb_atlas_uv(c_long(200), c_int(59), FAKE, NULL) != 0 and b"60" in err()
    assert L.rb_tb_bin_count(FAKE, c_long(4), c_int(16385), FAKE, NULL) != 0 and b"16384" in err()
    assert L.rb_tb_bin_count(NULL, c_long(4), c_int(64), FAKE, NULL) != 0 and b"null pointer" in err()
    assert L.rb_tb_bin_count(NULL, c_long(0), c_int(64), NULL, NULL) == 0
    assert L.rb_tb_bin_emit(FAKE, c_long(4), c_int(64), FAKE, big, FAKE, FAKE, NULL) != 0 and b"2^31" in err()
    assert L.rb_tb_bin_emit(FAKE, c_long(4), c_int(64), FAKE, c_long(-1), FAKE, FAKE, NULL) != 0 and b"negative" in err()
    assert L.rb_tb_bin_emit(FAKE, c_long(4), c_int(64), NULL, c_long(9), FAKE, FAKE, NULL) != 0 and b"null pointer" in err()
    assert L.rb_tb_bin_emit(NULL, c_long(4), c_int(64), NULL, c_long(0), NULL, NULL, NULL) == 0
    assert L.rb_tb_raster(FAKE, c_long(4), c_int(16385), FAKE, FAKE, c_long(4), FAKE, FAKE, NULL) != 0 and b"16384" in err()
    assert L.rb_tb_raster(FAKE, c_long(4), c_int(64), FAKE, FAKE, big, FAKE, FAKE, NULL) != 0 and b"2^31" in err()
    assert L.rb_tb_raster(FAKE, c_long(4), c_int(64), FAKE, FAKE, c_long(4), NULL, FAKE, NULL) != 0 and b"null pointer" in err()
    assert L.rb_tb_raster(FAKE, c_long(4), c_int(64), NULL, FAKE, c_long(4), FAKE, FAKE, NULL) != 0 and b"null pointer" in err()

    def interp(fid=FAKE, bary=FAKE, T=64, index=NULL, n=64, faces=FAKE, F=4, attr=FAKE, V=6, C=3, out=FAKE):
        return L.rb_tb_interp(fid, bary, c_long(T), index, c_long(n), faces, c_long(F), attr, c_long(V), c_int(C), out, NULL)
    assert interp(C=0) != 0 and b"C = 0" in err()
    assert interp(C=65) != 0 and b"C = 65" in err()
    assert interp(n=32) != 0 and b"image form" in err()
    assert interp(n=-1) != 0 and b"negative" in err()
    assert interp(index=FAKE, n=65) != 0 and b"65 outputs" in err()
    assert interp(out=NULL) != 0 and b"null pointer" in err()
    assert interp(faces=NULL) != 0 and b"null pointer" in err()
    assert interp(index=FAKE, n=0, fid=NULL, out=NULL) == 0

    def dil(img=FAKE, mask=FAKE, H=8, W=8, C=3, dst=ctypes.c_void_p(8192), mo=ctypes.c_void_p(12288)):
        return L.rb_tb_dilate(img, mask, c_int(H), c_int(W), c_int(C), dst, mo, NULL)
    assert dil(H=0) != 0 and b"empty image" in err()
    assert dil(W=16385) != 0 and b"16384" in err()
    assert dil(C=0) != 0 and b"C = 0" in err()
    assert dil(mask=NULL) != 0 and b"null pointer" in err()
    assert dil(dst=FAKE) != 0 and b"alias" in err()
    assert dil(mo=FAKE) != 0 and b"alias" in err()

    def samp(pos=FAKE, R=64, uv=FAKE, n=8, x=FAKE):
        return L.rb_tb_sample(pos, FAKE, FAKE, c_int(R), uv, c_long(n), c_float(1.0), x, FAKE, FAKE, FAKE, FAKE, NULL)
    assert samp(R=0) != 0 and b"empty texture" in err()
    assert samp(n=-1) != 0 and b"negative" in err()
    assert samp(pos=NULL) != 0 and b"null pointer" in err()
    assert samp(x=NULL) != 0 and b"null pointer" in err()
    assert samp(n=0, pos=NULL, uv=NULL, x=NULL) == 0


def test_missing_texbake_library_has_its_own_message(monkeypatch, tmp_path):
    from robir_amd import _lib
    monkeypatch.setattr(_lib, "_texbake", None)
    monkeypatch.setattr(_lib, "TEXBAKE_PATH", str(tmp_path / "nope_texbake.so"))
    with pytest.raises(_lib.RobirHipError, match="TEXTURE-BAKING library") as e:
        _lib.call_texbake("rb_tb_raster")
    msg = str(e.value)
    assert "make -C robir_amd/csrc texbake" in msg and "librobir_hip_texbake.so" in msg and "LEGACY" not in msg


@pytest.mark.parametrize("F,R", tr.ATLAS_CASES)
def test_atlas_properties_on_the_restatement(F, R):
    """UVs in [0,1]; every face owns at least one texel; no texel centre is covered by two faces; no uncovered texel is 8-adjacent to covered
    texels of two faces (one dilation ring never mixes faces)."""
    uv = tr.atlas_uv(F, R)
    assert uv.dtype == np.float32 and uv.shape == (F, 3, 2) and float(uv.min()) >= 0.0 and float(uv.max()) <= 1.0
    face_id, _ = tr.raster(uv, R)
    owned = np.bincount(face_id[face_id >= 0], minlength=F)
    assert owned.shape == (F,) and int(owned.min()) >= 1, owned
    assert int(tr.owners(uv, R).max()) == 1
    assert tr.gutter_is_clean(face_id)
    S = tr.atlas_cell(F, R)
    # the closed form: a lower triangle owns the centres with c, r >= 1 and c + r <= S - 4 of its cell
    assert int(owned[0]) == sum(1 for c in range(1, S) for r in range(1, S) if c + r <= S - 4)
    if F > 1:
        assert int(owned[1]) == int(owned[0])                       # the upper triangle is its point reflection


def test_gutter_check_sees_a_dirty_gutter():
    """The property test can fail: two faces one empty texel apart."""
    fid = np.full((5, 5), -1)
    fid[1, 1], fid[1, 3] = 0, 1
    assert not tr.gutter_is_clean(fid)
    fid[1, 3] = 0
    assert tr.gutter_is_clean(fid)
    # a hypotenuse offset of 2.0: the two halves of a cell come within one empty diagonal of each other
    S = 12
    lower = np.array([[1, 1], [S - 3, 1], [1, S - 3]], dtype=np.float64)
    upper = np.array([[S - 1, S - 1], [3, S - 1], [S - 1, 3]], dtype=np.float64)
    bad, _ = tr.raster(tr._uv_of_texels(np.stack([lower, upper]), S), S)
    assert not tr.gutter_is_clean(bad)


def test_raster_cases_say_what_they_claim():
    cases = tr.raster_cases()
    fid, _ = tr.raster(*cases["quad_diagonal"])
    assert (fid >= 0).all() and all(fid[15 - c, c] == 0 for c in range(16)) and int((fid == 1).sum()) == 120
    assert int(tr.owners(*cases["quad_diagonal"])[np.arange(15, -1, -1), np.arange(16)].min()) == 2       # the diagonal is claimed by both
    uv, R = cases["tiles_r20"]
    a = tr.Face(uv[0], R)
    assert float(a.x.max()) == 8.0 and a.c1 == 7 and a.r1 == 7          # the box ends exactly on the tile boundary: tile column 1 is not touched
    assert list(tr.bin_counts(uv, R)) == [1, 9, 2] and tr.Face(uv[2], R).c0 == 0
    fid, _ = tr.raster(uv, R)
    assert set(np.unique(fid)) == {-1, 0, 1, 2}
    fid, bary = tr.raster(*cases["degenerate_first"])
    alone, bary_alone = tr.raster(*cases["good_alone"])
    assert list(tr.bin_counts(*cases["degenerate_first"])[:3]) == [0, 0, 0]
    assert np.array_equal(fid, np.where(alone >= 0, 3, -1)) and np.array_equal(bary.view(np.uint32), bary_alone.view(np.uint32))
    assert int((tr.raster(*cases["slivers"])[0] >= 0).sum()) == 0 and list(tr.bin_counts(*cases["slivers"])) == [0, 4]
    uv, R = cases["overlap"]
    fid, _ = tr.raster(uv, R)
    n = tr.owners(uv, R)
    assert int(n.max()) == 3 and (fid[n == 3] == 0).all() and int((fid == 2).sum()) > 0
    crowd = tr.bin_counts(*cases["crowded_tile"])
    assert int(crowd.max()) == 1 and int(crowd.sum()) > 3 * 64          # one tile, more faces than it has threads
    assert len(np.unique(tr.raster(*cases["crowded_tile"])[0])) > 20
    assert (tr.raster(*cases["no_faces"])[0] == -1).all()
    for variant in ("irrational", "half_texel"):
        vt, faces, R = tr.fan(variant)
        fid, _ = tr.raster(vt[faces], R)
        inner = tr.fan_interior(vt, R)
        assert int(inner.sum()) > 1500 and (fid[inner] >= 0).all(), variant
        assert len(np.unique(fid[inner])) == 9
    vt, faces, R = tr.fan("half_texel")
    assert tr.raster(vt[faces], R)[0][32, 32] == 0                  # the hub is a texel centre: all nine claim it, the lowest wins
    assert int(tr.owners(vt[faces], R)[32, 32]) == 9


def _host_tool():
    spec = importlib.util.spec_from_file_location("check_texbake_host", os.path.join(ROOT, "tools", "check_texbake_host.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_host_build_of_the_math_equals_the_restatement():
    """tools/check_texbake_host.py: texbake_math.h compiled with the host C++ compiler as a stand-alone program (tools/texbake_host.cpp
    supplies main and the loops) against the numpy restatement, bit for bit: tile counts, face_id and barycentrics of every raster case,
    the atlas UVs and their ownership map."""
    tool = _host_tool()
    if tool.compiler() is None:
        pytest.skip("no host C++ compiler")
    rows = tool.check(tool.build())
    assert len(rows) == 3 * len(tr.raster_cases()) + 2 * len(tr.ATLAS_CASES) + 1
    assert [what for what, ok in rows if not ok] == []


def _decode_png(blob):
    """A test-side decoder of what save_png writes: 8-bit grey or RGB, non-interlaced, every scanline of filter type 0."""
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(blob):
        n, tag = struct.unpack(">I4s", blob[pos:pos + 8])
        data = blob[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", blob[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF
        chunks.append((tag, data))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and colour in (0, 2)
    ch = 3 if colour == 2 else 1
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(H, 1 + W * ch)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(H, W, ch) if ch == 3 else raw[:, 1:].reshape(H, W)


def test_png_round_trip(tmp_path):
    from robir_amd import texture
    rng = np.random.default_rng(3)
    for shape in ((13, 11, 3), (7, 9), (5, 4, 1), (1, 1)):
        img = rng.uniform(-0.2, 1.2, shape).astype(np.float32)
        want = np.round(np.clip(img.astype(np.float64), 0, 1) * 255).astype(np.uint8)
        want = want[..., 0] if want.ndim == 3 and want.shape[2] == 1 else want
        path = str(tmp_path / "a.png")
        texture.save_png(path, img)
        assert np.array_equal(_decode_png(open(path, "rb").read()), want)
        try:
            from PIL import Image
        except ImportError:
            continue
        assert np.array_equal(np.asarray(Image.open(path)), want)
    u8 = rng.integers(0, 256, (6, 5, 3), dtype=np.uint8)
    assert np.array_equal(_decode_png(texture.png_bytes(u8)), u8)
    with pytest.raises(ValueError, match="save_png"):
        texture.png_bytes(np.zeros((4, 4, 2)))


def test_obj_round_trip_and_mtl(tmp_path):
    """export, then load_obj: vertices, normals, UVs and index triples come back exactly; the MTL names the four maps."""
    from robir_amd import mesh, texture
    rng = np.random.default_rng(5)
    V, F, R = 7, 6, 32
    verts = torch.from_numpy(rng.normal(size=(V, 3)).astype(np.float32))
    nrm = torch.from_numpy(rng.normal(size=(V, 3)).astype(np.float32))
    faces = torch.from_numpy(rng.integers(0, V, (F, 3)).astype(np.int32))
    uv = torch.from_numpy(tr.atlas_uv(F, R))
    fid, bary = tr.raster(uv.numpy(), R)
    planes = {k: torch.from_numpy(rng.uniform(0, 1, (R, R, 3) if k in ("albedo", "normal", "position") else (R, R)).astype(np.float32))
              for k in ("albedo", "roughness", "metallic", "normal", "position", "mask")}
    ts = texture.TextureSet(mesh.Mesh(verts, faces, nrm), uv, torch.from_numpy(fid), torch.from_numpy(bary), **planes)
    paths = ts.export(str(tmp_path / "out"))
    assert sorted(os.path.basename(p) for p in paths) == sorted(texture.FILES) and all(os.path.getsize(p) > 0 for p in paths)
    o = texture.load_obj(str(tmp_path / "out" / "mesh.obj"))
    assert np.array_equal(o["vertices"].view(np.uint32), verts.numpy().view(np.uint32))
    assert np.array_equal(o["vn"].view(np.uint32), nrm.numpy().view(np.uint32))
    assert np.array_equal(o["faces"], faces.numpy()) and np.array_equal(o["faces_vn"], faces.numpy())
    assert np.array_equal(o["vt"][o["faces_vt"]].view(np.uint32), uv.numpy().view(np.uint32))
    mtl = open(str(tmp_path / "out" / "mesh.mtl")).read()
    assert "map_Kd albedo.png" in mtl and "map_Pr roughness.png" in mtl and "map_Pm metallic.png" in mtl
    assert any(ln.startswith("#") and "normal.png" in ln for ln in mtl.splitlines())
    assert "mtllib mesh.mtl" in open(str(tmp_path / "out" / "mesh.obj")).read()
    z = np.load(str(tmp_path / "out" / "maps.npz"))
    for k, v in planes.items():
        assert np.array_equal(z[k].view(np.uint32), v.numpy().view(np.uint32)), k
    assert np.array_equal(z["face_id"], fid)
    rgb = _decode_png(open(str(tmp_path / "out" / "albedo.png"), "rb").read())
    assert np.array_equal(rgb, np.round(mesh._srgb(planes["albedo"].numpy().astype(np.float64)) * 255).astype(np.uint8))
    nm = _decode_png(open(str(tmp_path / "out" / "normal.png"), "rb").read())
    assert np.array_equal(nm, np.round(np.clip(planes["normal"].numpy().astype(np.float64) * 0.5 + 0.5, 0, 1) * 255).astype(np.uint8))
    # a user's file: shared vt indices, negative indices, no normals
    p = tmp_path / "user.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nvt 1 1\nf 1/1 2/2 3/3\nf -3/-3 -1/-1 -2/-2\n")
    o = texture.load_obj(str(p))
    assert o["faces"].tolist() == [[0, 1, 2], [1, 3, 2]] and o["faces_vt"].tolist() == [[0, 1, 2], [1, 3, 2]] and "vn" not in o
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nf 1 2 3 4\n")
    with pytest.raises(ValueError, match="only triangles"):
        texture.load_obj(str(p))


def dilate_case(H=13, W=11, C=3, seed=11):
    """A non-square random mask with isolated texels and texels on all four borders."""
    rng = np.random.default_rng(seed)
    mask = (rng.uniform(size=(H, W)) < 0.2).astype(np.uint8)
    mask[0, 3] = mask[H - 1, 5] = mask[4, 0] = mask[7, W - 1] = mask[0, 0] = 1
    mask[5:8, 4:7] = 0
    mask[6, 5] = 1                                                   # isolated
    return rng.normal(size=(H, W, C)).astype(np.float32), mask


def test_dilate_restatement_against_float64_form():
    img, mask = dilate_case()
    out, mo = tr.dilate(img, mask)
    ref, mref = tr.dilate64(img, mask)
    assert np.array_equal(mo != 0, mref) and int(mo.sum()) > int(mask.sum())
    assert np.array_equal(out[mask != 0].view(np.uint32), img[mask != 0].view(np.uint32))              # covered texels are copied
    assert np.array_equal(out[mo == 0].view(np.uint32), img[mo == 0].view(np.uint32))                  # and so are the far ones
    assert rel_err(out, ref) <= 4 * 2.0 ** -24 * 8                  # at most eight fp32 additions and one division per texel
    e, m0 = tr.dilate(img, np.zeros_like(mask))
    assert np.array_equal(e.view(np.uint32), img.view(np.uint32)) and int(m0.sum()) == 0
    f, m1 = tr.dilate(img, np.ones_like(mask))
    assert np.array_equal(f.view(np.uint32), img.view(np.uint32)) and int(m1.sum()) == mask.size


def sampler_case(R=64, n=400, seed=13):
    """Random position / normal maps under an atlas-like mask (zeros where empty), and UVs: random ones, ones within a texel of every border
    (some outside [0,1]) and the centres of covered texels."""
    rng = np.random.default_rng(seed)
    mask = (tr.raster(tr.atlas_uv(30, R), R)[0] >= 0).astype(np.float32)
    pos = rng.normal(size=(R, R, 3)).astype(np.float32) * mask[..., None]
    nrm = rng.normal(size=(R, R, 3)).astype(np.float32) * mask[..., None]
    uv = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    edge = rng.uniform(-1.0 / R, 1.0 / R, (n // 4, 2)).astype(np.float32)
    edge[::2] += 1.0
    edge[:, 1] = np.where(rng.uniform(size=n // 4) < 0.5, rng.uniform(0, 1, n // 4), edge[:, 1]).astype(np.float32)
    return pos, nrm, mask, np.concatenate([uv, edge, edge[:, ::-1]]).astype(np.float32)


def test_sampler_restatement_against_float64_grid_sample():
    """The fp32 restatement of rb_tb_sample against the reference's own lines on float64 PyTorch grid_sample, under the project's rule
    e <= max(2 e_torch, 1e-5) with e_torch the distance of the same lines in float32 (1 - v and u + 0.001 round before they are scaled by R:
    both fp32 forms carry that error)."""
    pos, nrm, mask, uv = sampler_case()
    got = tr.sample(pos, nrm, mask, uv, scale=0.5)
    ref = tr.sample_torch(pos, nrm, mask, uv, scale=0.5, dtype=torch.float64)
    t32 = tr.sample_torch(pos, nrm, mask, uv, scale=0.5, dtype=torch.float32)
    f64 = tr.sample(pos, nrm, mask, uv, scale=0.5, dt=np.float64)
    for k in ("x", "normal", "tangent_u", "tangent_v", "mask_value"):
        assert got[k].dtype == np.float32
        assert rel_err(f64[k], ref[k]) <= 1e-9, k                    # the two float64 forms agree
        e, e_torch = rel_err(got[k], ref[k]), rel_err(t32[k], ref[k])
        assert e <= max(2 * e_torch, 1e-5), (k, e, e_torch)
    sure = np.abs(ref["mask_value"] - 0.1) > 1e-5
    assert np.array_equal(got["object_mask"][sure], ref["object_mask"][sure]) and 0 < int(got["object_mask"].sum()) < uv.shape[0]
    # texel centres return the stored texel: u R is exact for a power of two
    rows, cols = np.nonzero(mask)
    centres = np.stack([(cols + 0.5) / 64, 1.0 - (rows + 0.5) / 64], -1).astype(np.float32)
    c = tr.sample(pos, nrm, mask, centres)
    assert np.array_equal(c["x"].view(np.uint32), (pos[rows, cols] + np.float32(0)).view(np.uint32)) and c["object_mask"].all()
