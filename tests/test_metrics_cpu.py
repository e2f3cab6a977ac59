"""The metrics library and its Python surface without a GPU: librobir_hip_metrics.so against its header, its argument checks and size
queries, the host build of metrics_math.h against tests/metrics_oracle.py, the oracle's two SSIM forms against each other, the readers of
robir_amd/evaluate.py on fixtures written here, and the JSON document's schema."""
import ctypes
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import metrics_oracle as mo
from conftest import ROOT

c_long, c_int = ctypes.c_long, ctypes.c_int
NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(4096)                    # never read: every call below is refused, or has nothing to do, before a launch
OTHER_HEADERS = ("robir_hip.h", "robir_hip_legacy.h", "robir_hip_train.h", "robir_hip_vistrain.h", "robir_hip_illumtrain.h",
                 "robir_hip_cesrtrain.h", "robir_hip_lightfit.h", "robir_hip_texbake.h", "robir_hip_observe.h", "robir_hip_photoloss.h")
EXPORTS = ["rb_mt_abi_version", "rb_mt_angular_scratch_bytes", "rb_mt_angular_stats", "rb_mt_groups", "rb_mt_last_error",
           "rb_mt_pair_scratch_bytes", "rb_mt_pair_stats", "rb_mt_ssim", "rb_mt_ssim_scratch_bytes", "rb_mt_ssim_tiles"]
BIG = 1 << 40


def _header_symbols(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return sorted(set(re.findall(r"^(?:int|long|const char\*) (rb_[a-z0-9_]+)\s*\(", hdr, re.M)))


def _mt_lib():
    from robir_amd import _lib
    if not os.path.exists(_lib.METRICS_PATH):
        _lib.build(legacy=False)
    return _lib.metrics()


def test_metrics_library_exports_its_header():
    """librobir_hip_metrics.so loads without a GPU and exports exactly what include/robir_hip_metrics.h declares, every name rb_mt_*; no rb_
    name is shared with the other ten headers, and none of them names this one."""
    from robir_amd import _lib
    L = _mt_lib()
    assert L.rb_mt_abi_version() == _lib.METRICS_ABI_VERSION == 1
    syms = _header_symbols("robir_hip_metrics.h")
    assert syms == EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.METRICS_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[-1] for l in out.splitlines() if " T rb_" in l) == syms
    others = set()
    for h in OTHER_HEADERS:
        text = open(os.path.join(ROOT, "include", h)).read()
        others |= set(_header_symbols(h))
        assert "rb_mt_" not in text and "robir_hip_metrics" not in text
    assert not set(syms) & others
    text = open(os.path.join(ROOT, "include", "robir_hip_metrics.h")).read()
    assert "#define RB_MT_ABI_VERSION 1" in text
    assert f"#define RB_MT_SSIM_TILE {mo.TILE}" in text and f"#define RB_MT_ROWS {mo.ROWS}" in text      # the shapes the GPU tests are built on


def test_build_checks_and_names_the_metrics_library():
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '(_lib.metrics(), ("robir_hip_metrics.h",))' in src and "_lib.METRICS_PATH" in src
    mk = open(os.path.join(ROOT, "robir_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\$\(MOUT\)", mk, re.M) and re.search(r"^default:.*\$\(MOUT\)", mk, re.M) and "photoloss metrics,$(eval" in mk


def test_missing_metrics_library_has_its_own_message(monkeypatch, tmp_path):
    from robir_amd import _lib
    monkeypatch.setattr(_lib, "_metrics", None)
    monkeypatch.setattr(_lib, "METRICS_PATH", str(tmp_path / "nope_metrics.so"))
    with pytest.raises(_lib.RobirHipError, match="METRICS library") as e:
        _lib.call_metrics("rb_mt_ssim")
    msg = str(e.value)
    assert "make -C robir_amd/csrc metrics" in msg and "librobir_hip_metrics.so" in msg and "LEGACY" not in msg


def test_metrics_size_queries():
    L = _mt_lib()
    for P, g in ((-1, -1), (0, 0), (1, 1), (255, 1), (256, 1), (257, 2), (70001, 274), (256 * 1024, 1024), (256 * 1024 + 1, 1024),
                 ((1 << 31) - 1, 1024), (1 << 31, -1)):
        assert L.rb_mt_groups(c_long(P)) == g, P
        for V in (1, 3):
            for C in (1, 3, 4):
                assert L.rb_mt_pair_scratch_bytes(c_long(V), c_long(P), c_int(C)) == (8 * V * g * (1 + 5 * C) if g >= 0 else -1), (V, P, C)
            assert L.rb_mt_angular_scratch_bytes(c_long(V), c_long(P)) == (16 * V * g if g >= 0 else -1), (V, P)
    assert L.rb_mt_pair_scratch_bytes(c_long(0), c_long(100), c_int(3)) == 0
    for bad in ((-1, 8, 3), (65536, 8, 3), (1, 8, 0), (1, 8, 5), (1, -8, 3)):
        assert L.rb_mt_pair_scratch_bytes(c_long(bad[0]), c_long(bad[1]), c_int(bad[2])) == -1, bad
    assert L.rb_mt_angular_scratch_bytes(c_long(-1), c_long(8)) == -1 and L.rb_mt_angular_scratch_bytes(c_long(0), c_long(8)) == 0
    T = mo.TILE
    for (H, W), t in (((-1, 20), -1), ((20, -1), -1), ((0, 20), 0), ((20, 0), 0), ((10, 20), -1), ((20, 10), -1), ((11, 11), 1), ((11, 12), 1),
                      ((T + 10, T + 10), 1), ((T + 11, T + 13), 4), ((45, 53), 9), ((800, 800), 2500), ((1 << 16, 1 << 16), -1)):
        assert L.rb_mt_ssim_tiles(c_long(H), c_long(W)) == t, (H, W)
        assert L.rb_mt_ssim_scratch_bytes(c_long(3), c_long(H), c_long(W)) == (48 * t if t >= 0 else -1), (H, W)
    assert L.rb_mt_ssim_scratch_bytes(c_long(-1), c_long(20), c_long(20)) == -1 and L.rb_mt_ssim_scratch_bytes(c_long(0), c_long(20), c_long(20)) == 0


def test_metrics_argument_errors_before_any_launch():
    L = _mt_lib()
    err = L.rb_mt_last_error

    def pair(pred=FAKE, gt=FAKE, V=1, P=8, C=3, mask=NULL, scale=NULL, transfer=0, stats=FAKE, scratch=FAKE, nbytes=BIG):
        return L.rb_mt_pair_stats(pred, gt, c_long(V), c_long(P), c_int(C), mask, scale, c_int(transfer), stats, scratch, c_long(nbytes), NULL)
    assert pair(V=-1) != 0 and b"negative" in err()
    assert pair(P=-1) != 0 and b"negative" in err()
    assert pair(V=65536) != 0 and b"65535" in err()
    assert pair(P=1 << 31) != 0 and b"2^31" in err()
    assert pair(C=5) != 0 and b"C = 5" in err()
    assert pair(C=0) != 0 and b"C = 0" in err()
    assert pair(transfer=4) != 0 and b"transfer = 4" in err()
    assert pair(transfer=-1) != 0 and b"transfer = -1" in err()
    assert pair(pred=NULL) != 0 and b"null pointer" in err()
    assert pair(gt=NULL) != 0 and b"null pointer" in err()
    assert pair(stats=NULL) != 0 and b"null pointer: stats" in err()
    assert pair(scratch=NULL) != 0 and b"scratch" in err()
    assert pair(scratch=ctypes.c_void_p(4100)) != 0 and b"aligned" in err()
    assert pair(V=3, P=257, nbytes=8 * 3 * 2 * 16 - 1) != 0 and b"scratch_bytes = 767" in err()
    assert pair(V=0, pred=NULL, gt=NULL, stats=NULL, scratch=NULL, nbytes=0) == 0
    assert pair(P=0, pred=NULL, gt=NULL, stats=NULL, scratch=NULL, nbytes=0) == 0
    assert pair(V=0, C=5) != 0                                       # an argument error even where there is nothing to do

    def ang(a=FAKE, b=FAKE, V=1, P=8, mask=NULL, stats=FAKE, scratch=FAKE, nbytes=BIG):
        return L.rb_mt_angular_stats(a, b, c_long(V), c_long(P), mask, stats, scratch, c_long(nbytes), NULL)
    assert ang(V=-2) != 0 and b"negative" in err()
    assert ang(P=-2) != 0 and b"negative" in err()
    assert ang(a=NULL) != 0 and b"null pointer" in err()
    assert ang(b=NULL) != 0 and b"null pointer" in err()
    assert ang(stats=NULL) != 0 and b"null pointer: stats" in err()
    assert ang(scratch=NULL) != 0 and b"scratch" in err()
    assert ang(P=600, nbytes=32) != 0 and b"scratch_bytes = 32" in err()
    assert ang(V=0, a=NULL, b=NULL, stats=NULL, scratch=NULL) == 0
    assert ang(P=0, a=NULL, b=NULL, stats=NULL, scratch=NULL) == 0

    def ssim(pred=FAKE, gt=FAKE, V=1, H=20, W=20, C=3, mask=NULL, scale=NULL, transfer=0, stats=FAKE, out=NULL, scratch=FAKE, nbytes=BIG):
        return L.rb_mt_ssim(pred, gt, c_long(V), c_long(H), c_long(W), c_int(C), mask, scale, c_int(transfer), stats, out, scratch,
                            c_long(nbytes), NULL)
    assert ssim(V=-1) != 0 and b"negative" in err()
    assert ssim(H=-1) != 0 and b"negative" in err()
    assert ssim(H=10) != 0 and b"11 x 11" in err()
    assert ssim(W=10) != 0 and b"11 x 11" in err()
    assert ssim(V=0, H=10) != 0 and b"11 x 11" in err()
    assert ssim(H=1 << 16, W=1 << 16) != 0 and b"2^31" in err()
    assert ssim(C=5) != 0 and b"C = 5" in err()
    assert ssim(transfer=7) != 0 and b"transfer = 7" in err()
    assert ssim(pred=NULL) != 0 and b"null pointer" in err()
    assert ssim(gt=NULL) != 0 and b"null pointer" in err()
    assert ssim(stats=NULL) != 0 and b"null pointer: stats" in err()
    assert ssim(scratch=NULL) != 0 and b"scratch" in err()
    assert ssim(V=2, H=45, W=53, nbytes=16 * 2 * 9 - 1) != 0 and b"scratch_bytes = 287" in err()
    assert ssim(V=0, pred=NULL, gt=NULL, stats=NULL, scratch=NULL) == 0


def _host_tool():
    spec = importlib.util.spec_from_file_location("check_metrics_host", os.path.join(ROOT, "tools", "check_metrics_host.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_host_build_of_the_math_equals_the_oracle(tmp_path):
    """tools/check_metrics_host.py: metrics_math.h compiled with the host C++ compiler as a stand-alone program (tools/metrics_host.cpp
    supplies main and the loops).  Sums to a relative 1e-9, map entries to 1e-5 absolute, exact zeros at the windows that are not counted,
    SSIM(x, x) == 1 exactly."""
    tool = _host_tool()
    assert tool.compiler() is not None, "no host C++ compiler, not even the clang++ beside hipcc"
    rows = tool.check(tool.build(out_dir=str(tmp_path)))
    assert len(rows) == 87
    assert [(what, fig, bound) for what, fig, bound, ok in rows if not ok] == []


def test_oracle_ssim_forms_agree_and_fp32_restatement_does_not():
    """Inside the oracle the explicit 11 x 11 window and scipy's gaussian_filter cropped by 5 agree to 1e-10 on the three image kinds
    (mo.ssim asserts it per channel); the fp32 PyTorch restatement is more than 1e-4 off on the flat-bright pair -- the defect the fp64
    kernels exist for."""
    for kind in ("noise", "smooth", "flat"):
        p, g = mo.images(kind, 1, 45, 53, 3)
        n, s, ref = mo.ssim(p, g)
        assert n[0] == 35 * 43 and ref.shape == (1, 35, 43, 3)
        if kind == "flat":
            e32 = float(np.abs(mo.ssim_f32_torch(p[0], g[0]).astype(np.float64) - ref[0]).max())
            assert e32 > 1e-4, e32
    assert abs(mo.window().sum() - 1.0) < 1e-15 and mo.window()[5] == mo.window().max()


def test_oracle_transfers_ratio_and_angle():
    x = np.array([-0.5, 0.0, 0.2, 1.0, 1.7])
    assert np.array_equal(mo.transfer(x, mo.CLIP), [0.0, 0.0, 0.2, 1.0, 1.0])
    assert np.allclose(mo.transfer(x, mo.GAMMA22), [0.0, 0.0, 0.2 ** (1 / 2.2), 1.0, 1.0], rtol=0, atol=1e-15)
    q = mo.transfer(x, mo.GAMMA22_Q8)
    assert np.array_equal(q * 255, np.round(q * 255)) and q[2] == np.floor(255 * 0.2 ** (1 / 2.2)) / 255
    p = np.random.default_rng(1).random((50, 3)).astype(np.float32) + 0.1
    g = p * np.array([0.5, 2.0, 1.5], np.float32)
    assert np.abs(mo.ratio_lsq(p, g) - [0.5, 2.0, 1.5]).max() < 1e-6 and np.abs(mo.ratio_median(p, g) - [0.5, 2.0, 1.5]).max() < 1e-6
    assert np.array_equal(mo.ratio_lsq(np.zeros((4, 3), np.float32), g[:4]), [1.0, 1.0, 1.0])
    a = np.array([[[1, 0, 0], [0, 0, 0], [2, 2, 0]]], np.float32)
    b = np.array([[[0, 3, 0], [1, 0, 0], [4, 0, 0]]], np.float32)
    n, s = mo.angular_stats(a, b)
    assert n[0] == 2 and abs(s[0] - (np.pi / 2 + np.pi / 4)) < 1e-15


# ----------------------------------------------------------------------------------------- evaluate.py's readers and document
def _view(seed, H=24, W=20):
    rng = np.random.default_rng(seed)
    hit = rng.random((H, W, 1)) < 0.8
    nrm = rng.standard_normal((H, W, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    return {"sg_rgb": rng.random((H, W, 3), dtype=np.float32), "indir_rgb": 0.1 * rng.random((H, W, 3), dtype=np.float32),
            "diffuse_albedo": rng.random((H, W, 3), dtype=np.float32), "roughness": rng.random((H, W, 1), dtype=np.float32),
            "normals": nrm * hit, "network_object_mask": hit}


def test_readers_on_fixtures_written_here(tmp_path):
    """PNG files written by texture.save_png and read back through PIL: colour levels come back as the linear centre of their bin (the
    8-bit gamma transfer returns the level exactly), roughness as k / 255, normals as 2 k / 255 - 1, masks as k >= 128; files pair with the
    predictions by sorted order; .npz inputs are stacked per view."""
    from robir_amd import evaluate, texture
    H, W = 24, 20
    rng = np.random.default_rng(3)
    d = tmp_path / "gt"
    d.mkdir()
    levels = {}
    for i in (1, 0):                                                     # written out of order: the reader sorts
        for kind in ("rgb", "albedo", "normal"):
            levels[kind, i] = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            texture.save_png(str(d / f"{kind}_{i:03d}.png"), levels[kind, i])
        for kind in ("roughness", "mask"):
            levels[kind, i] = rng.integers(0, 256, (H, W), dtype=np.uint8)
            texture.save_png(str(d / f"{kind}_{i:03d}.png"), levels[kind, i])
    gt = evaluate.read_gt(str(d), 2)
    assert sorted(gt) == ["albedo", "mask", "normal", "rgb", "roughness"]
    for i in (0, 1):
        for kind in ("rgb", "albedo"):
            assert gt[kind].shape == (2, H, W, 3) and gt[kind].dtype == np.float32
            k = levels[kind, i].astype(np.float64)
            assert np.array_equal(mo.transfer(gt[kind][i], mo.GAMMA22_Q8) * 255.0, np.minimum(k, 255.0))
            assert np.abs(mo.transfer(gt[kind][i], mo.GAMMA22)[k < 255] * 255.0 - (k[k < 255] + 0.5)).max() < 1e-4
        assert np.array_equal(gt["roughness"][i][..., 0], (levels["roughness", i] / 255.0).astype(np.float32))
        assert np.array_equal(gt["normal"][i], (2.0 * levels["normal", i] / 255.0 - 1.0).astype(np.float32))
        assert gt["mask"].dtype == bool and np.array_equal(gt["mask"][i], levels["mask", i] >= 128)
    with pytest.raises(ValueError, match="2 rgb_"):
        evaluate.read_gt(str(d), 3)
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="no rgb_"):
        evaluate.read_gt(str(empty), 1)
    paths = []
    for i in range(2):
        paths.append(str(tmp_path / f"view{i}.npz"))
        np.savez_compressed(paths[-1], **_view(i, H, W))
    pred = evaluate.read_preds(paths)
    assert pred["sg_rgb"].shape == (2, H, W, 3) and pred["network_object_mask"].shape == (2, H, W, 1)
    assert np.array_equal(pred["roughness"][1], _view(1, H, W)["roughness"])
    one = evaluate._batched(evaluate.read_gt(paths[0], 1), 1)
    assert one["diffuse_albedo"].shape == (1, H, W, 3) and one["network_object_mask"].shape == (1, H, W, 1)
    assert evaluate._batched({"mask": np.ones((H, W), bool)}, 1)["mask"].shape == (1, H, W)
    np.savez(str(tmp_path / "other.npz"), x=np.zeros(3))
    with pytest.raises(ValueError, match="robir_amd.render"):
        evaluate.read_preds([str(tmp_path / "other.npz")])


def test_json_document_schema_and_table():
    from robir_amd import evaluate
    res = {"views": [{"psnr": float("inf"), "ssim": 1.0, "albedo_psnr": 31.5, "albedo_ssim": 0.9, "roughness_mse": 0.0, "normal_mae_deg": 2.5,
                      "albedo_ratio": [1.0, 1.0, 1.0]},
                     {"psnr": 30.0, "ssim": float("nan"), "albedo_psnr": 30.5, "albedo_ssim": 0.8, "roughness_mse": 0.1, "normal_mae_deg": 3.5,
                      "albedo_ratio": [1.0, 1.0, 1.0]}],
           "mean": {"psnr": float("inf"), "ssim": float("nan"), "albedo_psnr": 31.0, "albedo_ssim": 0.85, "roughness_mse": 0.05, "normal_mae_deg": 3.0},
           "albedo_ratio": [1.0, 1.0, 1.0]}
    doc = evaluate.to_json(res, "gamma22", ["a.npz", "b.npz"])
    back = json.loads(json.dumps(doc, allow_nan=False))                 # strict JSON: no bare Infinity / NaN
    assert sorted(back) == ["albedo_ratio", "mean", "pred", "transfer", "views"]
    assert back["transfer"] == "gamma22" and back["pred"] == ["a.npz", "b.npz"] and back["albedo_ratio"] == [1.0, 1.0, 1.0]
    assert back["views"][0]["psnr"] == "inf" and back["views"][1]["ssim"] == "nan" and back["mean"]["psnr"] == "inf"
    assert sorted(back["mean"]) == sorted(evaluate.KEYS) and sorted(back["views"][0]) == sorted(evaluate.KEYS + ("albedo_ratio",))
    lines = evaluate.table(res).splitlines()
    assert lines[0].split() == ["view"] + list(evaluate.KEYS) and lines[1].split()[:2] == ["0", "inf"] and lines[3].split()[0] == "mean"
    assert lines[4] == "albedo_ratio 1 1 1"


def test_python_surface_refuses_what_it_cannot_take():
    import torch
    from robir_amd import metrics
    with pytest.raises(ValueError, match="transfer"):
        metrics._transfer("srgb")
    assert [metrics._transfer(t) for t in ("none", "clip", "gamma22", "GAMMA22_Q8", None, 2)] == [0, 1, 2, 3, 0, 2]
    with pytest.raises(TypeError, match="CUDA float32"):
        metrics.psnr(torch.zeros(4, 4, 3), torch.zeros(4, 4, 3))
    with pytest.raises(TypeError, match="CUDA float32"):
        metrics.ssim(np.zeros((12, 12, 3), np.float32), np.zeros((12, 12, 3), np.float32))
