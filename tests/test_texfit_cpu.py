"""The atlas-fitting library and robir_amd/texfit.py as far as they go without a GPU: loading, the export list, argument errors before any
launch, the host build of csrc/texfit/texfit_math.h against the restatement bit for bit (tools/check_texfit_host.py), and the rules
themselves on the float64 restatement (tests/texfit_restatement.py): the scatter is the adjoint of the fetch, the dense gradient is
grid_sample's, one lazy Adam step is torch.optim.Adam's on the touched entries and leaves the others alone."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import texfit_restatement as tf
from conftest import ROOT

c_long, c_int, c_double = ctypes.c_long, ctypes.c_int, ctypes.c_double
NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(4096)                    # never read: every call below is refused, or has nothing to do, before a launch
OTHER_HEADERS = ("robir_hip.h", "robir_hip_legacy.h", "robir_hip_train.h", "robir_hip_vistrain.h", "robir_hip_illumtrain.h",
                 "robir_hip_cesrtrain.h", "robir_hip_lightfit.h", "robir_hip_texbake.h", "robir_hip_observe.h", "robir_hip_photoloss.h",
                 "robir_hip_metrics.h", "robir_hip_raster.h")
F64 = np.float64


def _header_symbols(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return sorted(set(re.findall(r"^(?:int|long|const char\*) (rb_[a-z0-9_]+)\s*\(", hdr, re.M)))


def _tf_lib():
    from robir_amd import _lib
    if not os.path.exists(_lib.TEXFIT_PATH):
        _lib.build(legacy=False)
    return _lib.texfit()


def test_texfit_library_exports_its_header():
    """librobir_hip_texfit.so loads without a GPU and exports exactly what include/robir_hip_texfit.h declares, every name rb_tf_*; its header
    names no other library (no prefix, no header file), and no other header names this one."""
    from robir_amd import _lib
    L = _tf_lib()
    assert L.rb_tf_abi_version() == _lib.TEXFIT_ABI_VERSION == 1
    syms = _header_symbols("robir_hip_texfit.h")
    assert syms == ["rb_tf_abi_version", "rb_tf_adam", "rb_tf_fetch", "rb_tf_last_error", "rb_tf_scatter", "rb_tf_taps"]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.TEXFIT_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[-1] for l in out.splitlines() if " T rb_" in l) == syms
    mine = open(os.path.join(ROOT, "include", "robir_hip_texfit.h")).read()
    assert "#define RB_TF_ABI_VERSION 1" in mine
    assert set(re.findall(r"\brb_[a-z]+_", mine, re.I)) <= {"rb_tf_", "RB_TF_"} and re.findall(r"robir_hip\w*\.h", mine) == ["robir_hip_texfit.h"]
    for h in OTHER_HEADERS:
        text = open(os.path.join(ROOT, "include", h)).read()
        assert "rb_tf_" not in text and "robir_hip_texfit" not in text, h
        assert not set(syms) & set(_header_symbols(h))
    assert len(OTHER_HEADERS) == 12


def test_build_checks_and_names_the_texfit_library():
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '(_lib.texfit(), ("robir_hip_texfit.h",))' in src and "_lib.TEXFIT_PATH" in src
    mk = open(os.path.join(ROOT, "robir_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\$\(XOUT\)", mk, re.M) and re.search(r"^default:.*\$\(XOUT\)", mk, re.M) and "$(eval $(call TRAINLIB,texfit))" in mk
    assert "build/texfit/texfit.o: texfit/texfit_math.h" in mk


def test_texfit_argument_errors_before_any_launch():
    L = _tf_lib()
    err = L.rb_tf_last_error

    def taps(uv=FAKE, n=5, R=16, filt=1, tt=FAKE, tw=FAKE):
        return L.rb_tf_taps(uv, c_long(n), c_int(R), c_int(filt), tt, tw, NULL)
    assert taps(uv=NULL) != 0 and b"null pointer" in err()
    assert taps(tw=NULL) != 0 and b"null pointer" in err()
    assert taps(n=-1) != 0 and b"negative" in err()
    assert taps(n=1 << 29) != 0 and b"2^29" in err()
    assert taps(R=0) != 0 and b"R = 0" in err()
    assert taps(R=16385) != 0 and b"R = 16385" in err()
    assert taps(filt=2) != 0 and b"filter" in err()
    assert taps(n=0, uv=NULL, tt=NULL, tw=NULL) == 0

    def fetch(planes=FAKE, R=16, Cs=8, tt=FAKE, tw=FAKE, n=5, C=4, tex=FAKE):
        return L.rb_tf_fetch(planes, c_int(R), c_int(Cs), tt, tw, c_long(n), c_int(C), tex, NULL)
    assert fetch(C=9) != 0 and b"C = 9" in err()
    assert fetch(C=0) != 0 and b"C = 0" in err()
    assert fetch(Cs=17, C=17) != 0 and b"Cs = 17" in err()
    assert fetch(R=16385) != 0 and b"R = 16385" in err()
    assert fetch(n=-3) != 0 and b"negative" in err()
    assert fetch(n=1 << 29) != 0 and b"2^29" in err()
    assert fetch(planes=NULL) != 0 and b"null pointer" in err()
    assert fetch(tex=NULL) != 0 and b"null pointer" in err()
    assert fetch(n=0, planes=NULL, tt=NULL, tw=NULL, tex=NULL) == 0

    def scatter(pr=FAKE, pw=FAKE, P=20, ss=FAKE, T=3, g=FAKE, n=5, C=4, grad=FAKE):
        return L.rb_tf_scatter(pr, pw, c_long(P), ss, c_long(T), g, c_long(n), c_int(C), grad, NULL)
    assert scatter(P=-1) != 0 and b"negative" in err()
    assert scatter(T=-1) != 0 and b"negative" in err()
    assert scatter(n=-1) != 0 and b"negative" in err()
    assert scatter(n=1 << 29) != 0 and b"2^29" in err()
    assert scatter(P=21) != 0 and b"4 n" in err()
    assert scatter(T=21) != 0 and b"segments" in err()
    assert scatter(C=17) != 0 and b"C = 17" in err()
    assert scatter(pr=NULL) != 0 and b"null pointer" in err()
    assert scatter(grad=NULL) != 0 and b"null pointer" in err()
    assert scatter(T=0, pr=NULL, pw=NULL, ss=NULL, g=NULL, grad=NULL) == 0
    assert scatter(P=0, T=0, pr=NULL, pw=NULL, ss=NULL, g=NULL, grad=NULL) == 0

    three = (c_double * 16)(*([0.1] * 16))
    lo, hi = (c_double * 16)(*([0.0] * 16)), (c_double * 16)(*([1.0] * 16))

    def adam(planes=FAKE, m=FAKE, v=FAKE, st=FAKE, g=FAKE, T=3, R=16, Cs=8, C=4, lr=three, lo_=lo, hi_=hi, b1=0.9, b2=0.999, eps=1e-8,
             bc1=0.1, bc2=0.001):
        return L.rb_tf_adam(planes, m, v, st, g, c_long(T), c_int(R), c_int(Cs), c_int(C), lr, lo_, hi_, c_double(b1), c_double(b2),
                            c_double(eps), c_double(bc1), c_double(bc2), NULL)
    assert adam(C=9) != 0 and b"C = 9" in err()
    assert adam(R=0) != 0 and b"R = 0" in err()
    assert adam(R=16385) != 0 and b"R = 16385" in err()
    assert adam(T=-1) != 0 and b"negative" in err()
    assert adam(T=257, R=16) != 0 and b"touched" in err()
    assert adam(lr=NULL) != 0 and b"null pointer" in err()
    assert adam(planes=NULL) != 0 and b"null pointer" in err()
    assert adam(v=NULL) != 0 and b"null pointer" in err()
    assert adam(b1=1.0) != 0 and b"beta" in err()
    assert adam(bc2=0.0) != 0 and b"bias" in err()
    assert adam(lo_=hi, hi_=lo) != 0 and b"clamp" in err()
    assert adam(T=0, planes=NULL, m=NULL, v=NULL, st=NULL, g=NULL) == 0


def test_missing_texfit_library_has_its_own_message(monkeypatch, tmp_path):
    from robir_amd import _lib
    monkeypatch.setattr(_lib, "_texfit", None)
    monkeypatch.setattr(_lib, "TEXFIT_PATH", str(tmp_path / "nope_texfit.so"))
    with pytest.raises(_lib.RobirHipError, match="ATLAS-FITTING library") as e:
        _lib.call_texfit("rb_tf_taps")
    msg = str(e.value)
    assert "make -C robir_amd/csrc texfit" in msg and "librobir_hip_texfit.so" in msg and "LEGACY" not in msg


def test_python_refuses_before_the_library():
    from robir_amd import ops, texfit
    with pytest.raises(ValueError, match="16384"):
        ops.tf_taps(torch.zeros(3, 2), 16385)
    with pytest.raises(ValueError, match="Cs"):
        ops._tf_atlas(torch.zeros(4, 4, 17))
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match="uv"):
            texfit.fetch(torch.zeros(4, 4, 2), torch.zeros(3, 2, requires_grad=True))
    with pytest.raises(ValueError, match="vis"):
        texfit.AtlasFit("nowhere", {}, light=torch.zeros(4, 7), vis="traced")
    with pytest.raises(ValueError, match="model or a light"):
        texfit.AtlasFit("nowhere", {})
    poses = texfit.orbit_poses(np.eye(4), 4)
    assert poses.shape == (4, 4, 4) and np.array_equal(poses[0], np.eye(4, dtype=np.float32))
    assert np.allclose(poses[1][:3, :3] @ poses[1][:3, :3].T, np.eye(3), atol=1e-6) and np.allclose(poses[2][:3, :3], np.diag([-1, 1, -1]), atol=1e-6)


def test_host_build_equals_the_restatement_bit_for_bit():
    spec = importlib.util.spec_from_file_location("check_texfit_host", os.path.join(ROOT, "tools", "check_texfit_host.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if mod.compiler() is None:
        pytest.skip("no host C++ compiler")
    rows = mod.check()
    assert len(rows) >= 50
    assert not [what for what, ok in rows if not ok]


# ----------------------------------------------------------------------------------------- the rules, on the float64 restatement
def _finite_uvs(R):
    uv = tf.tap_uvs(R)
    return uv[np.isfinite(uv).all(-1) & (np.abs(uv) < 100).all(-1)].astype(F64)


@pytest.mark.parametrize("R", (1, 8, 64))
def test_taps_say_what_they_are_meant_to(R):
    uv = tf.tap_uvs(R)
    texel, weight = tf.taps(uv, R, 1)
    inside = texel >= 0
    assert ((weight == 0) | inside).all() and (texel < R * R).all() and not np.signbit(weight).any()
    bad = ~np.isfinite(uv).all(-1)
    assert bad.sum() >= 5 and (texel[bad] == -1).all() and (weight[bad] == 0).all()
    # rows whose four taps are inside: the weights sum to one within rounding; a texel centre gives exactly (1, 0, 0, 0)
    full = inside.all(-1)
    assert R == 1 or (full.sum() > 100 and np.abs(weight[full].astype(F64).sum(-1) - 1).max() < 1e-5)
    centre = np.array([[(1 + 0.5) / R, 1.0 - (2 + 0.5) / R]], dtype=np.float32) if R >= 8 else np.array([[0.5, 0.5]], dtype=np.float32)
    t, w = tf.taps(centre, R, 1)
    assert t[0, 0] == (2 * R + 1 if R >= 8 else 0) and list(w[0]) == [1, 0, 0, 0]
    t0, w0 = tf.taps(uv, R, 0)
    assert (t0[:, 0] >= 0).all() and (t0[:, 0] < R * R).all() and (t0[:, 1:] == -1).all() and (w0[:, 0] == 1).all() and not w0[:, 1:].any()
    # the taps reproduce the view's own fetch (meshrender_restatement) bit for bit where the uv is finite
    planes = np.random.default_rng(R).uniform(0.05, 1.0, (R, R, 8)).astype(np.float32)
    ok = np.isfinite(uv).all(-1)
    for filt, ref in ((0, tf.mr.fetch_nearest), (1, tf.mr.fetch_bilinear)):
        t, w = tf.taps(uv[ok], R, filt)
        assert np.array_equal(tf.fetch(planes, t, w).view(np.uint32), ref(planes, uv[ok, 0], uv[ok, 1]).view(np.uint32)), filt


@pytest.mark.parametrize("R", (1, 8, 64))
def test_scatter_is_the_adjoint_of_the_fetch(R):
    """<fetch(A), g> = <A, scatter(g)> in float64 to 1e-12 relative."""
    rng = np.random.default_rng(R)
    uv = _finite_uvs(R)
    A, g = rng.normal(size=(R, R, 4)), rng.normal(size=(len(uv), 4))
    texel, weight = tf.taps(uv, R, 1, dtype=F64)
    pr, pw, st, ss = tf.sort_pairs(texel, weight, R)
    lhs = float((tf.fetch(A, texel, weight, dtype=F64) * g).sum())
    rhs = float((A * tf.dense(st, tf.scatter(pr, pw, ss, g, dtype=F64), R)).sum())
    assert abs(lhs) > 1e-3 and abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    assert ss[0] == 0 and ss[-1] == (texel >= 0).sum() and (np.diff(ss) > 0).all() and (np.diff(st) > 0).all()
    order = 4 * pr[:ss[-1]].astype(np.int64)          # pairs of one texel stay in ascending row order
    assert all((np.diff(order[ss[s]:ss[s + 1]]) >= 0).all() for s in range(len(st)))


@pytest.mark.parametrize("R", (1, 8, 64))
def test_dense_gradient_equals_grid_samples_autograd(R):
    """torch.nn.functional.grid_sample (bilinear, align_corners=False, zero padding) at (2 u - 1, 1 - 2 v) is an independent statement of the
    same convention: value and gradient to the image agree in float64 to 1e-12."""
    rng = np.random.default_rng(100 + R)
    uv = _finite_uvs(R)
    A, g = rng.normal(size=(R, R, 4)), rng.normal(size=(len(uv), 4))
    texel, weight = tf.taps(uv, R, 1, dtype=F64)
    pr, pw, st, ss = tf.sort_pairs(texel, weight, R)
    mine = tf.dense(st, tf.scatter(pr, pw, ss, g, dtype=F64), R)
    img = torch.from_numpy(A).permute(2, 0, 1)[None].clone().requires_grad_(True)
    grid = torch.from_numpy(np.stack([2 * uv[:, 0] - 1, 1 - 2 * uv[:, 1]], -1))[None, :, None, :]
    with torch.enable_grad():
        val = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0, :, :, 0].T
        (val * torch.from_numpy(g)).sum().backward()
    scale = float(np.abs(A).max())
    assert np.abs(val.detach().numpy() - tf.fetch(A, texel, weight, dtype=F64)).max() <= 1e-12 * scale
    theirs = img.grad[0].permute(1, 2, 0).numpy()
    assert np.abs(theirs).max() > 0.1 and np.abs(mine - theirs).max() <= 1e-12 * np.abs(theirs).max()


def test_one_adam_step_equals_torch_adam_on_the_touched_entries():
    """Three steps of the restatement in float64 without a clamp against torch.optim.Adam on the touched entries, to 1e-12; the untouched
    entries and their moments keep their bits."""
    case = tf.adam_case(8, 4, 37, 1)
    R, C = 8, 4
    lr = 0.02
    planes, m, v = case["planes"].astype(F64), np.zeros((R, R, C)), np.zeros((R, R, C))
    start = planes.copy()
    tex = case["seg_texel"]
    ok = (tex >= 0) & (tex < R * R)
    assert ok.sum() == 35
    idx = tex[ok].astype(np.int64)
    p = torch.from_numpy(start.reshape(R * R, 8)[idx, :C].copy()).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    rng = np.random.default_rng(4)
    inf = np.full(C, np.inf)
    for t in (1, 2, 3):
        grad = rng.normal(size=(len(tex), C))
        tf.adam(planes, m, v, tex, grad, np.full(C, lr), -inf, inf, 0.9, 0.999, 1e-8, t, dtype=F64)
        p.grad = torch.from_numpy(grad[ok].copy())
        opt.step()
        got = planes.reshape(R * R, 8)[idx, :C]
        assert np.abs(got - p.detach().numpy()).max() <= 1e-12, t
    assert np.abs(planes - start).max() > 1e-2
    rest = np.ones(R * R, dtype=bool)
    rest[idx] = False
    assert np.array_equal(planes.reshape(R * R, 8)[rest], start.reshape(R * R, 8)[rest])
    assert np.array_equal(planes[..., C:], start[..., C:])                      # the frozen channels of touched texels
    assert not m.reshape(R * R, C)[rest].any() and not v.reshape(R * R, C)[rest].any() and m.reshape(R * R, C)[idx].all()


def test_the_clamp_acts_in_the_adam_cases():
    for Cs, C, T, t in tf.ADAM_CASES[:2]:
        case = tf.adam_case(Cs, C, T, t)
        planes, m, v = case["planes"].copy(), case["m"].copy(), case["v"].copy()
        tf.adam(planes, m, v, case["seg_texel"], case["grad"], case["lr"], case["lo"], case["hi"], 0.9, 0.999, 1e-8, t)
        moved = planes[..., :C][planes[..., :C] != case["planes"][..., :C]]
        assert (moved == np.float32(0.25)).any() and np.isin(moved, case["hi"].astype(np.float32)).any()


def test_scatter_case_and_loop_scene_say_what_they_are_meant_to():
    pr, pw, ss, g = tf.scatter_case(4)
    assert list(np.diff(ss)) == list(tf.SEGMENTS) and ss[-1] < len(pr) <= 4 * g.shape[0] and g.shape[0] % 64
    assert (pr[ss[-1]:] >= g.shape[0]).all() and ((pr[:ss[-1]] < 0) | (pr[:ss[-1]] >= g.shape[0])).sum() == 4
    grad = tf.scatter(pr, pw, ss, g)
    assert np.array_equal(grad[0], (pw[0].astype(F64) * g[pr[0]].astype(F64)).astype(np.float32))
    scene = tf.loop_scene()
    hits = [len(r["idx"]) for r in scene["rows"]]
    assert all(300 < h < 700 for h in hits), hits
    rows = tf.loop_rows(scene)
    texel, _ = tf.taps(rows["uv"], tf.LOOP["R"], 1)
    touched = np.unique(texel[texel >= 0]).size
    assert 1000 < touched < 3500 and np.abs(scene["start"][..., :4] - scene["truth"][..., :4]).mean() > 0.08
    assert np.array_equal(scene["start"][..., 4:], scene["truth"][..., 4:])
