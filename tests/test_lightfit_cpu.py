"""The light-fitting library and robir_amd/lightfit.py as far as they go without a GPU: loading, the export list, argument errors before any
launch, the size and geometry queries against the header's formula, the refusal of a viewdirs gradient, and the derivation's check -- the
per-pair arithmetic of csrc/lightfit/lightfit_math.h built for the host (tools/check_lightfit_host.py) against the float64 autograd of
tests/lightfit_oracle.py."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import lightfit_oracle as lfo
from conftest import ROOT, record_metric, rel_err

c_long, c_int, c_double = ctypes.c_long, ctypes.c_int, ctypes.c_double
NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(4096)                    # 8-byte aligned, never read: every call below is refused, or has nothing to do, before a launch
OTHER_HEADERS = ("robir_hip.h", "robir_hip_legacy.h", "robir_hip_train.h", "robir_hip_vistrain.h", "robir_hip_illumtrain.h", "robir_hip_cesrtrain.h")


def _header_symbols(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return sorted(set(re.findall(r"^(?:int|long|const char\*) (rb_[a-z0-9_]+)\s*\(", hdr, re.M)))


def _lf_lib():
    from robir_amd import _lib
    if not os.path.exists(_lib.LIGHTFIT_PATH):
        _lib.build(legacy=False)
    return _lib.lightfit()


def test_lightfit_library_exports_its_header():
    """librobir_hip_lightfit.so loads without a GPU and exports exactly what include/robir_hip_lightfit.h declares, every name rb_lf_*; no rb_
    name is shared with the other six headers, and none of them names this one."""
    from robir_amd import _lib
    L = _lf_lib()
    assert L.rb_lf_abi_version() == _lib.LIGHTFIT_ABI_VERSION == 1
    syms = _header_symbols("robir_hip_lightfit.h")
    assert syms == ["rb_lf_abi_version", "rb_lf_area_resize", "rb_lf_envmap_sg_bwd", "rb_lf_fit_steps", "rb_lf_groups", "rb_lf_last_error",
                    "rb_lf_scratch_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIGHTFIT_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[-1] for l in out.splitlines() if " T rb_" in l) == syms
    others = set()
    for h in OTHER_HEADERS:
        text = open(os.path.join(ROOT, "include", h)).read()
        others |= set(_header_symbols(h))
        assert "rb_lf_" not in text and "lightfit" not in text
    assert not set(syms) & others
    assert "#define RB_LF_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "robir_hip_lightfit.h")).read()


def test_size_and_geometry_queries():
    L = _lf_lib()
    g = lambda n: L.rb_lf_groups(c_long(n))
    assert (g(0), g(1), g(4), g(5), g(240), g(2048), g(2049), g(131072)) == (0, 1, 1, 2, 60, 512, 512, 512)
    assert g(-1) == -1 and b"negative" in L.rb_lf_last_error()
    q = lambda n, M: L.rb_lf_scratch_bytes(c_long(n), c_int(M))
    # the header's formula: 8 (groups(n) (7 M + 1) + (M > 128 ? 3 n : 0))
    for n, M in ((1, 1), (240, 130), (512, 8), (512, 128), (512, 129), (131072, 128), (131072, 256), (7, 1000)):
        assert q(n, M) == 8 * (g(n) * (7 * M + 1) + (3 * n if M > 128 else 0)), (n, M)
    assert q(0, 8) == 0
    assert q(-1, 8) == -1 and b"negative" in L.rb_lf_last_error()
    assert q(8, 0) == -1 and b"at least one lobe" in L.rb_lf_last_error()
    assert q(8, 128 * 65535 + 1) == -1 and b"lobe tiles" in L.rb_lf_last_error()
    assert "8 (rb_lf_groups(n) (7 M + 1) + (M > 128 ? 3 n : 0))" in open(os.path.join(ROOT, "include", "robir_hip_lightfit.h")).read()


def test_lightfit_argument_errors_before_any_launch():
    L = _lf_lib()
    err = L.rb_lf_last_error

    def bwd(lgt=FAKE, M=8, dirs=FAKE, n=64, g=FAKE, d_lgt=FAKE, scratch=FAKE, nbytes=1 << 40):
        return L.rb_lf_envmap_sg_bwd(lgt, c_int(M), dirs, c_long(n), g, d_lgt, scratch, c_long(nbytes), NULL)

    def fit(lgt=FAKE, m=FAKE, v=FAKE, M=8, dirs=FAKE, target=FAKE, n=64, first=0, steps=3, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, hist=FAKE,
            scratch=FAKE, nbytes=1 << 40):
        return L.rb_lf_fit_steps(lgt, m, v, c_int(M), dirs, target, c_long(n), c_long(first), c_long(steps), c_double(lr), c_double(b1),
                                 c_double(b2), c_double(eps), hist, scratch, c_long(nbytes), NULL)

    need = L.rb_lf_scratch_bytes(c_long(64), c_int(8))
    for call in (bwd, fit):
        for k in ("lgt", "dirs", "scratch") + (("g", "d_lgt") if call is bwd else ("m", "v", "target", "hist")):
            assert call(**{k: NULL}) != 0 and b"null pointer" in err(), k
        assert call(M=0) != 0 and b"at least one lobe" in err()
        assert call(M=-3) != 0 and b"at least one lobe" in err()
        assert call(n=-1) != 0 and b"negative" in err()
        assert call(nbytes=need - 8) != 0 and b"scratch too small" in err()
        assert call(scratch=ctypes.c_void_p(4100)) != 0 and b"aligned" in err()
        # nothing to do: no launch, no error, whatever the pointers
        assert call(n=0, lgt=NULL, dirs=NULL, scratch=NULL, nbytes=0) == 0
    assert fit(steps=0, lgt=NULL, hist=NULL, scratch=NULL, nbytes=0) == 0
    assert fit(steps=-1) != 0 and b"n_steps" in err()
    assert fit(first=-1) != 0 and b"first_step" in err()
    assert fit(b1=1.0) != 0 and b"beta1" in err()
    assert fit(b2=-0.1) != 0 and b"beta2" in err()
    assert fit(eps=-1e-8) != 0 and b"eps" in err()
    assert fit(lr=float("nan")) != 0 and b"lr" in err()

    def resize(src=FAKE, H0=16, W0=32, dst=FAKE, H=8, W=16):
        return L.rb_lf_area_resize(src, c_int(H0), c_int(W0), dst, c_int(H), c_int(W), NULL)
    assert resize(H=17) != 0 and b"up-sampling refused" in err()
    assert resize(W=33) != 0 and b"up-sampling refused" in err()
    assert resize(src=NULL) != 0 and b"null pointer" in err()
    assert resize(dst=NULL) != 0 and b"null pointer" in err()
    assert resize(H=0) != 0 and b"empty image" in err()
    assert resize(H0=1 << 16, W0=(1 << 15) + 1) != 0 and b"2^31" in err()


def test_missing_lightfit_library_has_its_own_message(monkeypatch, tmp_path):
    from robir_amd import _lib
    monkeypatch.setattr(_lib, "_lightfit", None)
    monkeypatch.setattr(_lib, "LIGHTFIT_PATH", str(tmp_path / "nope_lightfit.so"))
    with pytest.raises(_lib.RobirHipError, match="LIGHT-FITTING library") as e:
        _lib.call_lightfit("rb_lf_fit_steps")
    msg = str(e.value)
    assert "make -C robir_amd/csrc lightfit" in msg and "librobir_hip_lightfit.so" in msg and "LEGACY" not in msg


def test_viewdirs_gradient_is_refused():
    """The direction grid is a constant of this path: a viewdirs that requires grad is refused before any kernel, not given a silent zero."""
    from robir_amd import lightfit
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match="viewdirs"):
            lightfit.render_envmap_sg(torch.zeros(8, 7, requires_grad=True), torch.zeros(4, 3, requires_grad=True))
    assert torch.equal(lightfit.envmap_dirs(12, 20).reshape(-1, 3), lfo.envmap_dirs(12, 20))
    assert torch.equal(lightfit.envmap_dirs(5, 7, True).reshape(-1, 3), lfo.envmap_dirs(5, 7, True))
    assert torch.equal(lightfit.init_light_sgs(24, 5), lfo.init_light_sgs(24, 5))


def test_oracle_area_resize_is_the_box_mean():
    rng = np.random.default_rng(0)
    img = rng.uniform(0, 4, (16, 32, 3))
    assert np.allclose(lfo.area_resize(img, 8, 16), img.reshape(8, 2, 16, 2, 3).mean((1, 3)), rtol=0, atol=1e-14)
    assert np.array_equal(lfo.area_resize(img, 16, 32), img)
    frac = lfo.area_resize(img[:15, :31], 4, 7)
    assert frac.shape == (4, 7, 3) and abs(frac.mean() - img[:15, :31].mean()) < 1e-13          # an area mean keeps the mean
    assert np.allclose(lfo.area_resize(np.full((15, 31, 3), 0.7), 4, 7), 0.7, rtol=0, atol=1e-15)


def _host_tool():
    spec = importlib.util.spec_from_file_location("check_lightfit_host", os.path.join(ROOT, "tools", "check_lightfit_host.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_host_build_of_the_math_matches_float64_autograd():
    """tools/check_lightfit_host.py: lightfit_math.h compiled with the host C++ compiler (tools/lightfit_host.cpp supplies the loops) against
    the oracle's float64 autograd -- the gradient for a random upstream, the MSE and its gradient, on every case: 1e-10, both being float64.
    Then the fused step on the CPU: 50 steps of the smallest trajectory case against the float64 Adam loop under the parity rule."""
    tool = _host_tool()
    if tool.compiler() is None:
        pytest.skip("no host C++ compiler")
    L = tool.build()
    rows = tool.check(L, trajectories=False)
    assert len(rows) == 3 * len(lfo.CASES)
    for what, e, bound in rows:
        record_metric("lightfit/host/" + what, e=e, bound=bound)
        assert bound == 1e-10 and e <= bound, (what, e)
    c = lfo.make_case("16x32x8")
    p64, m64, v64, h64 = lfo.fit(c["lgt"], c["dirs"], c["target"], 50)
    p32, m32, v32, h32 = lfo.fit(c["lgt"], c["dirs"], c["target"], 50, torch.float32)
    p, m, v, h = tool.host_fit(L, c["lgt"], c["dirs"], c["target"], 50)
    for what, mine, t32, ref in (("parameters", p, p32, p64), ("exp_avg", m, m32, m64), ("exp_avg_sq", v, v32, v64), ("losses", h, h32, h64)):
        e, e_torch = rel_err(mine, ref), rel_err(t32, ref)
        record_metric("lightfit/host/16x32x8: 50 steps, " + what, e=e, e_torch=e_torch)
        assert e <= max(2 * e_torch, 1e-5), (what, e, e_torch)
    # 50 steps in one call = 5 calls of 10 with first_step advanced, bit for bit
    q, qm, qv = c["lgt"], None, None
    parts = []
    for i in range(5):
        qn, qm, qv, hh = tool.host_fit(L, q, c["dirs"], c["target"], 10, first_step=10 * i, moments=None if qm is None else (qm, qv))
        q = torch.from_numpy(qn)
        parts.append(hh)
    assert np.array_equal(qn, p) and np.array_equal(qm, m) and np.array_equal(qv, v) and np.array_equal(np.concatenate(parts), h)
