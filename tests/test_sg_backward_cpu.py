"""The CPU side of the SG shading backward: the C entry point exists and validates before any launch, the refusals that need no GPU, and
the gradient fixtures are complete."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

NULL = ctypes.c_void_p(0)


def _bwd(L, n, M=4, ptrs=NULL, scratch=NULL, scratch_floats=0, d_f0=NULL):
    a = [ptrs, ptrs, ptrs, ctypes.c_int(0), ctypes.c_int(M), ptrs, ptrs, ptrs, NULL, NULL, ptrs, NULL, ctypes.c_int(0), ctypes.c_long(n),
         ptrs, ptrs, ptrs, ptrs, NULL, NULL, NULL, NULL, NULL, NULL, NULL, d_f0, scratch, ctypes.c_long(scratch_floats), NULL]
    return L.rb_sg_shade_bwd(*a)


def test_entry_point_validates_before_any_launch():
    from robir_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "rb_sg_shade_bwd") and hasattr(L, "rb_sg_shade_bwd_scratch_floats") and hasattr(L, "rb_sg_shade_bwd_groups")
    assert _bwd(L, 8) != 0 and b"null pointer" in L.rb_last_error()
    assert _bwd(L, 0) == 0 and _bwd(L, -3) == 0
    buf = (ctypes.c_float * 64)()
    some = ctypes.cast(buf, ctypes.c_void_p)
    assert _bwd(L, 8, M=0, ptrs=some) != 0 and b"lobe" in L.rb_last_error()
    assert _bwd(L, 8, ptrs=some, d_f0=some) != 0 and b"null pointer" in L.rb_last_error()            # d_f0 wanted, no scratch
    assert _bwd(L, 8, ptrs=some, d_f0=some, scratch=some, scratch_floats=16) != 0 and b"scratch" in L.rb_last_error()
    assert L.rb_abi_version() == 8


def test_launch_geometry_queries():
    from robir_amd import _lib
    L = _lib.lib()
    assert L.rb_sg_shade_bwd_scratch_floats(ctypes.c_int(128)) == 2 * 512 * (7 * 128 + 1)
    assert L.rb_sg_shade_bwd_scratch_floats(ctypes.c_int(0)) == 0
    g = lambda n: L.rb_sg_shade_bwd_groups(ctypes.c_long(n))
    assert (g(0), g(1), g(4), g(5), g(2048), g(2049), g(1 << 19)) == (0, 1, 1, 2, 512, 512, 512)


def test_header_declares_the_backward():
    src = open(os.path.join(ROOT, "include", "robir_hip.h")).read()
    for name in ("rb_sg_shade_bwd", "rb_sg_shade_bwd_scratch_floats", "rb_sg_shade_bwd_groups"):
        assert re.search(r"^(int|long) " + name + r"\(", src, re.M), name


def test_geometry_refusal_needs_no_gpu():
    from robir_amd import sg_autograd, sg_render
    n = 3
    z = lambda *s: torch.zeros(*s)
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match="normal"):
            sg_render.render_with_all_sg(z(n, 3), z(n, 3).requires_grad_(), z(n, 3), z(8, 7), z(1, 1), z(n, 1), z(n, 3))
        with pytest.raises(NotImplementedError, match="viewdirs"):
            sg_autograd.sg_shade(z(n, 3), z(n, 3).requires_grad_(), z(8, 7), z(1), z(n), z(n, 3), z(n))
    sg_autograd.refuse_geometry_grad(normal=z(n, 3).requires_grad_())          # grad mode off (the suite's default): nothing to refuse


def test_shared_light_behind_an_expanded_view():
    from robir_amd import sg_autograd
    p = torch.randn(16, 7, requires_grad=True)
    assert sg_autograd.shared_light(p) is p
    sh = sg_autograd.shared_light(p.unsqueeze(0).expand(5, 16, 7))
    assert tuple(sh.shape) == (16, 7) and sh.data_ptr() == p.data_ptr()
    with torch.enable_grad():
        (sg_autograd.shared_light(p.unsqueeze(0).expand(5, 16, 7)) * 2.0).sum().backward()
    assert tuple(p.grad.shape) == (16, 7) and bool((p.grad == 2.0).all())
    assert sg_autograd.shared_light(torch.randn(5, 16, 7)) is None


@pytest.mark.parametrize("tag", ["init", "sharp"])
def test_gradient_fixtures_are_complete(tag):
    fx, base = load_golden("sg_grad_" + tag), load_golden("sg_" + tag)
    cases = json.loads(str(fx["cases"]))
    assert set(cases) == {"direct", "direct_lin_met", "indirect", "indirect_lin_met", "indirect_sg_diffuse", "clamped"}
    n = base["normal"].shape[0]
    for case, cfg in cases.items():
        assert fx[f"{case}.in.g_spec"].shape == (n, 3) and fx[f"{case}.in.g_diff"].shape == (n, 3)
        bv = fx[f"{case}.in.bvis"]
        assert 0.0 in bv and 1.0 in bv and bv.min() >= 0 and bv.max() <= 1
        if cfg["comp_vis"]:
            lv = fx[f"{case}.in.light_vis"]
            assert 0.0 in lv and 1.0 in lv and lv.min() >= 0 and lv.max() <= 1
        grads = {k for k in fx if k.startswith(case + ".grad.")}
        assert grads and all(fx[k].dtype == np.float64 and np.isfinite(fx[k]).all() for k in grads)
        assert all(float(fx[k]) <= 1e-10 for k in fx if k.startswith(case + ".oracle_dist."))
