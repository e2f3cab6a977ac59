#!/usr/bin/env python
"""Checks the hand-derived backward of the light-SG environment map and the fused step on the CPU: compiles tools/lightfit_host.cpp
(= robir_amd/csrc/lightfit/lightfit_math.h built for the host, with plain loops) with the host C++ compiler and compares, on every case of
tests/lightfit_oracle.py,

    the gradient for a random upstream and the MSE with its gradient    with the oracle's float64 autograd: 1e-10, both being float64;
    50 fused Adam steps on the trajectory cases                         with the oracle's float64 loop: max(2 e_torch, 1e-5), DESIGN 4.3.

    python tools/check_lightfit_host.py          prints every distance; exit status 1 if one is over its bound
"""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import lightfit_oracle as lfo  # noqa: E402

BOUND = 1e-10


def rel_err(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float(((a - b).abs() / (b.abs() + b.abs().mean() + 1e-30)).max()) if b.numel() else 0.0


def compiler():
    return os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def build():
    cxx = compiler()
    if cxx is None:
        raise SystemExit("no host C++ compiler found (set CXX)")
    out = os.path.join(tempfile.mkdtemp(prefix="lf_host_"), "lightfit_host.so")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "robir_amd", "csrc"),
                    os.path.join(ROOT, "tools", "lightfit_host.cpp"), "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.lf_host_loss_grad.restype = ctypes.c_double
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_bwd(L, lgt, dirs, g_rgb):
    a = [np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (lgt, dirs, g_rgb)]
    grad = np.zeros((lgt.shape[0], 7), dtype=np.float64)
    L.lf_host_bwd(_p(a[0]), ctypes.c_int(lgt.shape[0]), _p(a[1]), ctypes.c_long(dirs.shape[0]), _p(a[2]), _p(grad))
    return grad


def host_loss_grad(L, lgt, dirs, target):
    a = [np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (lgt, dirs, target)]
    grad = np.zeros((lgt.shape[0], 7), dtype=np.float64)
    loss = L.lf_host_loss_grad(_p(a[0]), ctypes.c_int(lgt.shape[0]), _p(a[1]), _p(a[2]), ctypes.c_long(dirs.shape[0]), _p(grad))
    return loss, grad


def host_fit(L, lgt, dirs, target, steps, first_step=0, lr=1e-2, moments=None):
    p = np.ascontiguousarray(lgt.numpy(), dtype=np.float32).copy()
    m, v = (np.zeros_like(p), np.zeros_like(p)) if moments is None else (moments[0].copy(), moments[1].copy())
    d, t = (np.ascontiguousarray(x.numpy(), dtype=np.float32) for x in (dirs, target))
    hist = np.zeros(steps, dtype=np.float64)
    D = ctypes.c_double
    L.lf_host_fit(_p(p), _p(m), _p(v), ctypes.c_int(p.shape[0]), _p(d), _p(t), ctypes.c_long(d.shape[0]), ctypes.c_long(first_step),
                  ctypes.c_long(steps), D(lr), D(0.9), D(0.999), D(1e-8), _p(hist))
    return p, m, v, hist


def check(L=None, trajectories=True):
    """-> [(what, distance, bound)] over every case."""
    L = L or build()
    rows = []
    for name in lfo.CASES:
        c = lfo.make_case(name)
        g64 = lfo.backward(c["lgt"], c["dirs"], c["g_rgb"])
        rows.append((f"{name}: backward", rel_err(host_bwd(L, c["lgt"], c["dirs"], c["g_rgb"]), g64), BOUND))
        loss64, lg64 = lfo.loss_and_grad(c["lgt"], c["dirs"], c["target"])
        loss, lg = host_loss_grad(L, c["lgt"], c["dirs"], c["target"])
        rows.append((f"{name}: loss", abs(loss - loss64) / abs(loss64), BOUND))
        rows.append((f"{name}: loss gradient", rel_err(lg, lg64), BOUND))
        if name == "signs":
            assert g64[2, 5] == 0.0 and host_bwd(L, c["lgt"], c["dirs"], c["g_rgb"])[2, 5] == 0.0, "the gradient at mu_raw = 0 is 0"
    for name in lfo.TRAJECTORY_CASES if trajectories else ():
        c = lfo.make_case(name)
        p64, m64, v64, h64 = lfo.fit(c["lgt"], c["dirs"], c["target"], 50)
        p32, m32, v32, h32 = lfo.fit(c["lgt"], c["dirs"], c["target"], 50, torch.float32)
        p, m, v, h = host_fit(L, c["lgt"], c["dirs"], c["target"], 50)
        for what, mine, t32, ref in (("parameters", p, p32, p64), ("exp_avg", m, m32, m64), ("exp_avg_sq", v, v32, v64), ("losses", h, h32, h64)):
            rows.append((f"{name}: 50 steps, {what}", rel_err(mine, ref), max(2.0 * rel_err(t32, ref), 1e-5)))
    return rows


def main():
    bad = 0
    for what, e, bound in check():
        print(f"{what:44s} {e:9.2e}   (bound {bound:.1e})" + ("" if e <= bound else "   OVER"))
        bad += not e <= bound
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
