#!/usr/bin/env python
"""Checks the photometric loss's arithmetic on the CPU: compiles tools/photoloss_host.cpp (= robir_amd/csrc/photoloss/photoloss_math.h built
for the host as a stand-alone program, with plain loops) with the host C++ compiler, runs it on cases of tests/photoloss_oracle.py and
compares with that oracle:

  * value_f32 (the fp32 forward) against the float64 oracle by the training tests' rule e <= max(2 e_torch, 1e-5), e_torch the error of the
    oracle run in float32;
  * value_d1 (value and both partial derivatives, fp64) and the loss rows against float64 autograd to 1e-10 (conftest.rel_err's measure):
    both sides are fp64 evaluations of different but equivalent expressions, eps 1.1e-16 times the curves' condition on the tested domain
    (< 1e3) times a few dozen operations.

    python tools/check_photoloss_host.py          prints one line per case; exit status 1 if one is out of bounds
"""
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
import photoloss_oracle as plo  # noqa: E402

FLOOR, TOL64 = 1e-5, 1e-10


def compiler():
    """$CXX, the system's C++ compiler, or the clang++ that ships with the HIP compiler the library itself was built with."""
    found = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if found:
        return found
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"      # csrc/Makefile's default
    for root in (os.environ.get("ROCM_PATH"), os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))):
        cand = os.path.join(root, "llvm", "bin", "clang++") if root else None
        if cand and os.path.exists(cand):
            return cand
    return None


def build(extra=(), out_dir=None):
    """-> path of the program, in out_dir (the caller's to remove) or in a fresh temporary directory that main() removes.
    extra: more compiler flags (e.g. -fsanitize=address,undefined: the program has its own main)."""
    cxx = compiler()
    if cxx is None:
        raise SystemExit("no host C++ compiler found (set CXX)")
    out = os.path.join(out_dir or tempfile.mkdtemp(prefix="pl_host_"), "photoloss_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "robir_amd", "csrc"),
                    os.path.join(ROOT, "tools", "photoloss_host.cpp"), "-o", out], check=True)
    return out


def _run(prog, header, arrays):
    d = os.path.dirname(prog)
    src, dst = os.path.join(d, "case.in"), os.path.join(d, "case.out")
    with open(src, "wb") as f:
        f.write(np.array(header, dtype=np.int32).tobytes() + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays))
    subprocess.run([prog, src, dst], check=True)
    return open(dst, "rb").read()


def _split(blob, layout):
    pos, out = 0, []
    for dt, shape in layout:
        n = int(np.prod(shape))
        out.append(torch.from_numpy(np.frombuffer(blob, dtype=dt, count=n, offset=pos).reshape(shape).copy()))
        pos += n * np.dtype(dt).itemsize
    assert pos == len(blob), (pos, len(blob))
    return out


def host_curve(prog, x, shift, curve, inverse):
    """-> (y fp32, y, dx, dt fp64), each [n,3]."""
    n = x.shape[0]
    blob = _run(prog, [0, n, curve, int(inverse), 0 if shift.numel() == 1 and n != 1 else 1, 0], [x.numpy().astype(np.float32), shift.numpy().astype(np.float32)])
    return _split(blob, [(np.float32, (n, 3))] + [(np.float64, (n, 3))] * 3)


def host_loss(prog, case, curve, l2):
    """-> (loss [1], gx [n,3], gshift [n]) fp64."""
    n = case["sg_rgb"].shape[0]
    sh = case["shift"] if case["shift"] is not None else torch.ones(1)
    arrays = [case["sg_rgb"].numpy()] + ([case["indir_rgb"].numpy()] if case["indir_rgb"] is not None else []) + [
        case["gt"].numpy(), case["net_mask"].numpy().astype(np.uint8), case["obj_mask"].numpy().astype(np.uint8), sh.numpy().astype(np.float32)]
    blob = _run(prog, [1, n, curve, int(l2), 0 if sh.numel() == 1 and n != 1 else 1, int(case["indir_rgb"] is not None)], arrays)
    return _split(blob, [(np.float64, (1,)), (np.float64, (n, 3)), (np.float64, (n,))])


def rel_err(a, b):
    """conftest.rel_err's measure: max |a - b| / (|b| + mean |b|)."""
    a, b = a.double(), b.double()
    if a.numel() == 0:
        return 0.0
    return float(((a - b).abs() / (b.abs() + b.abs().mean() + 1e-30)).max())


def elementwise_truth(x, shift, curve, inverse):
    """float64 (y, dy/dx, dy/dt) per element: the shift expanded to one leaf per element, clamped by make_shift."""
    with torch.enable_grad():
        xx = x.double().clone().requires_grad_(True)
        tt = shift.double().reshape(-1, 1).expand(x.shape[0], 3).clone().requires_grad_(True)
        t = plo.make_shift(tt)
        y = plo.curve_inv(xx, t, curve) if inverse else plo.curve_fn(xx, t, curve)
        gx, gt = torch.autograd.grad(y.sum(), [xx, tt], allow_unused=True)
    return y.detach(), gx, torch.zeros_like(tt) if gt is None else gt


def check(prog):
    """prog: build()'s program -> [(what, figure, bound, ok)]."""
    rows = []
    for curve in plo.CURVES + (plo.RATIONAL,):
        for inverse in ((False,) if curve == plo.RATIONAL else (False, True)):
            for per_row in (False, True):
                x, t, _ = plo.tonemap_case(257, min(curve, 3), inverse, per_row)
                if per_row:                       # both sides of the clamp, and its closed upper end
                    t[:3] = torch.tensor([0.0, 1.5, 1.0])
                    if inverse:                   # x tc stays below aces_inv's pole with tc = 1
                        x[:3] = x[:3].clamp(max=0.6)
                y32, y64, dx, dt = host_curve(prog, x, t, curve, inverse)
                ry, rdx, rdt = elementwise_truth(x, t, curve, inverse)
                y_t32 = plo.curve_inv(x, plo.make_shift(t).reshape(-1, 1), curve) if inverse else plo.curve_fn(x, plo.make_shift(t).reshape(-1, 1), curve)
                tag = f"curve {curve} {'ldr2hdr' if inverse else 'hdr2ldr'} {'row' if per_row else 'one'} shift"
                e, et = rel_err(y32, ry), rel_err(y_t32.expand_as(ry), ry)
                rows.append((f"{tag}: value_f32", e, max(2 * et, FLOOR), e <= max(2 * et, FLOOR)))
                for name, a, b in (("value", y64, ry), ("d/dx", dx, rdx), ("d/dt", dt, rdt)):
                    e = rel_err(a, b)
                    rows.append((f"{tag}: value_d1 {name}", e, TOL64, e <= TOL64))
                if per_row:
                    z = float(dt[:2].abs().max())
                    rows.append((f"{tag}: d/dt outside the clamp", z, 0.0, z == 0.0))
    for curve in plo.CURVES + (plo.RATIONAL,):
        for l2 in (False, True):
            for per_row in (False, True):
                case = plo.loss_case(257, curve, per_row, l2, indir=not (l2 and per_row))
                loss, gx, gs = host_loss(prog, case, curve, l2)
                r_loss, r_sg, _, r_sh = plo.loss_grads(case, curve, l2, torch.float64)
                tag = f"loss curve {curve} {'L2' if l2 else 'L1'} {'row' if per_row else 'one'} shift"
                pairs = [("loss", loss.reshape(()), r_loss), ("d/d rgb", gx, r_sg)]
                if r_sh is not None:
                    pairs.append(("d/d shift", gs if per_row else gs.sum().reshape(1), r_sh.reshape(-1)))
                for name, a, b in pairs:
                    e = rel_err(a, b)
                    rows.append((f"{tag}: {name}", e, TOL64, e <= TOL64))
                outside = ~(case["net_mask"] & case["obj_mask"])
                z = float(gx[outside].abs().max()) if bool(outside.any()) else 0.0
                rows.append((f"{tag}: rows outside the mask", z, 0.0, z == 0.0))
    return rows


def main():
    bad = 0
    with tempfile.TemporaryDirectory(prefix="pl_host_") as d:
        for what, fig, bound, ok in check(build(out_dir=d)):
            print(f"{what:64s} {fig:.3e} (bound {bound:.1e}) {'ok' if ok else 'OUT OF BOUNDS'}")
            bad += not ok
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
