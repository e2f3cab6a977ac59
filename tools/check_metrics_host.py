#!/usr/bin/env python
"""Checks the image metrics' arithmetic on the CPU: compiles tools/metrics_host.cpp (= robir_amd/csrc/metrics/metrics_math.h built for the
host as a stand-alone program, with plain loops) with the host C++ compiler, runs it on cases of tests/metrics_oracle.py and compares with
that oracle:

  * the pair sums, the angular sums and the SSIM sums to a relative 1e-9 (both sides are fp64 sums of the same terms in another order, with
    the two libms' pow / acos: eps 1.1e-16 times a few thousand terms);
  * every SSIM map entry to an absolute 1e-5, the bound of the GPU tests (the figures are some 1e-13);
  * exact zeros at the windows that are not counted, and SSIM(x, x) == 1 exactly.

    python tools/check_metrics_host.py          prints one line per case; exit status 1 if one is out of bounds
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import metrics_oracle as mo  # noqa: E402

TOL_SUM, TOL_MAP = 1e-9, 1e-5


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
    """-> path of the program, in out_dir (the caller's to remove) or in a fresh temporary directory.
    extra: more compiler flags (e.g. -fsanitize=address,undefined: the program has its own main)."""
    cxx = compiler()
    if cxx is None:
        raise SystemExit("no host C++ compiler found (set CXX)")
    out = os.path.join(out_dir or tempfile.mkdtemp(prefix="mt_host_"), "metrics_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "robir_amd", "csrc"),
                    os.path.join(ROOT, "tools", "metrics_host.cpp"), "-o", out], check=True)
    return out


def _run(prog, header, arrays):
    d = os.path.dirname(prog)
    src, dst = os.path.join(d, "case.in"), os.path.join(d, "case.out")
    with open(src, "wb") as f:
        f.write(np.array(header, dtype=np.int32).tobytes() + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays if a is not None))
    subprocess.run([prog, src, dst], check=True)
    return np.fromfile(dst, dtype=np.float64)


def _opt(mask, scale):
    return (None if mask is None else np.asarray(mask).astype(np.uint8), None if scale is None else np.asarray(scale, np.float32))


def host_pair(prog, pred, gt, mask=None, t=0, scale=None):
    """pred, gt [P,C] -> (count, sums [C,5])"""
    P, C = pred.shape
    m, s = _opt(mask, scale)
    out = _run(prog, [0, P, 0, C, t, m is not None, s is not None], [pred, gt, m, s])
    return out[0], out[1:].reshape(C, 5)


def host_angular(prog, a, b, mask=None):
    m, _ = _opt(mask, None)
    out = _run(prog, [1, a.shape[0], 0, 3, 0, m is not None, 0], [a, b, m])
    return out[0], out[1]


def host_ssim(prog, pred, gt, mask=None, t=0, scale=None):
    """pred, gt [H,W,C] -> (count, sum, map [H-10,W-10,C])"""
    H, W, C = pred.shape
    m, s = _opt(mask, scale)
    out = _run(prog, [2, H, W, C, t, m is not None, s is not None], [pred, gt, m, s])
    return out[0], out[1], out[2:].reshape(H - 10, W - 10, C)


def check(prog):
    """prog: build()'s program -> [(what, figure, bound, ok)]."""
    rows = []
    for P in (1, mo.ROWS + 1, 1000):
        for C in (1, 3, 4):
            p, g, m = mo.rows(1, P, C)
            for t in mo.TRANSFERS:
                scale = None if t == mo.CLIP else np.linspace(0.5, 1.5, C).astype(np.float32)
                n, s = host_pair(prog, p[0], g[0], m[0], t, scale)
                rn, rs = mo.pair_stats(p, g, m, t, scale)
                e = max(mo.rel(n, rn[0]), mo.rel(s, rs[0]))
                rows.append((f"pair P={P} C={C} transfer {t}", e, TOL_SUM, e <= TOL_SUM))
    for P in (1, 1000):
        a, b, m = mo.normals(1, P)
        n, s = host_angular(prog, a[0], b[0], m[0])
        rn, rs = mo.angular_stats(a, b, m)
        e = max(mo.rel(n, rn[0]), mo.rel(s, rs[0]))
        rows.append((f"angular P={P}", e, TOL_SUM, e <= TOL_SUM))
    for kind in ("noise", "smooth", "flat"):
        for (H, W, C) in ((11, 11, 1), (11, 12, 3), (mo.TILE + 11, mo.TILE + 13, 3), (45, 53, 3)):
            p, g = mo.images(kind, 1, H, W, C)
            m = mo.masks(1, H, W)
            for t in ((mo.NONE, mo.GAMMA22_Q8) if kind == "noise" else (mo.NONE,)):
                n, s, mp = host_ssim(prog, p[0], g[0], m[0], t)
                rn, rs, rmap = mo.ssim(p, g, m, t)
                e = float(np.abs(mp - rmap[0]).max())
                rows.append((f"ssim {kind} {H}x{W}x{C} transfer {t}: map", e, TOL_MAP, e <= TOL_MAP))
                e = max(mo.rel(n, rn[0]), mo.rel(s, rs[0]))
                rows.append((f"ssim {kind} {H}x{W}x{C} transfer {t}: count, sum", e, TOL_SUM, e <= TOL_SUM))
                z = float(np.abs(mp[~m[0, 5:H - 5, 5:W - 5]]).max()) if not m[0, 5:H - 5, 5:W - 5].all() else 0.0
                rows.append((f"ssim {kind} {H}x{W}x{C} transfer {t}: windows that are not counted", z, 0.0, z == 0.0))
    p, _ = mo.images("noise", 1, 45, 53, 3)
    _, _, mp = host_ssim(prog, p[0], p[0], None, mo.GAMMA22)
    z = float(np.abs(mp - 1.0).max())
    rows.append(("ssim(x, x) - 1", z, 0.0, z == 0.0))
    return rows


def main():
    bad = 0
    with tempfile.TemporaryDirectory(prefix="mt_host_") as d:
        for what, fig, bound, ok in check(build(out_dir=d)):
            print(f"{what:64s} {fig:.3e} (bound {bound:.1e}) {'ok' if ok else 'OUT OF BOUNDS'}")
            bad += not ok
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
