#!/usr/bin/env python
"""Times PSNR and SSIM on the device and writes the record profiles/metrics_times.md:

    python tools/prof_metrics.py [--rounds 5] [--views 200] [--out profiles/metrics_times.md]

One call each of metrics.psnr and metrics.ssim (gamma 2.2 on both images, no mask, no map) on 1 view and on `--views` views of
800 x 800 x 3, against a PyTorch-ROCm fp32 restatement on the same device tensors (clamp / pow, a mean; two conv2d per moment):

  fused   librobir_hip_metrics.so: one launch pair for all views, fp64 arithmetic
  torch   fp32 eager ops -- NOT the same arithmetic: its SSIM is the restatement whose variance cancels in fp32

A figure is ms per call over `iters` calls, taken twice around the same window: HIP events recorded on the stream before the first and after
the last call (device time, enqueue gaps included), and the host clock from before the first call to after a device synchronise (what a
caller pays, Python included).  A round runs fused then torch, alternating; the table holds the median and the range over the rounds after
one warm-up round.  The two results are compared before timing."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import metrics_oracle as mo  # noqa: E402
from robir_amd import metrics  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--views", type=int, default=200)
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_times.md"))
a = ap.parse_args()
assert torch.cuda.is_available(), "prof_metrics needs the GPU"
dev = torch.device("cuda:0")
WIN = torch.tensor(mo.window(), dtype=torch.float32, device=dev)


def gamma(x):
    return x.clamp(min=0).pow(1.0 / 2.2).clamp(0, 1)


def torch_psnr(p, g):
    return -10.0 * torch.log10(((gamma(p) - gamma(g)) ** 2).mean(dim=(1, 2, 3)))


def torch_ssim(p, g):
    V, H, W, C = p.shape
    x, y = (gamma(t).permute(0, 3, 1, 2).reshape(V * C, 1, H, W) for t in (p, g))
    f = lambda z: F.conv2d(F.conv2d(z, WIN.view(1, 1, 1, 11)), WIN.view(1, 1, 11, 1))
    ux, uy = f(x), f(y)
    vx, vy, vxy = f(x * x) - ux * ux, f(y * y) - uy * uy, f(x * y) - ux * uy
    s = ((2 * ux * uy + mo.C1) * (2 * vxy + mo.C2)) / ((ux * ux + uy * uy + mo.C1) * (vx + vy + mo.C2))
    return s.reshape(V, -1).mean(1)


def timed(call, iters):
    """-> (ms per call by HIP events, ms per call by the host clock), the same window"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    start.record()
    for _ in range(iters):
        call()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters, (time.perf_counter() - t) / iters * 1e3


rows = []
for V, iters in ((1, 200), (a.views, 4)):
    gen = torch.Generator(device=dev).manual_seed(V)
    g = torch.rand(V, a.size, a.size, 3, device=dev, generator=gen)
    p = (g + 0.05 * torch.randn(V, a.size, a.size, 3, device=dev, generator=gen)).contiguous()
    for name, fused, eager in (("psnr", lambda: metrics.psnr(p, g, None, "gamma22"), lambda: torch_psnr(p, g)),
                               ("ssim", lambda: metrics.ssim(p, g, None, "gamma22"), lambda: torch_ssim(p, g))):
        agree = float((fused().cpu() - eager().double().cpu()).abs().max())
        assert agree < (1e-3 if name == "psnr" else 1e-4), (name, V, agree)
        timed(fused, iters), timed(eager, iters)                       # warm-up round
        tf, te = [], []
        for _ in range(a.rounds):
            tf.append(timed(fused, iters))
            te.append(timed(eager, iters))
        rows.append((name, V, iters, tf, te, agree))
    del p, g
    torch.cuda.empty_cache()

fmt = lambda v: f"{statistics.median(v):.3f} [{min(v):.3f} .. {max(v):.3f}]"
lines = ["# PSNR and SSIM: librobir_hip_metrics.so against a PyTorch fp32 restatement on the device (MI355X)", "",
         f"Written by `tools/prof_metrics.py`.  One call of `metrics.psnr` / `metrics.ssim` (gamma 2.2 on both images, no mask, no map) on V views of",
         f"{a.size} x {a.size} x 3.  ms per call over `iters` calls, by HIP events on the stream around the calls and by the host clock ending in a device",
         f"synchronise (Python included); median [min .. max] over {a.rounds} rounds after one warm-up round, fused and torch alternating.  The torch side is",
         "fp32 eager ops and does not compute the same thing to the same accuracy (its SSIM variance cancels in fp32).", "",
         "| metric | V | iters | fused, events ms | fused, host ms | torch, events ms | torch, host ms | torch / fused (events) | largest difference of the results |",
         "|---|---|---|---|---|---|---|---|---|"]
for name, V, iters, tf, te, agree in rows:
    fe, fh, ee, eh = [x[0] for x in tf], [x[1] for x in tf], [x[0] for x in te], [x[1] for x in te]
    lines.append(f"| {name} | {V} | {iters} | {fmt(fe)} | {fmt(fh)} | {fmt(ee)} | {fmt(eh)} | {statistics.median(ee) / statistics.median(fe):.2f} | {agree:.1e} |")
lines += ["", "Not measured: kernel times on their own (no profiler run), other sizes, masks, the map output, other transfers, C other than 3.",
          "No test asserts a speed."]
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
print("wrote", a.out)
