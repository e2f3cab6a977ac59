#!/usr/bin/env python
"""Times the photometric loss + gradient on the device and writes the record profiles/photoloss_times.md:

    python tools/prof_photoloss.py [--rounds 5] [--out profiles/photoloss_times.md]

Two ways to get loss, d loss / d sg_rgb, d loss / d indir_rgb and d loss / d adapt_illum of model/loss.py:97-110 with the scale_aces curve,
L1, two independent masks of ~80 % each (~64 % of the rows inside both):

  fused   training.photometric_loss with a marked ACESToneMapping + backward()      (librobir_hip_photoloss.so: two launches + torch's scaling)
  torch   PyTorch-ROCm autograd of the same formulas (tests/photoloss_oracle.py) on the same device tensors + backward()

at the confs' batch (num_pixels = 1024 rows) and at one 800 x 800 view (640 000 rows).  A figure is the host clock around `iters` steps that
end in a device synchronise, divided by `iters` -- what a training step pays, Python included; a round runs fused then torch, alternating,
and the table holds the median and the range over the rounds after one warm-up round.  The two results are compared before timing."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import photoloss_oracle as plo  # noqa: E402
from robir_amd import nets, training  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photoloss_times.md"))
a = ap.parse_args()
assert torch.cuda.is_available(), "prof_photoloss needs the GPU"
dev = torch.device("cuda:0")
SIZES = ((1024, 4000, "the confs' batch, num_pixels = 1024"), (800 * 800, 2000, "one 800 x 800 view"))


def timed(step, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e3


rows = []
for n, iters, what in SIZES:
    case = plo.loss_case(n, 0, False, False)
    d = {k: (None if v is None else v.to(dev)) for k, v in case.items()}
    tone = training.enable_tonemap_training(nets.ACESToneMapping(hdr_mode=0).to(dev))
    sg, ind = d["sg_rgb"].clone().requires_grad_(True), d["indir_rgb"].clone().requires_grad_(True)
    leaves = (sg, ind, tone.adapt_illum)

    def zero():
        for t in leaves:
            t.grad = None

    def fused():
        zero()
        loss = training.photometric_loss(sg, ind, d["gt"], d["net_mask"], d["obj_mask"], tone=tone)
        loss.backward()
        return loss

    def eager():
        zero()
        loss = plo.image_loss(sg, ind, d["gt"], d["net_mask"], d["obj_mask"], tone.as_input().reshape(1), 0)
        loss.backward()
        return loss

    lf = fused()
    gf = [t.grad.clone() for t in leaves]
    le = eager()
    ge = [t.grad.clone() for t in leaves]
    rel = lambda x, y: float((x - y).abs().max() / (y.abs().max() + 1e-30))
    agree = max([rel(lf.detach(), le.detach())] + [rel(x, y) for x, y in zip(gf, ge)])
    assert agree < 1e-4, agree
    timed(fused, iters), timed(eager, iters)                       # warm-up round
    tf, te = [], []
    for _ in range(a.rounds):
        tf.append(timed(fused, iters))
        te.append(timed(eager, iters))
    rows.append((n, what, iters, statistics.median(tf), min(tf), max(tf), statistics.median(te), min(te), max(te), agree))

lines = ["# Photometric loss + gradient: fused HIP op against PyTorch autograd on the device (MI355X)", "",
         "Written by `tools/prof_photoloss.py`.  Loss, d/d sg_rgb, d/d indir_rgb and d/d adapt_illum of `model/loss.py:97-110` (scale_aces, L1,",
         "~64 % of the rows inside both masks).  ms per step = host clock around `iters` forward + backward steps ending in a device synchronise,",
         f"divided by `iters` (Python included); median [min .. max] over {a.rounds} rounds after one warm-up round, fused and torch alternating.", "",
         "| rows | | iters | fused ms | torch autograd ms | ratio | largest relative difference of the results |", "|---|---|---|---|---|---|---|"]
for n, what, iters, mf, lf_, hf, me, le_, he, agree in rows:
    lines.append(f"| {n} | {what} | {iters} | {mf:.3f} [{lf_:.3f} .. {hf:.3f}] | {me:.3f} [{le_:.3f} .. {he:.3f}] | {me / mf:.2f} | {agree:.1e} |")
lines += ["", "A 1024-row step is launch-bound on both sides: the figure there is the number of launches and the Python around them, not the",
          "arithmetic; where the 640 000-row figure equals it within the spread, the same holds there.  Kernel times were not measured.",
          "These are the only two settings measured; no test asserts a speed."]
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
print("wrote", a.out)
