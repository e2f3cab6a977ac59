#!/usr/bin/env python
"""Times the light-SG fit (robir_amd/lightfit.py, librobir_hip_lightfit.so): `python tools/prof_lightfit.py [out.md]` ->
profiles/lightfit_times.md.  HIP-event ms per step at 256 x 512 pixels x 128 lobes (the reference's fit) and at 64 x 128 x 32: blocks of STEPS
fused steps (rb_lf_fit_steps: forward, MSE, gradient, Adam, two launches each) against, on the same box and timed alternately, the same number
of steps of the PyTorch-ROCm fp32 autograd loop of the same formulas with torch.optim.Adam (tests/lightfit_oracle.py on the device) -- the
yardstick, since no parent implementation exists.  Median of 5 blocks after 1 warm-up block.  All values are recorded only: nothing asserts a
speed."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from robir_amd import lightfit  # noqa: E402
import lightfit_oracle as lfo  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "lightfit_times.md")
dev = torch.device("cuda:0")
STEPS = 50


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def median_ms(*fns, reps=5, warm=1):
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ts[i].append(timed(fn))
    return [statistics.median(t) for t in ts]


def peak_extra_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


res = {}
for H, W, M in ((256, 512, 128), (64, 128, 32)):
    c = lfo.make_case("prof", H, W, M, 128)
    env = c["target"].reshape(H, W, 3).to(dev)
    dirs, target = c["dirs"].to(dev), c["target"].to(dev)

    def hip_block():
        lightfit.fit_envmap(env, num_sg=M, iters=STEPS, size=(H, W), seed=5, block=STEPS)

    def torch_block():
        with torch.enable_grad():
            p = torch.nn.Parameter(c["lgt"].to(dev).clone())
            opt = torch.optim.Adam([p], lr=1e-2)
            for _ in range(STEPS):
                opt.zero_grad()
                ((lfo.envmap(p, dirs) - target) ** 2).mean().backward()
                opt.step()

    hip_ms, torch_ms = median_ms(hip_block, torch_block)
    q = {"pixels": H * W, "lobes": M, "hip_ms_per_step": hip_ms / STEPS, "torch_fp32_ms_per_step": torch_ms / STEPS,
         "hip_peak_extra_MiB": peak_extra_mib(hip_block), "torch_fp32_peak_extra_MiB": peak_extra_mib(torch_block)}
    res[f"{H} x {W} x {M}"] = q
    print(json.dumps(q), flush=True)

lines = ["# Light-SG fit: times (one MI355X, `python tools/prof_lightfit.py`)", "",
         f"HIP events around a block of {STEPS} steps, median of 5 blocks after 1 warm-up block, divided by {STEPS}; recorded only, no test asserts a speed.",
         "A HIP block is one `lightfit.fit_envmap` call (the resize of the target, the allocation of its state and one read-back of the block's",
         "losses included); the PyTorch block is the reference's loop -- fp32 autograd of the same formulas and `torch.optim.Adam` on the device,",
         "no read-back.  The HIP step is fp64 where the PyTorch step is fp32: not the same arithmetic.", "",
         "| pixels x lobes | HIP step | torch fp32 step | HIP peak memory beyond its inputs | torch peak |", "|---|---|---|---|---|"]
for name, q in res.items():
    lines.append(f"| {name} | {q['hip_ms_per_step']:.4f} ms | {q['torch_fp32_ms_per_step']:.4f} ms | {q['hip_peak_extra_MiB']:.1f} MiB | "
                 f"{q['torch_fp32_peak_extra_MiB']:.1f} MiB |")
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print(json.dumps(res))
print("wrote", out_path)
