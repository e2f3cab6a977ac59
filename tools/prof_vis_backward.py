#!/usr/bin/env python
"""Times the visibility network's forward (the policy's forward kernel) and its reverse mode (rb_vt_vis_bwd):
`python tools/prof_vis_backward.py [out.md] [--no-torch]` -> profiles/vis_backward_times.md.  HIP-event ms, medians after warm-up, at
M = 84992 rows (166 surface points x 512 directions: 256 pixels x 65 % hits of the shipped illum_num_pixels) and M = 2^20 (2048 points x 512),
with all ten gradients, with the last layer's two only, and with part_rows = slab_rows (the unsplit reduction) against the default split --
those two timed alternately in one loop; the scratch of one backward; and, as the comparison a user has without the kernel, the same step
through PyTorch-ROCm fp32 autograd of the oracle's formulas (tests/vis_train_oracle.py) on the same GPU.  All values are recorded only: nothing
asserts a speed."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from robir_amd import nets, ops, synth  # noqa: E402
import vis_train_oracle as vto  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "vis_backward_times.md")
dev = torch.device("cuda:0")
REP = 512
SIZES = (166 * REP, 1 << 20)
LAST = ("vis_layer.8.weight", "vis_layer.8.bias")
# multiply-adds per row of one pass through the network; a backward with all gradients is three such passes (activations, dZ, dW)
MAC_ROW = 126 * 256 + 3 * 256 * 256 + 256 * 2


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def median_ms(*fns, reps=15, warm=3):
    """Medians of the given thunks, timed alternately (a, b, a, b, ...) after `warm` rounds of each."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ts[i].append(timed(fn))
    out = [statistics.median(t) for t in ts]
    return out[0] if len(out) == 1 else out


sd = synth.synth_state_dict(0, variance=0.3)
net = nets.VisNetwork(points_multires=10, dirs_multires=10, dims=[256] * 4)
net.load_state_dict({k[len(vto.PREFIX):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(vto.PREFIX)})
net = net.to(dev).eval()
params = [p.detach() for p in (t for i in range(5) for t in (net.vis_layer[2 * i].weight, net.vis_layer[2 * i].bias))]
res = {}


def make_inputs(M):
    g = torch.Generator(device=dev).manual_seed(M)
    pts = torch.randn(M // REP, 3, device=dev, generator=g) * 0.5
    dirs = torch.nn.functional.normalize(torch.randn(M, 3, device=dev, generator=g), dim=-1)
    return pts, dirs, torch.randn(M, 2, device=dev, generator=g) / M


with torch.no_grad():
    for M in SIZES:
        pts, dirs, gl = make_inputs(M)
        reps = 15 if M < (1 << 19) else 7
        slab = ops.VIS_SLAB_ROWS
        bwd = lambda want=ops.VIS_PARAM_NAMES, part=None: ops.vis_backward(pts, dirs, REP, params, gl, want=want, part_rows=part)
        split_ms, unsplit_ms = median_ms(bwd, lambda: bwd(part=slab), reps=reps)
        r = {"forward_ms": median_ms(lambda: net.logits_from_points(pts, dirs, REP), reps=reps), "backward_all_ms": split_ms,
             "backward_all_unsplit_ms": unsplit_ms, "backward_last_layer_ms": median_ms(lambda: bwd(LAST), reps=reps)}
        (a, st), (b, st_un), (_, st_last) = bwd(), bwd(part=slab), bwd(LAST)
        r.update(scratch_MiB=st["scratch_bytes"] / 2 ** 20, scratch_unsplit_MiB=st_un["scratch_bytes"] / 2 ** 20, launches_all=st["launches"],
                 launches_unsplit=st_un["launches"], launches_last_layer=st_last["launches"], partitions=st["partitions"],
                 fp64_tflops_all=3 * 2 * MAC_ROW * M / (split_ms * 1e-3) / 1e12,
                 split_vs_unsplit_max_rel_diff=max(float(((a[k] - b[k]).abs() / (b[k].abs() + b[k].abs().mean())).max()) for k in a))
        res[M] = r
        print(M, json.dumps(r), flush=True)

if "--no-torch" not in sys.argv:
    P = dict(zip(vto.NAMES, params))
    for M in SIZES:
        pts, dirs, gl = make_inputs(M)

        def step(names=vto.NAMES):
            with torch.enable_grad():
                L = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in P.items()}
                y = vto.vis_forward(L, pts, dirs, REP)
                torch.autograd.grad((y * gl).sum(), [L[k] for k in names])
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res[M]["torch_fp32_fwd_bwd_all_ms"] = median_ms(step, reps=7)
        res[M]["torch_fp32_peak_extra_MiB"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        res[M]["torch_fp32_fwd_bwd_last_layer_ms"] = median_ms(lambda: step(LAST), reps=7)
        print(M, json.dumps(res[M]), flush=True)

f = lambda v, u="": "-" if v is None else f"{v:.3f}{u}"
lines = ["# Visibility-network backward: times (one MI355X, `python tools/prof_vis_backward.py`)", "",
         "HIP events around one call, median of 15 calls (7 at 2^20 rows) after 3 warm-up calls; recorded only, no test asserts a speed.  Forward: the",
         "default policy's forward kernel (`VisNetwork.logits_from_points`, rep 512).  Backward: `rb_vt_vis_bwd`, fp64 on `v_mfma_f64_16x16x4_f64`,",
         f"`slab_rows` {ops.VIS_SLAB_ROWS}; split = the default `part_rows` {ops.VIS_PART_ROWS} ({ops.VIS_SLAB_ROWS // ops.VIS_PART_ROWS} partitions x 20 output",
         "tiles = 320 workgroups in the widest weight-gradient launch), unsplit = `part_rows = slab_rows` (20 workgroups).  The two were timed",
         "alternately in one loop.  A backward call includes the allocation of its scratch from torch's caching allocator.", "",
         "| M | forward | backward, all 10, split (default) | backward, all 10, unsplit | backward, last layer only | scratch split / unsplit | "
         "kernels enqueued (all / unsplit / last layer) | fp64 rate of the split backward (3 x 2 x 229 k x M flop over its time) | "
         "split vs unsplit, largest rel. difference of a gradient entry |",
         "|---|---|---|---|---|---|---|---|---|"]
for M, r in res.items():
    lines.append(f"| {M} | {f(r['forward_ms'], ' ms')} | {f(r['backward_all_ms'], ' ms')} | {f(r['backward_all_unsplit_ms'], ' ms')} | "
                 f"{f(r['backward_last_layer_ms'], ' ms')} | {r['scratch_MiB']:.1f} / {r['scratch_unsplit_MiB']:.1f} MiB | "
                 f"{r['launches_all']} / {r['launches_unsplit']} / {r['launches_last_layer']} | {r['fp64_tflops_all']:.2f} TFLOP/s | "
                 f"{r['split_vs_unsplit_max_rel_diff']:.1e} |")
if "--no-torch" not in sys.argv:
    lines += ["", "Comparison -- the same step (forward + backward) through PyTorch-ROCm fp32 autograd of the oracle's formulas",
              "(`tests/vis_train_oracle.py`), same GPU, median of 7.  It is fp32 where the kernel is fp64: not the same arithmetic.", "",
              "| M | torch fp32 forward + backward, all | torch fp32, last layer only | torch peak memory beyond its inputs | HIP forward + backward, all |",
              "|---|---|---|---|---|"]
    for M, r in res.items():
        lines.append(f"| {M} | {f(r['torch_fp32_fwd_bwd_all_ms'], ' ms')} | {f(r['torch_fp32_fwd_bwd_last_layer_ms'], ' ms')} | "
                     f"{r['torch_fp32_peak_extra_MiB']:.1f} MiB | {f(r['forward_ms'] + r['backward_all_ms'], ' ms')} |")
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print(json.dumps(res))
print("wrote", out_path)
