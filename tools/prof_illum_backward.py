#!/usr/bin/env python
"""Times the three Functions of the trainable indirect-illumination path (robir_amd/illum_autograd.py):
`python tools/prof_illum_backward.py [out.md]` -> profiles/illum_backward_times.md.  HIP-event ms, medians after warm-up, at n = 650 surface
points (a 1024-pixel chunk at 65 % hits) and n = 2048, S = 512 directions, 24 lobes: forward and backward of LobeFn (the policy's lobe kernel |
rb_it_lobe_bwd), IntegralFn (the auto-encoder's forward kernels | rb_train_ae_bwd) and SGQueryFn (rb_it_sg_query | rb_it_sg_query_bwd), the
scratch of the lobe backward, the peak allocated memory of one whole step, and -- timed alternately with it -- the same step through
PyTorch-ROCm fp32 autograd of the oracle's formulas (tests/illum_train_oracle.py) on the same GPU.  All values are recorded only: nothing
asserts a speed."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from robir_amd import illum_autograd, nets, ops, synth, training  # noqa: E402
import illum_train_oracle as ito  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "illum_backward_times.md")
dev = torch.device("cuda:0")
S, SIZES = 512, (650, 2048)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def median_ms(*fns, reps=11, warm=3):
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
net = nets.IndirctIllumNetwork(multires=10, dims=[512] * 4, num_lgt_sgs=24)
net.load_state_dict({k[len(ito.PREFIX):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(ito.PREFIX)})
net = training.enable_illumination_training(net.to(dev).train())
lobe_p = [p.detach() for p in illum_autograd.lobe_params(net)]
ae_p = [p.detach() for p in illum_autograd.ae_autograd.linear_params(net.integral_layer)]
P = {k: p.detach() for k, p in net.named_parameters()}
res = {}

for n in SIZES:
    g = torch.Generator(device=dev).manual_seed(n)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    pts, hdr, noise = r(n, 3) * 0.5, torch.full((n, 1), 0.5, device=dev), r(n, 64)
    dirs = torch.nn.functional.normalize(r(n, S, 3), dim=-1)
    g_sgs, g_int = r(n, 24, 7) / n, r(n, 3) / n
    g_rad = r(n, S, 3) * (torch.rand(n, S, 1, device=dev, generator=g) >= 0.4) / (n * S)
    t_rad, t_int = torch.rand(n, S, 3, device=dev, generator=g), torch.rand(n, 3, device=dev, generator=g)
    with torch.no_grad():
        sgs = net._lobes(pts, hdr)
        X = ops.feat_pe10(pts, extra=hdr)
        Xn = ops.axpy(X, noise, 0.02)
        pre = net.integral_layer.run_pass(Xn)
        q = {"lobe_forward_ms": median_ms(lambda: net._lobes(pts, hdr)),
             "lobe_backward_ms": median_ms(lambda: ops.illum_lobe_backward(pts, hdr, lobe_p, g_sgs)),
             "integral_forward_ms": median_ms(lambda: net._integral(X, noise)),
             "integral_backward_ms": median_ms(lambda: ops.ae_backward(Xn, ae_p, g_out=g_int * torch.sign(pre), latent_act=1, sigmoid_out=False,
                                                                       in_dim=64, out_dim=3)),
             "query_forward_ms": median_ms(lambda: ops.sg_query(sgs, dirs)),
             "query_backward_ms": median_ms(lambda: ops.sg_query_backward(sgs, dirs, g_rad))}
        q["lobe_scratch_MiB"] = ops.illum_lobe_backward(pts, hdr, lobe_p, g_sgs)[1]["scratch_bytes"] / 2 ** 20
    mask = torch.ones(n, dtype=torch.bool, device=dev)
    trace = {"sample_dirs": dirs, "indir_mask": g_rad.abs().sum(-1) > 0, "trace_radiance": t_rad, "gt_integral": t_int}

    def hip_step():
        with torch.enable_grad():
            net.zero_grad(set_to_none=True)
            s_, i_ = net(pts, hdr, noise=noise)
            training.radiance_loss({"network_object_mask": mask, "indirect_sgs": s_, "indir_integral": i_}, trace).backward()

    def torch_step():
        with torch.enable_grad():
            lv = {k: v.clone().requires_grad_(True) for k, v in P.items()}
            loss = ito.radiance_loss(ito.lobes_forward(lv, pts, hdr), ito.integral_forward(lv, Xn), trace, mask)
            torch.autograd.grad(loss, list(lv.values()))

    q["hip_step_ms"], q["torch_fp32_step_ms"] = median_ms(hip_step, torch_step, reps=7)
    for name, fn in (("hip", hip_step), ("torch_fp32", torch_step)):
        net.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        q[name + "_peak_extra_MiB"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    def torch_query():
        with torch.enable_grad():
            x = sgs.clone().requires_grad_(True)
            torch.autograd.grad((ito.query(x, dirs) * g_rad).sum(), x)
    q["query_fwd_bwd_ms"], q["torch_fp32_query_fwd_bwd_ms"] = median_ms(
        lambda: (ops.sg_query(sgs, dirs), ops.sg_query_backward(sgs, dirs, g_rad)), torch_query, reps=7)
    res[n] = q
    print(n, json.dumps(q), flush=True)

f = lambda v: f"{v:.3f} ms"
lines = ["# Indirect-illumination training: times (one MI355X, `python tools/prof_illum_backward.py`)", "",
         "HIP events around one call, median of 11 calls (7 for whole steps) after 3 warm-up calls; recorded only, no test asserts a speed.",
         f"S = {S} directions per point, 24 lobes, all gradients wanted, `slab_rows` {ops.ILLUM_SLAB_ROWS}, `part_rows` {ops.ILLUM_PART_ROWS}.  A backward",
         "call includes the allocation of its outputs and scratch from torch's caching allocator.", "",
         "| n | LobeFn forward / backward | lobe scratch | IntegralFn forward / backward | SGQueryFn forward / backward |", "|---|---|---|---|---|"]
for n, q in res.items():
    lines.append(f"| {n} | {f(q['lobe_forward_ms'])} / {f(q['lobe_backward_ms'])} | {q['lobe_scratch_MiB']:.1f} MiB | "
                 f"{f(q['integral_forward_ms'])} / {f(q['integral_backward_ms'])} | {f(q['query_forward_ms'])} / {f(q['query_backward_ms'])} |")
lines += ["", "The whole step (network forward, `radiance_loss` with 60 % of the samples kept, backward to all 26 parameters) against the same step",
          "through PyTorch-ROCm fp32 autograd of the oracle's formulas (`tests/illum_train_oracle.py`), timed alternately, and the query alone",
          "against its PyTorch expansion.  The PyTorch step is fp32 where the kernels are fp64: not the same arithmetic.", "",
          "| n | HIP step | torch fp32 step | HIP peak memory beyond its inputs | torch peak | fused query forward + backward | torch fp32 query forward + backward |",
          "|---|---|---|---|---|---|---|"]
for n, q in res.items():
    lines.append(f"| {n} | {f(q['hip_step_ms'])} | {f(q['torch_fp32_step_ms'])} | {q['hip_peak_extra_MiB']:.1f} MiB | {q['torch_fp32_peak_extra_MiB']:.1f} MiB | "
                 f"{f(q['query_fwd_bwd_ms'])} | {f(q['torch_fp32_query_fwd_bwd_ms'])} |")
slower = [n for n, q in res.items() if q["query_fwd_bwd_ms"] >= q["torch_fp32_query_fwd_bwd_ms"]]
lines += ["", ("The fused query is NOT faster than the PyTorch expansion at n = " + ", ".join(map(str, slower)) + " (S = 512); it is written for "
               "correctness first and was not tuned.") if slower else "The fused query is faster than the PyTorch expansion at both sizes."]
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print(json.dumps(res))
print("wrote", out_path)
