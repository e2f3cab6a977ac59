#!/usr/bin/env python
"""Times the trainable CESR networks (robir_amd/cesr_autograd.py): `python tools/prof_cesr_backward.py [out.md]` ->
profiles/cesr_backward_times.md.  HIP-event ms, median of 11 calls after 3 warm-up calls.  Rows: shadow_net at n = 64 and n = 940 points x 128
labels (a 1024-pixel chunk sends about 940 x 128 = 120 000 rows through it) and normal_net at n = 940.  Per row: the forward (the policy's
kernel plus the head), the backward (rb_ct_cesr_bwd), its scratch, the achieved fp64 TFLOP/s of the backward, and -- timed alternately --
forward + backward through the Function against PyTorch-ROCm fp32 autograd of the oracle's softplus_net512 on the expanded rows, with peak
memory.  Then the (slab_rows, part_rows) candidates of ops.CESR_SLAB_ROWS / CESR_PART_ROWS on the 120 000-row case, and the whole CESRHook
step (forward, L1 image loss + gradient_error, backward to both networks) on the hit points of one synthetic 1024-pixel chunk.  All values
are recorded only: nothing asserts a speed."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from robir_amd import cesr_autograd, nets, ops, renderer, synth, training  # noqa: E402
import cesr_train_oracle as cto  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "cesr_backward_times.md")
dev = torch.device("cuda:0")
FP64_MATRIX_PEAK_TF = 78.6          # AMD's published peak FP64 matrix rate of the MI355X
CANDIDATES = ((4096, 512), (16384, 1024), (16384, 2048))


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


def backward_flop(kind, M):
    """fp64 FLOP of one rb_ct_cesr_bwd call with every gradient wanted: the recomputed forward, dZ and dW | db (2 per multiply-add)."""
    d_in, d_out = cto.DIMS[kind]
    n_out = [512, 512, 512, 512 - d_in, 512, 512, 512, 512, d_out]
    k_in = [d_in] + [512] * 8
    fwd = sum(n * k for n, k in zip(n_out, k_in))
    dz = sum(n_out[l] * n_out[l - 1] for l in range(1, 9))
    dw = sum(n * (k + 1) for n, k in zip(n_out, k_in))
    return 2.0 * M * (fwd + dz + dw)


def peak_extra_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def make_net(kind):
    net = nets.SDFNetwork(191, 2, 512, 8, [4], 0) if kind == "shadow" else nets.SDFNetwork(63, 3, 512, 8, [4], 0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_cesr_nets(0)[kind + "_net"].items()})
    return training.enable_cesr_training(net.to(dev).train())


NETS = {k: make_net(k) for k in ("shadow", "normal")}
res, cand = {}, {}
for kind, n, n_label, head in (("shadow", 64, 128, 1), ("shadow", 940, 128, 1), ("normal", 940, 1, 2)):
    net = NETS[kind]
    M = n * n_label
    g = torch.Generator(device=dev).manual_seed(n)
    pts = torch.randn(n, 3, device=dev, generator=g) * 0.5
    g_out = torch.randn(*((M,) if head == 1 else (M, 3)), device=dev, generator=g) / M
    params = [p.detach() for p in cesr_autograd.cesr_params(net)]
    P = {k: p.detach() for k, p in zip(cto.NAMES, params)}
    fwd = (lambda: net.diffuse_vis(pts, n_label)) if kind == "shadow" else (lambda: net.unit_normal(pts))
    bwd = lambda **kw: ops.cesr_backward(pts, M, kind, params, g_out, head=head, n_label=n_label, **kw)
    with torch.no_grad():
        q = {"rows": M, "forward_ms": median_ms(fwd), "backward_ms": median_ms(bwd)}
        q["scratch_MiB"] = bwd()[1]["scratch_bytes"] / 2 ** 20
    q["backward_fp64_tflops"] = backward_flop(kind, M) / (q["backward_ms"] * 1e-3) / 1e12
    q["fraction_of_fp64_matrix_peak"] = q["backward_fp64_tflops"] / FP64_MATRIX_PEAK_TF
    rows32 = cto.rows_of_points(pts.cpu(), n_label, kind, torch.float32).to(dev)          # the expanded rows PyTorch differentiates through

    def hip_step():
        with torch.enable_grad():
            net.zero_grad(set_to_none=True)
            (fwd() * g_out).sum().backward()

    def torch_step():
        with torch.enable_grad():
            lv = {k: v.clone().requires_grad_(True) for k, v in P.items()}
            torch.autograd.grad((cto.forward(lv, rows32, kind, 1, head) * g_out).sum(), list(lv.values()))

    q["hip_step_ms"], q["torch_fp32_step_ms"] = median_ms(hip_step, torch_step)
    q["hip_peak_extra_MiB"], q["torch_fp32_peak_extra_MiB"] = peak_extra_mib(hip_step), peak_extra_mib(torch_step)
    net.zero_grad(set_to_none=True)
    res[f"{kind}_net n = {n} x {n_label}"] = q
    print(kind, n, json.dumps(q), flush=True)
    if kind == "shadow" and n == 940:
        with torch.no_grad():
            for slab, part in CANDIDATES:
                cand[(slab, part)] = (median_ms(lambda: bwd(slab_rows=slab, part_rows=part)), bwd(slab_rows=slab, part_rows=part)[1]["scratch_bytes"] / 2 ** 20)
                print("candidate", slab, part, cand[(slab, part)], flush=True)

# the whole hook step on one synthetic 1024-pixel chunk
model = renderer.build_synthetic_model(dev, seed=0, variance=0.3).eval()
model.deferred_chunks = 0
uv, pose, K = synth.synth_camera(64, 64)
inp = {"uv": torch.from_numpy(uv[1024:2048]).to(dev)[None], "pose": torch.from_numpy(pose).to(dev)[None], "intrinsics": torch.from_numpy(K).to(dev)[None],
       "object_mask": torch.ones(1, 1024, dtype=torch.bool, device=dev), "hdr_shift": torch.full((1024, 1), 0.5, device=dev)}
model.get_sg_render = renderer.CESRHook(model, NETS["shadow"], NETS["normal"], is_training=True, cur_iter=2000, prefit="explore")
with torch.no_grad():
    out0 = model(inp, trainstage="Material", lin_diff=True, train_spec=True)
hit = out0["network_object_mask"]
target = out0["sg_rgb"][hit] * 0.7 + 0.05


def hook_step():
    with torch.enable_grad():
        for net in NETS.values():
            net.zero_grad(set_to_none=True)
        out = model(inp, trainstage="Material", lin_diff=True, train_spec=True)
        ((out["sg_rgb"][hit] - target).abs().mean() + out["gradient_error"]).backward()


def hook_forward():
    with torch.no_grad():
        model(inp, trainstage="Material", lin_diff=True, train_spec=True)


hook = {"hit_points": int(hit.sum()), "forward_only_ms": median_ms(hook_forward), "step_ms": median_ms(hook_step)}
hook["step_peak_extra_MiB"] = peak_extra_mib(hook_step)
print("hook", json.dumps(hook), flush=True)

f = lambda v: f"{v:.3f} ms"
lines = ["# CESR-network training: times (one MI355X, `python tools/prof_cesr_backward.py`)", "",
         "HIP events around one call, median of 11 calls after 3 warm-up calls; recorded only, no test asserts a speed.  All gradients wanted,",
         f"`slab_rows` {ops.CESR_SLAB_ROWS}, `part_rows` {ops.CESR_PART_ROWS}.  A backward call includes the allocation of its outputs and scratch from",
         "torch's caching allocator.  fp64 TFLOP/s: the call's multiply-adds (recomputed forward, dZ, dW | db) x 2 over its time, against",
         f"AMD's published peak FP64 matrix rate of the MI355X, {FP64_MATRIX_PEAK_TF} TFLOP/s: what `k_gemm64` achieves as it stands (untuned; the weight-norm",
         "fold, the encoding and the reductions are inside the time).", "",
         "| network, points x labels | rows | forward (head included) | backward | scratch | backward fp64 TFLOP/s | of the fp64 matrix peak |", "|---|---|---|---|---|---|---|"]
for name, q in res.items():
    lines.append(f"| {name} | {q['rows']} | {f(q['forward_ms'])} | {f(q['backward_ms'])} | {q['scratch_MiB']:.1f} MiB | {q['backward_fp64_tflops']:.2f} | "
                 f"{100 * q['fraction_of_fp64_matrix_peak']:.1f} % |")
lines += ["", "Forward + backward through the Function (`<g, head(net)>`, all 27 gradients) against the same step through PyTorch-ROCm fp32 autograd of",
          "the oracle's `softplus_net512` (`tests/cesr_train_oracle.py`) on the expanded `[n x labels, 191]` rows, timed alternately.  The PyTorch step",
          "is fp32 where the kernels are fp64: not the same arithmetic.", "",
          "| network, points x labels | HIP step | torch fp32 step | HIP peak memory beyond its inputs | torch peak |", "|---|---|---|---|---|"]
for name, q in res.items():
    lines.append(f"| {name} | {f(q['hip_step_ms'])} | {f(q['torch_fp32_step_ms'])} | {q['hip_peak_extra_MiB']:.1f} MiB | {q['torch_fp32_peak_extra_MiB']:.1f} MiB |")
slower = [name for name, q in res.items() if q["hip_step_ms"] >= q["torch_fp32_step_ms"]]
lines += ["", ("The PyTorch fp32 step is FASTER than the HIP step at: " + "; ".join(slower) + ".  The HIP backward is fp64 on an untuned engine; what it "
               "buys is the memory column and the accuracy (DESIGN 4.7).") if slower else "The HIP step is faster than the PyTorch fp32 step at every size.",
          "", "The `(slab_rows, part_rows)` candidates on shadow_net, 940 x 128 rows (the backward alone):", "",
          "| slab_rows | part_rows | backward | scratch |", "|---|---|---|---|"]
for (slab, part), (ms, mib) in cand.items():
    lines.append(f"| {slab} | {part} | {f(ms)} | {mib:.1f} MiB |")
lines += ["", f"The whole CESRHook step on one synthetic 1024-pixel chunk ({hook['hit_points']} hit points x 128 labels through shadow_net, model in `eval()`, both",
          "networks marked and in `train()`, loss = L1 image term + `gradient_error`, backward to all 54 tensors):", "",
          "| chunk forward, forward-only | chunk forward + loss + backward | peak memory of the step beyond its inputs |", "|---|---|---|",
          f"| {f(hook['forward_only_ms'])} | {f(hook['step_ms'])} | {hook['step_peak_extra_MiB']:.1f} MiB |"]
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print(json.dumps({"rows": res, "candidates": {f"{s}x{p}": v for (s, p), v in cand.items()}, "hook": hook}))
print("wrote", out_path)
