#!/usr/bin/env python
"""Times the spec auto-encoder's forward (the policy's forward kernels) and its reverse mode (rb_train_ae_bwd):
`python tools/prof_material_backward.py [out.md] [--no-torch]` -> profiles/material_backward_times.md.  HIP-event ms, median of 25 after
warm-up, at n = 2048 and n = 65536, with all sixteen gradients and with the decoder's six only; the scratch of one backward; and, as the
comparison a user has without the kernel, the same step through PyTorch-ROCm fp32 autograd of the oracle's formulas
(tests/material_train_oracle.py) on the same GPU.  All values are recorded only: nothing asserts a speed."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from robir_amd import nets, ops, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "material_backward_times.md")
dev = torch.device("cuda:0")
MAT = "envmap_material_network."


def median_ms(fn, reps=25, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


sd = synth.synth_state_dict(0, variance=0.3)
net = nets.EnvmapMaterialNetwork(multires=10, num_lgt_sgs=128, specular_albedo=0.05)
net.load_state_dict({k[len(MAT):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(MAT)})
ae = net.to(dev).eval().spec_brdf_encoder_layer
params = [p.detach() for p in (t for i in range(5) for t in (ae.brdf_encoder_layer[2 * i].weight, ae.brdf_encoder_layer[2 * i].bias))] \
    + [p.detach() for p in (t for i in range(3) for t in (ae.brdf_decoder_layer[2 * i].weight, ae.brdf_decoder_layer[2 * i].bias))]
DEC = tuple(k for k in ops.AE_PARAM_NAMES if k.startswith("brdf_decoder_layer."))
res = {}
with torch.no_grad():
    for n in (2048, 65536):
        g = torch.Generator(device=dev).manual_seed(n)
        pts = torch.randn(n, 3, device=dev, generator=g) * 0.5
        noise = torch.randn(n, 32, device=dev, generator=g)
        go, gx, gr = (torch.randn(n, c, device=dev, generator=g) for c in (5, 5, 32))
        X = ops.feat_pe10(pts)
        bwd = lambda want=ops.AE_PARAM_NAMES: ops.ae_backward(X, params, go, gx, gr, noise=noise, want=want)
        r = {"forward_ms": median_ms(lambda: ae.run_points(pts, noise)), "backward_all_ms": median_ms(bwd),
             "backward_decoder_only_ms": median_ms(lambda: bwd(DEC))}
        _, st = bwd()
        _, st_dec = bwd(DEC)
        r.update(scratch_MiB=st["scratch_bytes"] / 2 ** 20, launches_all=st["launches"], launches_decoder_only=st_dec["launches"])
        res[n] = r
        print(n, json.dumps(r))

if "--no-torch" not in sys.argv:
    import material_train_oracle as mto  # noqa: E402
    P = {k: p.clone() for k, p in zip(mto.NAMES, params)}
    for n in (2048, 65536):
        g = torch.Generator(device=dev).manual_seed(n)
        pts = torch.randn(n, 3, device=dev, generator=g) * 0.5
        noise = torch.randn(n, 32, device=dev, generator=g)
        go, gx, gr = (torch.randn(n, c, device=dev, generator=g) for c in (5, 5, 32))
        X = ops.feat_pe10(pts)

        def step(names=mto.NAMES):
            with torch.enable_grad():
                L = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in P.items()}
                x = X[:, :63]
                sdd = {"ae." + k: v for k, v in L.items()}
                o, ox = mto.on.sparse_ae(sdd, "ae", x, noise, True, torch.sigmoid, torch.sigmoid, var=torch.zeros(32, device=dev))
                raw = mto.on._seq(sdd, "ae.brdf_encoder_layer.", 5, x, lambda t: torch.nn.functional.leaky_relu(t, 0.2))
                torch.autograd.grad((o * go).sum() + (ox * gx).sum() + (raw * gr).sum(), [L[k] for k in names])
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res[n]["torch_fp32_fwd_bwd_all_ms"] = median_ms(step, reps=25, warm=3)
        res[n]["torch_fp32_peak_extra_MiB"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        res[n]["torch_fp32_fwd_bwd_decoder_only_ms"] = median_ms(lambda: step(DEC), reps=25, warm=3)
        print(n, json.dumps(res[n]))

f = lambda v, u="": "-" if v is None else f"{v:.3f}{u}"
lines = ["# Spec auto-encoder backward: times (one MI355X, `python tools/prof_material_backward.py`)", "",
         "HIP events, median of 25 launches after 3 warm-up launches; recorded only, no test asserts a speed.  Forward: the default policy's forward",
         "kernels (`SparseAE.run_points`).  Backward: `rb_train_ae_bwd`, fp64 on `v_mfma_f64_16x16x4_f64`, default `slab_rows` 16384.", "",
         "| n | forward | backward, all 16 gradients | backward, decoder's 6 only | scratch of one backward | kernels enqueued (all / decoder only) |",
         "|---|---|---|---|---|---|"]
for n, r in res.items():
    lines.append(f"| {n} | {f(r['forward_ms'], ' ms')} | {f(r['backward_all_ms'], ' ms')} | {f(r['backward_decoder_only_ms'], ' ms')} | "
                 f"{r['scratch_MiB']:.1f} MiB | {r['launches_all']} / {r['launches_decoder_only']} |")
if "--no-torch" not in sys.argv:
    lines += ["", "Comparison -- the same step (forward + backward) through PyTorch-ROCm fp32 autograd of the oracle's formulas",
              "(`tests/material_train_oracle.py`), same GPU, median of 25.  It is fp32 where the kernel is fp64: not the same arithmetic.", "",
              "| n | torch fp32 forward + backward, all | torch fp32, decoder only | torch peak memory beyond its inputs | HIP forward + backward, all |",
              "|---|---|---|---|---|"]
    for n, r in res.items():
        lines.append(f"| {n} | {f(r['torch_fp32_fwd_bwd_all_ms'], ' ms')} | {f(r['torch_fp32_fwd_bwd_decoder_only_ms'], ' ms')} | "
                     f"{r['torch_fp32_peak_extra_MiB']:.1f} MiB | {f(r['forward_ms'] + r['backward_all_ms'], ' ms')} |")
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print(json.dumps(res))
print("wrote", out_path)
