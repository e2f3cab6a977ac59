#!/usr/bin/env python
"""Times the SG shading forward (rb_sg_shade) and its reverse mode (rb_sg_shade_bwd) on one 800 x 800 view's worth of hit points:
`python tools/prof_sg_backward.py [n_points] [--no-torch]` -> HIP-event ms, median of 25 launches after warm-up, for the direct pass
(M = 128, shared light, light visibility) and the indirect pass (M = 24, per-point lights, indirect integral); the peak device memory of
one backward; and, as the comparison a user has today, PyTorch-ROCm fp32 autograd of the oracle's formulas (tests/sg_backward_oracle.py) on
the same GPU at a batch that fits, scaled per point.  Run the same command under `rocprofv3 --kernel-trace --stats` for the second clock."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from robir_amd import ops, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 416000
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
R = lambda *s: torch.rand(*s, device=dev, generator=g)
N = lambda *s: torch.randn(*s, device=dev, generator=g)


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


def inputs(n, M, per_point):
    lgt = torch.from_numpy(synth.synth_light_sgs(3, M, sharp=True)).float().to(dev)
    if per_point:
        lgt = (lgt[None] * (1.0 + 0.3 * N(n, M, 7))).contiguous()
    nrm = torch.nn.functional.normalize(N(n, 3), dim=-1)
    view = torch.nn.functional.normalize(nrm + 0.8 * N(n, 3), dim=-1)
    d = dict(normal=nrm, view=view, lgt=lgt, f0=torch.full((1,), 0.05, device=dev), rough=R(n) * 0.9 + 0.09, albedo=R(n, 3), bvis=R(n))
    d.update(indir_integral=R(n, 3)) if per_point else d.update(light_vis=R(n, M))
    return d, N(n, 3), N(n, 3)


res = {"n": n}
for tag, M, per_point in (("direct_M128_shared", 128, False), ("indirect_M24_per_point", 24, True)):
    a, gs, gd = inputs(n, M, per_point)
    kw = dict(light_vis=a.get("light_vis"), indir_integral=a.get("indir_integral"))
    fwd = lambda: ops.sg_shade(a["normal"], a["view"], a["lgt"], a["f0"], a["rough"], a["albedo"], a["bvis"], want_shadow=True, **kw)
    _, spec, diff, _ = fwd()
    names = ("lgt", "f0", "rough", "albedo", "bvis", "light_vis", "indir_integral")
    bwd = lambda want=names: ops.sg_shade_backward(a["normal"], a["view"], a["lgt"], a["f0"], a["rough"], a["albedo"], a["bvis"], spec, diff, gs,
                                                   gd, want=want, **kw)
    r = {"forward_ms": median_ms(fwd), "backward_all_ms": median_ms(bwd), "backward_light_only_ms": median_ms(lambda: bwd(("lgt",))),
         "backward_no_vis_ms": median_ms(lambda: bwd(("lgt", "f0", "rough", "albedo")))}
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = bwd(("lgt", "f0", "rough", "albedo"))
    torch.cuda.synchronize()
    r["backward_no_vis_peak_extra_MiB"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    r["one_n_x_M_fp32_tensor_MiB"] = n * M * 4 / 2 ** 20
    del out
    res[tag] = r
    print(tag, json.dumps(r))

if "--no-torch" not in sys.argv:
    import sg_backward_oracle as sbo  # noqa: E402
    for tag, M, per_point, nt in (("direct_M128_shared", 128, False, 32768), ("indirect_M24_per_point", 24, True, 131072)):
        a, gs, gd = inputs(nt, M, per_point)
        leaves = [k for k in ("lgt", "f0", "rough", "albedo", "bvis", "light_vis", "indir_integral") if k in a]

        def step():
            with torch.enable_grad():
                L = {k: (v.clone().requires_grad_(True) if k in leaves else v) for k, v in a.items()}
                s, d = sbo.shade(L["normal"], L["view"], L["lgt"], L["f0"], L["rough"], L["albedo"], L["bvis"], light_vis=L.get("light_vis"),
                                 indir_integral=L.get("indir_integral"))
                torch.autograd.grad((s * gs).sum() + (d * gd).sum(), [L[k] for k in leaves])
        torch.cuda.reset_peak_memory_stats()
        ms = median_ms(step, reps=20, warm=2)
        r = {"torch_autograd_n": nt, "torch_autograd_fwd_bwd_ms": ms, "torch_autograd_us_per_point": 1e3 * ms / nt,
             "torch_autograd_scaled_to_n_ms": ms * n / nt, "torch_autograd_peak_MiB": torch.cuda.max_memory_allocated() / 2 ** 20,
             "hip_fwd_bwd_us_per_point": 1e3 * (res[tag]["forward_ms"] + res[tag]["backward_all_ms"]) / n}
        res[tag].update(r)
        print(tag, json.dumps(r))
print(json.dumps(res))
