"""Gradient fixture of the spec auto-encoder: tests/golden/ae_grad.npz.

Runs the REFERENCE's own SparseAE (model/sg_envmap_material.py:40-99) on the CPU in float64 with autograd, on 32 rows of the synthetic state
dict (robir_amd.synth: seed 0) with pinned latent noise: the module's torch.randn draw is replaced for the one call by the stored tensor.
The loss is <g_out, out> + <g_out_xi, out_xi> + <g_raw, encode(x)> with seeded random upstream gradients.  Stored (data only): the inputs
that robir_amd.synth does not give (points, noise, upstream gradients), every bias gradient, and for each weight gradient its first 8 rows,
first 8 columns, sum and Frobenius norm.  In the same run the oracle (tests/material_train_oracle.py, float64) is pinned against each of these
and the distance is printed and stored: the GPU tests differentiate the oracle where the reference is not available.

    python tools/gen_material_grad_golden.py          (needs the reference tree; see oracle/ref_shim.py)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import ref_shim  # noqa: E402

ref_shim.install()
import model.sg_envmap_material as rmat  # noqa: E402
import material_train_oracle as mto  # noqa: E402
from robir_amd import synth  # noqa: E402
from robir_oracle.encoding import pe  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
N = 32


def rel_err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float(((a - b).abs() / (b.abs() + b.abs().mean() + 1e-30)).max())


def summary(g):
    """What is stored of one gradient tensor."""
    g = torch.as_tensor(g).double()
    if g.dim() == 1:
        return {"full": g}
    return {"rows8": g[:8].clone(), "cols8": g[:, :8].clone(), "sum": g.sum(), "fro": g.norm()}


def main():
    sd = synth.synth_state_dict(0, variance=0.3)
    params = mto.ae_params({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    g = np.random.default_rng(4242)
    pts = (g.standard_normal((N, 3)) * 0.5).astype(np.float32)
    noise = g.standard_normal((N, 32)).astype(np.float32)
    ups = {"g_out": g.standard_normal((N, 5)).astype(np.float32), "g_out_xi": g.standard_normal((N, 5)).astype(np.float32),
           "g_raw": g.standard_normal((N, 32)).astype(np.float32)}
    x32 = pe(torch.from_numpy(pts), 10)                      # the fp32 feature rows: what the float64 evaluations are fed
    X = torch.zeros(N, 64)
    X[:, :63] = x32
    with ref_shim.CpuMode():
        ae = rmat.SparseAE(63, 5, high_lr=True).double()
        ae.var = torch.zeros(32, dtype=torch.float64)
        ae.load_state_dict({k: v.double() for k, v in params.items()})
        real_randn = torch.randn
        torch.randn = lambda *a, **k: torch.from_numpy(noise).double()
        try:
            out, out_xi = ae(x32.double())
        finally:
            torch.randn = real_randn
        raw = ae.encode(x32.double())
    f64 = lambda a: torch.from_numpy(a).double()
    loss = (out * f64(ups["g_out"])).sum() + (out_xi * f64(ups["g_out_xi"])).sum() + (raw * f64(ups["g_raw"])).sum()
    named = dict(ae.named_parameters())
    ref = dict(zip(mto.NAMES, torch.autograd.grad(loss, [named[k] for k in mto.NAMES])))
    og = mto.ae_grads(params, X, torch.from_numpy(noise), f64(ups["g_out"]), f64(ups["g_out_xi"]), f64(ups["g_raw"]), torch.float64)
    oo, oxi, oraw = mto.ae_forward({k: v.double() for k, v in params.items()}, X, torch.from_numpy(noise))
    print(f"forward oracle-vs-reference: out {rel_err(oo, out):.2e} out_xi {rel_err(oxi, out_xi):.2e} raw {rel_err(oraw, raw):.2e}")
    store = {"points": pts, "noise": noise, **ups}
    for k in mto.NAMES:
        for part, v in summary(ref[k]).items():
            dist = rel_err(summary(og[k])[part], v)
            store[f"grad.{k}.{part}"] = v.numpy().astype(np.float64)
            store[f"oracle_dist.{k}.{part}"] = np.float64(dist)
            print(f"    d {k:32s} {part:6s} max|ref64| {float(v.abs().max()):.4e}   oracle64 vs reference64 rel_err {dist:.2e}")
    path = os.path.join(GOLD, "ae_grad.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
