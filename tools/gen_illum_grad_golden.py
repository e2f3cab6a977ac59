"""Gradient fixture of the indirect-illumination network: tests/golden/illum_grad.npz.

Runs the REFERENCE's own IndirctIllumNetwork (model/implicit_differentiable_renderer.py:170-222) and query_indir_illum
(model/loss.py:128-141) on the CPU in float64 with autograd, on 16 points x 8 directions of the synthetic state dict (robir_amd.synth: seed 0)
with pinned points, hdr shift, directions, targets and mask; the auto-encoder's torch.randn draw is replaced for the one call by the stored
tensor.  The loss is the radiance term of IllumLoss.forward (model/loss.py:156-171, nn.L1Loss) with every point a surface point.  Stored (data
only): the inputs that robir_amd.synth does not give, the loss, every bias gradient, and for each weight gradient its first 8 rows, first 8
columns, sum and Frobenius norm.  In the same run the oracle (tests/illum_train_oracle.py, float64) is pinned against each of these and the
distance is printed and stored: the GPU tests differentiate the oracle where the reference is not available.

    python tools/gen_illum_grad_golden.py          (needs the reference tree; see oracle/ref_shim.py)
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
import model.implicit_differentiable_renderer as ridr  # noqa: E402
import model.loss as rloss  # noqa: E402
import illum_train_oracle as ito  # noqa: E402
from robir_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
N, S, ANNEAL_T = 16, 8, 0.125


def rel_err(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return float(((a - b).abs() / (b.abs() + b.abs().mean() + 1e-30)).max())


def summary(g):
    """What is stored of one gradient tensor."""
    g = torch.as_tensor(g).double()
    if g.dim() == 1:
        return {"full": g}
    return {"rows8": g[:8].clone(), "cols8": g[:, :8].clone(), "sum": g.sum(), "fro": g.norm()}


def main():
    sd = synth.synth_state_dict(0, variance=0.3)
    params = ito.illum_params({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    g = np.random.default_rng(2626)
    pts = (g.standard_normal((N, 3)) * 0.5).astype(np.float32)
    hdr = g.uniform(0.0, 1.0, (N, 1)).astype(np.float32)
    noise = g.standard_normal((N, 64)).astype(np.float32)
    dirs = g.standard_normal((N, S, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    indir_mask = g.uniform(size=(N, S)) < 0.6
    trace_radiance = g.uniform(0.0, 1.0, (N, S, 3)).astype(np.float32)
    gt_integral = g.uniform(0.0, 1.0, (N, 3)).astype(np.float32)
    T = torch.from_numpy
    l1 = torch.nn.L1Loss(reduction="mean")
    with ref_shim.CpuMode():
        net = ridr.IndirctIllumNetwork(multires=10, dims=[512] * 4, num_lgt_sgs=24).double()
        net.load_state_dict({k: v.double() for k, v in params.items()})
        real_randn = torch.randn
        torch.randn = lambda *a, **k: T(noise).double()
        try:
            sgs, env_int = net(T(pts).double(), T(hdr).double())
        finally:
            torch.randn = real_randn
        pred = rloss.query_indir_illum(sgs, T(dirs).double())
    mask = T(indir_mask)
    loss = l1(T(trace_radiance).double()[mask] + ANNEAL_T, pred[mask]) + l1(T(gt_integral).double(), env_int)
    named = dict(net.named_parameters())
    ref = dict(zip(ito.NAMES, torch.autograd.grad(loss, [named[k] for k in ito.NAMES])))
    trace = {"sample_dirs": T(dirs), "indir_mask": mask, "trace_radiance": T(trace_radiance), "gt_integral": T(gt_integral)}
    every = torch.ones(N, dtype=torch.bool)

    def oracle_loss(lv):
        o_sgs, o_int = ito.both_forward(lv, T(pts), T(hdr), T(noise))
        return ito.radiance_loss(o_sgs, o_int, trace, every, ANNEAL_T, "L1")
    ol, og = ito.grads_of(oracle_loss, params, torch.float64)
    o_sgs, o_int = ito.both_forward({k: v.double() for k, v in params.items()}, T(pts), T(hdr), T(noise))
    print(f"forward oracle-vs-reference: sgs {rel_err(o_sgs, sgs):.2e} env_int {rel_err(o_int, env_int):.2e} "
          f"query {rel_err(ito.query(o_sgs, T(dirs)), pred):.2e} loss {abs(ol - float(loss)):.2e}")
    print(f"lobe amplitudes > 0: {100 * float((sgs[..., 4:] > 0).double().mean()):.0f} %   lambda {float(sgs[..., 3].min()):.2f} .. "
          f"{float(sgs[..., 3].max()):.2f}   samples kept {100 * indir_mask.mean():.0f} %")
    store = {"points": pts, "hdr_shift": hdr, "noise": noise, "sample_dirs": dirs, "indir_mask": indir_mask, "trace_radiance": trace_radiance,
             "gt_integral": gt_integral, "anneal_t": np.float64(ANNEAL_T), "loss": np.float64(float(loss))}
    for k in ito.NAMES:
        for part, v in summary(ref[k]).items():
            dist = rel_err(summary(og[k])[part], v)
            store[f"grad.{k}.{part}"] = v.numpy().astype(np.float64)
            store[f"oracle_dist.{k}.{part}"] = np.float64(dist)
            print(f"    d {k:46s} {part:6s} max|ref64| {float(v.abs().max()):.4e}   oracle64 vs reference64 rel_err {dist:.2e}")
    path = os.path.join(GOLD, "illum_grad.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
