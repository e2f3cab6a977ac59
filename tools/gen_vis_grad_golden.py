"""Gradient fixture of the visibility network: tests/golden/vis_grad.npz.

Runs the REFERENCE's own VisNetwork (model/implicit_differentiable_renderer.py:225-258) on the CPU in float64 with autograd, on 32 rows
(8 points x 4 directions each) of the synthetic state dict (robir_amd.synth: seed 0) with pinned points, directions and labels.  The loss is
nn.CrossEntropyLoss() of the logits against the labels.  Stored (data only): the inputs that robir_amd.synth does not give (points, directions,
labels), every bias gradient, and for each weight gradient its first 8 rows, first 8 columns, sum and Frobenius norm.  In the same run the
oracle (tests/vis_train_oracle.py, float64) is pinned against each of these and the distance is printed and stored: the GPU tests differentiate
the oracle where the reference is not available.

    python tools/gen_vis_grad_golden.py          (needs the reference tree; see oracle/ref_shim.py)
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
import vis_train_oracle as vto  # noqa: E402
from robir_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
N_POINTS, REP = 8, 4


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
    params = vto.vis_params({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    g = np.random.default_rng(2424)
    pts = (g.standard_normal((N_POINTS, 3)) * 0.5).astype(np.float32)
    dirs = g.standard_normal((N_POINTS * REP, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    labels = g.integers(0, 2, N_POINTS * REP).astype(np.int64)
    tp, td, tl = torch.from_numpy(pts), torch.from_numpy(dirs), torch.from_numpy(labels)
    with ref_shim.CpuMode():
        net = ridr.VisNetwork(points_multires=10, dirs_multires=10, dims=[256] * 4).double()
        net.load_state_dict({k: v.double() for k, v in params.items()})
        logits = net(tp.double().repeat_interleave(REP, 0), td.double())
    loss = torch.nn.CrossEntropyLoss()(logits, tl)
    named = dict(net.named_parameters())
    ref = dict(zip(vto.NAMES, torch.autograd.grad(loss, [named[k] for k in vto.NAMES])))
    ol, og = vto.loss_grads(params, tp, td, lambda y: torch.nn.CrossEntropyLoss()(y, tl), rep=REP, dtype=torch.float64)
    oy = vto.vis_forward({k: v.double() for k, v in params.items()}, tp, td, REP)
    print(f"forward oracle-vs-reference: logits {rel_err(oy, logits):.2e}  loss {abs(ol - float(loss)):.2e}")
    store = {"points": pts, "dirs": dirs, "labels": labels, "rep": np.int64(REP), "loss": np.float64(float(loss))}
    for k in vto.NAMES:
        for part, v in summary(ref[k]).items():
            dist = rel_err(summary(og[k])[part], v)
            store[f"grad.{k}.{part}"] = v.numpy().astype(np.float64)
            store[f"oracle_dist.{k}.{part}"] = np.float64(dist)
            print(f"    d {k:24s} {part:6s} max|ref64| {float(v.abs().max()):.4e}   oracle64 vs reference64 rel_err {dist:.2e}")
    path = os.path.join(GOLD, "vis_grad.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
