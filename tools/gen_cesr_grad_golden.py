"""Gradient fixture of the CESR networks: tests/golden/cesr_grad.npz (shadow_net) and tests/golden/cesr_grad_normal.npz (normal_net) -- one
layout, two files: together the float64 pieces are 1.13 MB, more than a committed file may hold.

Runs the REFERENCE's own SDFNetwork (model/neus_model.py:312-417) in both CESR shapes -- shadow_net = SDFNetwork(63 + 128, 2, 512, 8, [4], 0),
normal_net = SDFNetwork(63, 3, 512, 8, [4], 0) (training/train_cesr.py:107-110) -- on the CPU in float64 with autograd, on the synthetic
weights (robir_amd.synth.synth_cesr_nets(0)) with pinned inputs: shadow 2 points x 4 labels as dense one-hot rows, normal 8 rows; the loss is
<g, output> with a pinned random g.  Stored (data only): the inputs, the outputs, every bias and weight_g gradient in full, and for each
weight_v gradient its first 8 rows, first 8 columns, sum and Frobenius norm.  In the same run the oracle (tests/cesr_train_oracle.py, float64)
is pinned against each of these and the distance is printed and stored: the GPU tests differentiate the oracle where the reference is not
available.

    python tools/gen_cesr_grad_golden.py          (needs the reference tree; see oracle/ref_shim.py)
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
import model.neus_model as rneus  # noqa: E402
import cesr_train_oracle as cto  # noqa: E402
from robir_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def rel_err(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return float(((a - b).abs() / (b.abs() + b.abs().mean() + 1e-30)).max())


def summary(name, g):
    """What is stored of one gradient tensor."""
    g = torch.as_tensor(g).double()
    if not name.endswith("weight_v"):
        return {"full": g}
    return {"rows8": g[:8].clone(), "cols8": g[:, :8].clone(), "sum": g.sum(), "fro": g.norm()}


def main():
    rng = np.random.default_rng(2727)
    nets = synth.synth_cesr_nets(0)
    T = torch.from_numpy
    for kind, name, n_pts, n_label in (("shadow", "shadow_net", 2, 4), ("normal", "normal_net", 8, 1)):
        d_in, d_out = cto.DIMS[kind]
        params = cto.cesr_params({k: T(np.asarray(v)) for k, v in nets[name].items()})
        pts = (rng.standard_normal((n_pts, 3)) * 0.5).astype(np.float32)
        rows = cto.rows_of_points(T(pts), n_label, kind, torch.float32).numpy().astype(np.float32)      # dense fp32 rows, one-hot included
        g = rng.standard_normal((rows.shape[0], d_out)).astype(np.float32)
        with ref_shim.CpuMode():
            net = rneus.SDFNetwork(d_in, d_out, 512, 8, [4], 0).double()
            net.load_state_dict({k: v.double() for k, v in params.items()})
            out = net(T(rows).double())
        loss = (out * T(g).double()).sum()
        named = dict(net.named_parameters())
        ref = dict(zip(cto.NAMES, torch.autograd.grad(loss, [named[k] for k in cto.NAMES])))
        og = cto.grads(params, T(rows), kind, T(g), torch.float64)
        o_out = cto.forward({k: v.double() for k, v in params.items()}, T(rows), kind)
        print(f"{name}: forward oracle-vs-reference {rel_err(o_out, out):.2e}   |out| max {float(out.detach().abs().max()):.3f}")
        store = {}
        store.update({f"{kind}.points": pts, f"{kind}.n_label": np.int64(n_label), f"{kind}.rows": rows, f"{kind}.g_out": g,
                      f"{kind}.out": out.detach().numpy(), f"{kind}.loss": np.float64(float(loss))})
        for k in cto.NAMES:
            for part, v in summary(k, ref[k]).items():
                dist = rel_err(summary(k, og[k])[part], v)
                store[f"{kind}.grad.{k}.{part}"] = v.numpy().astype(np.float64)
                store[f"{kind}.oracle_dist.{k}.{part}"] = np.float64(dist)
                print(f"    d {k:18s} {part:6s} max|ref64| {float(v.abs().max()):.4e}   oracle64 vs reference64 rel_err {dist:.2e}")
        path = os.path.join(GOLD, "cesr_grad.npz" if kind == "shadow" else "cesr_grad_normal.npz")
        np.savez_compressed(path, **store)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
