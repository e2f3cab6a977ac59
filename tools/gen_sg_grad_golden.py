"""Gradient fixtures of the SG shading: tests/golden/sg_grad_{init,sharp}.npz.

Runs the REFERENCE's model.sg_render.render_with_sg on the CPU in float64 with autograd, on the inputs already stored in
tests/golden/sg_{init,sharp}.npz.  The reference module's get_diffuse_visibility / get_specular_visibility are replaced at run time by stubs
that return recorded leaf tensors (seeded uniform values in [0,1] with exact 0 and 1 among them), so the visibilities are inputs, their
gradients are recorded too, and no visibility network or random draw is involved.  The upstream gradients are seeded random [n,3] tensors.
Stored per case (data only): the inputs the existing files do not hold, the upstream gradients, the float64 gradients.  In the same run the
oracle (tests/sg_backward_oracle.py = robir_oracle.sg with the visibilities injected, float64) is pinned against those gradients and the
distance is printed and stored: the GPU tests differentiate the oracle where the reference is not available.

    python tools/gen_sg_grad_golden.py          (needs the reference tree; see oracle/ref_shim.py)
"""
import json
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
import model.sg_render as rsg  # noqa: E402
import sg_backward_oracle as sbo  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
# name -> (light, comp_vis, indir_integral given, lin_diff, metallic given)
CASES = {
    "direct": ("shared", True, False, False, False),
    "direct_lin_met": ("shared", True, False, True, True),
    "indirect": ("per_point", False, True, False, False),
    "indirect_lin_met": ("per_point", False, True, True, True),
    "indirect_sg_diffuse": ("per_point", False, False, False, True),      # comp_vis=False without the integral: the SG diffuse sum is live
    "clamped": ("away", True, False, False, False),                       # per-point lights, half of the points lit from below the horizon
}


def rel_err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float(((a - b).abs() / (b.abs() + b.abs().mean() + 1e-30)).max())


def reference_grads(d, case, vis, g_spec, g_diff):
    light, comp_vis, with_int, lin_diff, with_met = CASES[case]
    f64 = lambda a: torch.from_numpy(np.asarray(a)).double()
    n = d["normal"].shape[0]
    leaves = {"lgt": f64(vis["lgt"]), "f0": f64(d["f0"]), "rough": f64(d["roughness"]), "albedo": f64(d["albedo"]), "bvis": f64(vis["bvis"])}
    if comp_vis:
        leaves["light_vis"] = f64(vis["light_vis"])
    if with_met:
        leaves["metallic"] = f64(vis["metallic"]).reshape(n, 1)
    if with_int:
        leaves["indir_integral"] = f64(d["indir_int"])
    leaves = {k: v.requires_grad_(True) for k, v in leaves.items()}
    lgt = leaves["lgt"]
    lgt_in = lgt.unsqueeze(0).expand(n, lgt.shape[0], 7) if lgt.dim() == 2 else lgt
    rsg.get_diffuse_visibility = lambda *a, **k: leaves["light_vis"].t()            # the reference expects [M, n]
    rsg.get_specular_visibility = lambda *a, **k: leaves["bvis"]
    with ref_shim.CpuMode():
        out = rsg.render_with_sg(f64(d["points"]), f64(d["normal"]), f64(d["view"]), lgt_in, leaves["f0"], leaves["rough"], leaves["albedo"],
                                 comp_vis=comp_vis, VisModel=None, lin_diff=lin_diff, testing=True,
                                 indir_integral=leaves.get("indir_integral"), metallic=leaves.get("metallic"))
    spec, diff = out["sg_specular_rgb"], out["sg_diffuse_rgb"]
    loss = (spec * f64(g_spec)).sum() + (diff * f64(g_diff)).sum()
    gs = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(leaves, gs)}
    return grads, spec.detach(), diff.detach()


def main():
    for tag in ("init", "sharp"):
        d = dict(np.load(os.path.join(GOLD, f"sg_{tag}.npz"), allow_pickle=False))
        n, M = d["normal"].shape[0], d["lgtSGs"].shape[0]
        store = {"cases": np.array(json.dumps({k: dict(zip(("light", "comp_vis", "indir_integral", "lin_diff", "metallic"), v))
                                                for k, v in CASES.items()}))}
        for ci, case in enumerate(CASES):
            light = CASES[case][0]
            g = np.random.default_rng(1000 + 17 * ci + (0 if tag == "init" else 500))
            lv = g.uniform(0, 1, (n, M)).astype(np.float32)
            lv[g.uniform(size=lv.shape) < 0.05] = 0.0
            lv[g.uniform(size=lv.shape) < 0.05] = 1.0
            bv = g.uniform(0, 1, n).astype(np.float32)
            bv[:2] = (0.0, 1.0)
            met = g.uniform(0, 1, n).astype(np.float32)
            g_spec = g.standard_normal((n, 3)).astype(np.float32)
            g_diff = g.standard_normal((n, 3)).astype(np.float32)
            if light == "shared":
                lgt = d["lgtSGs"]
            elif light == "per_point":
                lgt = d["indir_sgs"]
            else:
                # first half of the points: 24 sharp lobes (sharpness 8000) 0.2 below each point's horizon -- every specular and diffuse sum there
                # is negative in float64 and in fp32 alike and is clamped, so those rows get no gradient at all; the other half keeps the
                # stored per-point lights and stays live
                lgt = d["indir_sgs"].copy()
                h = n // 2
                nrm = d["normal"][:h]
                t = np.cross(nrm, g.standard_normal((h, 3)))
                t /= np.linalg.norm(t, axis=-1, keepdims=True)
                b = np.cross(nrm, t)
                ang = g.uniform(0, 2 * np.pi, (h, 24, 1))
                axis = (t[:, None] * np.cos(ang) + b[:, None] * np.sin(ang)) * np.sqrt(1 - 0.04) - 0.2 * nrm[:, None]
                lgt[:h, :, :3] = axis
                lgt[:h, :, 3] = 8000.0
                lgt[:h, :, 4:] = g.uniform(0.5, 2.0, (h, 24, 3))
                lgt = lgt.astype(np.float32)
                lv = lv[:, :24].copy()
                bv[:2] = (0.3, 1.0)
                bv[h:h + 2] = (0.0, 1.0)
            vis = {"lgt": lgt, "bvis": bv, "light_vis": lv, "metallic": met}
            grads, spec, diff = reference_grads(d, case, vis, g_spec, g_diff)
            # the same through the oracle's formulas, float64
            inp = dict(normal=d["normal"], view=d["view"], lgt=lgt, f0=d["f0"], rough=d["roughness"].reshape(-1), albedo=d["albedo"], bvis=bv,
                       light_vis=lv if CASES[case][1] else None, metallic=met if CASES[case][4] else None,
                       indir_integral=d["indir_int"] if CASES[case][2] else None, lin_diff=CASES[case][3])
            og, ospec, odiff = sbo.grads(inp, g_spec, g_diff, torch.float64)
            print(f"sg_grad_{tag}/{case}: spec==0 {int((spec == 0).sum())}/{spec.numel()} diff==0 {int((diff == 0).sum())}/{diff.numel()}  "
                  f"forward oracle-vs-reference spec {rel_err(ospec, spec):.2e} diff {rel_err(odiff, diff):.2e}")
            for k, gr in grads.items():
                dist = rel_err(og[k].reshape(gr.shape), gr)
                print(f"    d {k:15s} max|ref64| {float(gr.abs().max()):.4e}   oracle64 vs reference64 rel_err {dist:.2e}")
                store[f"{case}.grad.{k}"] = gr.numpy().astype(np.float64).reshape(og[k].shape)
                store[f"{case}.oracle_dist.{k}"] = np.float64(dist)
            store[f"{case}.in.bvis"] = bv
            store[f"{case}.in.g_spec"] = g_spec
            store[f"{case}.in.g_diff"] = g_diff
            if CASES[case][1]:
                store[f"{case}.in.light_vis"] = lv
            if CASES[case][4]:
                store[f"{case}.in.metallic"] = met
            if light == "away":
                store[f"{case}.in.lgt"] = lgt
        path = os.path.join(GOLD, f"sg_grad_{tag}.npz")
        np.savez_compressed(path, **store)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
