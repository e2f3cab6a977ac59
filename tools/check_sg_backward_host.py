#!/usr/bin/env python
"""Checks the hand-derived SG shading backward on the CPU: compiles tools/sg_backward_host.cpp (= robir_amd/csrc/sg_shade_bwd_math.h built for the
host) with the host C++ compiler and compares its gradients with the reference's float64 autograd stored in tests/golden/sg_grad_*.npz, next
to PyTorch's fp32 autograd of the oracle's formulas (tests/sg_backward_oracle.py).  The clamp masks come from the oracle's fp32 forward.

    python tools/check_sg_backward_host.py                      every fixture case: rel_err of the host build / of fp32 autograd
    python tools/check_sg_backward_host.py --no-zero-reeval     the build in which a stored 0 never passes a gradient
    python tools/check_sg_backward_host.py --low-roughness      the fun_spec regime (roughness * 0.8 + 0.05 on sg_sharp): with the fp32 forward's
                                                                outputs as the clamp mask, and with float64's
"""
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import sg_backward_oracle as sbo  # noqa: E402


def rel_err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float(((a - b).abs() / (b.abs() + b.abs().mean() + 1e-30)).max()) if b.numel() else 0.0


def build(no_zero_reeval):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        raise SystemExit("no host C++ compiler found (set CXX)")
    out = os.path.join(tempfile.mkdtemp(prefix="sgb_host_"), "sg_backward_host.so")
    cmd = [cxx, "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-w", "-I", os.path.join(ROOT, "robir_amd", "csrc"),
           os.path.join(ROOT, "tools", "sg_backward_host.cpp"), "-o", out] + (["-DSGB_NO_ZERO_REEVAL"] if no_zero_reeval else [])
    subprocess.run(cmd, check=True)
    return ctypes.CDLL(out)


def run(lib, inp, gs, gd, spec32, diff32):
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    f = lambda k: None if inp.get(k) is None else np.ascontiguousarray(inp[k], dtype=np.float32)
    n = inp["normal"].shape[0]
    lgt = f("lgt")
    M = lgt.shape[-2]
    z = lambda *s: np.zeros(s, dtype=np.float64)
    out = dict(rough=z(n), albedo=z(n, 3), metallic=z(n), bvis=z(n), light_vis=z(n, M), indir_integral=z(n, 3), lgt=z(*lgt.shape), f0=z(1))
    a = {k: f(k) for k in ("normal", "view", "rough", "albedo", "metallic", "light_vis", "bvis", "indir_integral")}
    c32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    keep = [c32(gs), c32(gd), c32(spec32), c32(diff32)]
    lib.sgb_cpu(P(a["normal"]), P(a["view"]), P(lgt), int(lgt.ndim == 3), M, ctypes.c_float(float(np.asarray(inp["f0"]).reshape(-1)[0])),
                P(a["rough"]), P(a["albedo"]), P(a["metallic"]), P(a["light_vis"]), P(a["bvis"]), P(a["indir_integral"]),
                int(bool(inp["lin_diff"])), ctypes.c_long(n), P(keep[2]), P(keep[3]), P(keep[0]), P(keep[1]), P(out["rough"]), P(out["albedo"]),
                P(out["metallic"]), P(out["bvis"]), P(out["light_vis"]), P(out["indir_integral"]), P(out["lgt"]), P(out["f0"]))
    return out


def report(tag, host, g32, ref64):
    for k, r in ref64.items():
        print(f"{tag:34s} d {k:15s} host build {rel_err(host[k].reshape(r.shape), r):9.2e}   fp32 autograd {rel_err(g32[k].reshape(r.shape), r):9.2e}")


def main():
    lib = build("--no-zero-reeval" in sys.argv)
    gold = os.path.join(ROOT, "tests", "golden")
    if "--low-roughness" in sys.argv:
        d = np.load(os.path.join(gold, "sg_sharp.npz"))
        rng = np.random.default_rng(1)
        n = 40
        inp = dict(normal=d["normal"], view=d["view"], f0=d["f0"], rough=(d["roughness"] * 0.8 + 0.05).reshape(-1), albedo=d["albedo"],
                   bvis=rng.uniform(0, 1, n).astype(np.float32), lgt=d["lgtSGs"], light_vis=rng.uniform(0, 1, (n, 128)).astype(np.float32),
                   lin_diff=False)
        gs, gd = rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)
        g64, s64, d64 = sbo.grads(inp, gs, gd, torch.float64)
        g32, s32, d32 = sbo.grads(inp, gs, gd, torch.float32)
        print("outputs that are 0 in fp32 and not in float64:", int(((s32 == 0) & (s64 != 0)).sum()), "specular,",
              int(((d32 == 0) & (d64 != 0)).sum()), "diffuse")
        report("clamp mask = fp32 forward", run(lib, inp, gs, gd, s32.numpy(), d32.numpy()), g32, g64)
        report("clamp mask = float64 forward", run(lib, inp, gs, gd, s64.float().numpy(), d64.float().numpy()), g32, g64)
        return
    for tag in ("init", "sharp"):
        base, fx = np.load(os.path.join(gold, f"sg_{tag}.npz")), np.load(os.path.join(gold, f"sg_grad_{tag}.npz"))
        for case, cfg in json.loads(str(fx["cases"])).items():
            I = lambda k: fx[f"{case}.in.{k}"]
            lgt = {"shared": base["lgtSGs"], "per_point": base["indir_sgs"]}.get(cfg["light"])
            lgt = I("lgt") if lgt is None else lgt
            inp = dict(normal=base["normal"], view=base["view"], lgt=lgt, f0=base["f0"], rough=base["roughness"].reshape(-1),
                       albedo=base["albedo"], bvis=I("bvis"), light_vis=I("light_vis") if cfg["comp_vis"] else None,
                       metallic=I("metallic") if cfg["metallic"] else None, indir_integral=base["indir_int"] if cfg["indir_integral"] else None,
                       lin_diff=cfg["lin_diff"])
            ref64 = {k[len(case) + 6:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(case + ".grad.")}
            g32, s32, d32 = sbo.grads(inp, I("g_spec"), I("g_diff"), torch.float32)
            report(f"sg_grad_{tag}/{case}", run(lib, inp, I("g_spec"), I("g_diff"), s32.numpy(), d32.numpy()), g32, ref64)


if __name__ == "__main__":
    main()
