"""Fit light SGs to an environment map: the reference's envmaps/fit_envmap_with_sg.py on the device (robir_amd/lightfit.py).

    python -m robir_amd.fit_light --envmap envmaps/mine.exr [--num_sg 128] [--iters 100000] [--lr 1e-2] [--size 256 512] [--seed 0] [--resume]

reads envmaps/mine.exr (robir_amd.exr.read_exr; a .npy holding [H, W, 3] is accepted too) and writes envmaps/mine/sg_128.npy, fp32 [128, 7] --
the reference's layout (fit_envmap_with_sg.py:31,68) -- after every block of steps and at the end, so that

    python -m robir_amd.render ... --light envmaps/mine

and EnvmapMaterialNetwork.load_light work with no further step.  Next to it, fit_128.npz keeps Adam's two moments and the step count:
--resume continues from both files (from sg_128.npy alone, e.g. one of the reference's fits, with fresh moments: the reference's resume).
The loss is printed per block.  No PNG log is written."""
import argparse
import os

import numpy as np
import torch

from . import lightfit


def read_map(path):
    if path.lower().endswith(".npy"):
        img = np.load(path)
        if img.ndim != 3 or img.shape[2] < 3:
            raise SystemExit(f"{path}: an array [H, W, 3] is needed, got {img.shape}")
        return np.ascontiguousarray(img[:, :, :3], dtype=np.float32)
    from .exr import read_exr
    return np.ascontiguousarray(read_exr(path)[:, :, :3])


def main(argv=None):
    ap = argparse.ArgumentParser(description="fit light SGs to an environment map on the device")
    ap.add_argument("--envmap", required=True, help="the map: .exr, or .npy holding [H, W, 3]")
    ap.add_argument("--num_sg", type=int, default=128)
    ap.add_argument("--iters", type=int, default=100000)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--size", type=int, nargs=2, default=(256, 512), metavar=("H", "W"), help="the map is area-resized to at most this size")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--block", type=int, default=1000, help="steps per enqueued block (one loss line and one save each)")
    ap.add_argument("--resume", action="store_true", help="continue from <map>/sg_<M>.npy (and fit_<M>.npz if it is there)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("fit_light needs the GPU: there is no CPU path")
    path = os.path.abspath(a.envmap)
    out_dir = os.path.splitext(path)[0]
    os.makedirs(out_dir, exist_ok=True)
    sg_file = os.path.join(out_dir, f"sg_{a.num_sg}.npy")
    state_file = os.path.join(out_dir, f"fit_{a.num_sg}.npz")
    init, state = None, {}
    if a.resume:
        if not os.path.isfile(sg_file):
            raise SystemExit(f"--resume: {sg_file} not found")
        init = np.load(sg_file)
        if os.path.isfile(state_file):
            st = np.load(state_file)
            if st["lgtSGs"].shape == init.shape and np.array_equal(st["lgtSGs"], init):      # the moments belong to these parameters
                state = {"adam_m": st["adam_m"], "adam_v": st["adam_v"], "step": int(st["step"])}
        print(f"resuming from {sg_file} at step {state.get('step', 0)}" + ("" if state else " (no matching fit state: fresh moments)"))

    def save(step, loss, lgt):
        sg = lgt.detach().cpu().numpy().astype(np.float32)
        np.save(sg_file, sg)
        np.savez(state_file, lgtSGs=sg, adam_m=state["adam_m"].cpu().numpy(), adam_v=state["adam_v"].cpu().numpy(), step=np.int64(state["step"]))
        print(f"step: {step}, loss: {loss}", flush=True)

    lgt, hist = lightfit.fit_envmap(read_map(path), num_sg=a.num_sg, iters=a.iters, lr=a.lr, size=tuple(a.size), init=init, seed=a.seed,
                                    block=a.block, callback=save, state=state)
    if a.iters <= 0:
        save(state["step"], float("nan"), lgt)
    print(f"wrote {sg_file}: {a.num_sg} light SGs after {state['step']} steps" + (f", loss {hist[0]:.6g} -> {hist[-1]:.6g}" if len(hist) else ""))
    return {"sg_file": sg_file, "state_file": state_file, "step": state["step"], "loss": hist}


if __name__ == "__main__":
    main()
