#!/usr/bin/env python
"""Times the multi-view observation path on the synthetic scene and writes the record profiles/observe_times.md:

    python tools/prof_observe.py [--cameras 100] [--image 800] [--points 262144] [--texture 1024] [--out profiles/observe_times.md]

HIP-event times (median of 5 after one warm-up) of the kernels of csrc/observe/observe.hip on `--points` surface points of the 33^3 mesh's
bake seen by `--cameras` look-at views of `--image`^2 random pixels, with the achieved bytes/s over each kernel's MINIMUM traffic beside
the 6.3 TB/s streaming figure; and wall-clock seconds (ONE run each, around synchronised calls) of visible_views -- the scatter, the
compaction and the secondary cast of the valid pairs -- of observed_color and of TextureSet.bake_observations at `--texture`^2."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robir_amd import mesh, observe, ops, renderer, texture  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cameras", type=int, default=100)
ap.add_argument("--image", type=int, default=800)
ap.add_argument("--points", type=int, default=1 << 18)
ap.add_argument("--texture", type=int, default=1024)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "observe_times.md"))
a = ap.parse_args()
dev = torch.device("cuda:0")
STREAM_TBS, REPS = 6.3, 5


def event_ms(fn):
    fn()
    ts = []
    for _ in range(REPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts), out


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def look_at(c):
    back = c / np.linalg.norm(c)
    right = np.cross([0.0, 0.0, 1.0], back)
    right /= np.linalg.norm(right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, np.cross(back, right), back, c
    return pose


with torch.no_grad():
    M, S, N = a.cameras, a.image, a.points
    model = renderer.build_synthetic_model(dev, scene="sphere")
    m = mesh.extract_mesh(model, resolution=33)
    ts = texture.bake(model, m, resolution=a.texture)
    rng = np.random.default_rng(0)
    d = rng.normal(size=(M, 3))
    d[:, 2] *= 0.5
    pose = np.stack([look_at(v / np.linalg.norm(v) * 0.9) for v in d]).astype(np.float32)
    K = np.tile(np.array([[1.39 * S, 0, 0.5 * S], [0, 1.39 * S, 0.5 * S], [0, 0, 1]], dtype=np.float32), (M, 1, 1))
    images = torch.rand(M, S, S, 3, device=dev)
    fs = observe.FocusSampler(images, None, torch.from_numpy(pose).to(dev), torch.from_numpy(K).to(dev))
    s = ts.sampler().sample(N)
    x, nrm = s["x"].contiguous(), s["normal"].contiguous()
    cams = fs.cameras()
    tb = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12
    rows = []
    chunk = observe._chunk_points(M)
    xs, ns = x[:chunk].contiguous(), nrm[:chunk].contiguous()
    n = xs.shape[0]
    ms, sc = event_ms(lambda: ops.ob_scatter(xs, *cams))
    rows.append(("scatter", n, ms, tb(M * n * (33 + 48) + 12 * n, ms)))            # outputs, four taps of three floats, the point
    vis = sc[3].contiguous()
    draws = torch.rand(M, n, device=dev)
    ms, (index, _) = event_ms(lambda: ops.ob_select(vis, draws, 3))
    rows.append(("select, n_obs = 3", n, ms, tb(5 * M * n + 16 * n, ms)))
    ms, _ = event_ms(lambda: ops.ob_gather(index, xs, *cams))
    rows.append(("gather, n_obs = 3", n, ms, tb(3 * n * (33 + 48 + 4) + 12 * n, ms)))
    ms, _ = event_ms(lambda: ops.ob_accumulate(xs, ns, *cams[:4], vis))
    rows.append(("accumulate", n, ms, tb(M * n + int(vis.sum()) * 48 + 24 * n + 32 * n, ms)))
    t_vis, v = wall(lambda: observe.visible_views(model, fs, xs, ns))
    pairs, seen = int(vis.sum()), int(v.sum())
    t_col, _ = wall(lambda: observe.observed_color(model, fs, x, nrm))
    t_bake, _ = wall(lambda: ts.bake_observations(model, fs))
    covered = int((ts.mask > 0).sum())
    lines = [f"# Multi-view observation times (MI355X, synthetic sphere, {M} views of {S}^2, random pixels)", "",
             "Written by `tools/prof_observe.py`.  Kernels of `csrc/observe/observe.hip`: HIP events, median of "
             f"{REPS} runs after one warm-up, on one chunk of points (the size `observed_color` uses for this many cameras); TB/s = minimum",
             f"traffic / time, to be read beside the {STREAM_TBS} TB/s streaming figure of the microarchitecture guide.", "",
             "| kernel | points | ms | TB/s |", "|---|---|---|---|"]
    lines += [f"| {k} | {p} | {t:.3f} | {r:.3f} |" for k, p, t, r in rows]
    lines += ["", "Wall clock around synchronised calls, ONE run each (a single run, not a median):", "",
              f"- `visible_views` of {n} points: {t_vis:.3f} s -- the scatter, the compaction and ONE secondary cast of the {pairs} valid pairs of",
              f"  {M * n}; {seen} pairs are visible.",
              f"- `observed_color` of {N} points ({(N + chunk - 1) // chunk} chunks of {chunk}): {t_col:.3f} s.",
              f"- `TextureSet.bake_observations` at {a.texture}^2 ({covered} covered texels, 4 rings on three planes): {t_bake:.3f} s."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", a.out)
