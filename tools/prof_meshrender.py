#!/usr/bin/env python
"""Times a view of the baked synthetic scene and writes the record profiles/meshrender_times.md:

    python tools/prof_meshrender.py [--size 800] [--mesh-res 256] [--resolution 4096] [--bench-line '{...}'] [--out profiles/meshrender_times.md]

The synthetic model's surface is extracted at --mesh-res, baked at --resolution, and drawn at --size x --size from synth_camera with
vis="none" (direct SG shading).  Per stage, HIP events around warm calls, the median of 10 after 3 warm-ups: project (rb_rs_project), bin
(rb_rs_bin_count, the prefix sum, the host read of the pair count, rb_rs_bin_emit, the stable sort, the tile offsets), raster
(rb_rs_raster), gbuffer (rb_rs_gbuffer, list form on the hit rows, 8 plane channels, bilinear), shade (sg_render.render_with_all_sg with
VisModel=None on the hit rows), and render_mesh as a whole (wall clock).  Each kernel's MINIMUM traffic is set beside the 6.3 TB/s
streaming figure that the other profiles use.  --bench-line: the JSON line `bench.py --gpus 1` printed in the same session, for the neural
view's rate beside these times."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robir_amd import mesh, meshrender, ops, renderer, synth, texture  # noqa: E402

STREAM_TBS, WARM, REPS = 6.3, 3, 10


def event_ms(fn):
    for _ in range(WARM):
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--mesh-res", type=int, default=256)
    ap.add_argument("--resolution", type=int, default=4096)
    ap.add_argument("--bench-line", help="the JSON line of bench.py from the same session")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshrender_times.md"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    H = W = a.size
    with torch.no_grad():
        model = renderer.build_synthetic_model(dev, build_octrees=False)
        m = mesh.extract_mesh(model, resolution=a.mesh_res, device=dev)
        ts = texture.bake(model, m, resolution=a.resolution)
        asset = meshrender.load_asset(ts, dev)
        _, pose, K = synth.synth_camera(H, W)
        pose, K = torch.from_numpy(pose).to(dev), torch.from_numpy(K).to(dev)
        pinv, cam = meshrender.pose_inverse(pose)
        V, F, R, C = asset.vertices.shape[0], asset.faces.shape[0], asset.planes.shape[0], asset.planes.shape[2]
        near, cull = 1e-4, 0
        ntiles = ((W + 7) // 8) * ((H + 7) // 8)

        t_project, screen = event_ms(lambda: ops.rs_project(asset.vertices, pinv, K))

        def bin_():
            counts = ops.rs_bin_count(screen, asset.faces, H, W, near, cull)
            incl = torch.cumsum(counts.to(torch.int64), 0)
            P = int(incl[-1])
            pair_tile, pair_face = ops.rs_bin_emit(screen, asset.faces, H, W, near, cull, (incl - counts).contiguous(), P)
            tiles, order = torch.sort(pair_tile, stable=True)
            start = torch.searchsorted(tiles, torch.arange(ntiles + 1, dtype=torch.int32, device=dev)).to(torch.int32)
            return start, pair_face[order].contiguous(), counts, incl, P

        t_bin, (tile_start, pair_face, counts, incl, P) = event_ms(bin_)
        t_count, _ = event_ms(lambda: ops.rs_bin_count(screen, asset.faces, H, W, near, cull))
        base = (incl - counts).contiguous()
        t_emit, _ = event_ms(lambda: ops.rs_bin_emit(screen, asset.faces, H, W, near, cull, base, P))
        t_raster, (face_id, bary, depth) = event_ms(lambda: ops.rs_raster(screen, asset.faces, H, W, near, cull, tile_start, pair_face))
        idx = (face_id.reshape(-1) >= 0).nonzero()[:, 0].contiguous()
        n = idx.numel()
        t_gbuf, g = event_ms(lambda: meshrender.gbuffer(face_id, bary, asset.vertices, asset.faces, asset.uv, cam, asset.planes, 1, None, idx))
        tex = g["tex"]
        nrm = meshrender._unit(tex[:, 5:8])
        alb, rough = tex[:, 0:3].contiguous(), tex[:, 3:4].contiguous()
        t_shade, _ = event_ms(lambda: meshrender.shade_rows(g["position"], nrm, g["view_dir"], alb, rough, model=model, vis="none"))

        def whole():
            torch.cuda.synchronize()
            t = time.perf_counter()
            meshrender.render_mesh(asset, pose, K, H, W, model=model, vis="none")
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3

        for _ in range(WARM):
            whole()
        t_whole = statistics.median(whole() for _ in range(REPS))
        longest = int(torch.diff(tile_start.long()).max())

    # minimum traffic in bytes: what each kernel must read and write once
    traffic = {"project": 28 * V, "bin_count": 12 * F + 16 * V + 4 * F, "bin_emit": 12 * F + 16 * V + 8 * F + 8 * P,
               "raster": 4 * P + 4 * ntiles + 12 * F + 16 * V + 16 * H * W, "gbuffer": n * (8 + 4 + 8 + 12 + 4 * (3 + 2 + 3 + C)) + n * 4 * 4 * C}
    rows = [("project", t_project, traffic["project"]), ("bin (all of it)", t_bin, None), ("  bin_count", t_count, traffic["bin_count"]),
            ("  bin_emit", t_emit, traffic["bin_emit"]), ("raster", t_raster, traffic["raster"]), ("gbuffer", t_gbuf, traffic["gbuffer"]),
            ("shade (vis none)", t_shade, None), ("render_mesh, wall clock", t_whole, None)]
    lines = [f"# Mesh view times (MI355X, synthetic sphere, {H} x {W} view, mesh lattice {a.mesh_res}^3, {R}^2 atlas)", "",
             "Written by `tools/prof_meshrender.py`.  HIP events around warm calls, the median of 10 after 3 warm-ups; the last row is wall clock",
             "around synchronised `render_mesh(..., vis=\"none\")` calls, which also holds the hit-row compaction, the output buffers and the",
             "pose inverse.  `bin (all of it)` is the count kernel, torch's prefix sum, the ONE host read of the pair count, the emit kernel,",
             "torch's stable sort by tile and the tile offsets.  TB/s = minimum traffic / time, to be read beside the 6.3 TB/s streaming figure;",
             "the rasteriser is bound by the faces each tile walks, not by bytes.", "",
             f"V = {V}, F = {F}, (tile, face) pairs P = {P}, tiles = {ntiles}, longest tile list = {longest} faces, hit pixels n = {n} of {H * W}, "
             f"plane channels C = {C}.", "",
             "Minimum traffic: project 28 V; bin_count 16 F + 16 V; bin_emit 20 F + 16 V + 8 P; raster 4 P + 4 tiles + 12 F + 16 V + 16 H W;",
             "gbuffer (list form, bilinear) n (32 + 4 (8 + C)) + 16 n C (four taps of C channels).", "",
             "| stage | ms | minimum traffic, MB | TB/s |", "|---|---|---|---|"]
    for name, ms, by in rows:
        lines.append(f"| {name} | {ms:.3f} | {'' if by is None else '%.2f' % (by / 1e6)} | {'' if by is None else '%.3f' % (by / (ms * 1e-3) / 1e12)} |")
    lines += ["", f"Streaming figure for comparison: {STREAM_TBS} TB/s."]
    if a.bench_line:
        b = json.loads(a.bench_line)
        lines += ["", "The neural view, `bench.py --gpus 1` in the same session on the same box:", "", "```", json.dumps(b), "```"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
