#!/usr/bin/env python
"""Times the texture bake of the synthetic scenes and writes the record profiles/texbake_times.md:

    python tools/prof_texbake.py [--mesh-res 256 512] [--resolution 4096] [--scenes sphere] [--out profiles/texbake_times.md]

Per scene and mesh resolution: seconds of the stages of robir_amd.texture.bake (wall clock around synchronised calls, ONE run each, after one
warm-up bake at a small size) and of the export; HIP-event times of every kernel of csrc/texbake/texbake.hip (median of 5) with its achieved
bytes/s over its MINIMUM traffic beside the 6.3 TB/s streaming figure that profiles/mesh_times.md uses; and, at the GPU tests' size (33^3
lattice, 512^2 texture), the largest and the mean |sdf| over the covered texels with project = 0 and project = 1."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robir_amd import mesh, ops, renderer, texture  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mesh-res", type=int, nargs="+", default=[256, 512])
ap.add_argument("--resolution", type=int, default=4096)
ap.add_argument("--scenes", nargs="+", default=["sphere"])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texbake_times.md"))
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


stages, kernels, project = [], [], []


def write():
    R = a.resolution
    lines = [f"# Texture bake times (MI355X, synthetic scenes, {R}^2 texture, per-triangle atlas)", "",
             "Written by `tools/prof_texbake.py`.  Stage times are wall clock around synchronised calls, ONE run each (a single run, not a",
             "median), after a warm-up bake at 33^3 / 512^2: mesh = `extract_mesh`; raster = atlas + binning + sort + rasteriser; bake = per chunk of",
             "2^18 covered texels the interpolation, one Newton step, the SDF gradient and the material networks; dilate = 4 rings on five planes;",
             "export = the PNG / OBJ / NPZ writers on the host (zlib level 6).", "",
             "| scene | lattice | V | F | cell | covered | mesh s | raster ms | bake s | dilate ms | export s |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    lines += [f"| {r[0]} | {r[1]}^3 | {r[2]} | {r[3]} | {r[4]} | {r[5]:.4f} | {r[6]:.3f} | {1e3 * r[7]:.3f} | {r[8]:.3f} | {1e3 * r[9]:.3f} | {r[10]:.3f} |" for r in stages]
    lines += ["", f"Kernels of `csrc/texbake/texbake.hip`: HIP events, median of {REPS} runs after one warm-up; TB/s = minimum traffic / time, to be read",
              f"beside the {STREAM_TBS} TB/s streaming figure of the microarchitecture guide.  Minimum traffic: atlas 24 F; bin_count 28 F; bin_emit",
              "32 F + 8 P; raster 24 F + 4 P + 4 tiles + 12 R^2; interp (image form, C = 3) 24 R^2 + 12 F + 12 V; interp (list form, n covered texels)",
              "32 n + 12 F + 12 V; dilate (C = 3) 26 R^2; sample (n = 2^20) 84 n.  P = (tile, face) pairs.", "",
              "| scene | lattice | F | P | kernel | ms | TB/s |", "|---|---|---|---|---|---|---|"]
    lines += [f"| {r[0]} | {r[1]}^3 | {r[2]} | {r[3]} | {r[4]} | {r[5]:.3f} | {r[6]:.3f} |" for r in kernels]
    lines += ["", "Largest and mean |sdf| over the covered texels at the GPU tests' size (33^3 lattice, 512^2 texture; one run): the damped Newton step",
              "of `project = 1` moves the interpolated points of the flat triangles towards the zero set and never raises a point's |sdf|.", "",
              "| scene | max, project = 0 | max, project = 1 | mean, project = 0 | mean, project = 1 |", "|---|---|---|---|---|"]
    lines += [f"| {r[0]} | {r[1]:.3e} | {r[2]:.3e} | {r[3]:.3e} | {r[4]:.3e} |" for r in project]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


with torch.no_grad():
    for scene in ("sphere", "nonconvex"):
        model = renderer.build_synthetic_model(dev, build_octrees=False, scene=scene)
        src = mesh._Source(model)
        m = mesh.extract_mesh(model, resolution=33)
        d = []
        for p in (0, 1):
            ts = texture.bake(model, m, resolution=512, project=p)       # doubles as the warm-up
            dist = src.value(ts.position[ts.face_id >= 0].contiguous()).abs()
            d.append((float(dist.max()), float(dist.mean())))
        project.append((scene, d[0][0], d[1][0], d[0][1], d[1][1]))
        print(project[-1], flush=True)
        write()
        if scene not in a.scenes:
            continue
        R = a.resolution
        for res in a.mesh_res:
            t_mesh, m = wall(lambda: mesh.extract_mesh(model, resolution=res))
            V, F = m.vertices.shape[0], m.faces.shape[0]
            t_all, ts = wall(lambda: texture.bake(model, m, resolution=R))
            with tempfile.TemporaryDirectory() as tmp:
                t_exp, _ = wall(lambda: ts.export(tmp))
            s = ts.stats
            stages.append((scene, res, V, F, s["cell"], s["covered_fraction"], t_mesh, s["raster_s"], s["bake_s"], s["dilate_s"], t_exp))
            print(stages[-1], flush=True)
            write()
            # the kernels one by one
            tb = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12
            ms, uv = event_ms(lambda: ops.tb_atlas_uv(F, R, dev))
            rows = [("atlas", ms, 24 * F)]
            ms, counts = event_ms(lambda: ops.tb_bin_count(uv, R))
            rows.append(("bin_count", ms, 28 * F))
            incl = torch.cumsum(counts.to(torch.int64), 0)
            P = int(incl[-1])
            base = (incl - counts).contiguous()
            ms, (pt, pf) = event_ms(lambda: ops.tb_bin_emit(uv, R, base, P))
            rows.append(("bin_emit", ms, 32 * F + 8 * P))
            tiles, order = torch.sort(pt, stable=True)
            pf = pf[order].contiguous()
            nt = (R + ops.TB_TILE - 1) // ops.TB_TILE
            start = torch.searchsorted(tiles, torch.arange(nt * nt + 1, dtype=torch.int32, device=dev)).to(torch.int32)
            ms, (fid, bary) = event_ms(lambda: ops.tb_raster(uv, R, start, pf))
            rows.append(("raster", ms, 24 * F + 4 * P + 4 * nt * nt + 12 * R * R))
            ms, img = event_ms(lambda: ops.tb_interp(fid, bary, m.faces, m.vertices))
            rows.append(("interp image", ms, 24 * R * R + 12 * F + 12 * V))
            idx = torch.nonzero(fid.reshape(-1) >= 0).reshape(-1).contiguous()
            ms, _ = event_ms(lambda: ops.tb_interp(fid, bary, m.faces, m.vertices, idx))
            rows.append(("interp list", ms, 32 * idx.numel() + 12 * F + 12 * V))
            mask8 = (fid >= 0).to(torch.uint8)
            ms, _ = event_ms(lambda: ops.tb_dilate(img, mask8))
            rows.append(("dilate", ms, 26 * R * R))
            n = 1 << 20
            uvs = torch.rand(n, 2, device=dev)
            maskf = mask8.float()
            ms, _ = event_ms(lambda: ops.tb_sample(ts.position, ts.normal, maskf, uvs, 1.0))
            rows.append(("sample", ms, 84 * n))
            kernels += [(scene, res, F, P, k, ms, tb(b, ms)) for k, ms, b in rows]
            print(kernels[-len(rows):], flush=True)
            write()
            del m, ts, uv, fid, bary, img, idx, mask8, maskf, uvs, pt, pf, tiles, order, start
        del model, src
write()
print("wrote", a.out)
