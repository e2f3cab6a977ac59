#!/usr/bin/env python
"""Times the mesh extraction of the synthetic scenes and writes the record profiles/mesh_times.md:

    python tools/prof_mesh.py [--res 256 512] [--scenes sphere nonconvex] [--grad-res 129] [--no-dense-above 256] [--out profiles/mesh_times.md]

Per scene and resolution, dense and culled (lip = robir_amd.mesh.LIP): seconds of the SDF fill (wall clock around a synchronised call), HIP-event
times of the three mesh kernels (median of 5), seconds of the attribute passes (normals; normals + one Newton step + materials), V, F
and the evaluated fraction; the mesh kernels' achieved bytes/s over their MINIMUM traffic (count: the field once; vertices: the field +
vbase + 12 V; faces: the field + 12 F) beside the 6.3 TB/s streaming figure; the largest |grad sdf| on a --grad-res lattice (the evidence
behind the default lip).  A dense fill above --no-dense-above is skipped (512^3 dense is 1.3e8 exact-threshold SDF evaluations)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robir_amd import mesh, ops, renderer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
ap.add_argument("--scenes", nargs="+", default=["sphere", "nonconvex"])
ap.add_argument("--grad-res", type=int, default=129)
ap.add_argument("--no-dense-above", type=int, default=512)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_times.md"))
a = ap.parse_args()
dev = torch.device("cuda:0")
STREAM_TBS = 6.3


def event_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
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


rows, grads = [], []


def write():
    lines = ["# Mesh extraction times (MI355X, synthetic scenes, box [-1,1]^3, threshold 0)", "",
             "Written by `tools/prof_mesh.py`.  fill = SDF lattice fill (wall clock, exact-threshold value kernel, chunks of 2^18 points; culled =",
             f"`lip = {mesh.LIP}`, blocks of 8^3); count / vertices / faces = the three kernels of `csrc/mesh.hip` (HIP events, median of 5) with their",
             f"achieved TB/s over the minimum traffic, to be read beside the {STREAM_TBS} TB/s streaming figure of the microarchitecture guide;",
             "normals = value + gradient pass at the vertices; all = one Newton step + normals + materials.", "",
             "| scene | lattice | fill | evaluated | fill s | count ms (TB/s) | vertices ms (TB/s) | faces ms (TB/s) | normals s | all s | V | F |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r[0]} | {r[1]}^3 | {r[2]} | {r[3]:.4f} | {r[4]:.3f} | {r[5]:.3f} ({r[6]:.2f}) | {r[7]:.3f} ({r[8]:.2f}) | "
                     f"{r[9]:.3f} ({r[10]:.2f}) | {r[11]:.3f} | {r[12]:.3f} | {r[13]} | {r[14]} |")
    lines += ["", "Largest |grad sdf| on the lattice (evidence for the default `lip`; the culling is exact when lip bounds the field's",
              "Lipschitz constant, and the tests use 1.5 x the lattice maximum):", "", "| scene | lattice | max abs grad | x 1.5 |", "|---|---|---|---|"]
    lines += [f"| {s} | {n}^3 | {g:.4f} | {1.5 * g:.4f} |" for s, n, g in grads]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


with torch.no_grad():
    for scene in a.scenes:
        model = renderer.build_synthetic_model(dev, build_octrees=False, scene=scene)
        src = mesh._Source(model)
        g = torch.linspace(-1.0, 1.0, a.grad_res, device=dev)
        pts = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        gmax = max(float(src.value_grad(pts[i:i + (1 << 18)].contiguous())[1].norm(dim=-1).max()) for i in range(0, pts.shape[0], 1 << 18))
        grads.append((scene, a.grad_res, gmax))
        print(f"{scene}: max |grad sdf| on {a.grad_res}^3 = {gmax:.4f}", flush=True)
        for res in a.res:
            xs = torch.linspace(-1.0, 1.0, res, device=dev)
            for lip in (None, mesh.LIP):
                if lip is None and res > a.no_dense_above:
                    continue
                t_fill, (field, frac) = wall(lambda: mesh.fill_lattice(src.value, xs, xs, xs, 0.0, lip))
                N = field.numel()
                ms_c, counts = event_ms(lambda: ops.mesh_count(field, 0.0))
                incl = torch.cumsum(counts.to(torch.int64), 0)
                V, F = (int(v) for v in incl[-1].tolist())
                base = (incl - counts).t().contiguous()
                ms_v, (verts, vbase) = event_ms(lambda: ops.mesh_emit_vertices(field, xs, xs, xs, 0.0, base[0], V))
                ms_f, faces = event_ms(lambda: ops.mesh_emit_faces(field, 0.0, base[1], vbase, V, F))
                del field, vbase
                t_n, _ = wall(lambda: mesh.vertex_attributes(src, verts, 0.0, 0, True, False))
                t_all, _ = wall(lambda: mesh.vertex_attributes(src, verts, 0.0, 1, True, True))
                tb = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12
                rows.append((scene, res, "dense" if lip is None else "culled", frac, t_fill, ms_c, tb(4 * N, ms_c), ms_v,
                             tb(8 * N + 12 * V, ms_v), ms_f, tb(4 * N + 12 * F, ms_f), t_n, t_all, V, F))
                print(rows[-1], flush=True)
                write()          # after every row: a run that is cut short still leaves its record
                del verts, faces
        del model, src
write()
print("wrote", a.out)
