#!/usr/bin/env python
"""bench.py -- PBR-stage rays/s of the MI355X-native renderer (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W          (N > 1 without a launcher: bench.py starts its own N ranks)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Workload (config 4 of BASELINE.json, the one the metric is quoted on; it fits one GPU): full PBR forward of a
synthetic 800x800 view -- camera rays, octree sphere trace of 625 lock-step chunks of 1024 pixels, SDF at every
ray, per-hit indirect-illumination / material networks, 128-lobe light-SG visibility (32 samples per lobe through the
visibility MLP), 8+8 BRDF-lobe visibility samples, SG shading (128 direct + 24 indirect lobes), scatter to per-ray
outputs.  Synthetic weights (robir_amd.synth, seed 0), random draws generated on the device inside the step.
One step = ONE such image rendered by all N GPUs together ("strong": rank r renders chunks {c : c mod N = r} of the view,
robir_amd.parallel.render_view_sharded, and the 17-float tiles are all-gathered over RCCL at the end of the step -- the
partition SURVEY.md 8e / north_star name).  `value` = rays of that image / step time.  With `--full` and N > 1 a secondary figure
times the weak form (rank r renders its own view r).  The octree build is one-off set-up and is reported separately.

Arithmetic (`--precision`): the headline is `exact` -- NOT narrower than the reference's fp32: the light-visibility MLP (98 % of
the FLOPs) carries every fp32 operand exactly as three f16 pieces and forms the six partial products of weight >= 2^-22 on the
f16 MFMA in three fp32 accumulators (csrc/vis_diffuse_x6.hip), every other MLP runs on the f32-input MFMA.  With `--full` at N = 1
the line also carries `legs` (the same view on the f32-input MFMA everywhere, and in split precision = 22-bit operand pairs, each
timed over its own loop, with image distances) and `configs` (BASELINE configs 1, 2, 3, 5; `--config N` prints one of them as
its own line).

Prints ONE JSON line (rank 0) with `roofline` (dominant kernel: fused light-SG visibility, MFMA bound, from HIP events around its
launches in the timed steps) and, with `--full` at N=1, `cpu_baseline` (the oracle restatement timed on this box's host cores on a
bounded sample of the same workload).  A plain run sets up, warms up, times the --steps steps, writes the last step's image under
`--dump-outputs DIR` if given, and prints the line; everything else runs only under `--full`.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

VIS_MACS_PER_EVAL = 229376          # 126*256 + 3*256*256 + 256*2
PEAK_FP32_MFMA_TFLOPS = 157.3       # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 / 32x32x2, dense
PEAK_F16_MFMA_TFLOPS = 2500.0      # MI355X_MICROARCH.md: dense f16/bf16 MFMA (not the 2:1-sparse marketing figure)
# HBM bytes per (point, direction) pair: (2 x FETCH_SIZE + WRITE_SIZE) / pairs at 32 chunks per launch.  DERIVED, not a counter of the
# timed run (PMC passes cannot run inside the timed region): f16x6 from the PMC passes of this round's kernel
# (profiles/r06_dvis_x6t_pmc.md: FETCH_SIZE / WRITE_SIZE equal r05's to 0.1 %), the split-precision kernel from profiles/r03_pmc_summary.md
# f16 mode, point-block form (profiles/r05_dvis_f16p_pmc.md, 64 chunks per launch): its pair values go out as 16-lane rows and its rounds
# fetch whole table rows (L2 / MALL hits mostly): more bytes per pair, still < 0.1 TB/s
TRAFFIC_B_PER_PAIR = {"f16x6": 33.0, "f16x1": 68.4, "default": 22.1}
TRAFFIC_PROFILE = {"f16x1": "profiles/r05_dvis_f16p_pmc.md"}
H = W = 800
CHUNK = 1024
STEP_SEED = 20260928                # torch's CPU and device generators are set to this at the start of every step


PRECISIONS = {
    # name: (light-visibility kernel, stand-alone MLP kernels, dtype string of the JSON line)
    "exact": ("f16x6", "f16x6",
              "f32 (every MLP -- light visibility, SDF values and reverse-mode gradient, colour, visibility, 512-wide and CESR nets: every "
              "fp32 operand exact as three f16 pieces, six MFMA products per multiply-add in three fp32 accumulators -- in the light-visibility "
              "kernel the two outer products of the 2^-22 class from bf8 copies of their operands, error against float64 unchanged; the 32 -> 128 "
              "-> 16 auto-encoder decoders on the f32-input MFMA) -- not narrower than the reference's fp32"),
    "fp32-mfma": ("fp32", "fp32", "f32 (every MLP on v_mfma_f32_16x16x4_f32)"),
    "f16": ("f16x1", "f16x3", "f16 (light-visibility MLP and the two CESR nets: ONE f16 MFMA product per multiply-add, f16 weights and f16 activations, fp32 accumulate; "
                              "every other net in split precision: f16 hi/lo pairs, 3 products) -- NARROWER than the reference's fp32: a labelled "
                              "throughput mode (BASELINE.json configs[4]: 'fp16 MLP weights on MFMA'), not a parity claim; error table in DESIGN.md"),
    "split": ("f16x3-auto", "f16x3", "f32 operands as 22-bit f16 hi/lo pairs, 3 f16 MFMA products per multiply-add, fp32 accumulate "
                                     "(parity-tested throughput mode; NARROWER than fp32)"),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", type=int, default=4, choices=[1, 2, 3, 4, 5],
                    help="BASELINE.json configuration to time: 4 (default) = the one the metric is quoted on, 800x800 full PBR; "
                         "1, 2, 3, 5 print one line for that configuration instead (tools/bench_configs.py; N = 1 only)")
    ap.add_argument("--precision", default="exact", choices=sorted(PRECISIONS),
                    help="arithmetic of the MLP layers.  exact (default, the headline): not narrower than fp32 -- the light-visibility "
                         "MLP with exact three-piece f16 operands (6 MFMA products per multiply-add), the other MLPs on the "
                         "f32-input MFMA; fp32-mfma: everything on the f32-input MFMA; split: 22-bit hi/lo operand pairs, 3 "
                         "products (faster, narrower than fp32); f16: the light-visibility MLP in plain f16, one product (throughput mode, NARROWER)")
    ap.add_argument("--chunks-per-batch", type=int, default=625,
                    help="1024-pixel chunks rendered per kernel pass (625 = the whole 800x800 view; 2.7 GB of tables)")
    ap.add_argument("--cpu-baseline-chunks", type=int, default=4)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-legs", action="store_true",
                    help="skip the side legs (N = 1): the same view in the other two precisions, each timed over --leg-steps steps "
                         "of its own, and the image distances from the f32-input-MFMA image")
    ap.add_argument("--leg-steps", type=int, default=3)
    ap.add_argument("--with-split", action="store_true",
                    help="also time the split-precision policy (legs and the configs sweep): a retired second product line kept for bit-identity "
                         "tests and ROBIR_PRECISION=f16's non-visibility nets; needs robir_amd/librobir_hip_legacy.so (ROBIR_BUILD_LEGACY=1). "
                         "Off by default since round 6: it cost GPU minutes every round for a mode no parity claim rests on")
    ap.add_argument("--no-configs", action="store_true",
                    help="skip the `configs` extras (N = 1): BASELINE configs 1, 2, 3, 5 timed after the headline")
    ap.add_argument("--config5-chunks", type=int, default=None,
                    help="chunks of the 1600x1200 CESR view (default: 1875 = the whole view for --config 5, a 125-chunk band "
                         "for the extras of the default line)")
    ap.add_argument("--cpu-baseline-1thread-pixels", type=int, default=256,
                    help="pixels of the single-thread CPU baseline sample (the runners force torch.set_num_threads(1))")
    ap.add_argument("--scene", default="sphere", choices=["sphere", "nonconvex"],
                    help="synthetic SDF: the geometric-init sphere (default; the scene of every earlier round) or the non-convex "
                         "fit of two spheres + a torus (robir_amd/data/nonconvex_sdf.npz); the default line carries the other "
                         "scene as an extra")
    ap.add_argument("--vis-precision", default=None, choices=["fp32", "f16x6", "f16x3-auto", "f16x3-v3", "f16x3-v2", "f16x3"],
                    help="override the light-visibility kernel of --precision (A/B runs)")
    ap.add_argument("--vis", default="mlp", choices=["mlp", "octree"],
                    help="light / BRDF-lobe visibility model: the visibility MLP (default, the reference's default) or traced "
                         "visibility = OctreeVisModel(octree_ray_tracer), the reference's `trace_vis` switch "
                         "(training/train_pbr.py:409-410): the MLP's 98 %% of the PBR FLOPs become octree gathers")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: the RCCL self-check (N = 1), package power during the timed steps, the "
                         "side legs in the other precisions, the other scene, the `configs` / `extras` figures and the CPU baseline (N = 1), "
                         "the weak-scaling views and the collective alone (N > 1).  Off: set up, warm up, time the steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the image the last timed step rendered as DIR/<field>.npy (float32, [H, W, "
                         "channels], the fields of robir_amd.parallel.TILE_FIELDS; 43.5 MB in all).  Every step draws its random numbers "
                         "from the same seed, so the same arguments give the same inputs run after run")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.config != 4:
        ap.error("--dump-outputs writes the headline workload's image (--config 4)")
    return args


def view_pose(rank, distance=0.9):
    """Camera `rank` of the multi-view job: rotate the synthetic camera about the y axis."""
    a = 0.35 * rank
    c, s = math.cos(a), math.sin(a)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = R
    pose[:3, 3] = R @ np.array([0, 0, distance], np.float32)
    return pose


class KernelTimer:
    """HIP-event timing of one kernel family on the stream it is launched on (torch's current stream)."""

    def __init__(self):
        self.pairs = []
        self.on = False

    def wrap(self, fn):
        def inner(*a, **k):
            if not self.on:
                return fn(*a, **k)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **k)
            e.record()
            self.pairs.append((s, e))
            return out
        return inner

    def stats(self):
        ms = [s.elapsed_time(e) for s, e in self.pairs]
        return (sum(ms) / len(ms), len(ms)) if ms else (0.0, 0)


def cpu_baseline(model, n_chunks, uv, pose, K, cores=None, pixels=CHUNK):
    """Oracle (CPU restatement of the reference) on `n_chunks` central chunks of `pixels` pixels of the same image."""
    from robir_oracle import nets as on, octree as ooct, renderer as orend
    from robir_amd import synth
    if cores is None:
        cores = min(16, os.cpu_count() or 1)  # more threads make the many small tensor ops of the reference slower
    torch.set_num_threads(cores)
    sd = on.as_torch(synth.synth_state_dict(0, variance=0.3))
    # geometry: the octree the device built, converted to the oracle's table format (same cells, no 10 s CPU rebuild)
    Td = model.ray_tracer.sdf_octree.tables
    node = Td.node.cpu()
    T = ooct.OctreeTables()
    T.root_min, T.root_size = torch.from_numpy(Td.root_min.copy()), torch.from_numpy(Td.root_size.copy())
    T.box_min, T.box_size, T.sdf_val = node[:, 0:3].contiguous(), node[:, 4:7].contiguous(), node[:, 7].contiguous()
    fc = node[:, 3].contiguous().view(torch.int32).long()
    T.is_split = fc >= 0
    T.child = torch.where(T.is_split[:, None], fc[:, None] + torch.arange(8)[None, :], torch.full((1, 8), -1))
    res = [int(v) for v in Td.res]
    T.base_index = torch.arange(res[0] * res[1] * res[2]).reshape(*res)
    T.sdf_nrm, T.centre = Td.nrm.cpu(), T.box_min + T.box_size * 0.5
    T.hit, T.min_step = T.sdf_val <= 1e-4, Td.min_step
    first = (H // 2) * W // CHUNK - n_chunks // 2            # chunks around the image centre (hit fraction ~ image mean x2)
    t0 = time.time()
    rays = hits = 0
    for c in range(first, first + n_chunks):
        sl = slice(c * CHUNK, c * CHUNK + pixels)
        uv_t = torch.from_numpy(uv[sl])[None]
        dirs, cam = orend.camera_rays(uv_t, torch.from_numpy(pose)[None], torch.from_numpy(K)[None])
        _, hit, _ = ooct.trace(T, cam, dirs, -1)
        n_hit = int(hit.sum())
        dr = {k: torch.from_numpy(v) for k, v in synth.pbr_draws(7, n_hit, chunk_id=c).items()}
        orend.forward(sd, T, uv_t, torch.from_numpy(pose)[None], torch.from_numpy(K)[None],
                      torch.ones(1, pixels, dtype=torch.bool), torch.full((pixels, 1), 0.5), dr, "Material", testing=True)
        rays += pixels
        hits += n_hit
    dt = time.time() - t0
    return {"value": rays / dt, "unit": "rays/s", "cores": cores, "kind": "port",
            "sample": f"{n_chunks} central {pixels}-px chunks of the 800x800 view ({hits} hit rays, {dt:.1f} s, "
                      f"oracle = PyTorch-CPU restatement of the reference, torch threads = {cores})",
            "hit_rays_per_s": hits / dt}


class PowerProbe:
    """Samples `rocm-smi --showpower` in a thread while the timed region runs: the dominant kernel sits on the package power
    cap, and the bench line should say so with a number.  Best effort: no rocm-smi, no field."""

    def __init__(self, period=0.4):
        import re
        import shutil
        import subprocess
        import threading
        self.samples, self.cap, self._stop = [], None, threading.Event()
        exe = shutil.which("rocm-smi") or ("/opt/rocm/bin/rocm-smi" if os.path.exists("/opt/rocm/bin/rocm-smi") else None)
        dev = int(os.environ.get("LOCAL_RANK", "0"))

        def read(extra):
            out = subprocess.run([exe, "-d", str(dev), "--showpower"] + extra, capture_output=True, text=True, timeout=3).stdout
            m = re.search(r"Package Power \(W\): ([0-9.]+)", out.split("Max")[0] if "Max" in out else out)
            c = re.search(r"Max Graphics Package Power \(W\): ([0-9.]+)", out)
            return (float(m.group(1)) if m else None), (float(c.group(1)) if c else None)

        def loop():
            try:
                _, self.cap = read(["--showmaxpower"])
                while not self._stop.wait(period):
                    w, _ = read([])
                    if w is not None:
                        self.samples.append(w)
            except Exception:
                pass

        self._thread = threading.Thread(target=loop, daemon=True) if exe else None
        if self._thread:
            self._thread.start()

    def stop(self):
        if not self._thread:
            return None
        self._stop.set()
        self._thread.join(timeout=5)
        if not self.samples:
            return None
        s = sorted(self.samples)
        return {"cap_w": self.cap, "max_w": s[-1], "median_w": s[len(s) // 2], "samples": len(s),
                "note": "rocm-smi package power sampled during the timed steps (samples between two launches read lower)"}


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU, the same command line
    under torch.distributed.run on 127.0.0.1) and hand their exit code back.  On a box with fewer than N devices the ranks
    share cuda:0 over gloo (RCCL refuses two ranks on one device) so that the multi-rank path can still be exercised; the
    JSON line says which backend ran."""
    import socket
    import subprocess
    env = dict(os.environ)
    n_dev = torch.cuda.device_count()
    if n_dev < args.gpus:
        env.setdefault("ROBIR_SHARE_GPU", "1")
        env.setdefault("ROBIR_DIST_BACKEND", "gloo")
        print(f"bench.py: {n_dev} device(s) visible for --gpus {args.gpus}: ranks share cuda:0 over "
              f"{env['ROBIR_DIST_BACKEND']} (functional run, not a scaling figure)", file=sys.stderr)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    # stdout carries ONE JSON line: anything else the ranks' libraries print there (gloo announces its peers on stdout) goes to stderr
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    for line in proc.stdout:
        out = (REAL_STDOUT or sys.stdout) if line.lstrip().startswith("{") else sys.stderr
        out.write(line)
        out.flush()
    raise SystemExit(proc.wait())


def set_precision(name, vis_override=None):
    """Select the arithmetic of every MLP kernel: returns (visibility-kernel mode, MLP mode, dtype string)."""
    from robir_amd import sg_render
    vis, mlp, dtype = PRECISIONS[name]
    vis = vis_override or vis
    sg_render.VIS_PRECISION = vis
    os.environ["ROBIR_MLP_PRECISION"] = mlp
    os.environ["ROBIR_CESR_PRECISION"] = "f16x1" if name == "f16" else mlp      # the f16 policy's CESR nets: plain f16 too (csrc/cesr_f16.hip, round 6)
    return vis, mlp, dtype


def vis_peak(vis):
    """Peak of the pipe the light-visibility kernel runs on, per ALGORITHMIC flop."""
    if vis == "fp32":
        return PEAK_FP32_MFMA_TFLOPS, "dense f32-input MFMA (v_mfma_f32_16x16x4_f32)"
    if vis == "f16x1":
        return PEAK_F16_MFMA_TFLOPS, "dense f16 MFMA 2500 TFLOP/s, one product per multiply-add (plain f16 operands: NARROWER than fp32)"
    if vis == "f16x6":
        from robir_amd import ops
        if ops.DVIS_X6_FP8:
            # k_dvis_x6t since round 6: four exact f16 products + the two outer products of the 2^-22 class as bf8 MFMAs at twice the f16 rate =
            # five f16-equivalent products per multiply-add: the bound of what the kernel executes MOVED UP with it (2500 / 5, not 2500 / 6)
            return PEAK_F16_MFMA_TFLOPS / 5.0, ("dense f16 MFMA 2500 TFLOP/s / 5 f16-equivalent products per multiply-add (three-piece operands: four exact f16 "
                                                "products + two bf8 products of the 2^-22 class on v_mfma_f32_16x16x128_f8f6f4 at twice the f16 rate)")
        return PEAK_F16_MFMA_TFLOPS / 6.0, "dense f16 MFMA 2500 TFLOP/s / 6 products per multiply-add (exact three-piece operands)"
    return PEAK_F16_MFMA_TFLOPS / 3.0, "dense f16 MFMA 2500 TFLOP/s / 3 (hi*hi, hi*lo, lo*hi products per multiply-add)"


REAL_STDOUT = None


def emit(line):
    out = REAL_STDOUT or sys.stdout
    out.write(json.dumps(line) + "\n")
    out.flush()


def dump_outputs(d, image):
    """The image of the last timed step, [H*W, 17] as render_view_sharded returns it, one float32 array [H, W, c] per field."""
    from robir_amd import parallel
    os.makedirs(d, exist_ok=True)
    img = image.float().cpu().numpy()
    widths = {"roughness": 1, "network_object_mask": 1}
    a = 0
    for name in parallel.TILE_FIELDS:
        c = widths.get(name, 3)
        np.save(os.path.join(d, name + ".npy"), np.ascontiguousarray(img[:, a:a + c].reshape(H, W, c)))
        a += c
    assert a == img.shape[1] == 17, (a, img.shape)


def runner_loop_replay(model, uv_d, pose_d, K_d, hdr, chunk=1024):
    """train_pbr.py:248-285 in its own shape: per 1024-pixel chunk one forward(), a few tone-mapped / detached fields kept, merged, read."""
    from robir_amd import deferred
    N = uv_d.shape[0]
    mask = torch.ones(1, N, dtype=torch.bool, device=uv_d.device)
    best = None
    with torch.no_grad():
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = []
            for a in range(0, N, chunk):
                sl = slice(a, min(N, a + chunk))
                out = model({"uv": uv_d[None, sl], "pose": pose_d[None], "intrinsics": K_d[None], "object_mask": mask[:, sl],
                             "hdr_shift": hdr[sl]}, trainstage="Material", train_spec=True)
                res.append({"sg_rgb": out["sg_rgb"].detach(), "indir_rgb": out["indir_rgb"].detach(), "vis_shadow": out["vis_shadow"].detach(),
                            "normal_map": out["normal_map"].detach(), "network_object_mask": out["network_object_mask"].detach()})
            merged = {k: torch.cat([r[k] for r in res], 0) for k in res[0]}
            host = {k: v.cpu() for k, v in merged.items()}
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
    assert host["sg_rgb"].shape[0] == N
    return {"value": N / best, "unit": "rays/s", "ms_per_view": best * 1e3, "chunks": (N + chunk - 1) // chunk,
            "deferred_chunks": int(model.__dict__.get("deferred_chunks", deferred.DEFAULT_CHUNKS)),
            "note": "unchanged call shape of the runners' plot loop, default settings; best of 2"}


def rccl_selfcheck(parallel, dev):
    import socket
    import torch.distributed as dist
    try:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(port))
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        parallel.init_distributed("nccl", dev)
        tiles = torch.rand(2048, 17, device=dev)
        ok = bool(torch.equal(parallel.gather_image(tiles, 2, 1024), tiles))
        res = {"backend": dist.get_backend(), "ranks": dist.get_world_size(), "device": str(dev), "tile_gather_ok": ok}
        dist.destroy_process_group()
        return res
    except Exception as e:  # noqa: BLE001   (reported, not fatal: the one-GPU measurement does not depend on it)
        return {"error": repr(e)[:200]}


def main():
    # stdout carries ONE JSON line and nothing else: file descriptor 1 is pointed at stderr for the whole run (RCCL prints a version
    # banner from C at communicator creation, the octree build prints like the reference), the line goes out through a saved duplicate
    global REAL_STDOUT
    sys.stdout.flush()
    REAL_STDOUT = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: start bench.py without a launcher (it starts its own "
                         f"ranks) or with torch.distributed.run --nproc-per-node {args.gpus}")
    # ROBIR_SHARE_GPU=1 + ROBIR_DIST_BACKEND=gloo: all ranks on cuda:0 (lets the multi-rank code path be exercised on a
    # 1-GPU box; RCCL refuses two ranks on one device).  Normal runs: one rank per GPU over RCCL ("nccl" on ROCm).
    if os.environ.get("ROBIR_SHARE_GPU") == "1":
        local = 0
    backend = os.environ.get("ROBIR_DIST_BACKEND", "nccl")
    from robir_amd import ops, renderer, synth, sg_render, parallel
    dev = parallel.bind_device(share_gpu=os.environ.get("ROBIR_SHARE_GPU") == "1")       # cuda:LOCAL_RANK
    assert dev.index == local
    dist = None
    rccl_check = None
    if world > 1:
        import torch.distributed as dist
        parallel.init_distributed(backend, dev)
    elif args.full and backend == "nccl" and os.environ.get("ROBIR_RCCL_SELFCHECK", "1") == "1":
        # one GPU: run the tile gather once through RCCL with a process group of one rank (outside the timed region), so that the line
        # says whether the collective backend of the multi-GPU path loads and runs on this box
        rccl_check = rccl_selfcheck(parallel, dev)

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_configs
    vis_mode, mlp_mode, dtype = set_precision(args.precision, os.environ.get("ROBIR_VIS_PRECISION") or args.vis_precision)
    t0 = time.time()
    import contextlib
    with contextlib.redirect_stdout(sys.stderr):     # the octree build prints like the reference; stdout carries only the JSON line
        model = renderer.build_synthetic_model(dev, seed=0, variance=0.3, scene=args.scene)
    torch.cuda.synchronize()
    build_s = time.time() - t0

    if args.config != 4:
        # one of the other BASELINE configurations as its own line (single GPU: they are parity-test cases, not scaling lines)
        if world > 1:
            raise SystemExit("--config 1/2/3/5 are single-GPU lines")
        bench_configs.install_timers()
        kw = {}
        if args.config == 5:
            n5 = args.config5_chunks or 1875
            kw = dict(first=0 if n5 == 1875 else (1875 - n5) // 2, nch=n5)
        with torch.no_grad():
            r = bench_configs.CONFIGS[args.config](model, reps=max(1, args.steps), **kw)
        ops.range_check(sync=True)
        line = {"metric": f"BASELINE.json configs[{args.config - 1}]: " + r["workload"], "value": r["value"], "unit": r["unit"],
                "n_gpus": 1, "steps": max(1, min(args.steps, bench_configs.REPS)), "warmup": 1, "ms_per_step": r["ms"],
                "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dtype, "data": "synthetic",
                "config": {"workload": r["workload"], "precision": args.precision, "octree_build_s": round(build_s, 2),
                           **{k: v for k, v in r.items() if k not in ("workload", "value", "unit", "ms", "roofline", "config")}},
                "roofline": r["roofline"],
                "note": "best of the timed repetitions; the headline metric is the default line (--config 4)"}
        emit(line)
        return

    timer = KernelTimer()
    if args.vis == "octree":
        from robir_amd.octree_tracing import OctreeVisModel
        model.visibility_network = OctreeVisModel(model.octree_ray_tracer)
        ops.dvis_octree = timer.wrap(ops.dvis_octree)
    else:
        ops.dvis_fused = timer.wrap(ops.dvis_fused)
    uv, _, K = synth.synth_camera(H, W)
    pose = view_pose(0)                                  # every rank works on the SAME view: the N = 1 workload
    uv_d, pose_d, K_d = torch.from_numpy(uv).to(dev), torch.from_numpy(pose).to(dev), torch.from_numpy(K).to(dev)
    hdr = torch.full((H * W, 1), 0.5, device=dev)
    stats = {}
    plan = parallel.plan_view(H * W, CHUNK, dev, interleave=True, chunks_per_pass=args.chunks_per_batch)

    def step():
        """One image: this rank's chunks (all of them at N = 1), then the all-gather of the tiles -> [H*W, 17] on every rank.
        Every step draws its random numbers from the same seed: the image does not depend on how many steps ran before it."""
        torch.manual_seed(STEP_SEED)
        return parallel.render_view_sharded(model, uv_d, pose_d, K_d, hdr, CHUNK, stats=stats, plan=plan)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    local_times = {}

    def timed(fn, steps, tag=None):
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = fn()
        torch.cuda.synchronize()
        t_own = time.perf_counter() - t0                  # this rank's own work, before it waits for the others
        barrier()
        dt = time.perf_counter() - t0
        if tag is not None:
            local_times[tag] = t_own
        if world > 1:
            tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dt = float(tmax)
        return dt, out

    def vis_roofline(vis, k_ms, k_n, evals):
        """`roofline` of the fused light-visibility kernel from its HIP-event durations and its own pair counter."""
        flops_per_launch = 2.0 * VIS_MACS_PER_EVAL * evals / max(k_n, 1)
        achieved = flops_per_launch / (k_ms * 1e-3) / 1e12 if k_ms > 0 else 0.0
        peak, note = vis_peak(vis)
        kern = "k_dvis_v2" if vis == "f16x3-auto" else ops.DVIS_KERNEL_NAMES.get(vis, "k_dvis_fused")
        traffic = TRAFFIC_B_PER_PAIR.get(vis, TRAFFIC_B_PER_PAIR["default"]) * evals / max(k_n, 1)
        hbm_gbs = traffic / (k_ms * 1e-3) / 1e9 if k_ms > 0 else 0.0
        return {"bound": "mfma", "kernel": kern + " (light-SG visibility MLP)", "achieved": achieved, "peak": peak,
                "unit": "TFLOP/s", "frac": achieved / peak,
                # BASELINE.json's metric also asks for the fraction of the HBM roofline: stated, although HBM does not bound this kernel
                "hbm_gb_s": hbm_gbs, "hbm_peak_gb_s": 8000.0, "hbm_frac": hbm_gbs / 8000.0,
                # HBM bytes per launch: B per (point, direction) pair measured with rocprofv3 --pmc FETCH_SIZE (x2 gfx950
                # correction) + WRITE_SIZE on this kernel family (profiles/), scaled to this launch's pair count: well under
                # 1 % of the HBM roofline -- the bound is the matrix pipe
                "traffic": traffic,
                "traffic_unit": "B/launch", "traffic_source": "derived",
                "pmc_file": TRAFFIC_PROFILE.get(vis, "profiles/r06_dvis_x6t_pmc.md"),
                "traffic_note": "bytes per pair of a separate PMC pass of the same kernel (2 x FETCH_SIZE + WRITE_SIZE) x this launch's pairs",
                "precision": vis, "peak_note": note, "frac_of_fp32_mfma_peak": achieved / PEAK_FP32_MFMA_TFLOPS,
                "frac_of_six_f16_products_bound": achieved / (PEAK_F16_MFMA_TFLOPS / 6.0) if vis == "f16x6" else None,
                "launches": k_n, "avg_launch_ms": k_ms, "evals_per_launch": evals / max(k_n, 1),
                "flops_per_eval": 2 * VIS_MACS_PER_EVAL}

    for _ in range(args.warmup):
        step()
    barrier()
    stats.clear()
    timer.on = True
    power = PowerProbe() if rank == 0 and args.full else None      # package power while the timed steps run (rocm-smi, best effort)
    dt, out = timed(step, args.steps, tag="step")
    power_line = power.stop() if power is not None else None
    timer.on = False
    ops.range_check(sync=True)                           # f16-piece activation-range sentinel: raises on overflow
    rays_total = H * W * args.steps
    hit_frac = float(out[:, 16].mean())
    evals = int(stats["diffuse_vis_evals"]) if "diffuse_vis_evals" in stats else 0
    k_ms, k_n = timer.stats()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out)

    per_rank = allgather_ms = None
    if world > 1:
        # SCALE-run diagnostics (VERDICT r5 task 6): what every rank did, so that a reader of the ONE line can tell load imbalance
        # (chunks, own step time, kernel time differ between ranks) from collective time (allgather_ms) from start-up skew (own step
        # times agree but the max-over-ranks wall time is longer).  Gathered OUTSIDE the timed region.
        n_own = sum(len(grp) for grp, _, _ in plan["passes"])
        mine = torch.tensor([float(n_own), local_times["step"] / args.steps * 1e3, k_ms * k_n / max(args.steps, 1), float(evals) / max(args.steps, 1)],
                            device=dev, dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        if dist.get_backend() == "nccl":
            dist.all_gather(allr, mine)
        else:
            host = [torch.zeros(4, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(host, mine.cpu())
            allr = host
        per_rank = [{"rank": r, "chunks": int(v[0]), "step_ms": float(v[1]), "dvis_kernel_ms_per_step": float(v[2]),
                     "visibility_pairs_per_step": float(v[3])} for r, v in enumerate(allr)]
        if args.full:
            # the collective alone: the padded tile gather of one view (what the end of every step does), timed over 5 repetitions
            per = (plan["n_chunks"] + world - 1) // world
            pad = torch.zeros(per * CHUNK, 17, device=dev)
            parallel.all_gather_tiles(pad)
            t_ag, _ = timed(lambda: parallel.all_gather_tiles(pad), 5)
            allgather_ms = t_ag / 5 * 1e3
        # the roofline of an N-rank line is the SLOWEST rank's kernel time over that rank's own pairs (rank 0's alone would mislead)
        slow = max(per_rank, key=lambda r: r["dvis_kernel_ms_per_step"])
        if slow["dvis_kernel_ms_per_step"] > 0 and k_n > 0:
            launches_per_step = k_n / max(args.steps, 1)
            k_ms, evals = slow["dvis_kernel_ms_per_step"] / launches_per_step, int(slow["visibility_pairs_per_step"] * args.steps)

    weak = None
    if world > 1 and args.full:
        # secondary figure: the weak form (rank r renders its own whole view r, tiles all-gathered)
        pose_r = torch.from_numpy(view_pose(rank)).to(dev)
        plan1 = dict(parallel.plan_view(H * W, CHUNK, dev), world=1)
        plan1["passes"] = [(list(range(H * W // CHUNK)), slice(0, H * W), False)]

        def weak_step():
            t = parallel.render_view_sharded(model, uv_d, pose_r, K_d, hdr, CHUNK, plan=plan1)
            return parallel.all_gather_tiles(t)
        weak_step()
        wdt, _ = timed(weak_step, 2)
        weak = {"value": world * H * W * 2 / wdt, "unit": "rays/s", "steps": 2, "ms_per_step": wdt / 2 * 1e3,
                "note": "one whole view per GPU (views differ in cost: hit fraction 0.65 .. 0.53)"}

    octree_line = None
    if args.vis == "octree":
        lay = [int(v) for v in ops.LAST_OCTREE_VIS_LAYOUT.cpu()]
        pairs, fetches, ray_steps = lay[0], lay[2], lay[3]
        # algorithmic bytes of one traced-visibility launch: the 32-byte octree records its lock-step iterations read, plus the
        # per-pair state written once and read once (pair 6 B, t 4, leaf 4, active 1, group 4) and the active flag re-read by
        # every one of the 33 iterations
        bytes_launch = 32.0 * fetches + pairs * (2 * 19.0 + 33.0)
        # Honest bound (VERDICT r5 task 7): the records are dependent 32-byte reads of a 29 MB table that sits in the L2 (4 MB per XCD) and
        # the 256 MB Infinity Cache, NOT in HBM -- so `achieved` / `peak` price the gathered bytes against the aggregate L2 bandwidth
        # (MI355X_MICROARCH.md: 34.5 TB/s), and the kernel is really latency x occupancy bound: `lockstep_iteration_ms` is what one
        # lock-step iteration costs per ray in flight.  The HBM reading of the same bytes is kept as a labelled side figure.
        gbs = bytes_launch / (k_ms * 1e-3) / 1e9 if k_ms > 0 else 0.0
        octree_line = {"bound": "hbm", "bound_note": "nominally the metric's HBM roofline; the table is L2 / Infinity-Cache resident, so the figures below are "
                                                     "against the AGGREGATE L2 bandwidth and as dependent-read latency -- this kernel is not an HBM-bandwidth kernel",
                       "kernel": "k_ovis_iter_list x33 + compaction / cull / fill / reduce (traced light visibility)",
                       "achieved": gbs, "peak": 34500.0, "unit": "GB/s", "frac": gbs / 34500.0,
                       "peak_note": "aggregate L2 bandwidth (MI355X_MICROARCH.md: 4 MiB per XCD, ~34.5 TB/s); the table never streams from HBM",
                       "if_priced_against_hbm_8TBs": gbs / 8000.0,
                       "traffic": None, "traffic_source": "not counted: gathers hit L2 / MALL (profiles/r05_bench_octree_vis_kernel_stats.md)",
                       "launches": k_n, "avg_launch_ms": k_ms, "pairs_per_launch": pairs,
                       "octree_records_read_per_ray": fetches / max(pairs, 1), "iterations_per_ray": ray_steps / max(pairs, 1),
                       "gathered_bytes_per_ray": 32.0 * fetches / max(pairs, 1),
                       "lockstep_iteration_ms": k_ms / max(ray_steps / max(pairs, 1), 1e-9) if k_ms > 0 else None,
                       "lockstep_iteration_note": "launch time / lock-step iterations per ray: the wall time of ONE dependent round of record reads "
                                                  "for all rays in flight (latency x occupancy is the real bound)"}
    line = None
    if rank == 0:
        roofline = vis_roofline(vis_mode, k_ms, k_n, evals)
        if power_line is not None:
            roofline["package_power"] = power_line
        line = {
            "metric": "PBR-stage rays/sec (128 SG lobes, 32 visibility samples/lobe), full forward render",
            "value": rays_total / dt, "unit": "rays/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": dtype, "data": "synthetic",
            "config": {"workload": "hotdog-like synthetic 800x800 full PBR forward (BASELINE.json configs[3]): ONE view = "
                                   "625 lock-step chunks of 1024 px, chunks sharded over the GPUs (c mod N), tiles all-gathered",
                       "image": [H, W], "chunk": CHUNK, "chunks_per_pass": args.chunks_per_batch,
                       "hit_fraction": round(hit_frac, 4), "octree_build_s": round(build_s, 2),
                       "octree_nodes": model.ray_tracer.sdf_octree.tables.B, "precision": args.precision, "scene": args.scene,
                       "visibility_kernel": vis_mode, "mlp_kernels": mlp_mode,
                       "ranks": world, "collective_backend": (("rccl (torch 'nccl')" if backend == "nccl" else backend) if world > 1 else None),
                       "rccl_selfcheck_world1": rccl_check,
                       "ranks_share_one_gpu": os.environ.get("ROBIR_SHARE_GPU") == "1" and world > 1,
                       "parallelism": f"chunk-shard x{world} of one view + all-gather"},
            "roofline": roofline if octree_line is None else octree_line,
        }
        if args.vis == "octree":
            line["metric"] = "PBR-stage rays/sec (128 SG lobes, 32 visibility samples/lobe), traced visibility (trace_vis)"
            line["config"]["visibility"] = "OctreeVisModel (secondary lock-step octree cast, max_iter 32, 2 M-pair batches)"
        if weak is not None:
            line["weak_views"] = weak
        if per_rank is not None:
            # DESIGN.md section 7's prediction for this N from the single-GPU step of the same precision (exact: 1358 ms of light
            # visibility + 54 ms of everything else, both proportional to a rank's chunks, + ~2 ms of per-pass launches and host
            # syncs + the tile gather): what the first SCALE run is held against
            base_ms = {"exact": 1260.0, "f16": 338.0, "split": 700.0, "fp32-mfma": 3650.0}.get(args.precision)
            line["per_rank"] = per_rank
            if allgather_ms is not None:
                line["allgather_ms"] = allgather_ms
            line["roofline"]["of_rank"] = max(per_rank, key=lambda r: r["dvis_kernel_ms_per_step"])["rank"]
            line["roofline"]["note_ranks"] = "kernel time and pair count of the SLOWEST rank (max over ranks of the per-step kernel time)"
            if base_ms is not None:
                line["predicted_ms_per_step"] = {"value": base_ms * math.ceil(625 / world) / 625 + 2.0 + 0.43 * (world - 1) / world,
                                                 "source": "DESIGN.md section 7: single-GPU step x ceil(625/N)/625 + ~2 ms per pass + tile gather at ~100 GB/s per "
                                                           "xGMI link; ranks sharing one GPU (functional runs) are NOT expected to meet it"}
    if args.full and world == 1 and not args.no_legs and args.vis == "mlp":
        # Side legs, each timed over its own loop: the same view and the same random draws in the other two precisions, and the
        # distance of every image from the f32-input-MFMA one (|a-b| / (|b| + mean|b|) over the 17 channels of all rays).
        images, legs = {}, {}
        for name in ("fp32-mfma", "exact") + (("split",) if args.with_split or args.precision == "split" else ()) + \
                ((args.precision,) if args.precision not in ("fp32-mfma", "exact", "split") else ()):
            v_mode, m_mode, leg_dtype = set_precision(name, None if name != args.precision else
                                                      (os.environ.get("ROBIR_VIS_PRECISION") or args.vis_precision))
            torch.manual_seed(20260928)
            images[name] = step()                           # also the warm-up of this precision (packs its weight blobs)
            if name == args.precision:
                continue
            timer.pairs.clear()
            timer.on = True
            stats.clear()
            t_leg, _ = timed(step, args.leg_steps)
            timer.on = False
            l_ms, l_n = timer.stats()
            l_evals = int(stats["diffuse_vis_evals"]) if "diffuse_vis_evals" in stats else 0
            legs[name] = {"value": H * W * args.leg_steps / t_leg, "unit": "rays/s", "steps": args.leg_steps, "warmup": 1,
                          "ms_per_step": t_leg / args.leg_steps * 1e3, "dtype": leg_dtype,
                          "roofline": vis_roofline(v_mode, l_ms, l_n, l_evals)}
        ops.range_check(sync=True)
        set_precision(args.precision, os.environ.get("ROBIR_VIS_PRECISION") or args.vis_precision)
        ref_img = images["fp32-mfma"]
        for name, img in images.items():
            if name == "fp32-mfma":
                continue
            ok = torch.isfinite(ref_img).all(-1) & torch.isfinite(img).all(-1)
            a, b = img[ok], ref_img[ok]
            rel = (a - b).abs() / (b.abs() + b.abs().mean(0, keepdim=True))
            flat = rel.flatten().float()
            flat = flat[torch.isfinite(flat)]
            q = torch.quantile(flat[:: max(1, flat.numel() // 4_000_000)], torch.tensor([0.5, 0.999], device=flat.device)) if flat.numel() else torch.zeros(2)
            d = {"max_rel_diff": float(rel.max()), "median_rel_diff": float(q[0]), "p99.9_rel_diff": float(q[1]),
                 "frac_entries_beyond_1e-4": float((rel > 1e-4).float().mean()),
                 "frac_entries_beyond_1e-5": float((rel > 1e-5).float().mean()), "rays_beyond_1e-3": int((rel > 1e-3).any(-1).sum())}
            (legs[name] if name in legs else line.setdefault("headline_image", {}))["distance_from_fp32_mfma_image"] = d
        line["legs"] = legs
        line["legs_note"] = ("same view, same draws; two fp32-accurate evaluations round differently (the exact-operand kernels are not "
                             "bitwise the f32-input MFMA's sums), so the entries beyond 1e-4 are rays on which a threshold decision -- "
                             "a sampled direction on the n.d > 1e-6 cull, a hit mask -- flips within that rounding; the median and the "
                             "99.9th percentile show the arithmetic (tests/test_precision_gpu.py anchors the modes on a float64 evaluation)")
    if args.full and world == 1 and not args.no_legs and args.vis == "mlp":
        # The other synthetic scene at the headline precision (2 steps): hit fraction, visibility pairs per hit ray and rate
        other = "nonconvex" if args.scene == "sphere" else "sphere"
        with contextlib.redirect_stdout(sys.stderr):
            model2 = renderer.build_synthetic_model(dev, seed=0, variance=0.3, scene=other)
        st2 = {}

        def step2():
            return parallel.render_view_sharded(model2, uv_d, pose_d, K_d, hdr, CHUNK, stats=st2, plan=plan)
        step2()
        st2.clear()
        t2, out2 = timed(step2, 2)
        hits2 = float(out2[:, 16].sum())
        line["other_scene"] = {"scene": other, "value": H * W * 2 / t2, "unit": "rays/s", "steps": 2, "ms_per_step": t2 / 2 * 1e3,
                               "hit_fraction": hits2 / (H * W), "octree_nodes": model2.ray_tracer.sdf_octree.tables.B,
                               "visibility_pairs_per_hit_ray": int(st2["diffuse_vis_evals"]) / 2 / max(hits2, 1.0),
                               "this_scene_pairs_per_hit_ray": evals / max(args.steps, 1) / max(hit_frac * H * W, 1.0)}
        del model2
    if args.full and world == 1 and not args.no_configs and args.vis == "mlp":
        # The other BASELINE configurations, outside the timed region, at the headline precision (--with-split: in split precision too)
        bench_configs.install_timers()
        cfgs = {}
        n5 = args.config5_chunks or 125
        for name in ((args.precision, "split") if args.with_split and args.precision != "split" else (args.precision,)):
            set_precision(name)
            with torch.no_grad():
                res = []
                for k in (1, 2, 3, 5):
                    kw = dict(first=(1875 - n5) // 2, nch=n5) if k == 5 else {}
                    r = bench_configs.CONFIGS[k](model, reps=2 if k != 5 else 1, **kw)
                    r["dtype"] = PRECISIONS[name][2]
                    res.append(r)
            cfgs[name] = res
        ops.range_check(sync=True)
        set_precision(args.precision, os.environ.get("ROBIR_VIS_PRECISION") or args.vis_precision)
        line["configs"] = cfgs
        line["configs_note"] = ("BASELINE.json configs 1, 2, 3, 5 (tools/bench_configs.py), best of 2 repetitions after a warm-up "
                                "(config 5: one pass over a band of chunks; `--config 5` times all 1875), single GPU, each with "
                                "the roofline of the op that dominates it from HIP events around that op")
    if args.full and world == 1 and not args.no_configs and args.vis == "mlp":
        # Three figures that used to be builder-only, outside the timed region, default settings:
        # (1) the whole BASELINE config 5 view, all 1875 chunks chunk by chunk (the `configs` entry above is a band of them)
        extras = {}
        with torch.no_grad():
            r5 = bench_configs.CONFIGS[5](model, reps=1, first=0, nch=1875)
        extras["config5_all_1875_chunks"] = {k: r5[k] for k in ("workload", "value", "unit", "ms") if k in r5}
        # (2) the same 800x800 view with TRACED light visibility (the reference's `trace_vis` switch: OctreeVisModel as VisModel)
        from robir_amd.octree_tracing import OctreeVisModel
        mlp_vis = model.visibility_network
        model.visibility_network = OctreeVisModel(model.octree_ray_tracer)
        try:
            def step_ov():
                return parallel.render_view_sharded(model, uv_d, pose_d, K_d, hdr, CHUNK, plan=plan)
            step_ov()
            t_ov, _ = timed(step_ov, 2)
        finally:
            model.visibility_network = mlp_vis
        extras["traced_visibility"] = {"value": H * W * 2 / t_ov, "unit": "rays/s", "steps": 2, "ms_per_step": t_ov / 2 * 1e3,
                                       "note": "`bench.py --vis octree` prints this mode as its own line with its roofline"}
        # (3) the reference's own call shape: the runners' plot loop (training/train_pbr.py:248-285) -- split_input into 1024-pixel
        # chunks, one forward() per chunk, merge_output, read the image -- replayed with DEFAULT settings (eval-mode chunk forwards
        # are recorded and run as passes of model.deferred_chunks chunks: robir_amd/deferred.py)
        extras["runner_plot_loop"] = runner_loop_replay(model, uv_d, pose_d, K_d, hdr)
        line["extras"] = extras
    if rank == 0:
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(model, args.cpu_baseline_chunks, uv, pose, K)
            # the reference's runners pin torch to one thread (training/train_pbr.py:24): that figure too, on a smaller sample
            one = cpu_baseline(model, 1, uv, pose, K, cores=1, pixels=args.cpu_baseline_1thread_pixels)
            line["cpu_baseline"]["single_thread"] = {k: one[k] for k in ("value", "unit", "cores", "sample", "hit_rays_per_s")}
        emit(line)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    main()
