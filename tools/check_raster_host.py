#!/usr/bin/env python
"""Checks the camera-space rasteriser's arithmetic on the CPU: compiles tools/raster_host.cpp (= robir_amd/csrc/raster/raster_math.h built
for the host as a stand-alone program, with plain loops) with the host C++ compiler, runs it on the projection of an icosphere, on every
raster case of tests/meshrender_restatement.py and on the G-buffer case, and compares the bytes with the numpy fp32 restatement: screen
coordinates, tile counts, face_id, weights, depth, position, uv, view direction, both plane filters, vertex normals.

    python tools/check_raster_host.py          prints one line per case; exit status 1 if one differs
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import meshrender_restatement as mr  # noqa: E402


def compiler():
    return os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def build(extra=()):
    """-> path of the program."""
    cxx = compiler()
    if cxx is None:
        raise SystemExit("no host C++ compiler found (set CXX)")
    out = os.path.join(tempfile.mkdtemp(prefix="rs_host_"), "raster_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "robir_amd", "csrc"),
                    os.path.join(ROOT, "tools", "raster_host.cpp"), "-o", out], check=True)
    return out


def _run(prog, mode, blob):
    d = os.path.dirname(prog)
    src, dst = os.path.join(d, mode + ".in"), os.path.join(d, mode + ".out")
    with open(src, "wb") as f:
        f.write(blob)
    subprocess.run([prog, mode, src, dst], check=True)
    return open(dst, "rb").read()


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def host_project(prog, vertices, pose_inv, K):
    v = f32(vertices).reshape(-1, 3)
    blob = _run(prog, "project", np.array([v.shape[0]], dtype=np.int32).tobytes() + f32(pose_inv).tobytes() + f32(K).tobytes() + v.tobytes())
    return np.frombuffer(blob, dtype=np.float32).reshape(-1, 4)


def host_raster(prog, screen, faces, H, W, near=mr.NEAR, cull=0):
    """-> (counts [F], face_id [H,W], bary [H,W,2], depth [H,W]) of the host program."""
    s, fc = f32(screen).reshape(-1, 4), np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    hdr = np.array([H, W, s.shape[0], fc.shape[0], cull], dtype=np.int32).tobytes() + np.array([near], dtype=np.float32).tobytes()
    blob = _run(prog, "raster", hdr + s.tobytes() + fc.tobytes())
    F, n = fc.shape[0], H * W
    counts = np.frombuffer(blob, dtype=np.int32, count=F)
    face_id = np.frombuffer(blob, dtype=np.int32, count=n, offset=4 * F).reshape(H, W)
    bary = np.frombuffer(blob, dtype=np.float32, count=2 * n, offset=4 * (F + n)).reshape(H, W, 2)
    depth = np.frombuffer(blob, dtype=np.float32, count=n, offset=4 * (F + 3 * n)).reshape(H, W)
    return counts, face_id, bary, depth


def host_gbuffer(prog, face_id, bary, faces, vertices, uv, cam, planes=None, filter=1, vnormals=None, index=None):
    H, W = face_id.shape
    fc, v = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3), f32(vertices).reshape(-1, 3)
    R, C = (planes.shape[0], planes.shape[2]) if planes is not None else (0, 0)
    n = H * W if index is None else len(index)
    hdr = np.array([H, W, v.shape[0], fc.shape[0], R, C, filter, vnormals is not None, -1 if index is None else n], dtype=np.int32)
    blob = hdr.tobytes() + np.ascontiguousarray(face_id, dtype=np.int32).tobytes() + f32(bary).tobytes() + fc.tobytes() + v.tobytes()
    blob += f32(uv).tobytes() + (f32(vnormals).tobytes() if vnormals is not None else b"") + f32(cam).tobytes()
    blob += (f32(planes).tobytes() if planes is not None else b"") + (np.ascontiguousarray(index, dtype=np.int64).tobytes() if index is not None else b"")
    a = np.frombuffer(_run(prog, "gbuffer", blob), dtype=np.float32)
    out, o = {}, 0
    for key, c in (("position", 3), ("uv", 2), ("view_dir", 3), ("tex", C), ("normal", 3 if vnormals is not None else 0)):
        if c:
            out[key] = a[o:o + n * c].reshape(n, c)
            o += n * c
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def camera(H=64, W=64):
    from robir_amd import synth
    _, _, K = synth.synth_camera(H, W)
    pose = mr.rotated_pose()
    return pose, mr.pose_inverse(pose), K


def check(prog=None):
    """-> [(what, equal)] over every case."""
    prog = prog or build()
    rows = []
    pose, pinv, K = camera()
    for sub in (1, 3):
        v, f = mr.icosphere(sub)
        screen = host_project(prog, v, pinv, K)
        ref = mr.project(v, pinv, K)
        rows.append((f"icosphere {f.shape[0]}: screen", np.array_equal(bits(screen), bits(ref))))
        for cull in (0, 1, 2):
            got, want = host_raster(prog, ref, f, 64, 64, cull=cull), mr.raster(ref, f, 64, 64, cull=cull)
            rows.append((f"icosphere {f.shape[0]} cull {cull}: face_id", np.array_equal(got[1], want[0])))
            rows.append((f"icosphere {f.shape[0]} cull {cull}: bary, depth",
                         np.array_equal(bits(got[2]), bits(want[1])) and np.array_equal(bits(got[3]), bits(want[2]))))
    for name, (screen, faces, H, W) in mr.raster_cases().items():
        for cull in (0, 1, 2):
            counts, face_id, bary, depth = host_raster(prog, screen, faces, H, W, cull=cull)
            ref_id, ref_bary, ref_depth = mr.raster(screen, faces, H, W, cull=cull)
            rows.append((f"raster {name} cull {cull}: tile counts", np.array_equal(counts, mr.bin_counts(screen, faces, H, W, cull=cull))))
            rows.append((f"raster {name} cull {cull}: face_id", np.array_equal(face_id, ref_id)))
            rows.append((f"raster {name} cull {cull}: bary, depth",
                         np.array_equal(bits(bary), bits(ref_bary)) and np.array_equal(bits(depth), bits(ref_depth))))
    verts, faces, uv, planes, vn = mr.gbuffer_case()
    pose, pinv, K = camera(13, 21)
    screen = mr.project(verts, pinv, K)
    face_id, bary, _ = mr.raster(screen, faces, 13, 21)
    hit = np.nonzero(face_id.reshape(-1) >= 0)[0]
    for filt in (0, 1):
        for index in (None, hit, np.array([0, 5, -1, 13 * 21, hit[0] if hit.size else 0], dtype=np.int64)):
            got = host_gbuffer(prog, face_id, bary, faces, verts, uv, pose[:3, 3], planes, filt, vn, index)
            want = mr.gbuffer(face_id, bary, faces, verts, uv, pose[:3, 3], planes, filt, vn, index)
            form = "image" if index is None else f"list {len(index)}"
            rows.append((f"gbuffer filter {filt} {form}", all(np.array_equal(bits(got[k]), bits(want[k])) for k in want) and set(got) == set(want)))
    return rows


def main():
    bad = 0
    for what, ok in check():
        print(f"{what:48s} {'equal' if ok else 'DIFFERS'}")
        bad += not ok
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
