#!/usr/bin/env python
"""Checks the texture-space rasteriser's arithmetic on the CPU: compiles tools/texbake_host.cpp (= robir_amd/csrc/texbake/texbake_math.h
built for the host as a stand-alone program, with plain loops) with the host C++ compiler, runs it on every raster case and every atlas
case of tests/texbake_restatement.py and compares the bytes with the numpy restatement: tile counts, face_id, barycentrics, atlas UVs.

    python tools/check_texbake_host.py          prints one line per case; exit status 1 if one differs
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
import texbake_restatement as tr  # noqa: E402


def compiler():
    return os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def build():
    """-> path of the program."""
    cxx = compiler()
    if cxx is None:
        raise SystemExit("no host C++ compiler found (set CXX)")
    out = os.path.join(tempfile.mkdtemp(prefix="tb_host_"), "texbake_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "robir_amd", "csrc"),
                    os.path.join(ROOT, "tools", "texbake_host.cpp"), "-o", out], check=True)
    return out


def host_raster(prog, uv, R):
    """-> (counts [F], face_id [R,R], bary [R,R,2]) of the host program."""
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 3, 2)
    d = os.path.dirname(prog)
    src, dst = os.path.join(d, "raster.in"), os.path.join(d, "raster.out")
    with open(src, "wb") as f:
        f.write(np.array([R, uv.shape[0]], dtype=np.int32).tobytes() + uv.tobytes())
    subprocess.run([prog, "raster", src, dst], check=True)
    blob = open(dst, "rb").read()
    F = uv.shape[0]
    counts = np.frombuffer(blob, dtype=np.int32, count=F)
    face_id = np.frombuffer(blob, dtype=np.int32, count=R * R, offset=4 * F).reshape(R, R)
    bary = np.frombuffer(blob, dtype=np.float32, count=2 * R * R, offset=4 * F + 4 * R * R).reshape(R, R, 2)
    return counts, face_id, bary


def host_atlas(prog, F, R):
    """-> uv [F,3,2], or None when the program refuses the cell size."""
    dst = os.path.join(os.path.dirname(prog), "atlas.out")
    r = subprocess.run([prog, "atlas", str(F), str(R), dst])
    if r.returncode == 2:
        return None
    if r.returncode != 0:
        raise RuntimeError(f"texbake_host atlas {F} {R}: exit status {r.returncode}")
    return np.fromfile(dst, dtype=np.float32).reshape(F, 3, 2)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(prog=None):
    """-> [(what, equal)] over every case."""
    prog = prog or build()
    rows = []
    for name, (uv, R) in tr.raster_cases().items():
        counts, face_id, bary = host_raster(prog, uv, R)
        ref_id, ref_bary = tr.raster(uv, R)
        rows.append((f"raster {name}: tile counts", np.array_equal(counts, tr.bin_counts(uv, R))))
        rows.append((f"raster {name}: face_id", np.array_equal(face_id, ref_id)))
        rows.append((f"raster {name}: bary", np.array_equal(bits(bary), bits(ref_bary))))
    for F, R in tr.ATLAS_CASES:
        uv = host_atlas(prog, F, R)
        rows.append((f"atlas F={F} R={R}: uv", uv is not None and np.array_equal(bits(uv), bits(tr.atlas_uv(F, R)))))
        rows.append((f"atlas F={F} R={R}: ownership", uv is not None and np.array_equal(host_raster(prog, uv, R)[1], tr.raster(uv, R)[0])))
    rows.append(("atlas F=200 R=59: refused", host_atlas(prog, 200, 59) is None))
    return rows


def main():
    bad = 0
    for what, ok in check():
        print(f"{what:48s} {'equal' if ok else 'DIFFERS'}")
        bad += not ok
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
