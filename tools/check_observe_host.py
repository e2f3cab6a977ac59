#!/usr/bin/env python
"""Checks the observation arithmetic on the CPU: compiles tools/observe_host.cpp (= robir_amd/csrc/observe/observe_math.h built for the
host as a stand-alone program, with plain loops) with the host C++ compiler, runs it on every case of tests/observe_restatement.py and
compares the bytes with the numpy fp32 restatement: the scatter, the selection for n_obs in (1, 3), the gather of the selected rows and
the weighted colour statistics.

    python tools/check_observe_host.py          prints one line per case; exit status 1 if one differs
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
import observe_restatement as obr  # noqa: E402


def compiler():
    return os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def build(extra=()):
    """-> path of the program.  extra: more compiler flags (e.g. -fsanitize=address,undefined: the program has its own main)."""
    cxx = compiler()
    if cxx is None:
        raise SystemExit("no host C++ compiler found (set CXX)")
    out = os.path.join(tempfile.mkdtemp(prefix="ob_host_"), "observe_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "robir_amd", "csrc"),
                    os.path.join(ROOT, "tools", "observe_host.cpp"), "-o", out], check=True)
    return out


def host_run(prog, case, n_obs, masks=True):
    """-> dict of the host program's outputs for one case."""
    M, N, H, W, C = case.M, case.N, case.H, case.W, case.images.shape[-1]
    d = os.path.dirname(prog)
    src, dst = os.path.join(d, "case.in"), os.path.join(d, "case.out")
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).tobytes()
    with open(src, "wb") as f:
        f.write(np.array([M, N, H, W, C, int(masks), n_obs], dtype=np.int32).tobytes() + f32(case.x) + f32(case.normals) + f32(case.cam_loc)
                + f32(case.pose_inv) + f32(case.K) + f32(case.images) + (f32(case.masks) if masks else b"")
                + np.ascontiguousarray(case.vis(), dtype=np.uint8).tobytes() + f32(case.draws))
    subprocess.run([prog, src, dst], check=True)
    blob, pos, out = open(dst, "rb").read(), 0, {}
    layout = [("uv", np.float32, (M, N, 2)), ("view_dir", np.float32, (M, N, 3)), ("rgb", np.float32, (M, N, C)), ("valid", np.uint8, (M, N)),
              ("index", np.int32, (n_obs, N)), ("seen", np.int32, (N,)),
              ("g_uv", np.float32, (n_obs, N, 2)), ("g_view_dir", np.float32, (n_obs, N, 3)), ("g_rgb", np.float32, (n_obs, N, C)),
              ("g_valid", np.uint8, (n_obs, N)),
              ("weight", np.float32, (N,)), ("mean", np.float32, (N, C)), ("var", np.float32, (N, C)), ("count", np.int32, (N,))]
    for name, dt, shape in layout:
        n = int(np.prod(shape))
        out[name] = np.frombuffer(blob, dtype=dt, count=n, offset=pos).reshape(shape)
        pos += n * np.dtype(dt).itemsize
    assert pos == len(blob), (pos, len(blob))
    return out


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_case(prog, case, n_obs, masks=True):
    """-> [(what, equal)] of one case."""
    got = host_run(prog, case, n_obs, masks)
    sc = case.scatter(np.float32, masks)
    index, seen = obr.select(case.vis(), case.draws, n_obs)
    g = obr.gather(index, sc)
    acc = obr.accumulate(case.x, case.normals, *case.cams(), case.images, case.vis())
    tag = f"{case.name} n_obs={n_obs}" + ("" if masks else " no masks")
    rows = [(f"{tag}: scatter {k}", same(got[k], sc[k])) for k in ("uv", "view_dir", "rgb", "valid")]
    rows += [(f"{tag}: select index", same(got["index"], index)), (f"{tag}: select count", same(got["seen"], seen))]
    rows += [(f"{tag}: gather {k}", same(got["g_" + k], g[k])) for k in ("uv", "view_dir", "rgb", "valid")]
    rows += [(f"{tag}: accumulate {k}", same(got[k], acc[k])) for k in ("weight", "mean", "var", "count")]
    return rows


def check(prog=None):
    """-> [(what, equal)] over every case and both n_obs, and one case without masks."""
    prog = prog or build()
    rows = []
    for case in obr.cases().values():
        for n_obs in obr.N_OBS:
            rows += check_case(prog, case, n_obs)
    rows += check_case(prog, obr.cases()["M5_N300_24x40_random"], 3, masks=False)
    return rows


def main():
    bad = 0
    for what, ok in check():
        print(f"{what:64s} {'equal' if ok else 'DIFFERS'}")
        bad += not ok
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
