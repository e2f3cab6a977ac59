#!/usr/bin/env python
"""Checks the atlas fit's arithmetic on the CPU: compiles tools/texfit_host.cpp (= robir_amd/csrc/texfit/texfit_math.h built for the host as
a stand-alone program, with plain loops) with the host C++ compiler, runs it on the uv cases, the pair lists and the Adam cases of
tests/texfit_restatement.py and compares the bytes with the numpy restatement: taps and fetch for both filters and several resolutions,
the gather that transposes the fetch, the lazy Adam step.

    python tools/check_texfit_host.py               prints one line per case; exit status 1 if one differs
    python tools/check_texfit_host.py --sanitize    the same with the program built under -fsanitize=address,undefined
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
import texfit_restatement as tf  # noqa: E402

SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")


def compiler():
    return os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def build(extra=()):
    """-> path of the program."""
    cxx = compiler()
    if cxx is None:
        raise SystemExit("no host C++ compiler found (set CXX)")
    out = os.path.join(tempfile.mkdtemp(prefix="tf_host_"), "texfit_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "robir_amd", "csrc"),
                    os.path.join(ROOT, "tools", "texfit_host.cpp"), "-o", out], check=True)
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


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def host_taps(prog, uv, R, filt):
    uv = f32(uv).reshape(-1, 2)
    n = uv.shape[0]
    blob = _run(prog, "taps", i32([n, R, filt]).tobytes() + uv.tobytes())
    return np.frombuffer(blob, dtype=np.int32, count=4 * n).reshape(n, 4), np.frombuffer(blob, dtype=np.float32, offset=16 * n).reshape(n, 4)


def host_fetch(prog, planes, texel, weight, C):
    R, Cs = planes.shape[0], planes.shape[2]
    n = texel.shape[0]
    blob = _run(prog, "fetch", i32([n, R, Cs, C]).tobytes() + f32(planes).tobytes() + i32(texel).tobytes() + f32(weight).tobytes())
    return np.frombuffer(blob, dtype=np.float32).reshape(n, C)


def host_scatter(prog, pair_row, pair_weight, seg_start, g_tex):
    n, C = g_tex.shape
    P, T = len(pair_row), len(seg_start) - 1
    blob = _run(prog, "scatter", i32([n, C, P, T]).tobytes() + i32(pair_row).tobytes() + f32(pair_weight).tobytes() + i32(seg_start).tobytes()
                + f32(g_tex).tobytes())
    return np.frombuffer(blob, dtype=np.float32).reshape(T, C)


def host_adam(prog, case):
    planes, m, v = case["planes"], case["m"], case["v"]
    R, Cs, C, T = planes.shape[0], planes.shape[2], m.shape[2], len(case["seg_texel"])
    t = case["t"]
    d = np.concatenate([case["lr"], case["lo"], case["hi"], [case["beta1"], case["beta2"], case["eps"], 1.0 - case["beta1"] ** t,
                                                              1.0 - case["beta2"] ** t]]).astype(np.float64)
    blob = _run(prog, "adam", i32([R, Cs, C, T]).tobytes() + d.tobytes() + f32(planes).tobytes() + f32(m).tobytes() + f32(v).tobytes()
                + i32(case["seg_texel"]).tobytes() + f32(case["grad"]).tobytes())
    a = np.frombuffer(blob, dtype=np.float32)
    np_, nm = R * R * Cs, R * R * C
    return a[:np_].reshape(R, R, Cs), a[np_:np_ + nm].reshape(R, R, C), a[np_ + nm:].reshape(R, R, C)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def restated_adam(case):
    planes, m, v = case["planes"].copy(), case["m"].copy(), case["v"].copy()
    tf.adam(planes, m, v, case["seg_texel"], case["grad"], case["lr"], case["lo"], case["hi"], case["beta1"], case["beta2"], case["eps"], case["t"])
    return planes, m, v


def check(prog=None):
    """-> [(what, equal)] over every case."""
    prog = prog or build()
    rows = []
    rng = np.random.default_rng(2)
    for R in (1, 8, 64):
        uv = tf.tap_uvs(R)
        planes = rng.uniform(0.05, 1.0, (R, R, 8)).astype(np.float32)
        for filt in (0, 1):
            for n in (1, 63, 64, 65, 257, len(uv)):
                got_t, got_w = host_taps(prog, uv[:n], R, filt)
                want_t, want_w = tf.taps(uv[:n], R, filt)
                rows.append((f"taps R {R} filter {filt} n {n}", np.array_equal(got_t, want_t) and np.array_equal(bits(got_w), bits(want_w))))
            for C in (4, 8):
                got = host_fetch(prog, planes, want_t, want_w, C)
                rows.append((f"fetch R {R} filter {filt} C {C}", np.array_equal(bits(got), bits(tf.fetch(planes, want_t, want_w, C)))))
    for C in (1, 4, 16):
        pr, pw, ss, g = tf.scatter_case(C)
        rows.append((f"scatter C {C}", np.array_equal(bits(host_scatter(prog, pr, pw, ss, g)), bits(tf.scatter(pr, pw, ss, g)))))
    uv = tf.tap_uvs(8)
    t, w = tf.taps(uv, 8, 1)
    pr, pw, st, ss = tf.sort_pairs(t, w, 8)
    g = rng.normal(size=(len(uv), 4)).astype(np.float32)
    rows.append(("scatter of the sorted taps, R 8", np.array_equal(bits(host_scatter(prog, pr, pw, ss, g)), bits(tf.scatter(pr, pw, ss, g)))))
    for Cs, C, T, step in tf.ADAM_CASES:
        case = tf.adam_case(Cs, C, T, step)
        got, want = host_adam(prog, case), restated_adam(case)
        rows.append((f"adam Cs {Cs} C {C} T {T} t {step}", all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, want))))
    return rows


def main():
    bad = 0
    for what, ok in check(build(SANITIZE) if "--sanitize" in sys.argv[1:] else None):
        print(f"{what:48s} {'equal' if ok else 'DIFFERS'}")
        bad += not ok
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
