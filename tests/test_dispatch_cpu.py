"""Kernel selection (robir_amd/dispatch.py) against tests/golden/dispatch_table.json, the behaviour recorded by tools/gen_dispatch_golden.py
before the selection logic moved behind the table.  No GPU, no built library: the recorder replaces the `ops` functions, the packers and the
entry-point calls.

  table     the pure functions return, for every case of the fixture, the route that was recorded;
  wiring    the real nets modules and the real ops.dvis_fused, driven through the recorder, reproduce the fixture case for case (fails if a
            caller ignores the table);
  default   under the default policy (and f16-vis, with and without the plain-f16 CESR nets) no call shape consults the legacy library or
            ops.sdf_ring_waves -- the host-side statement of tests/test_default_library_gpu.py;
  totality  every combination of valid inputs has a route, an invalid precision string raises precision.py's ValueError.
"""
import itertools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_dispatch_golden as gen  # noqa: E402
from robir_amd import dispatch, nets, packing, precision  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return gen.load()


def section(golden, name):
    """(case, recorded route or None) over the section, in the fixture's order."""
    s = golden["sections"][name]
    axes = [(a, [tuple(v) if isinstance(v, list) else v for v in vals]) for a, vals in s["axes"]]
    assert [(a, list(v)) for a, v in axes] == [(a, list(v)) for a, v in next(x[1] for x in gen.SECTIONS if x[0] == name)], "axes of the fixture"
    cases = list(gen.cases(axes))
    assert len(cases) == len(s["index"])
    return [(c, golden["routes"][i] if i >= 0 else None) for c, i in zip(cases, s["index"])]


def env_precisions(policy, mlp_override, cesr_override):
    """(mlp_precision(), cesr_precision()) as precision.py derives them from the three variables."""
    mlp = mlp_override or precision.POLICIES[policy][1]
    return mlp, cesr_override or ("f16x1" if policy == "f16" and not mlp_override else mlp)


def blob_matches(table, key, tag):
    """tag(s) recorded for a blob argument were made by the packer that table[key] names, with its keyword arguments."""
    packer, prefix, kw = table[key]
    tags = tag if isinstance(tag, list) else [tag]
    name = packer.__name__.lstrip("_") if callable(packer) else packer
    return all(t.startswith(name + "(") and ("first key " + prefix) in t and all(f"{k}={v!r}" in t for k, v in kw.items()) for t in tags)


SCALES = {"i": ("in_scale", 2.0), "o": ("out_scale", 0.25), "g": ("grad_scale", 0.5)}       # what gen.drive_sdf passes


def check_sdf_call(c, name, args, grad):
    assert name == c.fn
    blobs = [args[k] for k in ("blob", "back") if k in args]
    assert len(blobs) == len(c.blobs) and all(blob_matches(nets.SDFNetwork._BLOBS, k, t) for k, t in zip(c.blobs, blobs)), (c, args)
    assert tuple(args[k] for k in ("full", "mode") if k in args) == c.sel, (c, args)
    assert args.get("scale_log2") == (packing.H3_SCALE_LOG2 if c.scale_log2 else None), (c, args)
    for letter, (param, value) in SCALES.items():
        assert args.get(param, 1.0) == (value if letter in c.scales else 1.0), (c, args)


def test_table_sdf(golden):
    names = set()
    for case, rec in section(golden, "sdf_eval_points"):
        if rec is None:
            continue
        asked = []
        route = dispatch.sdf(ring_waves=lambda: asked.append(1) or case["ring_waves"], **{k: v for k, v in case.items() if k != "ring_waves"})
        calls = [c for c in rec["calls"] if c[0] != "feat_pe10"]
        feats = [c[1] for c in rec["calls"] if c[0] == "feat_pe10"]
        assert len(calls) == len(route.calls) and len(feats) == sum(c.rows for c in route.calls), (case, route)
        assert all(f["jvp"] == case["grad"] and f["scale"] == 2.0 for f in feats)
        for c, (name, args) in zip(route.calls, calls):
            check_sdf_call(c, name, args, case["grad"])
        assert bool(asked) == rec["ring_waves"] == rec["legacy"], (case, route)
        assert route.combine == ("precise" if len(calls) == 2 else route.combine)
        names.add(route.name + (" (waves asked)" if asked and route.name == "mlp_h3" else ""))
    assert names == {"value_grad_h3", "precise value + x6 gradient", "value_grad_x6", "value_grad_f32", "points_x6", "points_h3", "points_jvp_h3",
                     "mlp_points", "mlp_h3", "mlp_h3 (waves asked)", "mlp"}


# The network kernels each public call shape runs, as routes of the table (e: mlp, cesr, fused_pe of the case)
def _vis(e, points):
    return (dispatch.vis_mlp(e[0], e[2], points), nets.VisNetwork._BLOBS)


def _enc(e, points):
    return (dispatch.wide(e[0], e[2], points, encoder=True), nets.SparseAE._BLOBS)


def _lobe(e):
    return (dispatch.wide(e[0], e[2], True, encoder=False), nets.IndirctIllumNetwork._BLOBS)


def _cesr(e, points, fused=None):
    return (dispatch.cesr(e[0], e[1], e[2] if fused is None else fused, points), nets.SDFNetwork._BLOBS_512)


def _sdf(e, full, grad):
    r = dispatch.sdf(full, grad, False, 5, e[0], e[2], "ring", "reverse", True, lambda: 8)
    return [(c, nets.SDFNetwork._BLOBS) for c in r.calls]


NET_ROUTES = {
    "vis.logits_from_points": lambda e: [_vis(e, True)], "vis.logits_from_features": lambda e: [_vis(e, False)], "vis.forward": lambda e: [_vis(e, True)],
    "ae.run": lambda e: [_enc(e, False)], "ae.run(X_noisy)": lambda e: [_enc(e, False)] * 2, "ae.run(X_noisy, need_first=False)": lambda e: [_enc(e, False)],
    "ae.run_points": lambda e: [_enc(e, True)], "ae.run_pass": lambda e: [_enc(e, False)], "ae.encode": lambda e: [_enc(e, False)],
    "ae.forward": lambda e: [_enc(e, False)], "illum.forward": lambda e: [_lobe(e), _enc(e, False)], "illum.forward(no_hdr)": lambda e: [_lobe(e), _enc(e, False)],
    "material.forward": lambda e: [_enc(e, False), _enc(e, False), _enc(e, True)], "material.forward(train_norm)": lambda e: [_enc(e, False)] * 2,
    "color.forward": lambda e: [(dispatch.color(e[0], e[2]), nets.RenderingNetwork._BLOBS)],
    "sdf.forward": lambda e: _sdf(e, True, False), "sdf.sdf": lambda e: _sdf(e, False, False), "sdf.gradient": lambda e: _sdf(e, False, True),
    "normal.forward": lambda e: [_cesr(e, False)], "normal._cesr_points": lambda e: [_cesr(e, True, True)], "shadow.forward": lambda e: [_cesr(e, False)],
    "shadow.eval_point_labels(points)": lambda e: [_cesr(e, True, True)], "shadow.eval_point_labels(rows)": lambda e: [_cesr(e, False)],
}
HELPERS = ("feat_", "ae_latent", "ae_decode", "illum_decode", "axpy", "abs_scale", "normalize3", "material_decode")      # not selected by the table


def test_table_nets(golden):
    assert set(NET_ROUTES) == set(gen.NET_CALLS)
    for case, rec in section(golden, "nets"):
        mlp, cesr = env_precisions(case["policy"], case["mlp_override"], case["cesr_override"])
        want = NET_ROUTES[case["call"]]((mlp, cesr, case["fused_pe"]))
        got = [c for c in rec["calls"] if not c[0].startswith(HELPERS)]
        assert [r.fn for r, _ in want] == [c[0] for c in got], (case, want, got)
        for (r, table), (name, args) in zip(want, got):
            key = r.blobs[0] if isinstance(r, dispatch.SdfCall) else r.blob
            tag = args["blob"]
            if key == "ae":       # the encoder half of pack_sparse_ae
                assert tag.endswith("[0]")
            assert blob_matches(table, key, tag), (case, r, tag)
            assert args.get("scale_log2") == (packing.H3_SCALE_LOG2 if r.scale_log2 else None), (case, r, args)
            if isinstance(r, dispatch.Net):
                assert ("encoder" in args) == r.flag, (case, r, args)
        encodes = [r.encode for r, _ in want if isinstance(r, dispatch.Net)]
        if case["call"] in ("vis.logits_from_points", "vis.forward", "ae.run_points", "color.forward"):       # the route's own encoding step
            first = {"vis": "feat_vis", "ae.": "feat_pe10", "col": "feat_color"}[case["call"][:3]]
            assert (first in [c[0] for c in rec["calls"]]) == encodes[-1], (case, want)


def test_table_dvis(golden):
    for case, rec in section(golden, "dvis_fused"):
        asked = []
        args = dict(precision=case["precision"], n=case["n"], L=case["L_nsamp"][0], nsamp=case["L_nsamp"][1], x6_form=case["x6_form"],
                    f16_gen=case["f16_gen"], ascending=lambda: asked.append(1) or case["chunk_ids"] != "descending" or case["n"] < 2)      # what ops.chunk_ids_ascending answers
        if "raises" in rec:
            with pytest.raises(ValueError) as e:
                dispatch.dvis(**args)
            assert f"ValueError: {e.value}" == rec["raises"] and not rec["calls"]
            continue
        r = dispatch.dvis(**args)
        (entry, ints), = rec["calls"]
        blob = f"split[{r.blob!r}]"
        fmt = [] if r.fmt is None else [f"split[{r.fmt!r}]" if isinstance(r.fmt, str) else r.fmt]
        L, nsamp = case["L_nsamp"]
        want = {"pblock": [case["n"], blob, L, nsamp, 0, (case["n"] + 15) // 16 + (0 if case["chunk_ids"] == "none" else 1), 0],
                "stream": [case["n"], blob, L, nsamp, 0] + fmt + [0], "point": [case["n"], blob, L, nsamp, 0] + fmt,
                "gen1": [case["n"], blob, "split['w_last']", "split['b_last']", L, nsamp, 0, 5 if r.legacy else 0] + fmt}[r.layout]
        assert (entry, ints) == (r.entry, want), (case, r, rec)
        assert (r.legacy, bool(asked)) == (rec["legacy"], rec["ascending"]), (case, r, rec)
        assert r.form in dispatch.DVIS_FORMS


def test_wiring(golden):
    """The callers execute the table: nets, and ops.dvis_fused, through the generator's own recorder."""
    m = gen.build_nets()
    with gen.Recorder() as rec:
        for name, _, _ in gen.SECTIONS:
            got = gen.record(name, rec, m)
            want = section(golden, name)
            assert len(got) == len(want)
            for g, (case, w) in zip(got, want):
                assert (None if g is None else json.loads(json.dumps(g))) == w, (name, case)


@pytest.mark.parametrize("policy,cesr", [("exact", ""), ("f16-vis", ""), ("f16-vis", "f16x1")])
def test_default_policies_stay_in_the_default_library(golden, policy, cesr):
    seen = 0
    for case, rec in section(golden, "nets"):
        if (case["policy"], case["mlp_override"], case["cesr_override"], case["fused_pe"]) == (policy, "", cesr, True):
            assert not rec["legacy"] and not rec["ring_waves"], (case, rec)
            seen += 1
    assert seen == len(gen.NET_CALLS)
    mlp = precision.POLICIES[policy][1]
    for case, rec in section(golden, "sdf_eval_points"):       # every eval_points shape at the shipped settings of the toggles
        if rec is not None and (case["mlp"], case["fused_pe"], case["sdf_kernel"], case["sdf_grad"], case["precise_grad_split"]) == (mlp, True, "ring", "reverse", True):
            assert not rec["legacy"] and not rec["ring_waves"], (case, rec)
            r = dispatch.sdf(ring_waves=None, **{k: v for k, v in case.items() if k != "ring_waves"})      # never asked: None is not called
            assert all(c.fn in ("sdf_points_x6", "sdf_value_grad_x6", "sdf_mlp_points") for c in r.calls)
    vis = precision.POLICIES[policy][0]
    for case, rec in section(golden, "dvis_fused"):
        if (case["precision"], case["x6_form"], case["f16_gen"]) == (vis, "auto", 3) and "raises" not in rec:
            assert not rec["legacy"], (case, rec)


def test_totality():
    B = (False, True)
    for mlp, fused, points in itertools.product(("fp32", "f16x3", "f16x6"), B, B):
        for r in (dispatch.vis_mlp(mlp, fused, points), dispatch.color(mlp, fused), dispatch.wide(mlp, fused, points, True),
                  dispatch.wide(mlp, fused, points, False)) + tuple(dispatch.cesr(mlp, c, fused, points) for c in ("f16x1", "f16x3", "fp32", "f16x6")):
            assert isinstance(r, dispatch.Net) and r.fn and r.blob
            assert not (r.encode and not points) or r.fn == "color_mlp"        # rows never need encoding (the colour net always starts from points)
        for full, grad, precise, M, kernel, gmode, split, waves in itertools.product(B, B, B, (0, 1, 16384), ("ring", "v1"), ("reverse", "forward"), B, (4, 8)):
            if not (precise and full):
                assert dispatch.sdf(full, grad, precise, M, mlp, fused, kernel, gmode, split, lambda: waves).calls
    assert dispatch.vis_halves(True).fn == "linear_pe10_256" and dispatch.vis_halves(False).encode
    for bad in ("bf16", "", "f16x1"):
        with pytest.raises(ValueError, match="ROBIR_MLP_PRECISION must be f16x6, fp32 or f16x3"):
            dispatch.sdf(True, False, False, 1, bad, True, "ring", "reverse", True, lambda: 8)
        for fn in (lambda: dispatch.vis_mlp(bad, True, True), lambda: dispatch.color(bad, True), lambda: dispatch.wide(bad, True, True, True),
                   lambda: dispatch.cesr(bad, "f16x6", True, True)):
            with pytest.raises(ValueError, match="ROBIR_MLP_PRECISION"):
                fn()
    with pytest.raises(ValueError, match="ROBIR_CESR_PRECISION must be f16x1, f16x6, fp32 or f16x3"):
        dispatch.cesr("f16x6", "bf16", True, True)
    with pytest.raises(ValueError, match="ROBIR_VIS_PRECISION must be one of"):
        dispatch.dvis("f16", 1, 128, 32, "auto", 3, lambda: True)
    with pytest.raises(ValueError, match="ROBIR_DVIS_X6_FORM"):
        dispatch.dvis("f16x6", 1, 128, 32, "f16x6-2t", 3, lambda: True)


def test_dispatch_is_pure():
    """The table imports neither torch nor the library loader."""
    src = open(os.path.join(ROOT, "robir_amd", "dispatch.py")).read()
    assert "import torch" not in src and "_lib" not in src and "import ops" not in src


def test_dead_x6_fp8_variable_is_ignored():
    """ROBIR_DVIS_X6_FP8 once named the build form of k_dvis_x6t; there is one form now, and a fresh interpreter that finds the variable set to
    0 still routes the two-tile kernel to the bf8 weight layout (format 8)."""
    code = ("from robir_amd import dispatch, ops\n"
            "assert ops.DVIS_X6_FP8 is True\n"
            "r = dispatch.dvis('f16x6', 1, 128, 32, 'auto', 3, lambda: True)\n"
            "print(r.blob, r.fmt)\n")
    env = dict(os.environ, ROBIR_DVIS_X6_FP8="0", PYTHONPATH=os.pathsep.join([ROOT] + [p for p in (os.environ.get("PYTHONPATH"),) if p]))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["hidden_x6_head_fp8", "8"]
