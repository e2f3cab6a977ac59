"""Kernel-selection fixture: tests/golden/dispatch_table.json.

Which `ops` functions, packed blobs and entry points serve a call is host-side policy; this tool records it without a GPU or a built library.
The `ops` functions the networks call (sdf_*, feat_*, color_*, vis_*, wide_*, cesr_*, illum_*, ae_*, linear_*, axpy, abs_scale, normalize3,
material_decode), every packing.pack_*, ops.sdf_ring_waves, ops.call / ptr / stream_ptr and _lib.call_legacy are replaced by recorders; the
robir_amd.nets modules are built on the CPU and driven through every public call shape over the cross product of the settings, and the real
ops.dvis_fused over its own.  Per case, in call order: each ops function with its non-tensor arguments (bound to parameter names), for every
blob the packer that produced it, the entry point with its integer arguments and the pack_vis_split entries it was given, and whether the
legacy library, ops.sdf_ring_waves or ops.chunk_ids_ascending was consulted.  Distinct routes are stored once; a section maps its cases
(row-major over its axes) to route indices, -1 for a combination the call refuses by assertion.

    python tools/gen_dispatch_golden.py [output.json]

The tool touches only names that exist before and after the selection logic moved into robir_amd/dispatch.py: regenerate after adding a route
and review the diff of the fixture.  tests/test_dispatch_cpu.py imports the recorder and the sections from here.
"""
import ctypes
import inspect
import itertools
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from robir_amd import _lib, nets, ops, packing, precision  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch_table.json")
ENV = ("ROBIR_PRECISION", "ROBIR_MLP_PRECISION", "ROBIR_CESR_PRECISION", "ROBIR_VIS_PRECISION", "ROBIR_RANGE_CHECK")
OPS_PREFIXES = ("sdf_", "feat_", "color_", "vis_", "wide_", "cesr_", "illum_", "ae_", "linear_")
OPS_NAMES = ("axpy", "abs_scale", "normalize3", "material_decode")
OPS_TOGGLES = ("SDF_FUSED_PE", "SDF_KERNEL", "SDF_GRAD", "DVIS_X6_FORM", "DVIS_F16_GEN")
N_RESULTS = {"sdf_mlp": 2, "sdf_mlp_points": 2, "sdf_mlp_h3": 2, "sdf_points_jvp_h3": 2, "sdf_value_grad": 2, "sdf_value_grad_f32": 2,
             "sdf_value_grad_x6": 2, "ae_latent": 2, "material_decode": 6}
SPLIT_BLOBS = ("point", "dir", "hidden", "hidden_h3", "hidden_h3_head", "hidden_x6_head", "hidden_x6_head_fp8", "hidden_f16_head", "w_last",
               "b_last")
SPLIT_INTS = {"h3_scale_log2": 1005, "h3_head_scale_log2": 1003, "x6_head_scale_log2": 1006}      # values that name their key


def legacy_symbols():
    hdr = open(os.path.join(ROOT, "include", "robir_hip_legacy.h")).read()
    return set(re.findall(r"^(?:int|long|const char\*) (rb_[a-z0-9_]+)\s*\(", hdr, re.M))


class Blob:
    """Stand-in for a packed blob (or a tuple / dict of them): remembers the packer call that made it and the path into its result."""

    def __init__(self, tag):
        self.tag = tag

    def __getitem__(self, i):
        return Blob(f"{self.tag}[{i!r}]")

    def __iter__(self):
        return iter((self[0], self[1]))


class Fake:
    """Stand-in for an output tensor: every method and index gives another one."""
    shape = (1, 1)

    def __getitem__(self, i):
        return self

    def __getattr__(self, name):
        return lambda *a, **k: self


class _Ptr:
    def __init__(self, tag):
        self.tag = tag


def describe(v):
    if isinstance(v, Blob):
        return v.tag
    if isinstance(v, (torch.Tensor, Fake)):
        return "T"
    if isinstance(v, (tuple, list)):
        return [describe(x) for x in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return type(v).__name__


class Recorder:
    """Context manager: installs the recorders and restores every patched name, module toggle and environment variable on exit."""

    def __init__(self):
        self.waves = 8
        self._saved = []
        self._legacy_syms = legacy_symbols()
        self.begin()

    def begin(self):
        self.calls, self.flags = [], {"legacy": False, "ring_waves": False, "ascending": False}

    def end(self):
        return dict(self.flags, calls=self.calls)

    def _set(self, mod, name, value):
        self._saved.append((mod, name, getattr(mod, name)))
        setattr(mod, name, value)

    def _op(self, name, real):
        sig = inspect.signature(real)

        def rec(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            self.calls.append([name, {n: describe(v) for n, v in b.arguments.items()}])
            n_out = N_RESULTS.get(name, 1)
            return Fake() if n_out == 1 else tuple(Fake() for _ in range(n_out))
        return rec

    def _packer(self, name, real):
        sig = inspect.signature(real)

        def rec(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            sd = b.arguments.get("sd")
            args = [f"{n}={v!r}" for n, v in b.arguments.items() if n not in ("sd", "device", "layers")]
            if isinstance(sd, dict):
                args.append("first key " + min(sd))
            return Blob(f"{name}({', '.join(args)})")
        return rec

    def _entry(self, name, *args):
        if name in self._legacy_syms:
            self.flags["legacy"] = True
        keys = {v: k for k, v in SPLIT_INTS.items()}
        out = []
        for a in args:
            if isinstance(a, _Ptr):
                if a.tag is not None:
                    out.append(a.tag)
            elif isinstance(a, (ctypes.c_int, ctypes.c_long)):
                out.append(f"split[{keys[a.value]!r}]" if a.value in keys else a.value)
        self.calls.append([name, out])

    def _entry_legacy(self, name, *args):
        self.flags["legacy"] = True
        self._entry(name, *args)

    def _ring_waves(self):
        self.flags["legacy"] = self.flags["ring_waves"] = True
        return self.waves

    def __enter__(self):
        self._env = {k: os.environ.pop(k, None) for k in ENV}
        for name in OPS_TOGGLES:
            self._set(ops, name, getattr(ops, name))
        self._set(nets, "PRECISE_GRAD_SPLIT", nets.PRECISE_GRAD_SPLIT)
        for name, fn in list(vars(ops).items()):
            if inspect.isfunction(fn) and (name.startswith(OPS_PREFIXES) or name in OPS_NAMES):
                self._set(ops, name, self._op(name, fn))
        for name, fn in list(vars(packing).items()):
            if inspect.isfunction(fn) and name.startswith("pack_"):
                self._set(packing, name, self._packer(name, fn))
        self._set(ops, "sdf_ring_waves", self._ring_waves)
        self._set(ops, "call", self._entry)
        self._set(ops, "ptr", lambda t: _Ptr(t.tag if isinstance(t, Blob) else None))
        self._set(ops, "stream_ptr", lambda: None)
        self._set(_lib, "call_legacy", self._entry_legacy)
        real_ascending = ops.chunk_ids_ascending

        def ascending(chunk_id):
            self.flags["ascending"] = True
            return real_ascending(chunk_id)
        self._set(ops, "chunk_ids_ascending", ascending)
        return self

    def __exit__(self, *exc):
        for mod, name, value in reversed(self._saved):
            setattr(mod, name, value)
        self._saved = []
        for k, v in self._env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        return False

    def setenv(self, **kv):
        """ROBIR_<NAME> = value for each NAME=value; an empty value unsets."""
        for k, v in kv.items():
            os.environ.pop("ROBIR_" + k, None)
            if v:
                os.environ["ROBIR_" + k] = v


# ------------------------------------------------------------------------------------------------ the networks, on the CPU
def build_nets():
    torch.manual_seed(0)
    m = {"vis": nets.VisNetwork(10, 10, [256] * 4), "ae": nets.SparseAE(63, 5),
         "ae_input": nets.SparseAE(60, 3, out_act=None, smooth_on_latent=False),
         "illum": nets.IndirctIllumNetwork(10, [512] * 4, 24), "illum_no_hdr": nets.IndirctIllumNetwork(10, [512] * 4, 24, no_hdr=True),
         "material": nets.EnvmapMaterialNetwork(multires=10), "color": nets.RenderingNetwork(256, "idr", 9, 3, 256, 4),
         "sdf": nets.SDFNetwork(3, 257, 256, 8), "normal": nets.SDFNetwork(63, 3, 512, 8, multires=0),
         "shadow": nets.SDFNetwork(191, 2, 512, 8, multires=0)}
    for net in m.values():
        net.eval()
    return m


def _t(*shape):
    return torch.zeros(*shape)


NET_CALLS = {
    "vis.logits_from_points": lambda m: m["vis"].logits_from_points(_t(2, 3), _t(8, 3), rep=4),
    "vis.logits_from_features": lambda m: m["vis"].logits_from_features(_t(5, 128)),
    "vis.forward": lambda m: m["vis"](_t(5, 3), _t(5, 3)),
    "ae.run": lambda m: m["ae"].run(_t(5, 64), noise=_t(5, 32)),
    "ae.run(X_noisy)": lambda m: m["ae_input"].run(_t(5, 64), X_noisy=_t(5, 64)),
    "ae.run(X_noisy, need_first=False)": lambda m: m["ae_input"].run(_t(5, 64), X_noisy=_t(5, 64), need_first=False),
    "ae.run_points": lambda m: m["ae"].run_points(_t(5, 3), _t(5, 32)),
    "ae.run_pass": lambda m: m["ae_input"].run_pass(_t(5, 64)),
    "ae.encode": lambda m: m["ae"].encode(_t(5, 63)),
    "ae.forward": lambda m: m["ae"](_t(5, 63), noise=_t(5, 32)),
    "illum.forward": lambda m: m["illum"](_t(5, 3), _t(5, 1), noise=_t(5, 64)),
    "illum.forward(no_hdr)": lambda m: m["illum_no_hdr"](_t(5, 3), _t(5, 1), noise=_t(5, 63)),
    "material.forward": lambda m: m["material"](_t(5, 3), noise={"spec": _t(5, 32), "normal": _t(5, 60)}),
    "material.forward(train_norm)": lambda m: m["material"](_t(5, 3), train_norm=True, noise={"normal": _t(5, 60)}),
    "color.forward": lambda m: m["color"](_t(5, 3), _t(5, 3), _t(5, 3), _t(5, 256), x_scale=2.0),
    "sdf.forward": lambda m: m["sdf"](_t(5, 3)),
    "sdf.sdf": lambda m: m["sdf"].sdf(_t(5, 3)),
    "sdf.gradient": lambda m: m["sdf"].gradient(_t(5, 3)),
    "normal.forward": lambda m: m["normal"](_t(5, 63)),
    "normal._cesr_points": lambda m: m["normal"]._cesr_points(_t(5, 3), 5, 0),
    "shadow.forward": lambda m: m["shadow"](_t(5, 191)),
    "shadow.eval_point_labels(points)": lambda m: m["shadow"].eval_point_labels(_t(5, 3), 128),
    "shadow.eval_point_labels(rows)": lambda m: m["shadow"].eval_point_labels(_t(5, 64), 128),
}

SDF_AXES = (("mlp", ("fp32", "f16x3", "f16x6")), ("fused_pe", (False, True)), ("sdf_kernel", ("ring", "v1")),
            ("sdf_grad", ("reverse", "forward")), ("precise_grad_split", (True, False)), ("ring_waves", (8, 4)), ("full", (False, True)),
            ("grad", (False, True)), ("precise", (False, True)), ("M", (1, 16383, 16384)))
NETS_AXES = (("policy", tuple(precision.POLICIES)), ("mlp_override", ("", "fp32", "f16x3", "f16x6")), ("cesr_override", ("", "f16x1", "f16x6")),
             ("fused_pe", (False, True)), ("call", tuple(NET_CALLS)))
DVIS_AXES = (("precision", precision.VIS_MODES), ("n", (1, 8192, 8193)), ("L_nsamp", ((128, 32), (128, 8), (3, 8))),
             ("x6_form", ("auto", "f16x6-pt", "f16x6-stream", "f16x6-1t")), ("f16_gen", (1, 2, 3)),
             ("chunk_ids", ("ascending", "descending", "none")))


def cases(axes):
    names = [a[0] for a in axes]
    for combo in itertools.product(*(a[1] for a in axes)):
        yield dict(zip(names, combo))


def drive_sdf(rec, m, c):
    if c["precise"] and c["full"]:
        return None
    rec.setenv(PRECISION="", MLP_PRECISION=c["mlp"], CESR_PRECISION="")
    ops.SDF_FUSED_PE, ops.SDF_KERNEL, ops.SDF_GRAD = c["fused_pe"], c["sdf_kernel"], c["sdf_grad"]
    nets.PRECISE_GRAD_SPLIT, rec.waves = c["precise_grad_split"], c["ring_waves"]
    rec.begin()
    m["sdf"].eval_points(_t(c["M"], 3), 2.0, 0.25, full=c["full"], grad=c["grad"], precise=c["precise"])
    return rec.end()


def drive_nets(rec, m, c):
    rec.setenv(PRECISION=c["policy"], MLP_PRECISION=c["mlp_override"], CESR_PRECISION=c["cesr_override"])
    ops.SDF_FUSED_PE, ops.SDF_KERNEL, ops.SDF_GRAD, nets.PRECISE_GRAD_SPLIT, rec.waves = c["fused_pe"], "ring", "reverse", True, 8
    rec.begin()
    NET_CALLS[c["call"]](m)
    return rec.end()


class _Split(dict):
    """pack_vis_split's result with stand-in blobs and scale entries whose values name their keys."""

    def __init__(self):
        super().__init__({k: Blob(f"split[{k!r}]") for k in SPLIT_BLOBS}, **SPLIT_INTS)


def drive_dvis(rec, m, c):
    n, (L, nsamp) = c["n"], c["L_nsamp"]
    ops.DVIS_X6_FORM, ops.DVIS_F16_GEN = c["x6_form"], c["f16_gen"]
    chunk_id, C = None, 1
    if c["chunk_ids"] != "none":
        C = 2
        chunk_id = (torch.arange(n) >= n // 2).to(torch.int32)
        if c["chunk_ids"] == "descending":
            chunk_id = 1 - chunk_id
    LS = L * nsamp
    rec.begin()
    try:
        ops.dvis_fused(_t(n, 3), chunk_id, _t(1), _t(1), _t(C * LS, 3), _t(1), _t(1), _Split(), L, nsamp, precision=c["precision"])
    except ValueError as e:
        return dict(rec.end(), raises=f"ValueError: {e}")
    return rec.end()


SECTIONS = (("sdf_eval_points", SDF_AXES, drive_sdf), ("nets", NETS_AXES, drive_nets), ("dvis_fused", DVIS_AXES, drive_dvis))


def record(section, rec, m):
    """[route or None per case of the section, row-major over its axes]."""
    name, axes, drive = next(s for s in SECTIONS if s[0] == section)
    return [drive(rec, m, c) for c in cases(axes)]


def build_table():
    routes, index_of, sections = [], {}, {}
    m = build_nets()
    with Recorder() as rec:
        for name, axes, _ in SECTIONS:
            index = []
            for r in record(name, rec, m):
                if r is None:
                    index.append(-1)
                    continue
                key = json.dumps(r, sort_keys=True)
                if key not in index_of:
                    index_of[key] = len(routes)
                    routes.append(key)
                index.append(index_of[key])
            sections[name] = {"axes": [[a, list(v)] for a, v in axes], "index": index}
    return routes, sections


def dumps(routes, sections):
    """One route per line, 64 case indices per line: a changed route shows as a one-line diff."""
    out = ['{"routes": [', ",\n".join(routes), '],', '"sections": {']
    secs = []
    for name, s in sections.items():
        idx = s["index"]
        rows = ",\n".join(", ".join(str(i) for i in idx[a:a + 64]) for a in range(0, len(idx), 64))
        secs.append(f'{json.dumps(name)}: {{"axes": {json.dumps(s["axes"])},\n"index": [\n{rows}]}}')
    out += [",\n".join(secs), "}}"]
    return "\n".join(out) + "\n"


def load(path=GOLDEN):
    return json.load(open(path))


if __name__ == "__main__":
    text = dumps(*build_table())
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(path, "w") as f:
        f.write(text)
    t = json.loads(text)
    print(f"{path}: {len(t['routes'])} routes, " + ", ".join(f"{k}: {len(v['index'])} cases" for k, v in t["sections"].items()),
          f"({len(text)} bytes)")
