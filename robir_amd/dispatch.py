"""Which kernel family and which packed blob serve a call: the one table behind nets, sg_render, renderer and ops.dvis_fused.

Pure functions of plain Python values (no torch, no library).  The callers read the live settings (precision.mlp_precision(), the ops.*
toggles) on every call and pass them in; a setting that costs something to read (ops.sdf_ring_waves loads the legacy library,
ops.chunk_ids_ascending may read the device) is passed as a callable and asked only on the routes that depend on it.  Each function returns
an immutable route; tests/test_dispatch_cpu.py pins every row against tests/golden/dispatch_table.json (tools/gen_dispatch_golden.py).
"""
from collections import namedtuple

from .precision import check

# fn: the ops function; blob: key of the network's _BLOBS; scale_log2: pass packing.H3_SCALE_LOG2 (split-precision kernels); encode: the caller
# assembles feature rows first (no fused-encoding kernel on this route); flag: the 512-wide nets' `encoder` argument is passed
Net = namedtuple("Net", "fn blob scale_log2 encode flag", defaults=(False, False, False))
# fn(x | feature rows, M, *blobs, *sel, [scale_log2], *scales): sel = (full,) | (mode,) | (); scales over i = in_scale, o = out_scale, g = their
# product; rows: feature rows from ops.feat_pe10 (tangent rows with grad) instead of points
SdfCall = namedtuple("SdfCall", "fn blobs sel scale_log2 scales rows")
# combine: 'pair' (out, grad) as returned | 'value' (out, None) | 'column' (out[:, 0], grad) | 'precise' (out of the first call, grad of the second)
SdfRoute = namedtuple("SdfRoute", "name calls combine")
# resolved form, entry point, lives in the legacy library, weights and format (pack_vis_split keys, or an int), 'pblock' | 'stream' | 'point' | 'gen1'
Dvis = namedtuple("Dvis", "form entry legacy blob fmt layout")


# ------------------------------------------------------------------------------------------------ SDF network (NeuS shape)
def _sdf_route(name, fn, blobs, sel, scale_log2, scales, combine="pair", rows=False):
    return SdfRoute(name, (SdfCall(fn, blobs, sel, scale_log2, scales, rows),), combine)


# the rows of the table, built once; indexed by `full` or by mode = full + 2 grad + 4 precise
_NET, _NET_H3, _NET_X6 = ("sdf", "full"), ("sdf_h3", "full_h3"), ("x6_dist", "x6_full")
_VALUE_GRAD_H3 = _sdf_route("value_grad_h3", "sdf_value_grad", ("full_h3", "back_h3"), (), True, "io")
_VALUE_GRAD_X6 = [_sdf_route("value_grad_x6", "sdf_value_grad_x6", ("x6_full", "back_x6"), (), False, "io", c) for c in ("column", "pair")]
_VALUE_GRAD_F32 = [_sdf_route("value_grad_f32", "sdf_value_grad_f32", ("full", "back"), (), False, "io", c) for c in ("column", "pair")]
_PRECISE_SPLIT = SdfRoute("precise value + x6 gradient", (SdfCall("sdf_mlp_points", ("sdf",), (4,), False, "iog", False), _VALUE_GRAD_X6[1].calls[0]), "precise")
_POINTS_X6 = [_sdf_route("points_x6", "sdf_points_x6", (_NET_X6[f],), (bool(f),), False, "io", "value") for f in (0, 1)]
_POINTS_H3 = [_sdf_route("points_h3", "sdf_points_h3", (_NET_H3[f],), (bool(f),), True, "io", "value") for f in (0, 1)]
_POINTS_JVP_H3 = [_sdf_route("points_jvp_h3", "sdf_points_jvp_h3", (_NET_H3[f],), (bool(f),), True, "iog") for f in (0, 1)]
_MLP_POINTS = [_sdf_route("mlp_points", "sdf_mlp_points", (_NET[m & 1],), (m,), False, "iog") for m in range(8)]
_MLP_H3 = [_sdf_route("mlp_h3", "sdf_mlp_h3", (_NET_H3[m & 1],), (m,), True, "og", rows=True) for m in range(8)]
_MLP = [_sdf_route("mlp", "sdf_mlp", (_NET[m & 1],), (m,), False, "og", rows=True) for m in range(8)]


def sdf(full, grad, precise, M, mlp, fused_pe, sdf_kernel, sdf_grad, precise_grad_split, ring_waves, min_points=16384, f32_min_points=16384):
    """SDFNetwork.eval_points.  ring_waves: callable (ops.sdf_ring_waves), asked on the split-precision fused value route only;
    min_points / f32_min_points: ops.SDF_GRAD_MIN_POINTS / SDF_GRAD_F32_MIN_POINTS."""
    check("ROBIR_MLP_PRECISION", mlp)
    assert not (precise and full)
    mode = (1 if full else 0) + (2 if grad else 0) + (4 if precise else 0)
    h3, x6 = mlp == "f16x3", mlp == "f16x6"
    ring, reverse = sdf_kernel == "ring", sdf_grad == "reverse"
    if mode == 3 and h3 and ring and reverse and M >= min_points:
        return _VALUE_GRAD_H3       # values once + one row vector back through the transposed layers, instead of three tangent rows per point
    if grad and precise and x6 and fused_pe and reverse and precise_grad_split:
        # the octree's cell table (octree_tracing.build): the VALUE with the library-grade softplus (one row per point on the f32-input
        # MFMA), the GRADIENT by the policy's reverse pass on exact operands -- not three more tangent rows per point on the slow pipe
        return _PRECISE_SPLIT
    if grad and not precise and not h3 and fused_pe and reverse and M >= (1 if x6 else f32_min_points):
        # the same at the reference's precision: value pass on exact three-piece operands (three launches of 0.07 ms beat 0.31 at every
        # size) or the f32-input MFMA, + one pass over the transposed layers; all 257 outputs, of which sdf-only callers keep column 0
        return (_VALUE_GRAD_X6 if x6 else _VALUE_GRAD_F32)[mode & 1]
    if not grad and not precise and x6 and fused_pe:
        return _POINTS_X6[mode & 1]
    if not precise and h3 and ring and fused_pe:
        if grad:
            return _POINTS_JVP_H3[mode & 1]
        if ring_waves() == 8:       # value rows straight from the points: positional encoding fused into the network kernel (csrc/sdf_ring8.hip)
            return _POINTS_H3[mode & 1]
    if fused_pe and (precise or not h3):
        return _MLP_POINTS[mode]        # f32-input MFMA kernel with the encoding (tangent rows included) evaluated inside it
    return (_MLP_H3 if h3 and not precise else _MLP)[mode]       # feature rows


# ------------------------------------------------------------------------------------------------ the other stand-alone nets
def vis_mlp(mlp, fused_pe, points):
    """VisNetwork: points=True for (points, directions), False for feature rows [M,128] (the f32-input MFMA under 'fp32' and 'f16x6' alike)."""
    check("ROBIR_MLP_PRECISION", mlp)
    if points and fused_pe:
        return {"f16x6": Net("vis_x6_points", "full_x6"), "f16x3": Net("vis_mlp_points", "full_h3", True), "fp32": Net("vis_mlp_points", "full")}[mlp]
    return Net("vis_mlp_h3", "full_h3", True, points) if mlp == "f16x3" else Net("vis_mlp", "full", False, points)


def vis_halves(fused_pe):
    """The two first-layer halves of the fused light-visibility kernel (sg_render): straight from points / directions, or from PE rows."""
    return Net("linear_pe10_256", None) if fused_pe else Net("linear_64_256", None, False, True)


def color(mlp, fused_pe):
    """RenderingNetwork.forward; encode: assemble the [M,304] rows with ops.feat_color first."""
    check("ROBIR_MLP_PRECISION", mlp)
    if mlp == "f16x3":      # encoding inside the kernel | tail rows
        return Net("color_mlp_h3_points" if fused_pe else "color_mlp_h3_two", "c_h3", True)
    if not fused_pe:
        return Net("color_mlp", "c", False, True)
    return Net("color_x6_points", "c_x6") if mlp == "f16x6" else Net("color_mlp_points", "c")


def wide(mlp, fused_pe, points, encoder):
    """The 512-wide nets: encoder=True the SparseAE encoder (blob 'ae' = its half of pack_sparse_ae), False the indirect-illumination lobe net.
    Feature rows on exact operands exist for the encoder only; the lobe net's rows take the f32-input MFMA under 'f16x6'."""
    check("ROBIR_MLP_PRECISION", mlp)
    enc = points and not fused_pe
    h3, x6, f32 = ("enc_h3", "enc_x6", "ae") if encoder else ("lobe_h3", "lobe_x6", "lobe")
    if mlp == "f16x3":
        return Net("wide_mlp_points", h3, True, False, True) if points and fused_pe else Net("wide_mlp_h3", h3, True, enc, True)
    if mlp == "f16x6" and (encoder or (points and fused_pe)):
        return Net("wide_x6_points", x6, False, False, True) if points and fused_pe else Net("wide_x6", x6, False, enc, True)
    if points and fused_pe:
        return Net("wide_mlp_points", f32, False, False, True)
    return Net("ae_encode" if encoder else "illum_mlp", f32, False, enc)


def cesr(mlp, cesr, fused_pe, points):
    """The two CESR nets (shadow_net, normal_net).  points=True: the caller holds points; encode says whether it must encode them itself
    (ROBIR_SDF_FUSED_PE=0) and then take the rows route.  cesr_precision() selects the plain-f16 kernel only; the other fused kernels and
    the rows follow mlp_precision()."""
    check("ROBIR_MLP_PRECISION", mlp)
    check("ROBIR_CESR_PRECISION", cesr)
    if points and fused_pe:
        if cesr == "f16x1":     # plain f16, ONE product per multiply-add (csrc/cesr_f16.hip): the labelled throughput mode, NARROWER than fp32
            return Net("cesr_net_f16_points", "w512_f16")
        return {"f16x3": Net("cesr_net_points", "w512_h3", True), "f16x6": Net("cesr_net_x6_points", "w512_x6"), "fp32": Net("cesr_net_points", "w512")}[mlp]
    return Net("cesr_net_h3", "w512_h3", True, points) if mlp == "f16x3" else Net("cesr_net", "w512", False, points)


# ------------------------------------------------------------------------------------------------ fused light-visibility kernel
_X6_HEAD, _H3_HEAD = ("hidden_x6_head", "x6_head_scale_log2"), ("hidden_h3_head", "h3_head_scale_log2")
_DVIS = {       # resolved form: entry point, legacy library, weights and format (pack_vis_split keys or an int), layout
    "fp32": ("rb_dvis_fused", False, "hidden", 0, "gen1"),
    "f16x3": ("rb_dvis_fused", True, "hidden_h3", "h3_scale_log2", "gen1"),       # first generation: one 16-sample tile per wave, weights by LDS-DMA
    "f16x3-v2": ("rb_dvis_fused_v2", True, *_H3_HEAD, "point"),       # two tiles per wave, one workgroup per CU, head on the matrix pipe (vis_diffuse_v2.hip)
    "f16x3-v3": ("rb_dvis_stream", True, *_H3_HEAD, "stream"),        # global tile list + persistent grid (vis_diffuse_v3.hip)
    "f16x6-1t": ("rb_dvis_fused_x6", True, *_X6_HEAD, "point"),       # round 3's one tile per wave, one workgroup per point (vis_diffuse_x6.hip)
    # two tiles per wave, two of the six products on the bf8 MFMA (vis_diffuse_x6t.hip; format 8 names the bf8 weight layout)
    "f16x6-pt": ("rb_dvis_fused_x6t", False, "hidden_x6_head_fp8", 8, "point"),       # a persistent grid that takes point after point
    "f16x6-stream": ("rb_dvis_stream_x6", False, "hidden_x6_head_fp8", 8, "stream"),  # ... over the global tile list: bit-identical to -pt
    "f16x1": ("rb_dvis_stream_f16", False, *_X6_HEAD, "stream")}        # generation 1; 2: format 1 = the h-only blob; 3: the point-block form
DVIS_FORMS = tuple(_DVIS)


def dvis(precision, n, L, nsamp, x6_form, f16_gen, ascending, stream_max_points=8192, stream_short_list=1024):
    """ops.dvis_fused.  ascending: callable (chunk ids never decrease), asked for 'f16x1' with generation 3 only; stream_max_points /
    stream_short_list: ops.DVIS_STREAM_MAX_POINTS / DVIS_STREAM_SHORT_LIST."""
    check("ROBIR_VIS_PRECISION", precision)
    LS = L * nsamp
    tiles = LS % 16 == 0          # the tile-list forms cut a point's L*nsamp directions into whole 16-sample tiles
    if precision == "f16x3-auto":
        # same arithmetic, bit-identical results: the streaming family balances small launches (a single 1024-pixel chunk) over the CUs; at
        # whole-view sizes the one-point-per-workgroup kernel is as fast and needs no scratch
        precision = "f16x3-v3" if n <= stream_max_points and tiles else "f16x3-v2"
    if precision == "f16x6":
        # 'auto': the persistent tile-list form for launches up to stream_max_points points (balanced over the CUs, 0.4 % tile padding) and at
        # EVERY size for short direction lists (the CESR hook's nsamp = 8: the per-point prologue / half-empty last round weigh 5-6 %,
        # tools/ab_dvis_forms.py), one workgroup per point beyond (one launch, no 10 GB of scratch) and for lights that do not cut into tiles
        stream_ok = tiles and (n <= stream_max_points or LS <= stream_short_list)
        precision = x6_form if x6_form != "auto" else ("f16x6-stream" if stream_ok else "f16x6-pt")
    if precision not in DVIS_FORMS:
        raise ValueError("ROBIR_DVIS_X6_FORM must be auto, f16x6-pt, f16x6-stream or f16x6-1t")
    entry, legacy, blob, fmt, layout = _DVIS[precision]
    if precision == "f16x1":       # plain f16, one product: NARROWER than fp32
        if not tiles:
            raise ValueError(f"the f16 throughput kernel (ROBIR_PRECISION=f16) exists in the tile-list form only: L*nsamp = {L}*{nsamp} must be a "
                             "multiple of 16 -- use ROBIR_PRECISION=exact for this light")
        if f16_gen == 3 and ascending():       # csrc/vis_diffuse_f16p.hip; else csrc/vis_diffuse_f16t.hip
            entry, blob, fmt, layout = "rb_dvis_pblock_f16", "hidden_f16_head", None, "pblock"
        elif f16_gen >= 2:
            blob, fmt = "hidden_f16_head", 1
    return Dvis(precision, entry, legacy, blob, fmt, layout)
