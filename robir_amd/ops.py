"""Thin Python bindings over the C-ABI (include/robir_hip.h): allocate outputs with torch, pass raw pointers,
sizes and the current HIP stream.  No arithmetic happens here."""
import ctypes
import functools
import os

import torch

from . import _lib, dispatch
from ._lib import ptr, stream_ptr, call

c_long, c_int, c_float = ctypes.c_long, ctypes.c_int, ctypes.c_float


def _f32(t):
    assert t.dtype == torch.float32, t.dtype
    return t.contiguous()


RANGE_FAMILIES = ("light-visibility kernel (rb_dvis_fused*)", "visibility MLP (rb_vis_mlp_h3 / rb_vis_x6_points)",
                  "SDF MLP (rb_sdf_mlp_h3 / rb_sdf_x6_points / rb_sdf_value_grad*)", "colour MLP (rb_color_mlp_h3 / rb_color_x6_points)",
                  "512-wide nets (rb_wide_mlp_h3 / rb_wide_x6*)", "CESR nets (rb_cesr_net_h3 / rb_cesr_net_x6_points)")


def range_check(sync=False):
    """Raise RobirHipError if a split-precision or exact-operand kernel saw an activation beyond the f16 range of its leading operand piece
    (include/robir_hip.h: rb_range_check).  sync=False costs nothing and reports kernels that have completed; sync=True waits
    for the current stream first.  The legacy library keeps its own sentinel block: read too once it has been loaded."""
    mask = ctypes.c_uint(0)
    call("rb_range_check", c_int(1 if sync else 0), stream_ptr(), ctypes.byref(mask))
    bits = mask.value
    if _lib.legacy_loaded():
        rc = _lib.legacy().rb_range_check(c_int(0), stream_ptr(), ctypes.byref(mask))      # the stream has been waited for above
        if rc != 0:
            raise _lib.RobirHipError(f"rb_range_check (legacy library) failed ({rc})")
        bits |= mask.value
    if bits:
        fams = [RANGE_FAMILIES[i] for i in range(len(RANGE_FAMILIES)) if bits >> i & 1]
        raise _lib.RobirHipError(
            "f16-piece arithmetic (split precision f16x3 / exact operands f16x6) overflowed its activation range in: " + "; ".join(fams) + " -- the outputs of "
            "the call(s) since the last check are not fp32-accurate.  Select the exact f32-input MFMA kernels for this "
            "checkpoint: ROBIR_MLP_PRECISION=fp32 and ROBIR_VIS_PRECISION=fp32 (INTEGRATION.md, 'range limits')")


def feat_vis(p, d, rep=1):
    """p [M/rep,3] points, d [M,3] directions (rep consecutive directions per point)."""
    p, d = _f32(p), _f32(d)
    M = d.shape[0]
    assert p.shape[0] * rep == M
    X = torch.empty(M, 128, dtype=torch.float32, device=p.device)
    call("rb_feat_vis", ptr(p), ptr(d), c_long(M), c_int(rep), ptr(X), stream_ptr())
    return X


def feat_pe10(x, scale=1.0, extra=None, jvp=False):
    x = _f32(x)
    M = x.shape[0]
    X = torch.empty(M * (4 if jvp else 1), 64, dtype=torch.float32, device=x.device)
    e = _f32(extra).reshape(-1) if extra is not None else None
    call("rb_feat_pe10", ptr(x), c_long(M), c_float(scale), ptr(e), c_int(1 if jvp else 0), ptr(X), stream_ptr())
    return X


def feat_ipe(x, var=1e-5, noise=None, noise_scale=0.0):
    x = _f32(x)
    M = x.shape[0]
    X = torch.empty(M, 64, dtype=torch.float32, device=x.device)
    nz = _f32(noise) if noise is not None else None
    call("rb_feat_ipe", ptr(x), c_long(M), c_float(var), ptr(nz), c_float(noise_scale), ptr(X), stream_ptr())
    return X


def feat_color(x, view, normal, feat, x_scale=1.0, feat_scale=1.0):
    x, view, normal = _f32(x), _f32(view), _f32(normal)
    assert feat.dtype == torch.float32 and feat.stride(-1) == 1
    M = x.shape[0]
    X = torch.empty(M, 304, dtype=torch.float32, device=x.device)
    call("rb_feat_color", ptr(x), c_float(x_scale), ptr(view), ptr(normal), ctypes.c_void_p(feat.data_ptr()),
         c_long(feat.stride(0)), c_float(feat_scale), c_long(M), ptr(X), stream_ptr())
    return X


def _color_args(x, view, normal, feat):
    """Checked inputs of the colour kernels that read the feature columns in place, the row count and the rgb output."""
    assert feat.dtype == torch.float32 and feat.stride(-1) == 1
    return _f32(x), _f32(view), _f32(normal), x.shape[0], torch.empty(x.shape[0], 3, dtype=torch.float32, device=x.device)


def color_mlp_h3_two(x, view, normal, feat, blob, scale_log2, x_scale=1.0, feat_scale=1.0):
    """feat_color + color_mlp_h3 without the assembled [M,304] rows: the 256 feature columns are read where they are."""
    x, view, normal, M, rgb = _color_args(x, view, normal, feat)
    tail = torch.empty(M, 48, dtype=torch.float32, device=x.device)
    call("rb_feat_color_tail", ptr(x), c_float(x_scale), ptr(view), ptr(normal), c_long(M), ptr(tail), stream_ptr())
    call("rb_color_mlp_h3_two", ctypes.c_void_p(feat.data_ptr()), c_long(feat.stride(0)), c_float(feat_scale), ptr(tail), c_long(M),
         ptr(blob), c_int(scale_log2), ptr(rgb), stream_ptr())
    return rgb


def color_mlp_h3_points(x, view, normal, feat, blob, scale_log2, x_scale=1.0, feat_scale=1.0, ring=None):
    """The colour net with its encoding fused: feature columns read in place, [x | PE4(view) | normal] encoded inside the kernel.
    ring (the default: 0.040 vs 0.061 ms for one round): the eight-wave chunk-stream kernel (csrc/color_ring8.hip) -- bit-identical rgb."""
    x, view, normal, M, rgb = _color_args(x, view, normal, feat)
    if ring is None or ring:
        call("rb_color_ring_points", ctypes.c_void_p(feat.data_ptr()), c_long(feat.stride(0)), c_float(feat_scale), ptr(x),
             c_float(x_scale), ptr(view), ptr(normal), c_long(M), ptr(blob), c_int(scale_log2), ptr(rgb), c_int(0), stream_ptr())
        return rgb
    call("rb_color_mlp_h3_points", ctypes.c_void_p(feat.data_ptr()), c_long(feat.stride(0)), c_float(feat_scale), ptr(x), c_float(x_scale),
         ptr(view), ptr(normal), c_long(M), ptr(blob), c_int(scale_log2), ptr(rgb), stream_ptr())
    return rgb


def vis_mlp(X, blob):
    M = X.shape[0]
    Y = torch.empty(M, 2, dtype=torch.float32, device=X.device)
    call("rb_vis_mlp", ptr(X), c_long(M), ptr(blob), ptr(Y), stream_ptr())
    return Y


def vis_mlp_h3(X, blob, scale_log2):
    M = X.shape[0]
    Y = torch.empty(M, 2, dtype=torch.float32, device=X.device)
    call("rb_vis_mlp_h3", ptr(X), c_long(M), ptr(blob), c_int(scale_log2), ptr(Y), stream_ptr())
    return Y


def vis_mlp_points(p, d, blob, rep=1, scale_log2=None):
    """Visibility MLP straight from points p [M/rep,3] and directions d [M,3] (encoding fused): scale_log2 None = f32-input MFMA
    kernel (blob from pack_vis), else the split-precision kernel (blob from pack_vis_h3)."""
    p, d = _f32(p), _f32(d)
    M = d.shape[0]
    assert p.shape[0] * rep == M
    Y = torch.empty(M, 2, dtype=torch.float32, device=d.device)
    if scale_log2 is None:
        call("rb_vis_mlp_points", ptr(p), ptr(d), c_long(M), c_int(rep), ptr(blob), ptr(Y), stream_ptr())
    else:
        call("rb_vis_mlp_h3_points", ptr(p), ptr(d), c_long(M), c_int(rep), ptr(blob), c_int(scale_log2), ptr(Y), stream_ptr())
    return Y


def vis_x6_points(p, d, blob, rep=1):
    """vis_mlp_points on exact three-piece operands (csrc/vis_x6.hip; blob = packing.pack_vis_x6)."""
    p, d = _f32(p), _f32(d)
    M = d.shape[0]
    assert p.shape[0] * rep == M
    Y = torch.empty(M, 2, dtype=torch.float32, device=d.device)
    call("rb_vis_x6_points", ptr(p), ptr(d), c_long(M), c_int(rep), ptr(blob), ptr(Y), c_int(0), stream_ptr())
    return Y


def wide_x6_points(x, extra, blob, encoder):
    """wide_mlp_points on exact three-piece operands (csrc/wide_x6.hip; blob = packing.pack_wide_x6 / pack_illum_x6 / ..._encoder_x6)."""
    x = _f32(x)
    M = x.shape[0]
    e = _f32(extra).reshape(-1) if extra is not None else None
    Y = torch.empty(M, 32 if encoder else 144, dtype=torch.float32, device=x.device)
    if M > 0:
        call("rb_wide_x6_points", ptr(x), ptr(e), c_long(M), ptr(blob), c_int(1 if encoder else 0), ptr(Y), c_int(0), stream_ptr())
    return Y


def wide_x6(X, blob, encoder):
    """wide_x6_points on feature rows X [M,64]."""
    M = X.shape[0]
    Y = torch.empty(M, 32 if encoder else 144, dtype=torch.float32, device=X.device)
    if M > 0:
        call("rb_wide_x6", ptr(X), c_long(M), ptr(blob), c_int(1 if encoder else 0), ptr(Y), c_int(0), stream_ptr())
    return Y


def linear_pe10_256(x, blob):
    """linear_64_256(feat_pe10(x)) with the encoding fused."""
    x = _f32(x)
    M = x.shape[0]
    Y = torch.empty(M, 256, dtype=torch.float32, device=x.device)
    call("rb_linear_pe10_256", ptr(x), c_long(M), ptr(blob), ptr(Y), stream_ptr())
    return Y


def wide_mlp_points(x, extra, blob, encoder, scale_log2=None, ring=None):
    """512-wide nets on [PE10(x) | extra] with the encoding fused: encoder=False -> raw SG outputs [M,144], True -> raw latent [M,32];
    scale_log2 None = f32-input MFMA kernel, else split precision; ring (split precision; the default: it wins at every size, one round
    of 64 rows 0.067 vs 0.127 ms): the chunk-stream kernel (csrc/wide_ring.h) -- bit-identical outputs."""
    x = _f32(x)
    M = x.shape[0]
    e = _f32(extra).reshape(-1) if extra is not None else None
    Y = torch.empty(M, 32 if encoder else 144, dtype=torch.float32, device=x.device)
    if scale_log2 is None:
        call("rb_wide_mlp_points", ptr(x), ptr(e), c_long(M), ptr(blob), c_int(1 if encoder else 0), ptr(Y), stream_ptr())
    elif ring is None or ring:
        call("rb_wide_mlp_ring_points", ptr(x), ptr(e), c_long(M), ptr(blob), c_int(1 if encoder else 0), c_int(scale_log2), ptr(Y),
             c_int(0), stream_ptr())
    else:
        call("rb_wide_mlp_h3_points", ptr(x), ptr(e), c_long(M), ptr(blob), c_int(1 if encoder else 0), c_int(scale_log2), ptr(Y),
             stream_ptr())
    return Y


def linear_64_256(X, blob):
    M = X.shape[0]
    Y = torch.empty(M, 256, dtype=torch.float32, device=X.device)
    call("rb_linear_64_256", ptr(X), c_long(M), ptr(blob), ptr(Y), stream_ptr())
    return Y


def sdf_mlp(X, M, blob, mode, out_scale=1.0, grad_scale=1.0):
    full = mode in (1, 3)
    out0 = torch.empty((M, 257) if full else (M,), dtype=torch.float32, device=X.device)
    grad = torch.empty(M, 3, dtype=torch.float32, device=X.device) if (mode & 3) >= 2 else None
    call("rb_sdf_mlp", ptr(X), c_long(M), ptr(blob), c_int(mode), c_float(out_scale), c_float(grad_scale), ptr(out0),
         ptr(grad), stream_ptr())
    return out0, grad


def sdf_mlp_points(x, M, blob, mode, in_scale=1.0, out_scale=1.0, grad_scale=1.0):
    """rb_sdf_mlp (f32-input MFMA) straight from the points: the encoding, tangent rows included, is evaluated inside the kernel."""
    x = _f32(x)
    full = mode in (1, 3)
    out0 = torch.empty((M, 257) if full else (M,), dtype=torch.float32, device=x.device)
    grad = torch.empty(M, 3, dtype=torch.float32, device=x.device) if (mode & 3) >= 2 else None
    call("rb_sdf_mlp_points", ptr(x), c_long(M), c_float(in_scale), ptr(blob), c_int(mode), c_float(out_scale), c_float(grad_scale),
         ptr(out0), ptr(grad), stream_ptr())
    return out0, grad


def color_mlp_points(x, view, normal, feat, blob, x_scale=1.0, feat_scale=1.0):
    """rb_color_mlp (f32-input MFMA) with the feature columns read in place and [x | PE4(view) | normal] encoded in the kernel."""
    x, view, normal, M, rgb = _color_args(x, view, normal, feat)
    call("rb_color_mlp_points", ctypes.c_void_p(feat.data_ptr()), c_long(feat.stride(0)), c_float(feat_scale), ptr(x), c_float(x_scale),
         ptr(view), ptr(normal), c_long(M), ptr(blob), ptr(rgb), stream_ptr())
    return rgb


def color_x6_points(x, view, normal, feat, blob, x_scale=1.0, feat_scale=1.0, two_tile=None):
    """color_mlp_points on exact three-piece operands (blob = packing.pack_color_x6): csrc/color_x6t.hip (two tiles per wave, rounds of 128
    rows) from SDF_TWO_TILE_MIN_ROWS rows on, csrc/color_x6.hip (one tile, rounds of 64) below; two_tile forces either."""
    x, view, normal, M, rgb = _color_args(x, view, normal, feat)
    if two_tile is None:
        two_tile = sdf_two_tile(M)
    call("rb_color_x6_points", ctypes.c_void_p(feat.data_ptr()), c_long(feat.stride(0)), c_float(feat_scale), ptr(x), c_float(x_scale),
         ptr(view), ptr(normal), c_long(M), ptr(blob), ptr(rgb), c_int(1 if two_tile else 0), c_int(0), stream_ptr())
    return rgb


SDF_KERNEL = os.environ.get("ROBIR_SDF_KERNEL", "ring")     # "ring" | "v1" (first-generation k_sdf_mlp_h3)


def sdf_mlp_h3(X, M, blob, mode, scale_log2, out_scale=1.0, grad_scale=1.0):
    full = mode in (1, 3)
    out0 = torch.empty((M, 257) if full else (M,), dtype=torch.float32, device=X.device)
    grad = torch.empty(M, 3, dtype=torch.float32, device=X.device) if mode >= 2 else None
    if SDF_KERNEL == "ring":        # second generation: weight ring + activations between the MFMAs (csrc/sdf_ring.hip)
        call("rb_sdf_mlp_ring", ptr(X), c_long(M), ptr(blob), c_int(mode), c_int(scale_log2), c_float(out_scale),
             c_float(grad_scale), ptr(out0), ptr(grad), c_int(0), stream_ptr())
    else:
        call("rb_sdf_mlp_h3", ptr(X), c_long(M), ptr(blob), c_int(mode), c_int(scale_log2), c_float(out_scale),
             c_float(grad_scale), ptr(out0), ptr(grad), stream_ptr())
    return out0, grad


SDF_FUSED_PE = os.environ.get("ROBIR_SDF_FUSED_PE", "1") == "1"   # value rows / value+gradient straight from the points (csrc/sdf_ring8.hip)


def sdf_points_h3(x, M, blob, full, scale_log2, in_scale=1.0, out_scale=1.0):
    """SDF network on points x [M,3] (evaluated at x * in_scale) with the positional encoding fused into the kernel:
    -> [M,257] (full) or [M].  Bit-identical to feat_pe10 + sdf_mlp_h3 (modes 1 / 0)."""
    x = _f32(x)
    out0 = torch.empty((M, 257) if full else (M,), dtype=torch.float32, device=x.device)
    call("rb_sdf_points_ring", ptr(x), c_long(M), c_float(in_scale), ptr(blob), c_int(1 if full else 0), c_int(scale_log2),
         c_float(out_scale), ptr(out0), c_int(0), stream_ptr())
    return out0


def sdf_points_jvp_h3(x, M, blob, full, scale_log2, in_scale=1.0, out_scale=1.0, grad_scale=1.0):
    """Forward-mode value + gradient rows straight from the points (k_sdf_ring<2|3, FUSED>): -> (out0, grad [M,3])."""
    x = _f32(x)
    out0 = torch.empty((M, 257) if full else (M,), dtype=torch.float32, device=x.device)
    grad = torch.empty(M, 3, dtype=torch.float32, device=x.device)
    call("rb_sdf_points_ring_jvp", ptr(x), c_long(M), c_float(in_scale), ptr(blob), c_int(3 if full else 2), c_int(scale_log2),
         c_float(out_scale), c_float(grad_scale), ptr(out0), ptr(grad), c_int(0), stream_ptr())
    return out0, grad


SDF_GRAD = os.environ.get("ROBIR_SDF_GRAD", "reverse")     # "reverse" (csrc/sdf_value_grad.hip; split precision: sdf_back.hip) | "forward" (mode 3 rows)
SDF_GRAD_MIN_POINTS = 16384       # below this the three-launch reverse form does not pay (0.25 ms floor; measured crossover)
SDF_GRAD_F32_MIN_POINTS = 16384   # ... of the f32-input-MFMA form (three launches against one of the four-row forward-mode kernel)
SDF_GRAD_SLAB = 1 << 20           # points per slab of the reverse form (8.5 KB of scratch per point)
_sdf_grad_scratch = {}


def release_scratch():
    """Drop the cached per-(device, stream) scratch of sdf_value_grad (8.9 GB per stream at the default slab)."""
    _sdf_grad_scratch.clear()


def sdf_ring_waves():
    """Current setting of rb_sdf_ring_waves (8 = csrc/sdf_ring8.hip, 4 = csrc/sdf_ring.hip) without changing it."""
    return int(_lib.legacy().rb_sdf_ring_waves(0))


def _sdf_value_grad_slabs(x, M, scratch_floats, key, launch):
    """The frame the reverse-mode SDF forms share: out [M,257], grad [M,3], the cached per-(device, stream) scratch (entry `key`, sized by
    scratch_floats(points of a slab)) and launch(x, n, out, grad, scratch) on each slab of SDF_GRAD_SLAB points."""
    out0 = torch.empty(M, 257, dtype=torch.float32, device=x.device)
    grad = torch.empty(M, 3, dtype=torch.float32, device=x.device)
    if M == 0:
        return out0, grad
    slab = min(M, SDF_GRAD_SLAB)
    need = int(scratch_floats(c_long(slab)))
    key = (x.device, torch.cuda.current_stream().cuda_stream) + key
    scratch = _sdf_grad_scratch.get(key)
    if scratch is None or scratch.numel() < need:
        scratch = _sdf_grad_scratch[key] = torch.empty(need, dtype=torch.float32, device=x.device)
    x = _f32(x)
    for a in range(0, M, slab):
        n = min(slab, M - a)
        launch(x[a:a + n], n, out0[a:a + n], grad[a:a + n], scratch)
    return out0, grad


def sdf_value_grad(x, M, blob, back, scale_log2, in_scale=1.0, out_scale=1.0):
    """All 257 outputs + d sdf / dx by the reverse-mode pass: x [M,3] -> out [M,257], grad [M,3]."""
    wb, w8 = back

    def launch(x, n, out0, grad, scratch):
        if SDF_FUSED_PE and sdf_ring_waves() == 8:      # the encoding is fused into the eight-wave kernel
            call("rb_sdf_value_grad_points", ptr(x), c_long(n), c_float(in_scale), ptr(blob), ptr(wb), ptr(w8), c_int(scale_log2),
                 c_float(out_scale), c_float(out_scale * in_scale), ptr(out0), ptr(grad), ptr(scratch), c_int(0), stream_ptr())
        else:
            X = feat_pe10(x, scale=in_scale)
            call("rb_sdf_value_grad", ptr(X), c_long(n), ptr(blob), ptr(wb), ptr(w8), c_int(scale_log2), c_float(out_scale),
                 c_float(out_scale * in_scale), ptr(out0), ptr(grad), ptr(scratch), c_int(0), stream_ptr())
    return _sdf_value_grad_slabs(x, M, lambda n: _lib.legacy().rb_sdf_value_grad_scratch_floats(n), (), launch)


def sdf_value_grad_f32(x, M, blob, back, in_scale=1.0, out_scale=1.0):
    """sdf_value_grad at the reference's precision (f32-input MFMA; csrc/mlp_f32.h, mlp_f32.hip k_sdf_mlp<5> + k_sdf_back_f32): x [M,3] ->
    out [M,257], grad [M,3].  blob = packing.pack_sdf(full=True), back = packing.pack_sdf_back."""
    wt, w8 = back

    def launch(x, n, out0, grad, scratch):
        call("rb_sdf_value_grad_f32_points", ptr(x), c_long(n), c_float(in_scale), ptr(blob), ptr(wt), ptr(w8), c_float(out_scale),
             c_float(out_scale * in_scale), ptr(out0), ptr(grad), ptr(scratch), stream_ptr())
    return _sdf_value_grad_slabs(x, M, lambda n: _lib.lib().rb_sdf_value_grad_f32_scratch_floats(n), ("f32",), launch)


SDF_TWO_TILE_MIN_ROWS = int(os.environ.get("ROBIR_SDF_TWO_TILE_MIN_ROWS", "16385"))


@functools.lru_cache(None)
def _compute_units():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count if torch.cuda.is_available() else 256


def sdf_two_tile(M):
    """The exact-operand SDF / colour kernels come in two forms: two 16-row tiles per wave (rounds of 128 rows, half the LDS traffic per
    MFMA: csrc/sdf_x6t.hip, sdf_back_x6t.hip, color_x6t.hip) and one tile per wave (rounds of 64 rows).  Both run one persistent
    workgroup per compute unit, so a launch costs (rounds per workgroup) x (time of a round), and a two-tile round takes 1.42-1.5 x a
    one-tile round (tools/sweep_two_tile.py: 0.135 / 0.095 ms distance, 0.31 / 0.21 value + gradient, 0.083 / 0.055 colour): the
    two-tile form wins where it needs fewer than two thirds of the passes -- 16385..32768 rows, and everything beyond 49152 on 256
    compute units.  ROBIR_SDF_TWO_TILE_MIN_ROWS: rows below it always take the one-tile form (0: always two tiles).  The two forms
    agree to fp32 summation order."""
    if SDF_TWO_TILE_MIN_ROWS <= 0:
        return True
    if M < SDF_TWO_TILE_MIN_ROWS:
        return False
    cus = _compute_units()
    r1, r2 = -(-M // (64 * cus)), -(-M // (128 * cus))
    return 2 * r1 > 3 * r2


def sdf_points_x6(x, M, blob, full, in_scale=1.0, out_scale=1.0):
    """SDF value rows on exact three-piece operands (csrc/sdf_x6.hip, sdf_x6t.hip): x [M,3] -> out [M,257] | [M]; blob = packing.pack_sdf_x6(full)."""
    x = _f32(x)
    out0 = torch.empty((M, 257) if full else (M,), dtype=torch.float32, device=x.device)
    if M > 0:
        call("rb_sdf_x6_points", ptr(x), c_long(M), c_float(in_scale), ptr(blob), c_int(1 if full else 0), c_float(out_scale), ptr(out0),
             c_int(1 if sdf_two_tile(M) else 0), c_int(0), stream_ptr())
    return out0


def sdf_value_grad_x6(x, M, blob, back, in_scale=1.0, out_scale=1.0):
    """sdf_value_grad_f32 with both passes on exact three-piece operands (blob = packing.pack_sdf_x6(full=True), back =
    (packing.pack_sdf_back_x6(...), packing.pack_sdf_back_x6(..., two_tile=True)[0]) -- the one-tile kernel's transposed layers, the
    head row, the two-tile kernel's transposed layers; a 2-tuple (round 3's form) runs the one-tile kernels at every size)."""
    wt, w8 = back[0], back[1]
    wt2 = back[2] if len(back) > 2 else None

    def launch(x, n, out0, grad, scratch):
        two = wt2 is not None and sdf_two_tile(n)
        call("rb_sdf_value_grad_x6_points", ptr(x), c_long(n), c_float(in_scale), ptr(blob), ptr(wt2 if two else wt), ptr(w8), c_float(out_scale),
             c_float(out_scale * in_scale), ptr(out0), ptr(grad), ptr(scratch), c_int(1 if two else 0), stream_ptr())
    # the same scratch entry as sdf_value_grad_f32: the two never run at once on a stream
    return _sdf_value_grad_slabs(x, M, lambda n: _lib.lib().rb_sdf_value_grad_f32_scratch_floats(n), ("f32",), launch)


def color_mlp(X, blob):
    M = X.shape[0]
    Y = torch.empty(M, 3, dtype=torch.float32, device=X.device)
    call("rb_color_mlp", ptr(X), c_long(M), ptr(blob), ptr(Y), stream_ptr())
    return Y


def color_mlp_h3(X, blob, scale_log2):
    M = X.shape[0]
    rgb = torch.empty(M, 3, dtype=torch.float32, device=X.device)
    call("rb_color_mlp_h3", ptr(X), c_long(M), ptr(blob), c_int(scale_log2), ptr(rgb), stream_ptr())
    return rgb


def illum_mlp(X, blob):
    M = X.shape[0]
    raw = torch.empty(M, 144, dtype=torch.float32, device=X.device)
    call("rb_illum_mlp", ptr(X), c_long(M), ptr(blob), ptr(raw), stream_ptr())
    return raw


def wide_mlp_h3(X, blob, encoder, scale_log2, ring=None):
    """Split-precision 512-wide nets on feature rows: encoder=False -> raw SG outputs [M,144]; encoder=True -> raw latent [M,32].
    ring (the default): the chunk-stream kernel (csrc/wide_ring.h) -- bit-identical outputs."""
    M = X.shape[0]
    Y = torch.empty(M, 32 if encoder else 144, dtype=torch.float32, device=X.device)
    if ring is None or ring:
        call("rb_wide_mlp_ring", ptr(X), c_long(M), ptr(blob), c_int(1 if encoder else 0), c_int(scale_log2), ptr(Y), c_int(0), stream_ptr())
    else:
        call("rb_wide_mlp_h3", ptr(X), c_long(M), ptr(blob), c_int(1 if encoder else 0), c_int(scale_log2), ptr(Y), stream_ptr())
    return Y


def illum_decode(raw):
    M = raw.shape[0]
    sgs = torch.empty(M, 24, 7, dtype=torch.float32, device=raw.device)
    call("rb_illum_decode", ptr(raw), c_long(M), ptr(sgs), stream_ptr())
    return sgs


def ae_encode(X, blob):
    M = X.shape[0]
    raw = torch.empty(M, 32, dtype=torch.float32, device=X.device)
    call("rb_ae_encode", ptr(X), c_long(M), ptr(blob), ptr(raw), stream_ptr())
    return raw


def ae_latent(raw, var=None, act=0, noise=None, noise_scale=0.0):
    M = raw.shape[0]
    lat = torch.empty_like(raw)
    lat2 = torch.empty_like(raw) if noise is not None else None
    call("rb_ae_latent", ptr(raw), c_long(M), ptr(var), c_int(act), ptr(_f32(noise) if noise is not None else None),
         c_float(noise_scale), ptr(lat), ptr(lat2), stream_ptr())
    return lat, lat2


def ae_decode(lat, blob, n_out, sigmoid_out):
    M = lat.shape[0]
    Y = torch.empty(M, n_out, dtype=torch.float32, device=lat.device)
    call("rb_ae_decode", ptr(lat), c_long(M), ptr(blob), c_int(n_out), c_int(1 if sigmoid_out else 0), ptr(Y),
         stream_ptr())
    return Y


AE_PARAM_NAMES = tuple(f"brdf_encoder_layer.{2 * i}.{w}" for i in range(5) for w in ("weight", "bias")) \
    + tuple(f"brdf_decoder_layer.{2 * i}.{w}" for i in range(3) for w in ("weight", "bias"))
AE_SLAB_ROWS = 16384


def ae_backward(X, params, g_out=None, g_out_xi=None, g_raw=None, noise=None, var=None, latent_act=0, sigmoid_out=True, in_dim=63,
                out_dim=5, want=AE_PARAM_NAMES, slab_rows=None, noise_scale=0.01):
    """Reverse mode of one latent-smoothed SparseAE (rb_train_ae_bwd, include/robir_hip_train.h): X [n,64] the feature rows the forward saw,
    params = the sixteen nn.Linear tensors in AE_PARAM_NAMES order, the three upstream gradients (None = absent) on out / out_xi / the
    pre-activation latent.  -> (dict name -> gradient in the parameter's own shape for the names in `want`, stats dict: kernels enqueued,
    whether the encoder was differentiated, scratch bytes).  Allocates the wanted gradients and the scratch, nothing else."""
    X = _f32(X)
    n, dev = X.shape[0], X.device
    assert X.dim() == 2 and X.shape[1] == 64 and len(params) == 16
    params = [_f32(p.detach()) for p in params]
    opt = lambda t, cols: None if t is None else _f32(t.detach()).reshape(n, cols)
    g_out, g_out_xi, g_raw, noise = opt(g_out, out_dim), opt(g_out_xi, out_dim), opt(g_raw, 32), opt(noise, 32)
    var = None if var is None else _f32(var.detach()).reshape(32)
    slab = int(slab_rows or AE_SLAB_ROWS)
    stats = (c_int * 2)(0, 0)
    out, nbytes = _param_backward(
        "ae_backward", AE_PARAM_NAMES, params, want, rows=n, dev=dev, lib=_lib.train, query="rb_train_ae_bwd_scratch_bytes",
        query_args=(c_long(n), c_long(slab), c_int(in_dim), c_int(out_dim)),
        launch=lambda P, G, scratch, nbytes: _lib.call_train(
            "rb_train_ae_bwd", ptr(X), c_long(n), c_int(in_dim), ptr(noise), ctypes.c_double(noise_scale), ptr(var), c_int(latent_act),
            c_int(1 if sigmoid_out else 0), c_int(out_dim), P, ptr(g_out), ptr(g_out_xi), ptr(g_raw), G, c_long(slab), ptr(scratch),
            c_long(nbytes), stats, stream_ptr()))
    return out, {"launches": int(stats[0]), "encoder_pass": bool(stats[1]), "scratch_bytes": nbytes}


def _param_backward(who, names, params, want, *, rows, dev, lib, query, query_args, launch):
    """The common tail of the four *_backward functions (`who`, for the error text): allocates the gradients named in `want` (a subset of
    `names`, the order of `params`) and -- rows > 0 and something wanted -- the fp64 scratch that lib()'s `query` asks for, then runs
    launch(params' pointer array, gradients' pointer array with NULL for the unwanted, scratch, its bytes).  -> (dict name -> gradient,
    scratch bytes)."""
    unknown = set(want) - set(names)
    if unknown:
        raise KeyError(f"{who}: no such parameter: {sorted(unknown)}")
    alloc = torch.zeros if rows == 0 else torch.empty           # rows > 0: k_finish stores every element of every wanted gradient
    out = {k: alloc(p.shape, dtype=torch.float32, device=dev) for k, p in zip(names, params) if k in want}
    nbytes = 0
    if rows > 0 and out:
        nbytes = int(getattr(lib(), query)(*query_args))
        if nbytes < 0:
            raise _lib.RobirHipError(f"{query}: " + _lib.aux_error(lib()))
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        P = (ctypes.c_void_p * len(names))(*[p.data_ptr() for p in params])
        G = (ctypes.c_void_p * len(names))(*[out[k].data_ptr() if k in out else None for k in names])
        launch(P, G, scratch, nbytes)
    return out, nbytes


def _partitioned_backward(who, names, params, want, *, rows, dev, lib, query, launch, n_layers, slab_rows, part_rows, defaults):
    """The common tail of the three row-partitioned backwards: (slab_rows, part_rows) or the module's `defaults`, the library's three-int
    stats, _param_backward with launch(params' pointer array, gradients' pointer array, `tail`), `tail` being the arguments every such
    entry point ends in (slab_rows, part_rows, scratch, scratch_bytes, stats, stream), and the stats dict."""
    slab = int(slab_rows or defaults[0])
    part = int(part_rows or min(slab, defaults[1]))
    stats = (c_int * 3)(0, n_layers, 0)
    out, nbytes = _param_backward(
        who, names, params, want, rows=rows, dev=dev, lib=lib, query=query, query_args=(c_long(rows), c_long(slab), c_long(part)),
        launch=lambda P, G, scratch, nbytes: launch(P, G, (c_long(slab), c_long(part), ptr(scratch), c_long(nbytes), stats, stream_ptr())))
    return out, {"launches": int(stats[0]), "lowest_layer": int(stats[1]), "partitions": int(stats[2]), "scratch_bytes": nbytes}


VIS_PARAM_NAMES = tuple(f"vis_layer.{2 * i}.{w}" for i in range(5) for w in ("weight", "bias"))
# A full slab's widest weight gradient (256 x 257: 20 output tiles) is 20 * 16384 / 1024 = 320 workgroups on 256 compute units, and the
# scratch is 227 MB whatever the batch (profiles/vis_backward_times.md)
VIS_SLAB_ROWS = 16384
VIS_PART_ROWS = 1024


def vis_backward(points, dirs, rep, params, g_logits, want=VIS_PARAM_NAMES, slab_rows=None, part_rows=None):
    """Reverse mode of VisNetwork (rb_vt_vis_bwd, include/robir_hip_vistrain.h): points [M/rep,3], dirs [M,3] (rep consecutive directions per
    point), params = the ten nn.Linear tensors in VIS_PARAM_NAMES order, g_logits [M,2] the upstream gradient on the logits.  -> (dict name ->
    gradient in the parameter's own shape for the names in `want`, stats dict: kernels enqueued, lowest layer differentiated, partitions per
    full slab, scratch bytes).  Allocates the wanted gradients and the scratch, nothing else."""
    points, dirs = _f32(points.detach()), _f32(dirs.detach())
    M, dev = dirs.shape[0], dirs.device
    rep = int(rep)
    assert dirs.dim() == 2 and dirs.shape[1] == 3 and rep >= 1 and points.shape[0] * rep == M and len(params) == 10
    params = [_f32(p.detach()) for p in params]
    g_logits = _f32(g_logits.detach()).reshape(M, 2)
    return _partitioned_backward(
        "vis_backward", VIS_PARAM_NAMES, params, want, rows=M, dev=dev, lib=_lib.vistrain, query="rb_vt_vis_bwd_scratch_bytes", n_layers=5,
        slab_rows=slab_rows, part_rows=part_rows, defaults=(VIS_SLAB_ROWS, VIS_PART_ROWS),
        launch=lambda P, G, tail: _lib.call_vistrain(
            "rb_vt_vis_bwd", ptr(points), ptr(dirs), c_long(M), c_int(rep), P, ptr(g_logits), G, *tail))


ILLUM_PARAM_NAMES = tuple(f"lobe_layer.{2 * i}.{w}" for i in range(5) for w in ("weight", "bias"))
# A step of the "Illum" stage is n_hit rows (not n_hit x nsamp): at the 650 hit points of a 1024-pixel chunk, 256-row partitions make the
# widest weight gradient (512 x 513: 72 output tiles) 72 x 3 = 216 workgroups on 256 compute units.  The default rests on that workgroup
# count, not on a measured time.  Scratch: 148 MB for a full slab, 31 MB at 650 rows
ILLUM_SLAB_ROWS = 4096
ILLUM_PART_ROWS = 256


def illum_lobe_backward(points, hdr, params, g_sgs, want=ILLUM_PARAM_NAMES, slab_rows=None, part_rows=None):
    """Reverse mode of IndirctIllumNetwork's lobe net (rb_it_lobe_bwd, include/robir_hip_illumtrain.h): points [n,3], hdr [n,1] or None (the
    no_hdr net, whose first weight is [512,63]), params = the ten nn.Linear tensors in ILLUM_PARAM_NAMES order, g_sgs [n,24,7] the upstream
    gradient on the decoded lobes.  -> (dict name -> gradient in the parameter's own shape for the names in `want`, stats dict: kernels
    enqueued, lowest layer differentiated, partitions per full slab, scratch bytes).  Allocates the wanted gradients and the scratch,
    nothing else."""
    points = _f32(points.detach())
    n, dev = points.shape[0], points.device
    hdr = None if hdr is None else _f32(hdr.detach()).reshape(n, 1)
    assert points.dim() == 2 and points.shape[1] == 3 and len(params) == 10
    params = [_f32(p.detach()) for p in params]
    assert tuple(params[0].shape) == (512, 63 if hdr is None else 64), "lobe_layer.0.weight is [512,64] with hdr, [512,63] without"
    g_sgs = _f32(g_sgs.detach()).reshape(n, 24, 7)
    return _partitioned_backward(
        "illum_lobe_backward", ILLUM_PARAM_NAMES, params, want, rows=n, dev=dev, lib=_lib.illumtrain, query="rb_it_lobe_bwd_scratch_bytes",
        n_layers=5, slab_rows=slab_rows, part_rows=part_rows, defaults=(ILLUM_SLAB_ROWS, ILLUM_PART_ROWS),
        launch=lambda P, G, tail: _lib.call_illumtrain("rb_it_lobe_bwd", ptr(points), ptr(hdr), c_long(n), P, ptr(g_sgs), G, *tail))


CESR_PARAM_NAMES = tuple(f"lin{l}.{w}" for l in range(9) for w in ("weight_g", "weight_v", "bias"))
CESR_KINDS = {"normal": (0, 63, 3), "shadow": (1, 191, 2)}       # SDFNetwork.kind -> (the library's kind code, d_in, d_out)
# One 1024-pixel chunk sends ~940 points x 128 labels = 120 000 rows through shadow_net: seven full slabs and a short one at 16384 rows.
# The fastest on an MI355X of (4096, 512) 95 ms, (16384, 1024) 68 ms, (16384, 2048) 76 ms: profiles/cesr_backward_times.md.  Scratch: 42.6 KB
# per slab row, 727 MiB at these defaults
CESR_SLAB_ROWS = 16384
CESR_PART_ROWS = 1024


def cesr_backward(x, M, kind, params, g_out, head=0, n_label=1, want=CESR_PARAM_NAMES, slab_rows=None, part_rows=None):
    """Reverse mode of a CESR network (rb_ct_cesr_bwd, include/robir_hip_cesrtrain.h).  kind "normal" | "shadow"; x: points [M / n_label, 3]
    (the points form: encoded in fp64 by the library, the one-hot label block built from the row index) or dense rows [M, ld >= d_in] (the
    caller's fp32 rows); params = the 27 weight-norm tensors in CESR_PARAM_NAMES order; head 0: g_out [M, d_out] on the raw output, 1:
    g_out [M] on softmax2(., 1) (shadow), 2: g_out [M, 3] on normalize3(., 1e-4, 1) (normal).  -> (dict name -> gradient in the parameter's
    own shape for the names in `want`, stats dict: kernels enqueued, lowest layer differentiated, partitions per full slab, scratch bytes).
    Allocates the wanted gradients and the scratch, nothing else."""
    code, d_in, d_out = CESR_KINDS[kind]
    x = _f32(x.detach())
    M, dev = int(M), x.device
    points = x.dim() == 2 and x.shape[1] == 3
    assert x.dim() == 2 and len(params) == 27 and n_label >= 1 and M % n_label == 0
    assert (x.shape[0] * n_label == M) if points else (x.shape[0] == M and x.shape[1] >= d_in), "points [M / n_label, 3] or rows [M, >= d_in]"
    params = [_f32(p.detach()) for p in params]
    assert tuple(params[1].shape) == (512, d_in) and tuple(params[25].shape) == (d_out, 512), f"not the {kind} network's tensors"
    g_out = _f32(g_out.detach()).reshape((M,) if head == 1 else (M, d_out))
    return _partitioned_backward(
        "cesr_backward", CESR_PARAM_NAMES, params, want, rows=M, dev=dev, lib=_lib.cesrtrain, query="rb_ct_cesr_bwd_scratch_bytes", n_layers=9,
        slab_rows=slab_rows, part_rows=part_rows, defaults=(CESR_SLAB_ROWS, CESR_PART_ROWS),
        launch=lambda P, G, tail: _lib.call_cesrtrain(
            "rb_ct_cesr_bwd", ptr(x if points else None), ptr(None if points else x), c_long(x.shape[1]), c_long(M), c_int(code),
            c_int(n_label), c_int(head), P, ptr(g_out), G, *tail))


def _sg_query_args(sgs, dirs):
    sgs, dirs = _f32(sgs.detach()), _f32(dirs.detach())
    assert sgs.dim() == 3 and sgs.shape[2] == 7 and dirs.dim() == 3 and dirs.shape[2] == 3 and dirs.shape[0] == sgs.shape[0]
    return sgs, dirs, sgs.shape[0], sgs.shape[1], dirs.shape[1]


def sg_query(sgs, dirs):
    """query_indir_illum (model/loss.py:128-141), fused (rb_it_sg_query): sgs [n,L,7], dirs [n,S,3] -> radiance [n,S,3] =
    sum_j mu_j exp(lambda_j (d . l_j / |l_j| - 1)), fp64 from the fp32 inputs, rounded once."""
    sgs, dirs, n, L, S = _sg_query_args(sgs, dirs)
    rad = torch.empty(n, S, 3, dtype=torch.float32, device=sgs.device)
    _lib.call_illumtrain("rb_it_sg_query", ptr(sgs), ptr(dirs), c_long(n), c_int(L), c_long(S), ptr(rad), stream_ptr())
    return rad


def sg_query_backward(sgs, dirs, g):
    """d <g, sg_query(sgs, dirs)> / d sgs (rb_it_sg_query_bwd): g [n,S,3] dense, zeros at masked samples -> [n,L,7]."""
    sgs, dirs, n, L, S = _sg_query_args(sgs, dirs)
    g = _f32(g.detach()).reshape(n, S, 3)
    out = torch.empty(n, L, 7, dtype=torch.float32, device=sgs.device)
    _lib.call_illumtrain("rb_it_sg_query_bwd", ptr(sgs), ptr(dirs), ptr(g), c_long(n), c_int(L), c_long(S), ptr(out), stream_ptr())
    return out


def axpy(a, b, s):
    a, b = _f32(a), _f32(b)
    y = torch.empty_like(a)
    call("rb_axpy", ptr(a), ptr(b), c_float(s), c_long(a.numel()), ptr(y), stream_ptr())
    return y


def normalize3(x, eps, mode):
    x = _f32(x)
    y = torch.empty_like(x)
    call("rb_normalize3", ptr(x), c_long(x.shape[0]), c_float(eps), c_int(mode), ptr(y), stream_ptr())
    return y


def dvis_dirs(lgt, u_theta, u_phi, thr=1.0, direct=False):
    """lgt [L,7]; u_theta/u_phi [C,L,nsamp] (or [L,nsamp]).  -> dirs [C*L*nsamp,3], wdir [C*L*nsamp], wsum [C*L]."""
    lgt, u_theta, u_phi = _f32(lgt), _f32(u_theta), _f32(u_phi)
    if u_theta.dim() == 2:
        u_theta, u_phi = u_theta[None], u_phi[None]
    C, L, ns = u_theta.shape
    dev = lgt.device
    dirs = torch.empty(C * L * ns, 3, dtype=torch.float32, device=dev)
    wdir = torch.empty(C * L * ns, dtype=torch.float32, device=dev)
    wsum = torch.empty(C * L, dtype=torch.float32, device=dev)
    call("rb_dvis_dirs", ptr(lgt), c_int(L), c_int(ns), c_int(C), c_int(1 if direct else 0), ptr(u_theta.contiguous()), ptr(u_phi.contiguous()),
         c_float(thr), ptr(dirs), ptr(wdir), ptr(wsum), stream_ptr())
    return dirs, wdir, wsum


DVIS_KERNEL_NAMES = {"fp32": "k_dvis_fused<fp32>", "f16x6": "k_dvis_x6t", "f16x6-pt": "k_dvis_x6t", "f16x6-stream": "k_dvis_x6t<stream>",
                     "f16x6-1t": "k_dvis_x6", "f16x1": "k_dvis_f16p", "f16x3-auto": "k_dvis_v2", "f16x3-v3": "k_dvis3_stream",
                     "f16x3-v2": "k_dvis_v2", "f16x3": "k_dvis_fused<H3>"}


DVIS_STREAM_WORKGROUPS = 0        # persistent workgroups of the streaming visibility kernel; 0 = one per compute unit
# persistent workgroups of the per-point form (rb_dvis_fused_x6t); 0 = one per compute unit.  The library reads the environment variable at
# every launch (include/robir_hip.h): dvis_fused writes a changed value back to it
DVIS_PT_WORKGROUPS = int(os.environ.get("ROBIR_DVIS_PT_WORKGROUPS") or 0)
_dvis_pt_workgroups_env = DVIS_PT_WORKGROUPS
DVIS_STREAM_MAX_POINTS = 8192     # launches up to this many surface points take the tile-list (streaming) form
DVIS_STREAM_SHORT_LIST = 1024     # ... and any launch whose points have at most this many sampled directions (L * nsamp)
# the f16 throughput mode's kernel: 3 = the point-block form (csrc/vis_diffuse_f16p.hip: sixteen points x one direction per tile; needs
# ascending chunk ids, else 2), 2 = the per-point tile list, two-chunk steps, 1 = round 4's kernel -- the same bits, 1 / 2 kept for A/B
DVIS_F16_GEN = int(os.environ.get("ROBIR_DVIS_F16_GEN", "3"))


def chunk_ids_ascending(chunk_id):
    """True if chunk_id (int32 [n] or None) never decreases.  The answer is remembered ON the tensor (`_robir_ascending`): constructors that
    know (the renderer's hit lists: pixel order) set it and save the device -> host read this costs otherwise."""
    if chunk_id is None or chunk_id.numel() < 2:
        return True
    known = getattr(chunk_id, "_robir_ascending", None)
    if known is None:
        known = bool((chunk_id[1:] >= chunk_id[:-1]).all())
        chunk_id._robir_ascending = known
    return known
DVIS_X6_FP8 = True      # a constant: k_dvis_x6t forms two of its six products on the bf8 MFMA (bench.py reads this for its roofline bound)
DVIS_X6_FORM = os.environ.get("ROBIR_DVIS_X6_FORM", "auto")          # what "f16x6" runs: auto | f16x6-pt | f16x6-stream | f16x6-1t


def dvis_fused(normals, chunk_id, A, Bd, dirs, wdir, wsum, split, L, nsamp, argmax_vis=False, eval_count=None,
               precision="fp32"):
    """precision: 'fp32' (f32-input MFMA, exact fp32 fma chain), 'f16x6' (exact fp32 operands as three halves each, six f16
    MFMA products per multiply-add: not narrower than fp32), 'f16x3*' (split precision, 22-bit operands, ~2^-22 relative) or 'f16x1' (plain
    f16: NARROWER than fp32).  Which kernel form, weight blob and format serve the call: dispatch.dvis."""
    normals = _f32(normals)
    n, dev = normals.shape[0], normals.device
    r = dispatch.dvis(precision, n, L, nsamp, DVIS_X6_FORM, DVIS_F16_GEN, lambda: chunk_ids_ascending(chunk_id),
                      DVIS_STREAM_MAX_POINTS, DVIS_STREAM_SHORT_LIST)
    out = torch.empty(n, L, dtype=torch.float32, device=dev)
    if chunk_id is not None:
        assert chunk_id.dtype == torch.int32
    args = [ptr(normals), ptr(chunk_id), c_long(n), ptr(A), ptr(Bd), ptr(dirs), ptr(wdir), ptr(wsum), ptr(split[r.blob])]
    if r.layout == "gen1":      # rb_dvis_fused: the output layer in row-major form, precision code 5 = the split-precision kernel
        args += [ptr(split["w_last"]), ptr(split["b_last"])]
    args += [c_int(L), c_int(nsamp), c_int(1 if argmax_vis else 0)]
    if r.layout == "gen1":
        args.append(c_int(5 if r.legacy else 0))
    if r.fmt is not None:
        args.append(c_int(split[r.fmt] if isinstance(r.fmt, str) else r.fmt))
    LS = L * nsamp
    # the tile-list forms: scratch sized for the worst case (every direction front-facing) so that nothing has to be read back to the host
    if r.layout == "pblock":      # by items: a block of 16 points, two items where a block spans a chunk boundary
        items_max = (n + 15) // 16 + max(1, dirs.shape[0] // LS) - 1
        entries = torch.empty(items_max * LS, dtype=torch.int32, device=dev)
        pair_vis = torch.empty(items_max * LS * 16, dtype=torch.float32, device=dev)
        round_info = torch.empty(items_max * LS // 16, 4, dtype=torch.int32, device=dev)
        item_info = torch.empty(items_max, 4, dtype=torch.int32, device=dev)
        counters = torch.empty(4, dtype=torch.int64, device=dev)
        args += [c_int(items_max), ptr(entries), ptr(pair_vis), ptr(round_info), ptr(item_info), ptr(counters), c_int(DVIS_STREAM_WORKGROUPS)]
    elif r.layout == "stream":      # global tile list + persistent grid (csrc/vis_diffuse_v3.hip, vis_diffuse_x6t.hip, vis_diffuse_f16t.hip)
        pair_j = torch.empty(n * LS, dtype=torch.int16, device=dev)
        pair_vis = torch.empty(n * LS, dtype=torch.float32, device=dev)
        tile_info = torch.empty(n * LS // 16, 2, dtype=torch.int32, device=dev)
        point_info = torch.empty(n, 2, dtype=torch.int32, device=dev)
        counters = torch.empty(2, dtype=torch.int64, device=dev)
        args += [ptr(pair_j), ptr(pair_vis), ptr(tile_info), ptr(point_info), ptr(counters), c_int(DVIS_STREAM_WORKGROUPS)]
    elif r.entry == "rb_dvis_fused_x6t":      # persistent grid: its size reaches the library through the environment, written when it changes
        global _dvis_pt_workgroups_env
        if int(DVIS_PT_WORKGROUPS) != _dvis_pt_workgroups_env:
            _dvis_pt_workgroups_env = int(DVIS_PT_WORKGROUPS)
            os.environ["ROBIR_DVIS_PT_WORKGROUPS"] = str(max(0, _dvis_pt_workgroups_env))
    (_lib.call_legacy if r.legacy else call)(r.entry, *args, ptr(out), ptr(eval_count), stream_ptr())
    if r.layout == "pblock" and os.environ.get("ROBIR_RANGE_CHECK", "") == "sync" and int(counters[3].item()) != 0:
        # counters[3]: chunk ids not ascending (a list whose order was only ASSERTED through the `_robir_ascending` attribute) or more
        # items than the scratch holds -- the kernel then leaves its NaN fill in `out`.  Read in the debug mode only: a host sync.
        raise _lib.RobirHipError("rb_dvis_pblock_f16: chunk ids are not ascending or the item scratch overflowed -- the outputs "
                                 "of this call are NaN (ADVICE r5; run without the `_robir_ascending` tag to let ops check the order)")
    return out


def _spec_vis_buffers(n, ns, n_chunks, dev):
    """Outputs and scratch of the two spec_vis_sample forms: sharpness [n], per-chunk minimum, directions, weights, front-facing flags."""
    return (torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n_chunks, dtype=torch.int32, device=dev),
            torch.empty(n * ns, 3, dtype=torch.float32, device=dev), torch.empty(n * ns, dtype=torch.float32, device=dev),
            torch.empty(n * ns, dtype=torch.uint8, device=dev))


def spec_vis_sample(normal, view, rough, chunk_id, n_chunks, u_theta, u_phi):
    normal, view, rough = _f32(normal), _f32(view), _f32(rough).reshape(-1)
    u_theta, u_phi = _f32(u_theta), _f32(u_phi)
    n, ns = u_theta.shape
    sharp, cmin, dirs, wts, front = _spec_vis_buffers(n, ns, n_chunks, normal.device)
    call("rb_spec_vis_sample", ptr(normal), ptr(view), ptr(rough), ptr(chunk_id), c_long(n), c_int(n_chunks), c_int(ns),
         ptr(u_theta), ptr(u_phi), ptr(sharp), ptr(cmin), ptr(dirs), ptr(wts), ptr(front), stream_ptr())
    return dirs, wts, front


def spec_vis_sample_lobes(normal, view, lobes, lambdas, chunk_id, n_chunks, u_theta, u_phi):
    """spec_vis_sample for a caller's own lobes [n,3] / lambdas [n] (the reference's get_specular_visibility signature)."""
    normal, view, lobes, lambdas = _f32(normal), _f32(view), _f32(lobes), _f32(lambdas).reshape(-1)
    u_theta, u_phi = _f32(u_theta), _f32(u_phi)
    n, ns = u_theta.shape
    assert lobes.shape == (n, 3) and lambdas.shape == (n,), (lobes.shape, lambdas.shape)
    sharp, cmin, dirs, wts, front = _spec_vis_buffers(n, ns, n_chunks, normal.device)
    call("rb_spec_vis_sample_lobes", ptr(normal), ptr(view), ptr(lobes), ptr(lambdas), ptr(chunk_id), c_long(n), c_int(n_chunks), c_int(ns),
         ptr(u_theta), ptr(u_phi), ptr(sharp), ptr(cmin), ptr(dirs), ptr(wts), ptr(front), stream_ptr())
    return dirs, wts, front


def spec_vis_reduce(logits, front, wts, n, nsamp, inv, argmax_vis, testing):
    bvis = torch.empty(n, dtype=torch.float32, device=logits.device)
    call("rb_spec_vis_reduce", ptr(logits), ptr(front), ptr(wts), c_long(n), c_int(nsamp), c_int(int(inv)),
         c_int(int(argmax_vis)), c_int(int(testing)), ptr(bvis), stream_ptr())
    return bvis


def _f0_tensor(f0, dev):
    """f0 as a device tensor holding the scalar |specular_reflectance| (read by the kernel -- no host copy, no cache to go stale)."""
    if isinstance(f0, torch.Tensor):
        return f0.detach().to(device=dev, dtype=torch.float32).reshape(-1)[:1].contiguous()
    return torch.full((1,), float(f0), device=dev)


def sg_shade(normal, view, lgt, f0, rough, albedo, bvis, light_vis=None, metallic=None, indir_integral=None,
             lin_diff=False, want_shadow=False):
    normal, view, lgt, albedo = _f32(normal), _f32(view), _f32(lgt), _f32(albedo)
    rough = _f32(rough).reshape(-1)
    n = normal.shape[0]
    per_point = lgt.dim() == 3
    M = lgt.shape[-2]
    dev = normal.device
    rgb, spec, diff = (torch.empty(n, 3, dtype=torch.float32, device=dev) for _ in range(3))
    shadow = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_shadow else None
    f0 = _f0_tensor(f0, dev)
    call("rb_sg_shade", ptr(normal), ptr(view), ptr(lgt), c_int(1 if per_point else 0), c_int(M), ptr(f0), ptr(rough),
         ptr(albedo), ptr(_f32(metallic).reshape(-1) if metallic is not None else None),
         ptr(_f32(light_vis) if light_vis is not None else None), ptr(bvis),
         ptr(_f32(indir_integral) if indir_integral is not None else None), c_int(1 if lin_diff else 0), c_long(n),
         ptr(rgb), ptr(spec), ptr(diff), ptr(shadow), stream_ptr())
    return rgb, spec, diff, shadow


def sg_shade_backward(normal, view, lgt, f0, rough, albedo, bvis, spec, diff, g_spec, g_diff, light_vis=None, metallic=None,
                      indir_integral=None, lin_diff=False, want=("lgt", "f0", "rough", "albedo", "metallic", "bvis", "light_vis", "indir_integral")):
    """Reverse mode of sg_shade (rb_sg_shade_bwd): gradients of <g_spec, spec> + <g_diff, diff> for the inputs named in `want`, as a dict.
    spec / diff are sg_shade's own outputs for the same inputs (the clamp masks).  lgt [M,7] -> 'lgt' [M,7] summed over the points;
    [n,M,7] -> [n,M,7]; 'f0' [1] summed over the points.  Allocates the wanted outputs and the reduction scratch, nothing else: no
    [n,M] tensor unless 'light_vis' is asked for.  A name whose input is absent (metallic, light_vis, indir_integral = None) is skipped."""
    normal, view, lgt, albedo = _f32(normal), _f32(view), _f32(lgt), _f32(albedo)
    rough, bvis = _f32(rough).reshape(-1), _f32(bvis).reshape(-1)
    spec, diff, g_spec, g_diff = _f32(spec), _f32(diff), _f32(g_spec), _f32(g_diff)
    n = normal.shape[0]
    per_point = lgt.dim() == 3
    M = lgt.shape[-2]
    dev = normal.device
    f0 = _f0_tensor(f0, dev)
    metallic = _f32(metallic).reshape(-1) if metallic is not None else None
    light_vis = _f32(light_vis) if light_vis is not None else None
    indir_integral = _f32(indir_integral) if indir_integral is not None else None
    shapes = {"lgt": tuple(lgt.shape), "f0": (1,), "rough": (n,), "albedo": (n, 3), "bvis": (n,)}
    if metallic is not None:
        shapes["metallic"] = (n,)
    if light_vis is not None:
        shapes["light_vis"] = (n, M)
    if indir_integral is not None:
        shapes["indir_integral"] = (n, 3)
    alloc = torch.zeros if n == 0 else torch.empty           # n > 0: the kernels store every element of every wanted output
    out = {k: alloc(shapes[k], dtype=torch.float32, device=dev) for k in want if k in shapes}
    scratch, ns = None, 0
    if "f0" in out or ("lgt" in out and not per_point):
        ns = int(_lib.lib().rb_sg_shade_bwd_scratch_floats(c_int(M)))
        scratch = torch.empty(ns, dtype=torch.float32, device=dev)
    call("rb_sg_shade_bwd", ptr(normal), ptr(view), ptr(lgt), c_int(1 if per_point else 0), c_int(M), ptr(f0), ptr(rough), ptr(albedo),
         ptr(metallic), ptr(light_vis), ptr(bvis), ptr(indir_integral), c_int(1 if lin_diff else 0), c_long(n), ptr(spec), ptr(diff),
         ptr(g_spec), ptr(g_diff), ptr(out.get("rough")), ptr(out.get("albedo")), ptr(out.get("metallic")), ptr(out.get("bvis")),
         ptr(out.get("light_vis")), ptr(out.get("indir_integral")), ptr(out.get("lgt")), ptr(out.get("f0")), ptr(scratch), c_long(ns),
         stream_ptr())
    return out


def sg_shade_backward_groups(n):
    """Workgroups of rb_sg_shade_bwd's persistent grid for n points (four waves each; wave w of workgroup b: points 4b+w, 4b+w+4G, ...)."""
    return int(_lib.lib().rb_sg_shade_bwd_groups(c_long(n)))


# ------------------------------------------------------------------------------------------------ octree
def _host3(a, ctype):
    import numpy as np
    arr = np.ascontiguousarray(a, dtype=np.float32 if ctype is ctypes.c_float else np.int32)
    return (ctype * 3)(*[arr[i].item() for i in range(3)])


class OctreeTablesDev:
    """Device octree tables in the layout of include/robir_hip.h + host root description."""

    def __init__(self, node, nrm, B, root_min, root_size, res, min_step):
        self.node, self.nrm, self.B = node, nrm, int(B)
        self.root_min, self.root_size, self.res = root_min, root_size, res       # numpy float32[3], float32[3], int32[3]
        self.min_step = float(min_step)

    def args(self):
        return (ptr(self.node), ptr(self.nrm), c_long(self.B), _host3(self.root_min, ctypes.c_float),
                _host3(self.root_size, ctypes.c_float), _host3(self.res, ctypes.c_int))

    @property
    def clamp_dt(self):
        return self.min_step * 10


def octree_cast_batched(T, origins, per_ray_origin, dirs, batch, max_iter, step, sched_cap=0):
    dirs = _f32(dirs)
    origins = _f32(origins)
    R = dirs.shape[0]
    dev = dirs.device
    x = torch.empty(R, 3, dtype=torch.float32, device=dev)
    hit = torch.empty(R, dtype=torch.uint8, device=dev)
    t = torch.empty(R, dtype=torch.float32, device=dev)
    nb = (R + batch - 1) // batch
    sched = torch.zeros(nb, sched_cap, 2, dtype=torch.int32, device=dev) if sched_cap > 0 else None
    call("rb_octree_cast_batched", *T.args(), ptr(origins), c_int(1 if per_ray_origin else 0), ptr(dirs), c_long(R),
         c_int(batch), c_int(max_iter), ctypes.c_double(step), c_float(T.clamp_dt), ptr(x), ptr(hit), ptr(t), ptr(sched),
         c_int(sched_cap), stream_ptr())
    return x, hit.bool(), t, sched


CAST_ONE_LAUNCH = os.environ.get("ROBIR_CAST_ONE_LAUNCH", "1") == "1"    # the persistent-grid form of the general lock-step cast
CAST_COOP_REFUSED = 0              # how often the cooperative launch was refused and the per-iteration launches took over
CAST_ONE_LAUNCH_MAX_RAYS = 16384   # above this the per-iteration launches fill the chip and win (tools/ab_cast.py: 60 k rays 1.3 vs 2.1 ms)


def octree_cast_general(T, origins, dirs, max_iter, step, check_every=16, max_total=4096, one_launch=None):
    """One lock-step batch of any size: origins/dirs [R,3].  one_launch (default CAST_ONE_LAUNCH): init, every iteration and finish
    in one persistent launch (k_cast_coop) instead of one launch per iteration -- the same results bit for bit, no host sync."""
    dirs, origins = _f32(dirs), _f32(origins)
    R = dirs.shape[0]
    dev = dirs.device
    t = torch.empty(R, dtype=torch.float32, device=dev)
    leaf = torch.empty(R, dtype=torch.int32, device=dev)
    active = torch.empty(R, dtype=torch.uint8, device=dev)
    a = T.args()
    if (CAST_ONE_LAUNCH and R <= CAST_ONE_LAUNCH_MAX_RAYS) if one_launch is None else one_launch:
        counters = torch.zeros(max_total + 2, dtype=torch.int32, device=dev)
        arrive = torch.zeros(1024, dtype=torch.int64, device=dev)                # grid barrier: two 64-bit slots per workgroup (2 x 512, by epoch parity)
        x = torch.empty(R, 3, dtype=torch.float32, device=dev)
        hit = torch.empty(R, dtype=torch.uint8, device=dev)
        t_out = torch.empty(R, dtype=torch.float32, device=dev)
        rc = 0
        if R > 0:
            # status 2: the cooperative launch was refused by the runtime's STATIC occupancy check (or the device lacks cooperative
            # launches) and nothing ran -- the per-iteration launches below give the same bits.  The grid is at most one workgroup per
            # compute unit; residency beside concurrent work on other streams rests on the runtime's cooperative queue and is not
            # stress-tested here: ROBIR_CAST_ONE_LAUNCH=0 where in doubt (csrc/octree.hip)
            rc = _lib.lib().rb_octree_cast_coop(*a, ptr(origins), ptr(dirs), c_long(R), c_int(max_iter), ctypes.c_double(step),
                                                c_int(max_total), c_float(T.clamp_dt), ptr(t), ptr(leaf), ptr(active), ptr(counters),
                                                ptr(arrive), ptr(x), ptr(hit), ptr(t_out), stream_ptr())
            if rc not in (0, 2):
                raise _lib.RobirHipError(f"rb_octree_cast_coop failed ({rc}): {_lib.lib().rb_last_error().decode()}")
        if rc == 0:
            return x, hit.bool(), t_out, counters
        global CAST_COOP_REFUSED
        CAST_COOP_REFUSED += 1
    counters = torch.zeros(max_total + 2, dtype=torch.int32, device=dev)
    call("rb_octree_cast_init", *a, ptr(origins), ptr(dirs), c_long(R), c_int(max_iter), ptr(t), ptr(leaf), ptr(active),
         ptr(counters), stream_ptr())
    if max_iter > 0:
        call("rb_octree_cast_iter", *a, ptr(origins), ptr(dirs), c_long(R), c_int(max_iter), ctypes.c_double(step),
             c_int(0), c_int(max_iter + 1), ptr(t), ptr(leaf), ptr(active), ptr(counters), stream_ptr())
    else:
        it = 0
        while it < max_total:
            call("rb_octree_cast_iter", *a, ptr(origins), ptr(dirs), c_long(R), c_int(max_iter), ctypes.c_double(step),
                 c_int(it), c_int(check_every), ptr(t), ptr(leaf), ptr(active), ptr(counters), stream_ptr())
            it += check_every
            if int(counters[it].item()) == 0:      # host sync once per `check_every` iterations
                break
    x = torch.empty(R, 3, dtype=torch.float32, device=dev)
    hit = torch.empty(R, dtype=torch.uint8, device=dev)
    t_out = torch.empty(R, dtype=torch.float32, device=dev)
    call("rb_octree_cast_finish", *a, ptr(origins), ptr(dirs), c_long(R), c_int(max_iter), c_float(T.clamp_dt), ptr(t),
         ptr(leaf), ptr(x), ptr(hit), ptr(t_out), stream_ptr())
    return x, hit.bool(), t_out, counters


LAST_OCTREE_VIS_LAYOUT = None
OVIS_COMPACT = os.environ.get("ROBIR_OVIS_COMPACT", "1") == "1"   # stable compaction of the active rays between iterations
OVIS_CHUNKS_PER_CALL = 48       # chunks per traced-visibility launch group: bounds the scratch (28 B per pair slot) to ~5.6 GB


def dvis_octree(T, points, normals, chunk_id, n_chunks, dirs, wdir, wsum, L, nsamp, argmax_vis=False, eval_count=None,
                batch_pairs=2000000, max_iter=32, max_points_per_chunk=1024):
    """Traced light visibility (OctreeVisModel as the VisModel, csrc/octree_vis.hip) -> vis [n, L].  chunk_id ascending.
    Many chunks are walked in groups of OVIS_CHUNKS_PER_CALL (every chunk is its own set of lock-step groups, so the split
    changes nothing): the scratch is sized for the largest group instead of the whole view."""
    global LAST_OCTREE_VIS_LAYOUT
    points, normals = _f32(points), _f32(normals)
    n = points.shape[0]
    dev = points.device
    LS = L * nsamp
    out = torch.empty(n, L, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    if chunk_id is not None and n_chunks > OVIS_CHUNKS_PER_CALL:
        # first row of every chunk (chunk_id ascending): one small device -> host read per view
        bounds = torch.searchsorted(chunk_id, torch.arange(0, n_chunks + 1, OVIS_CHUNKS_PER_CALL, device=dev, dtype=chunk_id.dtype)
                                    ).tolist() + [n]
        total = None
        for k, c0 in enumerate(range(0, n_chunks, OVIS_CHUNKS_PER_CALL)):
            a, b = bounds[k], bounds[k + 1] if c0 + OVIS_CHUNKS_PER_CALL < n_chunks else n
            nc = min(OVIS_CHUNKS_PER_CALL, n_chunks - c0)
            if b > a:
                out[a:b] = _dvis_octree_impl(T, points[a:b], normals[a:b], (chunk_id[a:b] - c0).contiguous(), nc, dirs[c0 * LS:(c0 + nc) * LS],
                                       wdir[c0 * LS:(c0 + nc) * LS], wsum[c0 * L:(c0 + nc) * L], L, nsamp, argmax_vis, eval_count,
                                       batch_pairs, max_iter, max_points_per_chunk)
                total = LAST_OCTREE_VIS_LAYOUT.clone() if total is None else total + LAST_OCTREE_VIS_LAYOUT
        LAST_OCTREE_VIS_LAYOUT = total
        return out
    cap = n * LS
    # group table size: groups per chunk from the largest chunk population (k_ovis_layout would truncate the table otherwise).
    # Callers with chunks beyond 1024 points pass max_points_per_chunk; a count that cannot fit is caught here (host read
    # only in that case)
    per_chunk = n if chunk_id is None else max_points_per_chunk
    if chunk_id is not None and n > n_chunks * per_chunk:
        per_chunk = int(torch.bincount(chunk_id.long()).max())
    max_groups = n_chunks * ((per_chunk * LS + batch_pairs - 1) // batch_pairs) + 1
    i32 = lambda m: torch.empty(m, dtype=torch.int32, device=dev)
    i64 = lambda m: torch.empty(m, dtype=torch.int64, device=dev)
    pcount, prank, counters = i32(n), i32(n), i32(34 * max_groups)
    # layout: 4 scalars + 4096 per-workgroup (records read, ray steps) statistics slots (no device-wide atomics)
    chunk_tab, group_tab, point_span, layout = i64(4 * n_chunks + 4), i64(2 * max_groups), i64(2 * n), i64(4 + 2 * 4096)
    pair_p, leaf_st, grp = i32(cap), i32(cap), i32(cap)
    pair_j = torch.empty(cap, dtype=torch.int16, device=dev)
    t_st = torch.empty(cap, dtype=torch.float32, device=dev)
    act_st = torch.empty(cap, dtype=torch.uint8, device=dev)
    common = (*T.args(), ptr(points), ptr(normals), ptr(chunk_id), c_long(n), c_int(n_chunks), ptr(dirs), ptr(wdir),
              ptr(wsum), c_int(L), c_int(nsamp), c_int(1 if argmax_vis else 0), c_long(batch_pairs), c_int(max_iter), ptr(pcount),
              ptr(prank), ptr(chunk_tab), ptr(group_tab), c_int(max_groups), ptr(counters), ptr(pair_p), ptr(pair_j), ptr(t_st),
              ptr(leaf_st), ptr(act_st), ptr(grp), ptr(point_span), ptr(layout))
    if OVIS_COMPACT and cap < 2 ** 31 - 1:
        nblk = cap // 2048 + 2
        alive_a, alive_b, blk_cnt = i32(cap), i32(cap), i32(nblk)
        flags = torch.empty(cap + 8, dtype=torch.uint8, device=dev)
        blk_off, n_alive = i64(nblk), i64(2)
        call("rb_dvis_octree", *common, ptr(alive_a), ptr(alive_b), ptr(flags), ptr(blk_cnt), ptr(blk_off), ptr(n_alive),
             ptr(out), ptr(eval_count), stream_ptr())
    else:           # the plain walk: no compaction scratch
        call("rb_dvis_octree", *common, *([ptr(None)] * 6), ptr(out), ptr(eval_count), stream_ptr())
    lay4 = layout[:4].clone()            # device tensor [pairs, groups, node records read, ray-iterations] of the last call
    lay4[2:4] = layout[4:].view(4096, 2).sum(0)
    LAST_OCTREE_VIS_LAYOUT = lay4
    return out


_dvis_octree_impl = dvis_octree      # the chunk groups recurse through this name: a wrapper of ops.dvis_octree sees one call per view


def octree_cast_grouped(T, origins, dirs, group_start, max_iter=32):
    """Secondary lock-step cast of explicit rays in independent groups (group g = rays group_start[g]:group_start[g+1], a device
    int64 tensor of G+1 ascending offsets): what the reference computes calling the tracer once per group."""
    origins, dirs = _f32(origins), _f32(dirs)
    R = dirs.shape[0]
    dev = dirs.device
    G = group_start.numel() - 1
    assert group_start.dtype == torch.int64 and G >= 1
    x = torch.empty(R, 3, dtype=torch.float32, device=dev)
    hit = torch.empty(R, dtype=torch.uint8, device=dev)
    t = torch.empty(R, dtype=torch.float32, device=dev)
    if R == 0:
        return x, hit.bool(), t
    gsize = torch.empty(G, dtype=torch.int64, device=dev)
    grp, leaf_st = (torch.empty(R, dtype=torch.int32, device=dev) for _ in range(2))
    t_st = torch.empty(R, dtype=torch.float32, device=dev)
    act_st = torch.empty(R, dtype=torch.uint8, device=dev)
    counters = torch.empty(34 * G, dtype=torch.int32, device=dev)
    call("rb_octree_cast_grouped", *T.args(), ptr(origins), ptr(dirs), c_long(R), ptr(group_start.contiguous()), c_int(G),
         c_int(max_iter), c_float(T.clamp_dt), ptr(gsize), ptr(grp), ptr(t_st), ptr(leaf_st), ptr(act_st), ptr(counters), ptr(x),
         ptr(hit), ptr(t), stream_ptr())
    return x, hit.bool(), t


def pose_matrix(pose):
    """The 4x4 camera-to-world matrix of a pose given as 4x4 (returned as is) or as the 7-vector (qr, qi, qj, qk | cam_loc) of
    get_camera_params' quaternion branch (utils/rend_util.py:52-57; quat_to_rot, :107-124, normalises the quaternion first).  A host
    array stays a host array, a device tensor a device tensor (eleven scalar products of one pose: parameter conversion, no kernel)."""
    import numpy as np
    is_t = isinstance(pose, torch.Tensor)
    if (pose.numel() if is_t else np.asarray(pose).size) != 7:
        return pose
    q = (pose.detach().float().reshape(7) if is_t else torch.from_numpy(np.asarray(pose, dtype=np.float32).reshape(7)))
    loc = q[4:]
    qr, qi, qj, qk = (q[:4] / torch.clamp(q[:4].norm(), min=1e-12)).unbind(0)
    rows = [torch.stack([1 - 2 * (qj ** 2 + qk ** 2), 2 * (qj * qi - qk * qr), 2 * (qi * qk + qr * qj), loc[0]]),
            torch.stack([2 * (qj * qi + qk * qr), 1 - 2 * (qi ** 2 + qk ** 2), 2 * (qj * qk - qi * qr), loc[1]]),
            torch.stack([2 * (qk * qi - qj * qr), 2 * (qj * qk + qi * qr), 1 - 2 * (qi ** 2 + qj ** 2), loc[2]]),
            torch.tensor([0.0, 0.0, 0.0, 1.0], device=q.device)]
    m = torch.stack(rows)
    return m if is_t else m.numpy()


def camera_rays(pose, K, uv):
    """pose [4,4] (or the 7-vector quaternion form: pose_matrix), K [3,3]: host arrays, or device tensors (then they are read on the
    device: no blocking copy); uv [N,2] device."""
    import numpy as np
    pose = pose_matrix(pose)
    if isinstance(pose, torch.Tensor) and pose.is_cuda and isinstance(K, torch.Tensor) and K.is_cuda:
        uv = _f32(uv)
        N = uv.shape[0]
        dirs = torch.empty(N, 3, dtype=torch.float32, device=uv.device)
        call("rb_camera_rays_dev", ptr(_f32(pose.detach()).reshape(16)), ptr(_f32(K.detach()).reshape(9)), ptr(uv), c_long(N),
             ptr(dirs), stream_ptr())
        return dirs
    # host arrays: uploaded (one small blocking copy; the per-chunk path hands device tensors over)
    to_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    uv = _f32(uv)
    p = torch.from_numpy(np.ascontiguousarray(to_np(pose), dtype=np.float32).reshape(16).copy()).to(uv.device)
    k = torch.from_numpy(np.ascontiguousarray(to_np(K), dtype=np.float32).reshape(9).copy()).to(uv.device)
    N = uv.shape[0]
    dirs = torch.empty(N, 3, dtype=torch.float32, device=uv.device)
    call("rb_camera_rays_dev", ptr(p), ptr(k), ptr(uv), c_long(N), ptr(dirs), stream_ptr())
    return dirs


def points_along(origins, dirs, t, batch=None):
    """origins [N,3] (per ray) or [N/batch,3]."""
    origins, dirs, t = _f32(origins), _f32(dirs), _f32(t)
    N = dirs.shape[0]
    pts = torch.empty(N, 3, dtype=torch.float32, device=dirs.device)
    per_ray = batch is None
    call("rb_points_along", ptr(origins), c_int(1 if per_ray else 0), c_long(1 if per_ray else batch), ptr(dirs), ptr(t),
         c_long(N), ptr(pts), stream_ptr())
    return pts


def tonemap(x, shift, mode):
    x = _f32(x)
    shift = _f32(shift).reshape(-1)
    n = x.shape[0]
    y = torch.empty_like(x)
    stride = 0 if shift.numel() == 1 else 1
    assert stride == 0 or shift.numel() == n
    call("rb_tonemap", ptr(x), c_long(n), ptr(shift), c_int(stride), c_int(mode), ptr(y), stream_ptr())
    return y


# ------------------------------------------------------------------------------------------------ secondary rays / NeuS
def sphere_dirs(u1, u2, normals, points, nsamp):
    u1, u2, normals, points = _f32(u1).reshape(-1), _f32(u2).reshape(-1), _f32(normals), _f32(points)
    n = points.shape[0]
    dev = points.device
    dirs = torch.empty(n * nsamp, 3, dtype=torch.float32, device=dev)
    back = torch.empty(n * nsamp, dtype=torch.uint8, device=dev)
    cosw = torch.empty(n * nsamp, dtype=torch.float32, device=dev)
    origins = torch.empty(n, 3, dtype=torch.float32, device=dev)
    call("rb_sphere_dirs", ptr(u1), ptr(u2), ptr(normals), ptr(points), c_long(n), c_int(nsamp), ptr(dirs), ptr(back),
         ptr(cosw), ptr(origins), stream_ptr())
    return dirs, back, cosw, origins


def borrow_points(points, view, tk):
    points, view, tk = _f32(points), _f32(view), _f32(tk)
    m, ns = points.shape[0], tk.numel()
    x = torch.empty(m * ns, 3, dtype=torch.float32, device=points.device)
    d = torch.empty(m * ns, 3, dtype=torch.float32, device=points.device)
    call("rb_borrow_points", ptr(points), ptr(view), ptr(tk), c_long(m), c_int(ns), ptr(x), ptr(d), stream_ptr())
    return x, d


def neus_composite(sdf, color, inv_s, lo=0.0, hi=1.0, eps=1e-7, mask=None, want_weights=False):
    """sdf [m,ns]; color [m,ns,3] or None."""
    sdf = _f32(sdf)
    m, ns = sdf.shape
    dev = sdf.device
    rgb = torch.empty(m, 3, dtype=torch.float32, device=dev) if color is not None else None
    w = torch.empty(m, ns, dtype=torch.float32, device=dev) if want_weights else None
    call("rb_neus_composite", ptr(sdf), ptr(_f32(color) if color is not None else None),
         ptr(_f32(mask) if mask is not None else None), c_long(m), c_int(ns), c_float(inv_s), c_float(lo), c_float(hi),
         c_float(eps), ptr(rgb), ptr(w), stream_ptr())
    return rgb, w


def trace_integrate(rad, cosw, back, n, nsamp):
    out = torch.empty(n, 3, dtype=torch.float32, device=rad.device)
    call("rb_trace_integrate", ptr(_f32(rad)), ptr(cosw), ptr(back), c_long(n), c_int(nsamp), ptr(out), stream_ptr())
    return out


def envmap_sg(lgt, dirs):
    lgt, dirs = _f32(lgt), _f32(dirs)
    n = dirs.shape[0]
    rgb = torch.empty(n, 3, dtype=torch.float32, device=dirs.device)
    call("rb_envmap_sg", ptr(lgt), c_int(lgt.shape[0]), ptr(dirs), c_long(n), ptr(rgb), stream_ptr())
    return rgb


def envmap_lookup(env, dirs):
    env, dirs = _f32(env), _f32(dirs)
    H, W = env.shape[0], env.shape[1]
    n = dirs.shape[0]
    rgb = torch.empty(n, 3, dtype=torch.float32, device=dirs.device)
    call("rb_envmap_lookup", ptr(env), c_int(H), c_int(W), ptr(dirs), c_long(n), ptr(rgb), stream_ptr())
    return rgb


def cesr_net(X, M, kind, blob, n_label=1):
    """kind 0 normal_net (X[M,64] -> [M,3]); 1 shadow_net dense rows (X[M,192] -> [M,2]);
    2 shadow_net on (point, label) pairs (X = point features [M/n_label,64], M rows -> [M,2])."""
    n_out = 3 if kind == 0 else 2
    Y = torch.empty(M, n_out, dtype=torch.float32, device=X.device)
    call("rb_cesr_net", ptr(_f32(X)), c_long(M), c_int(kind), c_int(n_label), ptr(blob), ptr(Y), stream_ptr())
    return Y


def cesr_net_h3(X, M, kind, blob, scale_log2, n_label=1):
    n_out = 3 if kind == 0 else 2
    Y = torch.empty(M, n_out, dtype=torch.float32, device=X.device)
    call("rb_cesr_net_h3", ptr(_f32(X)), c_long(M), c_int(kind), c_int(n_label), ptr(blob), c_int(scale_log2), ptr(Y),
         stream_ptr())
    return Y


def cesr_net_points(x, M, kind, blob, n_label=1, scale_log2=None, ring=None):
    """cesr_net / cesr_net_h3 on PE10(x) with the encoding fused (kind 0: M = points; kind 2: M = points * n_label rows).
    ring (split precision; the default): the chunk-stream kernel (csrc/wide_ring.h) -- bit-identical outputs."""
    x = _f32(x)
    Y = torch.empty(M, 3 if kind == 0 else 2, dtype=torch.float32, device=x.device)
    if scale_log2 is None:
        call("rb_cesr_net_points", ptr(x), c_long(M), c_int(kind), c_int(n_label), ptr(blob), ptr(Y), stream_ptr())
    elif ring is None or ring:
        call("rb_cesr_net_ring_points", ptr(x), c_long(M), c_int(kind), c_int(n_label), ptr(blob), c_int(scale_log2), ptr(Y), c_int(0),
             stream_ptr())
    else:
        call("rb_cesr_net_h3_points", ptr(x), c_long(M), c_int(kind), c_int(n_label), ptr(blob), c_int(scale_log2), ptr(Y), stream_ptr())
    return Y


def scatter_rows(srcs, dst_widths, idx, N, fill=1.0):
    """Per-pixel outputs in one launch: srcs[k] [n, 1 or w_k] rows of the pixels idx -> list of K tensors [N, w_k] (other rows =
    fill); entries of srcs may be None (a block that only holds the default).  One allocation, one fill, one scatter."""
    dev = idx.device
    total = sum(dst_widths)
    flat = torch.full((N * total,), fill, dtype=torch.float32, device=dev)
    outs, off = [], 0
    for w in dst_widths:
        outs.append(flat[off:off + N * w].view(N, w))
        off += N * w
    n = idx.shape[0]
    live = [k for k, s in enumerate(srcs) if s is not None]
    if n > 0 and live:
        # blocks without a source must come last in the scatter's view of the buffer: keep the order, skip by offset instead
        assert live == list(range(len(live))), "sources first, default-only blocks last"
        keep = [_f32(srcs[k]) for k in live]
        K = len(keep)
        src_arr = (ctypes.c_void_p * K)(*[t.data_ptr() for t in keep])
        sw = (ctypes.c_int * K)(*[int(t.shape[-1]) for t in keep])
        dw = (ctypes.c_int * K)(*[int(dst_widths[k]) for k in live])
        call("rb_scatter_rows", src_arr, sw, dw, c_int(K), ptr(idx), c_long(n), c_long(N), ptr(flat), stream_ptr())
    return outs


def cesr_net_x6_points(x, M, kind, blob, n_label=1):
    """cesr_net_points on exact three-piece operands (csrc/cesr_x6.hip; blob = packing.pack_softplus512_x6)."""
    x = _f32(x)
    Y = torch.empty(M, 3 if kind == 0 else 2, dtype=torch.float32, device=x.device)
    if M > 0:
        call("rb_cesr_net_x6_points", ptr(x), c_long(M), c_int(kind), c_int(n_label), ptr(blob), ptr(Y), c_int(0), stream_ptr())
    return Y


CESR_F16_TILES = 3        # 16-row tiles per wave of the f16 CESR kernel (the one count the library carries: csrc/cesr_f16.hip FX_NTILES)


def cesr_net_f16_points(x, M, kind, blob, n_label=1):
    """The CESR nets in PLAIN f16 (csrc/cesr_f16.hip; blob = packing.pack_softplus512_f16): the f16 throughput mode -- NARROWER than fp32."""
    x = _f32(x)
    Y = torch.empty(M, 3 if kind == 0 else 2, dtype=torch.float32, device=x.device)
    if M > 0:
        call("rb_cesr_net_f16_points", ptr(x), c_long(M), c_int(kind), c_int(n_label), ptr(blob), ptr(Y), c_int(CESR_F16_TILES), c_int(0),
             stream_ptr())
    return Y


def material_decode(brdf, brdf_r):
    brdf, brdf_r = _f32(brdf), _f32(brdf_r)
    n, dev = brdf.shape[0], brdf.device
    mk = lambda c: torch.empty(n, c, dtype=torch.float32, device=dev)
    alb, rough, metal, alb_r, rough_r, metal_r = mk(3), mk(1), mk(1), mk(3), mk(1), mk(1)
    call("rb_material_decode", ptr(brdf), ptr(brdf_r), c_long(n), ptr(alb), ptr(rough), ptr(metal), ptr(alb_r), ptr(rough_r),
         ptr(metal_r), stream_ptr())
    return alb, rough, metal, alb_r, rough_r, metal_r


def abs_scale(x, s=1.0, take_abs=True):
    x = _f32(x)
    y = torch.empty_like(x)
    call("rb_abs_scale", ptr(x), c_long(x.numel()), c_float(s), c_int(1 if take_abs else 0), ptr(y), stream_ptr())
    return y


def softmax2(logits, which=1):
    logits = _f32(logits)
    n = logits.shape[0]
    p = torch.empty(n, dtype=torch.float32, device=logits.device)
    call("rb_softmax2", ptr(logits), c_long(n), c_int(which), ptr(p), stream_ptr())
    return p


def lin_diff_combine(diffuse, albedo, spec):
    diffuse, albedo, spec = _f32(diffuse), _f32(albedo), _f32(spec)
    rgb = torch.empty_like(diffuse)
    call("rb_lin_diff_combine", ptr(diffuse), ptr(albedo), ptr(spec), c_long(diffuse.shape[0]), ptr(rgb), stream_ptr())
    return rgb


# ---- IDR sphere tracer (use_octree=False) -----------------------------------------------------------------------------
class RayTraceState:
    """Device state of rb_raytrace_step for N rays (layout in include/robir_hip.h)."""

    def __init__(self, cam, dirs):
        self.cam, self.dirs = _f32(cam).reshape(-1, 3), _f32(dirs)
        self.N = N = self.dirs.shape[0]
        assert self.cam.shape[0] in (1, N)
        self.cs = 0 if self.cam.shape[0] == 1 else 3
        dev = dirs.device
        self.f = torch.zeros(6, N, dtype=torch.float32, device=dev)
        self.b = torch.zeros(4, N, dtype=torch.uint8, device=dev)
        self.pts = torch.zeros(2 * N, 3, dtype=torch.float32, device=dev)
        self.ctrl = torch.zeros(2, dtype=torch.int32, device=dev)

    def step(self, op, param=0.0, sdf2=None):
        s = _f32(sdf2) if sdf2 is not None else None
        call("rb_raytrace_step", c_int(op), ptr(self.cam), c_int(self.cs), ptr(self.dirs), c_long(self.N), c_float(param),
             ptr(s), ptr(self.f), ptr(self.b), ptr(self.pts), ptr(self.ctrl), stream_ptr())


def raytrace_samples(cam, dirs, lo, hi, lin):
    cam, dirs, lo, hi, lin = _f32(cam).reshape(-1, 3), _f32(dirs), _f32(lo), _f32(hi), _f32(lin)
    m, n = dirs.shape[0], lin.shape[0]
    z = torch.empty(m, n, dtype=torch.float32, device=dirs.device)
    P = torch.empty(m * n, 3, dtype=torch.float32, device=dirs.device)
    call("rb_raytrace_samples", ptr(cam), c_int(0 if cam.shape[0] == 1 else 3), ptr(dirs), ptr(lo), ptr(hi), ptr(lin),
         c_long(m), c_int(n), ptr(z), ptr(P), stream_ptr())
    return z, P


def raytrace_pick(sdf, z, P, obj):
    m, n = z.shape
    dev = z.device
    obj = obj.to(torch.uint8).contiguous()
    pts = torch.empty(m, 3, dtype=torch.float32, device=dev)
    dist = torch.empty(m, dtype=torch.float32, device=dev)
    hit = torch.empty(m, dtype=torch.uint8, device=dev)
    bracket = torch.empty(4, m, dtype=torch.float32, device=dev)
    call("rb_raytrace_pick", ptr(_f32(sdf)), ptr(z), ptr(P), ptr(obj), c_long(m), c_int(n), ptr(pts), ptr(dist), ptr(hit),
         ptr(bracket), stream_ptr())
    return pts, dist, hit, bracket


def raytrace_secant(cam, dirs, on, smid, phase, bracket, zp, pmid):
    cam = _f32(cam).reshape(-1, 3)
    s = _f32(smid) if smid is not None else None
    call("rb_raytrace_secant", ptr(cam), c_int(0 if cam.shape[0] == 1 else 3), ptr(dirs), ptr(on), ptr(s),
         c_long(dirs.shape[0]), c_int(phase), ptr(bracket), ptr(zp), ptr(pmid), stream_ptr())


# ------------------------------------------------------------------------------------------------ public helper names (csrc/surface.hip)
def pe_encode(x, freq, include_input=True):
    """x [n,d], freq [n_freq] device band values -> [n, (d if include_input) + 2 d n_freq]."""
    x, freq = _f32(x), _f32(freq)
    n, d = x.shape
    out = torch.empty(n, (d if include_input else 0) + 2 * d * freq.shape[0], dtype=torch.float32, device=x.device)
    call("rb_pe_encode", ptr(x), c_long(n), c_int(d), ptr(freq), c_int(freq.shape[0]), c_int(1 if include_input else 0), ptr(out),
         stream_ptr())
    return out


def expected_sin(x, var, want_var=True):
    x, var = _f32(x), _f32(var)
    assert x.shape == var.shape
    y = torch.empty_like(x)
    yv = torch.empty_like(x) if want_var else None
    call("rb_expected_sin", ptr(x), ptr(var), c_long(x.numel()), ptr(y), ptr(yv), stream_ptr())
    return y, yv


def tonemap_curve(x, shift, curve):
    """Free functions of model/color_correction.py:31-73 (no clamp).  x any shape; shift None, one value, [..., 1] against x [..., w], or
    anything that broadcasts to x's shape."""
    x = _f32(x)
    y = torch.empty_like(x)
    width, stride, sh = 1, 0, None
    if shift is not None:
        sh = shift.to(device=x.device, dtype=torch.float32)
        if sh.numel() == 1:
            sh = sh.reshape(1).contiguous()
        elif sh.dim() == x.dim() and sh.shape[-1] == 1 and sh.shape[:-1] == x.shape[:-1]:
            width, stride, sh = x.shape[-1], 1, sh.contiguous()
        else:
            width, stride, sh = 1, 1, sh.expand(x.shape).contiguous()
    call("rb_tonemap_curve", ptr(x), c_long(x.numel()), c_int(width), ptr(sh), c_int(stride), c_int(curve), ptr(y), stream_ptr())
    return y


def sample_pdf(bins, weights, u):
    """bins [R,n], weights [R,n-1], u [n_s] (shared) or [R,n_s] -> (samples [R,n_s], cdf [R,n])."""
    bins, weights, u = _f32(bins), _f32(weights), _f32(u)
    R, n = bins.shape
    assert weights.shape == (R, n - 1)
    n_s = u.shape[-1]
    assert u.dim() == 1 or u.shape == (R, n_s)
    cdf = torch.empty(R, n, dtype=torch.float32, device=bins.device)
    out = torch.empty(R, n_s, dtype=torch.float32, device=bins.device)
    call("rb_sample_pdf", ptr(bins), ptr(weights), c_long(R), c_int(n), ptr(u), c_long(0 if u.dim() == 1 else n_s), c_int(n_s), ptr(cdf),
         ptr(out), stream_ptr())
    return out, cdf


def neus_core_aux(sdf, sdf_stride, pts, z, R, n, inv_s, radius, sample_dist):
    dev = pts.device
    dists, cdf, inside = (torch.empty(R, n, dtype=torch.float32, device=dev) for _ in range(3))
    call("rb_neus_core_aux", ptr(sdf), c_long(sdf_stride), ptr(pts), ptr(z), c_long(R), c_int(n), c_float(inv_s), c_float(radius),
         c_float(sample_dist), ptr(dists), ptr(cdf), ptr(inside), stream_ptr())
    return dists, cdf, inside


def sample_dirs(normals, theta, phi):
    normals, theta, phi = _f32(normals), _f32(theta), _f32(phi)
    n = theta.numel()
    assert normals.numel() == 3 * n and phi.numel() == n
    out = torch.empty(n, 3, dtype=torch.float32, device=normals.device)
    call("rb_sample_dirs", ptr(normals), ptr(theta), ptr(phi), c_long(n), ptr(out), stream_ptr())
    return out


def intersect_sphere(origins, dirs, radius):
    origins, dirs = _f32(origins), _f32(dirs)
    n = origins.shape[0]
    out = torch.empty(n, 3, dtype=torch.float32, device=origins.device)
    call("rb_intersect_sphere", ptr(origins), ptr(dirs), c_long(n), c_float(radius), ptr(out), stream_ptr())
    return out


# ----------------------------------------------------------------------------------------- isosurface extraction (csrc/mesh.hip)
def mesh_groups(nx, ny, nz):
    L = _lib.lib()
    g = L.rb_mesh_groups(c_int(nx), c_int(ny), c_int(nz))
    if g < 0:
        raise _lib.RobirHipError(f"rb_mesh_groups failed: {L.rb_last_error().decode()}")
    return int(g)


def mesh_table():
    """The generated marching-tetrahedra table as a [6,16,7] int list: per (tetrahedron, inside mask) the triangle count and six tet edge ids."""
    buf = (ctypes.c_int * (6 * 16 * 7))()
    call("rb_mesh_table", buf)
    return [[list(buf[(t * 16 + m) * 7:(t * 16 + m) * 7 + 7]) for m in range(16)] for t in range(6)]


def mesh_count(field, iso):
    """field [nx,ny,nz] -> counts [G,2] int32: mesh vertices and triangles per workgroup of 256 lattice vertices."""
    field = _f32(field)
    nx, ny, nz = field.shape
    counts = torch.empty(mesh_groups(nx, ny, nz), 2, dtype=torch.int32, device=field.device)
    call("rb_mesh_count", ptr(field), c_int(nx), c_int(ny), c_int(nz), c_float(iso), ptr(counts), c_long(counts.numel()), stream_ptr())
    return counts


def mesh_emit_vertices(field, xs, ys, zs, iso, group_base, V):
    """group_base [G] int64 exclusive prefix of the vertex counts -> (verts [V,3], vbase [nx,ny,nz] int32)."""
    field, xs, ys, zs = _f32(field), _f32(xs), _f32(ys), _f32(zs)
    nx, ny, nz = field.shape
    assert (xs.numel(), ys.numel(), zs.numel()) == (nx, ny, nz) and group_base.dtype == torch.int64
    verts = torch.empty(V, 3, dtype=torch.float32, device=field.device)
    vbase = torch.empty(nx, ny, nz, dtype=torch.int32, device=field.device)
    call("rb_mesh_emit_vertices", ptr(field), ptr(xs), ptr(ys), ptr(zs), c_int(nx), c_int(ny), c_int(nz), c_float(iso), ptr(group_base),
         c_long(V), ptr(verts), ptr(vbase), stream_ptr())
    return verts, vbase


def mesh_emit_faces(field, iso, group_base, vbase, V, F):
    field = _f32(field)
    nx, ny, nz = field.shape
    assert group_base.dtype == torch.int64 and vbase.dtype == torch.int32 and vbase.numel() == field.numel()
    faces = torch.empty(F, 3, dtype=torch.int32, device=field.device)
    call("rb_mesh_emit_faces", ptr(field), c_int(nx), c_int(ny), c_int(nz), c_float(iso), ptr(group_base), ptr(vbase), c_long(V), c_long(F),
         ptr(faces), stream_ptr())
    return faces


def mesh_block_points(blocks, B, xs, ys, zs):
    """blocks [nb] int32 block ids -> pts [nb*B^3, 3]."""
    assert blocks.dtype == torch.int32
    n = blocks.numel() * B ** 3
    pts = torch.empty(n, 3, dtype=torch.float32, device=xs.device)
    call("rb_mesh_block_points", ptr(blocks), c_long(blocks.numel()), c_int(B), ptr(_f32(xs)), ptr(_f32(ys)), ptr(_f32(zs)),
         c_int(xs.numel()), c_int(ys.numel()), c_int(zs.numel()), ptr(pts), c_long(n), stream_ptr())
    return pts


def mesh_block_store(blocks, B, vals, field):
    assert blocks.dtype == torch.int32 and field.dtype == torch.float32 and field.is_contiguous()
    vals = _f32(vals)
    nx, ny, nz = field.shape
    call("rb_mesh_block_store", ptr(blocks), c_long(blocks.numel()), c_int(B), ptr(vals), c_long(vals.numel()), c_int(nx), c_int(ny),
         c_int(nz), ptr(field), stream_ptr())


def mesh_block_fill(blocks, B, vals, field):
    assert blocks.dtype == torch.int32 and field.dtype == torch.float32 and field.is_contiguous()
    vals = _f32(vals)
    assert vals.numel() == blocks.numel()
    nx, ny, nz = field.shape
    call("rb_mesh_block_fill", ptr(blocks), c_long(blocks.numel()), c_int(B), ptr(vals), c_int(nx), c_int(ny), c_int(nz), ptr(field),
         stream_ptr())


# ----------------------------------------------------------------------------------------- texture space (csrc/texbake/texbake.hip)
TB_TILE, TB_MAX_RESOLUTION = 8, 16384


def _tb_uv(uv):
    uv = _f32(uv)
    if uv.dim() != 3 or tuple(uv.shape[1:]) != (3, 2):
        raise ValueError(f"texture space: uv must be [F,3,2] per face corner, got {tuple(uv.shape)}")
    return uv


def tb_atlas_cell(n_faces, resolution):
    """Cell size S of the per-triangle atlas; ValueError (naming the smallest resolution that works) below S = 6."""
    L = _lib.texbake()
    S = L.rb_tb_atlas_cell(c_long(int(n_faces)), c_int(int(resolution)))
    if S < 0:
        raise ValueError("atlas_uv: " + _lib.aux_error(L))
    return int(S)


def tb_atlas_uv(n_faces, resolution, device):
    tb_atlas_cell(n_faces, resolution)
    uv = torch.empty(int(n_faces), 3, 2, dtype=torch.float32, device=device)
    _lib.call_texbake("rb_tb_atlas_uv", c_long(int(n_faces)), c_int(int(resolution)), ptr(uv), stream_ptr())
    return uv


def tb_bin_count(uv, R):
    """uv [F,3,2] -> counts [F] int32: tiles of 8 x 8 texels each face's texel box touches."""
    uv = _tb_uv(uv)
    counts = torch.empty(uv.shape[0], dtype=torch.int32, device=uv.device)
    _lib.call_texbake("rb_tb_bin_count", ptr(uv), c_long(uv.shape[0]), c_int(R), ptr(counts), stream_ptr())
    return counts


def tb_bin_emit(uv, R, base, P):
    """base [F] int64 exclusive prefix of the counts, P their total -> (pair_tile [P], pair_face [P]) int32 in face order."""
    uv = _tb_uv(uv)
    assert base.dtype == torch.int64 and base.numel() == uv.shape[0]
    pair_tile = torch.empty(P, dtype=torch.int32, device=uv.device)
    pair_face = torch.empty(P, dtype=torch.int32, device=uv.device)
    _lib.call_texbake("rb_tb_bin_emit", ptr(uv), c_long(uv.shape[0]), c_int(R), ptr(base), c_long(P), ptr(pair_tile), ptr(pair_face), stream_ptr())
    return pair_tile, pair_face


def tb_raster(uv, R, tile_start, pair_face):
    """-> (face_id [R,R] int32, bary [R,R,2])."""
    uv = _tb_uv(uv)
    ntiles = (R + TB_TILE - 1) // TB_TILE
    assert tile_start.dtype == torch.int32 and tile_start.numel() == ntiles * ntiles + 1 and pair_face.dtype == torch.int32
    face_id = torch.empty(R, R, dtype=torch.int32, device=uv.device)
    bary = torch.empty(R, R, 2, dtype=torch.float32, device=uv.device)
    P = pair_face.numel()
    _lib.call_texbake("rb_tb_raster", ptr(uv) if uv.numel() else None, c_long(uv.shape[0]), c_int(R), ptr(tile_start),
                      ptr(pair_face) if P else None, c_long(P), ptr(face_id), ptr(bary), stream_ptr())
    return face_id, bary


def tb_interp(face_id, bary, faces, attr, index=None):
    """attr [V,C] at the texels of face_id / bary -> [R,R,C] (index None) or [n,C] at the flat texel indices index [n] int64."""
    assert face_id.dtype == torch.int32 and face_id.is_contiguous() and faces.dtype == torch.int32
    bary, attr, faces = _f32(bary), _f32(attr), faces.contiguous()
    if attr.dim() != 2 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"interpolate: attr must be [V,C] and faces [F,3], got {tuple(attr.shape)}, {tuple(faces.shape)}")
    T, C = face_id.numel(), attr.shape[1]
    if index is None:
        n, out = T, torch.empty(*face_id.shape, C, dtype=torch.float32, device=face_id.device)
    else:
        assert index.dtype == torch.int64 and index.is_contiguous()
        n, out = index.numel(), torch.empty(index.numel(), C, dtype=torch.float32, device=face_id.device)
    nz = lambda t: ptr(t) if t.numel() else None
    _lib.call_texbake("rb_tb_interp", ptr(face_id), ptr(bary), c_long(T), None if index is None else nz(index), c_long(n), nz(faces),
                      c_long(faces.shape[0]), nz(attr), c_long(attr.shape[0]), c_int(C), nz(out), stream_ptr())
    return out


def tb_dilate(image, mask):
    """One ring: image [H,W,C], mask [H,W] uint8 -> (image', mask') in new tensors."""
    image = _f32(image)
    assert mask.dtype == torch.uint8 and mask.is_contiguous() and image.dim() == 3 and tuple(mask.shape) == tuple(image.shape[:2])
    H, W, C = image.shape
    dst, mask_out = torch.empty_like(image), torch.empty_like(mask)
    _lib.call_texbake("rb_tb_dilate", ptr(image), ptr(mask), c_int(H), c_int(W), c_int(C), ptr(dst), ptr(mask_out), stream_ptr())
    return dst, mask_out


def tb_sample(position, normal, mask, uv, scale):
    """position, normal [R,R,3], mask [R,R], uv [n,2] -> x, normal, object_mask (uint8), tangent_u, tangent_v."""
    position, normal, mask, uv = _f32(position), _f32(normal), _f32(mask), _f32(uv)
    R, n, dev = position.shape[0], uv.shape[0], position.device
    assert tuple(position.shape) == (R, R, 3) and tuple(normal.shape) == (R, R, 3) and tuple(mask.shape) == (R, R) and tuple(uv.shape) == (n, 2)
    x, nrm, tu, tv = (torch.empty(n, 3, dtype=torch.float32, device=dev) for _ in range(4))
    om = torch.empty(n, dtype=torch.uint8, device=dev)
    if n:
        _lib.call_texbake("rb_tb_sample", ptr(position), ptr(normal), ptr(mask), c_int(R), ptr(uv), c_long(n), c_float(scale), ptr(x), ptr(nrm),
                          ptr(om), ptr(tu), ptr(tv), stream_ptr())
    return x, nrm, om, tu, tv


# ----------------------------------------------------------------------------------------- observations (csrc/observe/observe.hip)
OB_MAX_CAMERAS, OB_MAX_OBS = 4096, 8


def _ob_cameras(cam_loc, pose_inv, K):
    cam_loc, pose_inv, K = _f32(cam_loc), _f32(pose_inv), _f32(K)
    M = cam_loc.shape[0]
    if tuple(cam_loc.shape) != (M, 3) or tuple(pose_inv.shape) != (M, 4, 4) or tuple(K.shape) != (M, 3, 3):
        raise ValueError(f"observations: cam_loc [M,3], pose_inv [M,4,4], intrinsics [M,3,3], got {tuple(cam_loc.shape)}, "
                         f"{tuple(pose_inv.shape)}, {tuple(K.shape)}")
    return cam_loc, pose_inv, K, M


def _ob_images(images, M):
    images = _f32(images)
    if images.dim() != 4 or images.shape[0] != M:
        raise ValueError(f"observations: images must be [M,H,W,C] for M = {M} cameras, got {tuple(images.shape)}")
    return images


def ob_scatter(x, cam_loc, pose_inv, K, images, masks=None):
    """x [N,3]; cam_loc [M,3], pose_inv [M,4,4], K [M,3,3]; images [M,H,W,C], masks [M,H,W] or None -> uv [M,N,2], view_dir [M,N,3],
    rgb [M,N,C], valid [M,N] uint8."""
    x = _f32(x)
    cam_loc, pose_inv, K, M = _ob_cameras(cam_loc, pose_inv, K)
    images = _ob_images(images, M)
    _, H, W, C = images.shape
    if masks is not None:
        masks = _f32(masks)
        if tuple(masks.shape) != (M, H, W):
            raise ValueError(f"observations: masks must be [M,H,W] = {(M, H, W)}, got {tuple(masks.shape)}")
    N, dev = x.shape[0], x.device
    assert tuple(x.shape) == (N, 3)
    uv = torch.empty(M, N, 2, dtype=torch.float32, device=dev)
    view_dir = torch.empty(M, N, 3, dtype=torch.float32, device=dev)
    rgb = torch.empty(M, N, C, dtype=torch.float32, device=dev)
    valid = torch.empty(M, N, dtype=torch.uint8, device=dev)
    nz = lambda t: ptr(t) if t.numel() else None
    _lib.call_observe("rb_ob_scatter", nz(x), c_long(N), ptr(cam_loc), ptr(pose_inv), ptr(K), c_int(M), ptr(images),
                      None if masks is None else ptr(masks), c_int(H), c_int(W), c_int(C), nz(uv), nz(view_dir), nz(rgb), nz(valid), stream_ptr())
    return uv, view_dir, rgb, valid


def ob_select(vis, draws, n_obs):
    """vis [M,N] uint8, draws [M,N] -> (index [n_obs,N] int32: the cameras of the n_obs largest keys vis + 0.01 draws, count [N] int32)."""
    draws = _f32(draws)
    assert vis.dtype == torch.uint8 and vis.is_contiguous() and vis.dim() == 2 and tuple(draws.shape) == tuple(vis.shape)
    M, N = vis.shape
    index = torch.empty(int(n_obs), N, dtype=torch.int32, device=vis.device)
    count = torch.empty(N, dtype=torch.int32, device=vis.device)
    nz = lambda t: ptr(t) if t.numel() else None
    _lib.call_observe("rb_ob_select", nz(vis), nz(draws), c_int(M), c_long(N), c_int(int(n_obs)), nz(index), nz(count), stream_ptr())
    return index, count


def ob_accumulate(x, normals, cam_loc, pose_inv, K, images, vis):
    """x, normals [N,3]; vis [M,N] uint8 -> (weight [N], mean [N,C], var [N,C], count [N] int32) of the colours the visible cameras see,
    weighted by max(-n . view_dir, 0)."""
    x, normals = _f32(x), _f32(normals)
    cam_loc, pose_inv, K, M = _ob_cameras(cam_loc, pose_inv, K)
    images = _ob_images(images, M)
    _, H, W, C = images.shape
    N, dev = x.shape[0], x.device
    assert tuple(x.shape) == (N, 3) and tuple(normals.shape) == (N, 3)
    assert vis.dtype == torch.uint8 and vis.is_contiguous() and tuple(vis.shape) == (M, N)
    weight = torch.empty(N, dtype=torch.float32, device=dev)
    mean = torch.empty(N, C, dtype=torch.float32, device=dev)
    var = torch.empty(N, C, dtype=torch.float32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    nz = lambda t: ptr(t) if t.numel() else None
    _lib.call_observe("rb_ob_accumulate", nz(x), nz(normals), c_long(N), ptr(cam_loc), ptr(pose_inv), ptr(K), c_int(M), ptr(images), c_int(H),
                      c_int(W), c_int(C), nz(vis), nz(weight), nz(mean), nz(var), nz(count), stream_ptr())
    return weight, mean, var, count


def ob_fetch(images, uv):
    """images [M,H,W,C], uv [M,N,2] pixel positions -> [M,N,C]: grid_sample(align_corners=True, zeros padding) per camera."""
    uv = _f32(uv)
    images = _ob_images(images, uv.shape[0])
    M, H, W, C = images.shape
    N = uv.shape[1]
    assert tuple(uv.shape) == (M, N, 2)
    out = torch.empty(M, N, C, dtype=torch.float32, device=images.device)
    nz = lambda t: ptr(t) if t.numel() else None
    _lib.call_observe("rb_ob_fetch", ptr(images), c_int(M), c_int(H), c_int(W), c_int(C), nz(uv), c_long(N), nz(out), stream_ptr())
    return out


def ob_gather(index, x, cam_loc, pose_inv, K, images, masks=None):
    """ob_scatter for the pairs (index[k][n], n) only: index [n_obs,N] int32 -> uv [n_obs,N,2], view_dir [n_obs,N,3], rgb [n_obs,N,C],
    valid [n_obs,N] uint8; zeros where the index is negative."""
    x = _f32(x)
    cam_loc, pose_inv, K, M = _ob_cameras(cam_loc, pose_inv, K)
    images = _ob_images(images, M)
    _, H, W, C = images.shape
    if masks is not None:
        masks = _f32(masks)
        assert tuple(masks.shape) == (M, H, W)
    N, dev = x.shape[0], x.device
    assert index.dtype == torch.int32 and index.is_contiguous() and index.dim() == 2 and index.shape[1] == N and tuple(x.shape) == (N, 3)
    n_obs = index.shape[0]
    uv = torch.empty(n_obs, N, 2, dtype=torch.float32, device=dev)
    view_dir = torch.empty(n_obs, N, 3, dtype=torch.float32, device=dev)
    rgb = torch.empty(n_obs, N, C, dtype=torch.float32, device=dev)
    valid = torch.empty(n_obs, N, dtype=torch.uint8, device=dev)
    nz = lambda t: ptr(t) if t.numel() else None
    _lib.call_observe("rb_ob_gather", nz(index), c_int(n_obs), nz(x), c_long(N), ptr(cam_loc), ptr(pose_inv), ptr(K), c_int(M), ptr(images),
                      None if masks is None else ptr(masks), c_int(H), c_int(W), c_int(C), nz(uv), nz(view_dir), nz(rgb), nz(valid), stream_ptr())
    return uv, view_dir, rgb, valid


# ------------------------------------------------------------------------------------------------ photometric loss (librobir_hip_photoloss.so)
PL_CURVE_IDENTITY, PL_CURVE_RATIONAL = 3, 4


def _pl_shift(shift, n, dev):
    """-> (tensor or None, stride): a single value or one per row."""
    if shift is None:
        return None, 0
    shift = _f32(shift).reshape(-1)
    if shift.numel() != 1 and shift.numel() != n:
        raise ValueError(f"photometric loss: the shift has {shift.numel()} values for {n} rows (one, or one per row)")
    return shift, (0 if shift.numel() == 1 else 1)


def _pl_scratch(n, dev):
    return torch.empty(max(16, int(_lib.photoloss().rb_pl_scratch_bytes(c_long(n)))), dtype=torch.uint8, device=dev)


def pl_tonemap(x, shift, curve, inverse=0):
    """x [n,3], shift [1] | [n] (None for curves 3 / 4) -> y [n,3]: the curve's fp32 forward out of photoloss_math.h (ops.tonemap's bits)."""
    x = _f32(x)
    n = x.shape[0]
    assert tuple(x.shape) == (n, 3)
    shift, stride = _pl_shift(shift, n, x.device)
    y = torch.empty_like(x)
    nz = lambda t: ptr(t) if t is not None and t.numel() else None
    _lib.call_photoloss("rb_pl_tonemap", nz(x), c_long(n), nz(shift), c_int(stride), c_int(int(curve)), c_int(int(inverse)), nz(y), stream_ptr())
    return y


def pl_tonemap_backward(x, shift, curve, inverse, gy, want_x=True, want_shift=True):
    """Reverse mode of a tone curve: x, gy [n,3], shift [1] | [n] -> (gx [n,3] or None, gshift like shift or None)."""
    x, gy = _f32(x), _f32(gy)
    n, dev = x.shape[0], x.device
    assert tuple(x.shape) == (n, 3) and tuple(gy.shape) == (n, 3)
    shift, stride = _pl_shift(shift, n, dev)
    gx = torch.empty_like(x) if want_x else None
    gshift = None
    if want_shift and shift is not None:
        gshift = torch.zeros(1, dtype=torch.float32, device=dev) if stride == 0 else torch.empty(n, dtype=torch.float32, device=dev)
    scratch = _pl_scratch(n, dev) if gshift is not None and stride == 0 else None
    nz = lambda t: ptr(t) if t is not None and t.numel() else None
    _lib.call_photoloss("rb_pl_tonemap_bwd", nz(x), c_long(n), nz(shift), c_int(stride), c_int(int(curve)), c_int(int(inverse)), nz(gy), nz(gx),
                        nz(gshift), nz(scratch), c_long(0 if scratch is None else scratch.numel()), stream_ptr())
    return gx, gshift


def pl_image_loss(sg_rgb, indir_rgb, gt, net_mask, obj_mask, shift, curve, l2=False, want_rgb=True, want_shift=True):
    """The fused image loss: sg_rgb, gt [N,3], indir_rgb [N,3] or None, the masks [N] bool / uint8, shift [1] | [N] | None ->
    (loss [] fp32, g_rgb [N,3] or None, g_shift like shift or None), the gradients for a unit upstream."""
    sg_rgb, gt = _f32(sg_rgb), _f32(gt)
    N, dev = sg_rgb.shape[0], sg_rgb.device
    assert tuple(sg_rgb.shape) == (N, 3) and tuple(gt.shape) == (N, 3)
    if indir_rgb is not None:
        indir_rgb = _f32(indir_rgb)
        assert tuple(indir_rgb.shape) == (N, 3)
    m1 = net_mask.reshape(-1).to(torch.uint8).contiguous()
    m2 = obj_mask.reshape(-1).to(torch.uint8).contiguous()
    assert m1.numel() == N and m2.numel() == N
    shift, stride = _pl_shift(shift, N, dev)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    g_rgb = torch.empty(N, 3, dtype=torch.float32, device=dev) if want_rgb else None
    g_shift = None
    if want_shift and shift is not None:
        g_shift = torch.zeros(1, dtype=torch.float32, device=dev) if stride == 0 else torch.empty(N, dtype=torch.float32, device=dev)
    scratch = _pl_scratch(N, dev)
    nz = lambda t: ptr(t) if t is not None and t.numel() else None
    _lib.call_photoloss("rb_pl_image_loss", nz(sg_rgb), nz(indir_rgb), nz(gt), nz(m1), nz(m2), c_long(N), nz(shift), c_int(stride),
                        c_int(int(curve)), c_int(1 if l2 else 0), ptr(loss), nz(g_rgb), nz(g_shift), ptr(scratch), c_long(scratch.numel()),
                        stream_ptr())
    return loss.reshape(()), g_rgb, g_shift


# ------------------------------------------------------------------------------------------------ camera-space rasteriser (librobir_hip_raster.so)
RS_TILE, RS_MAX_RESOLUTION, RS_MAX_CHANNELS = 8, 16384, 16


def _rs_mesh(screen, faces):
    screen = _f32(screen)
    if screen.dim() != 2 or screen.shape[1] != 4 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"rasteriser: screen must be [V,4] and faces [F,3], got {tuple(screen.shape)}, {tuple(faces.shape)}")
    assert faces.dtype == torch.int32 and faces.is_contiguous()
    return screen


def _rs_image(H, W):
    H, W = int(H), int(W)
    if not (1 <= H <= RS_MAX_RESOLUTION and 1 <= W <= RS_MAX_RESOLUTION):
        raise ValueError(f"rasteriser: image {H} x {W} outside 1 .. {RS_MAX_RESOLUTION} per side")
    return H, W


def rs_project(vertices, pose_inv, K):
    """vertices [V,3], pose_inv [4,4] (the inverse of the camera-to-world pose), K [3,3] -> screen [V,4] = (u, v, 1 / zc, zc)."""
    vertices, pose_inv, K = _f32(vertices), _f32(pose_inv), _f32(K)
    if vertices.dim() != 2 or vertices.shape[1] != 3 or tuple(pose_inv.shape) != (4, 4) or tuple(K.shape) != (3, 3):
        raise ValueError(f"rasteriser: vertices [V,3], pose_inv [4,4], K [3,3], got {tuple(vertices.shape)}, {tuple(pose_inv.shape)}, "
                         f"{tuple(K.shape)}")
    V = vertices.shape[0]
    screen = torch.empty(V, 4, dtype=torch.float32, device=vertices.device)
    if V:
        _lib.call_raster("rb_rs_project", ptr(vertices), c_long(V), ptr(pose_inv), ptr(K), ptr(screen), stream_ptr())
    return screen


def rs_bin_count(screen, faces, H, W, near, cull):
    """-> counts [F] int32: tiles of 8 x 8 pixels each face's pixel box touches (0: a skipped face)."""
    screen = _rs_mesh(screen, faces)
    H, W = _rs_image(H, W)
    nz = lambda t: ptr(t) if t.numel() else None
    counts = torch.empty(faces.shape[0], dtype=torch.int32, device=screen.device)
    _lib.call_raster("rb_rs_bin_count", nz(screen), c_long(screen.shape[0]), nz(faces), c_long(faces.shape[0]), c_int(H), c_int(W),
                     c_float(near), c_int(int(cull)), nz(counts), stream_ptr())
    return counts


def rs_bin_emit(screen, faces, H, W, near, cull, base, P):
    """base [F] int64 exclusive prefix of the counts, P their total -> (pair_tile [P], pair_face [P]) int32 in face order."""
    screen = _rs_mesh(screen, faces)
    H, W = _rs_image(H, W)
    assert base.dtype == torch.int64 and base.is_contiguous() and base.numel() == faces.shape[0]
    pair_tile = torch.empty(P, dtype=torch.int32, device=screen.device)
    pair_face = torch.empty(P, dtype=torch.int32, device=screen.device)
    nz = lambda t: ptr(t) if t.numel() else None
    _lib.call_raster("rb_rs_bin_emit", nz(screen), c_long(screen.shape[0]), nz(faces), c_long(faces.shape[0]), c_int(H), c_int(W),
                     c_float(near), c_int(int(cull)), nz(base), c_long(P), nz(pair_tile), nz(pair_face), stream_ptr())
    return pair_tile, pair_face


def rs_raster(screen, faces, H, W, near, cull, tile_start, pair_face):
    """-> (face_id [H,W] int32, bary [H,W,2], depth [H,W])."""
    screen = _rs_mesh(screen, faces)
    H, W = _rs_image(H, W)
    ntiles = ((W + RS_TILE - 1) // RS_TILE) * ((H + RS_TILE - 1) // RS_TILE)
    assert tile_start.dtype == torch.int32 and tile_start.numel() == ntiles + 1 and pair_face.dtype == torch.int32
    assert tile_start.is_contiguous() and pair_face.is_contiguous()
    dev = screen.device
    face_id = torch.empty(H, W, dtype=torch.int32, device=dev)
    bary = torch.empty(H, W, 2, dtype=torch.float32, device=dev)
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    nz = lambda t: ptr(t) if t.numel() else None
    _lib.call_raster("rb_rs_raster", nz(screen), c_long(screen.shape[0]), nz(faces), c_long(faces.shape[0]), c_int(H), c_int(W), c_float(near),
                     c_int(int(cull)), ptr(tile_start), nz(pair_face), c_long(pair_face.numel()), ptr(face_id), ptr(bary), ptr(depth),
                     stream_ptr())
    return face_id, bary, depth


def rs_gbuffer(face_id, bary, faces, vertices, uv, cam_loc, planes=None, filter=1, vnormals=None, index=None):
    """The G-buffer of the pixels of face_id / bary [H,W] (index None: all, rows [H W, .]) or of the flat pixel indices index [n] int64 ->
    (position [n,3], uv [n,2], view_dir [n,3], tex [n,C] or None, normal [n,3] or None).  faces [F,3] int32, vertices [V,3], uv [F,3,2],
    cam_loc [3], planes [R,R,C] or None, vnormals [V,3] or None."""
    assert face_id.dtype == torch.int32 and face_id.is_contiguous() and face_id.dim() == 2 and faces.dtype == torch.int32
    bary, vertices, uv, cam_loc, faces = _f32(bary), _f32(vertices), _f32(uv), _f32(cam_loc).reshape(-1), faces.contiguous()
    H, W = face_id.shape
    F, V, dev = faces.shape[0], vertices.shape[0], face_id.device
    if tuple(bary.shape) != (H, W, 2) or tuple(faces.shape) != (F, 3) or tuple(vertices.shape) != (V, 3) or tuple(uv.shape) != (F, 3, 2) \
            or cam_loc.numel() != 3:
        raise ValueError(f"gbuffer: bary [H,W,2], faces [F,3], vertices [V,3], uv [F,3,2], cam_loc [3], got {tuple(bary.shape)}, "
                         f"{tuple(faces.shape)}, {tuple(vertices.shape)}, {tuple(uv.shape)}, {tuple(cam_loc.shape)}")
    R = C = 0
    if planes is not None:
        planes = _f32(planes)
        if planes.dim() != 3 or planes.shape[0] != planes.shape[1] or not 1 <= planes.shape[2] <= RS_MAX_CHANNELS:
            raise ValueError(f"gbuffer: planes must be [R,R,C] with C <= {RS_MAX_CHANNELS}, got {tuple(planes.shape)}")
        R, C = planes.shape[0], planes.shape[2]
    if vnormals is not None:
        vnormals = _f32(vnormals)
        if tuple(vnormals.shape) != (V, 3):
            raise ValueError(f"gbuffer: vnormals must be [V,3] = {(V, 3)}, got {tuple(vnormals.shape)}")
    if index is None:
        n = H * W
    else:
        assert index.dtype == torch.int64 and index.is_contiguous()
        n = index.numel()
    new = lambda c: torch.empty(n, c, dtype=torch.float32, device=dev)
    position, uv_out, view_dir = new(3), new(2), new(3)
    tex = new(C) if planes is not None else None
    normal = new(3) if vnormals is not None else None
    nz = lambda t: ptr(t) if t is not None and t.numel() else None
    if n:
        _lib.call_raster("rb_rs_gbuffer", ptr(face_id), ptr(bary), c_int(H), c_int(W), None if index is None else ptr(index), c_long(n),
                         nz(faces), c_long(F), nz(vertices), c_long(V), nz(uv), nz(vnormals), ptr(cam_loc), nz(planes), c_int(R), c_int(C),
                         c_int(int(filter)), ptr(position), ptr(uv_out), ptr(view_dir), nz(tex), nz(normal), stream_ptr())
    return position, uv_out, view_dir, tex, normal


# ------------------------------------------------------------------------------------------------ atlas fit (librobir_hip_texfit.so)
TF_MAX_RESOLUTION, TF_MAX_CHANNELS, TF_MAX_ROWS = 16384, 16, 2 ** 29 - 1


def _tf_atlas(planes, C=None):
    """planes [R,R,Cs] -> (R, Cs, C): the resolution, the stack's channels and the leading channels a call works on."""
    if planes.dim() != 3 or planes.shape[0] != planes.shape[1] or not 1 <= planes.shape[2] <= TF_MAX_CHANNELS:
        raise ValueError(f"atlas fit: planes must be [R,R,Cs] with Cs <= {TF_MAX_CHANNELS}, got {tuple(planes.shape)}")
    R, Cs = planes.shape[0], planes.shape[2]
    C = Cs if C is None else int(C)
    if not 1 <= R <= TF_MAX_RESOLUTION or not 1 <= C <= Cs:
        raise ValueError(f"atlas fit: R = {R} outside 1 .. {TF_MAX_RESOLUTION} or C = {C} outside 1 .. Cs = {Cs}")
    assert planes.dtype == torch.float32 and planes.is_contiguous()
    return R, Cs, C


def tf_taps(uv, R, filter=1):
    """uv [n,2] -> (tap_texel [n,4] int32, tap_weight [n,4]): the four taps nw, ne, sw, se of the mesh view's plane fetch at uv on an R x R
    atlas; texel -1 and weight +0 for a tap outside the image.  filter 0: one tap of weight 1 at the containing texel."""
    uv = _f32(uv)
    n = uv.shape[0]
    if uv.dim() != 2 or uv.shape[1] != 2 or n > TF_MAX_ROWS or not 1 <= int(R) <= TF_MAX_RESOLUTION:
        raise ValueError(f"atlas fit: uv must be [n,2] with n < 2^29 and 1 <= R <= {TF_MAX_RESOLUTION}, got {tuple(uv.shape)}, R = {R}")
    texel = torch.empty(n, 4, dtype=torch.int32, device=uv.device)
    weight = torch.empty(n, 4, dtype=torch.float32, device=uv.device)
    if n:
        _lib.call_texfit("rb_tf_taps", ptr(uv), c_long(n), c_int(int(R)), c_int(int(filter)), ptr(texel), ptr(weight), stream_ptr())
    return texel, weight


def tf_fetch(planes, tap_texel, tap_weight, C=None):
    """planes [R,R,Cs], the taps of tf_taps -> tex [n,C]: ((a w0 + b w1) + c w2) + d w3 over the first C channels."""
    R, Cs, C = _tf_atlas(planes, C)
    n = tap_texel.shape[0]
    assert tap_texel.dtype == torch.int32 and tap_texel.is_contiguous() and tuple(tap_texel.shape) == (n, 4)
    assert tap_weight.dtype == torch.float32 and tap_weight.is_contiguous() and tuple(tap_weight.shape) == (n, 4)
    tex = torch.empty(n, C, dtype=torch.float32, device=planes.device)
    if n:
        _lib.call_texfit("rb_tf_fetch", ptr(planes), c_int(R), c_int(Cs), ptr(tap_texel), ptr(tap_weight), c_long(n), c_int(C), ptr(tex),
                         stream_ptr())
    return tex


def tf_scatter(pair_row, pair_weight, seg_start, g_tex):
    """The transpose of tf_fetch as a gather: pair_row [P] int32, pair_weight [P] (the pairs sorted by texel, stable), seg_start [T+1] int32,
    g_tex [n,C] -> grad [T,C], the fp64 sum over each segment's pairs in ascending order, rounded once."""
    g_tex = _f32(g_tex)
    n, C = g_tex.shape
    P, T = pair_row.numel(), seg_start.numel() - 1
    assert pair_row.dtype == torch.int32 and pair_row.is_contiguous() and seg_start.dtype == torch.int32 and seg_start.is_contiguous()
    assert pair_weight.dtype == torch.float32 and pair_weight.is_contiguous() and pair_weight.numel() == P and T >= 0
    if not 1 <= C <= TF_MAX_CHANNELS:
        raise ValueError(f"atlas fit: g_tex must be [n,C] with C <= {TF_MAX_CHANNELS}, got {tuple(g_tex.shape)}")
    grad = torch.empty(T, C, dtype=torch.float32, device=g_tex.device)
    if T and P:
        _lib.call_texfit("rb_tf_scatter", ptr(pair_row), ptr(pair_weight), c_long(P), ptr(seg_start), c_long(T), ptr(g_tex), c_long(n),
                         c_int(C), ptr(grad), stream_ptr())
    return grad


def tf_adam(planes, adam_m, adam_v, seg_texel, grad, lr, lo, hi, beta1, beta2, eps, step):
    """One lazy Adam step, in place, on the texels seg_texel [T] int32 (no texel twice) of the first C channels of planes [R,R,Cs]: adam_m,
    adam_v [R,R,C], grad [T,C]; lr, lo, hi: C floats each (step size and clamp per channel); step: the step number t >= 1, whose bias
    corrections 1 - beta^t are formed here in double."""
    T, C = grad.shape
    R, Cs, C = _tf_atlas(planes, C)
    assert tuple(adam_m.shape) == (R, R, C) and tuple(adam_v.shape) == (R, R, C) and adam_m.is_contiguous() and adam_v.is_contiguous()
    assert adam_m.dtype == torch.float32 and adam_v.dtype == torch.float32 and grad.dtype == torch.float32 and grad.is_contiguous()
    assert seg_texel.dtype == torch.int32 and seg_texel.is_contiguous() and seg_texel.numel() == T and int(step) >= 1
    arr = lambda a: (ctypes.c_double * C)(*[float(x) for x in a])
    if not (len(lr) == len(lo) == len(hi) == C):
        raise ValueError(f"atlas fit: lr, lo, hi need {C} values each")
    if T:
        _lib.call_texfit("rb_tf_adam", ptr(planes), ptr(adam_m), ptr(adam_v), ptr(seg_texel), ptr(grad), c_long(T), c_int(R), c_int(Cs),
                         c_int(C), arr(lr), arr(lo), arr(hi), ctypes.c_double(beta1), ctypes.c_double(beta2), ctypes.c_double(eps),
                         ctypes.c_double(1.0 - float(beta1) ** int(step)), ctypes.c_double(1.0 - float(beta2) ** int(step)), stream_ptr())
