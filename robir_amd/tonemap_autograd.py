"""Differentiable tone mapping and the fused photometric loss: two torch.autograd.Functions around rb_tonemap, rb_pl_tonemap_bwd and
rb_pl_image_loss (librobir_hip_photoloss.so).

  * TonemapFn: ACESToneMapping.hdr2ldr / ldr2hdr with a graph to x and to the shift.  The forward is ops.tonemap -- the forward-only path's
    bits; the backward is ONE call that forms both partial derivatives in fp64 from the saved fp32 x and shift.  rb_tonemap's op 2
    (ldr2hdr(x^2.2), trace_radiance under no_grad) has no backward: asking for one raises.
  * ImageLossFn: model/loss.py:97-110 in one pass -- hdr2ldr(sg_rgb + indir_rgb), the masked L1 / L2 sum over N and, from the same launch,
    the gradients for a unit upstream, which backward() multiplies by the upstream scalar.

Both are once_differentiable: a gradient of the gradient raises.  The masks and the target are constants.  ctx.needs_input_grad turns into
NULL pointers."""
import torch

from . import ops


def wants_grad(*tensors):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


class TonemapFn(torch.autograd.Function):
    """x [n,3], shift [1] | [n].  Saves both."""

    @staticmethod
    def forward(ctx, x, shift, curve, inverse):
        x, shift = x.detach().float().contiguous(), shift.detach().float().reshape(-1).contiguous()
        ctx.save_for_backward(x, shift)
        ctx.cfg = (int(curve), int(inverse))
        ctx.set_materialize_grads(False)
        return ops.tonemap(x, shift, inverse + 16 * curve)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, shift = ctx.saved_tensors
        need_x, need_s = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if gy is None or not (need_x or need_s):
            return None, None, None, None
        curve, inverse = ctx.cfg
        gx, gs = ops.pl_tonemap_backward(x, shift, curve, inverse, gy.float().contiguous(), want_x=need_x, want_shift=need_s)
        return gx, gs, None, None


def tonemap(x, shift, curve, mode):
    """x [n,3] fp32, shift [1] | [n] (a tensor: a Python number is the caller's to wrap), curve 0 .. 3, mode 0 (hdr2ldr) | 1 (ldr2hdr) ->
    y [n,3] with a graph to whichever of x / shift requires grad."""
    if mode not in (0, 1):
        raise NotImplementedError(f"tonemap_autograd: mode {mode} (ldr2hdr(x^2.2), IDRNetwork.trace_radiance's under no_grad) has no backward "
                                  "-- only hdr2ldr (0) and ldr2hdr (1) are differentiable")
    return TonemapFn.apply(x, shift, curve, mode)


class ImageLossFn(torch.autograd.Function):
    """Saves the unit-upstream gradients the forward's launch wrote -- nothing of the inputs."""

    @staticmethod
    def forward(ctx, sg_rgb, indir_rgb, shift, gt, net_mask, obj_mask, curve, l2):
        need_rgb = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        need_s = shift is not None and ctx.needs_input_grad[2]
        det = lambda t: None if t is None else t.detach().float().contiguous()
        loss, g_rgb, g_shift = ops.pl_image_loss(det(sg_rgb), det(indir_rgb), det(gt), net_mask, obj_mask, det(shift), curve, l2,
                                                 want_rgb=need_rgb, want_shift=need_s)
        ctx.has = (g_rgb is not None, g_shift is not None)
        ctx.shapes = (sg_rgb.shape, None if indir_rgb is None else indir_rgb.shape, None if shift is None else shift.shape)
        ctx.save_for_backward(*[t for t in (g_rgb, g_shift) if t is not None])
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        saved = list(ctx.saved_tensors)
        g_rgb = saved.pop(0) if ctx.has[0] else None
        g_shift = saved.pop(0) if ctx.has[1] else None
        if g is None:
            return (None,) * 8
        s_sg, s_in, s_sh = ctx.shapes
        scaled = g * g_rgb if g_rgb is not None else None
        d_sg = scaled.reshape(s_sg) if ctx.needs_input_grad[0] else None
        d_in = scaled.reshape(s_in) if ctx.needs_input_grad[1] and s_in is not None else None
        d_sh = (g * g_shift).reshape(s_sh) if g_shift is not None and ctx.needs_input_grad[2] else None
        return d_sg, d_in, d_sh, None, None, None, None, None


def image_loss(sg_rgb, indir_rgb, gt, net_mask, obj_mask, shift, curve, l2=False):
    """sum_{m} sum_c dist(curve(sg_rgb + indir_rgb, shift), gt) / N as a 0-dim tensor with a graph to sg_rgb, indir_rgb and shift.
    sg_rgb, gt [N,3]; indir_rgb [N,3] | None; the masks [N]; shift [1] | [N] | None (curves 3 and 4)."""
    return ImageLossFn.apply(sg_rgb.reshape(-1, 3), None if indir_rgb is None else indir_rgb.reshape(-1, 3), shift, gt.reshape(-1, 3),
                             net_mask, obj_mask, int(curve), bool(l2))
