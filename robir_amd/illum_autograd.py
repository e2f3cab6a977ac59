"""Differentiable indirect-illumination network: three torch.autograd.Functions around IndirctIllumNetwork's forward kernels, rb_it_lobe_bwd,
rb_train_ae_bwd and the fused SG query.

  * LobeFn: differentiable in the ten nn.Linear tensors of lobe_layer.  The forward is the policy's own lobe kernel plus ops.illum_decode --
    lgt_sgs is the forward-only path's, bit for bit.  The backward is ONE call into the illumination-training library, which recomputes the
    encoding, every activation and the head in fp64 from the fp32 coordinates and parameters.
  * IntegralFn: differentiable in the sixteen nn.Linear tensors of integral_layer, an input-perturbed SparseAE of which only the perturbed
    pass is used (implicit_differentiable_renderer.py:220): ONE clean pass on the perturbed feature rows, which rb_train_ae_bwd
    differentiates as it stands (no latent noise, softplus latent, no output activation).  The backward rebuilds the fp32 rows the forward
    saw with the same two kernels and multiplies the upstream gradient by the sign of the saved pre-abs output.
  * SGQueryFn: query_indir_illum, differentiable in the lobes.

The points, the hdr shift, the noise and the sample directions are constants: a tensor that requires grad there raises NotImplementedError
instead of receiving a silent zero.  ctx.needs_input_grad turns into NULL pointers."""
import torch

from . import ae_autograd, ops, param_autograd

SLAB_ROWS = ops.ILLUM_SLAB_ROWS      # rows per slab of the lobe net's backward (bounds its scratch independently of n); tests use small values
PART_ROWS = ops.ILLUM_PART_ROWS      # rows per partition of a weight gradient's row range inside a slab


def lobe_params(net):
    """The ten parameter tensors of lobe_layer in ops.ILLUM_PARAM_NAMES order."""
    return [t for i in range(5) for t in (net.lobe_layer[2 * i].weight, net.lobe_layer[2 * i].bias)]


def _opt(saved, present):
    return saved.pop(0) if present else None


class LobeFn(torch.autograd.Function):
    """Saves the points, the hdr shift and the parameters (param_autograd: what is saved, and why that way)."""

    @staticmethod
    def forward(ctx, net, points, hdr, *params):
        # autograd runs this with grad mode off: the ordinary kernels run
        sgs = net._lobes(points, hdr)
        ctx.has_hdr = hdr is not None
        ctx.save_for_backward(points, *([hdr] if hdr is not None else []), *params)
        ctx.cfg = (int(getattr(net, "_train_slab_rows", 0) or SLAB_ROWS), int(getattr(net, "_train_part_rows", 0) or 0))
        ctx.set_materialize_grads(False)
        return sgs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sgs):
        saved = list(ctx.saved_tensors)
        points = saved.pop(0)
        hdr = _opt(saved, ctx.has_hdr)
        params = saved
        slab, part = ctx.cfg
        want = tuple(k for k, need in zip(ops.ILLUM_PARAM_NAMES, ctx.needs_input_grad[3:]) if need)
        if g_sgs is None or not want:
            return (None,) * (3 + len(params))
        grads, _ = ops.illum_lobe_backward(points, hdr, params, g_sgs.float().contiguous(), want=want, slab_rows=slab,
                                           part_rows=part or min(slab, PART_ROWS))
        return param_autograd.backward_result(3, ops.ILLUM_PARAM_NAMES, params, grads)


class IntegralFn(torch.autograd.Function):
    """Saves the points, the hdr shift, the noise, `var`, the decoder's pre-abs output [n,3] and the parameters."""

    @staticmethod
    def forward(ctx, net, points, hdr, noise, *params):
        ae = net.integral_layer
        pre = ae.run_pass(ops.axpy(ops.feat_pe10(points, extra=hdr), noise, 0.02))
        var = ae._var(points.device)
        ctx.present = (hdr is not None, var is not None)
        ctx.save_for_backward(points, noise, pre, *([hdr] if hdr is not None else []), *([var] if var is not None else []), *params)
        ctx.cfg = (ae._latent_act_code(), ae._sigmoid_out(), ae.in_dim, ae.out_dim, int(getattr(ae, "_train_slab_rows", 0) or ae_autograd.SLAB_ROWS))
        ctx.set_materialize_grads(False)
        return ops.abs_scale(pre, 1.0)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_int):
        saved = list(ctx.saved_tensors)
        points, noise, pre = saved.pop(0), saved.pop(0), saved.pop(0)
        hdr = _opt(saved, ctx.present[0])
        var = _opt(saved, ctx.present[1])
        params = saved
        act, sig_out, in_dim, out_dim, slab = ctx.cfg
        want = tuple(k for k, need in zip(ops.AE_PARAM_NAMES, ctx.needs_input_grad[4:]) if need)
        if g_int is None or not want:
            return (None,) * (4 + len(params))
        Xn = ops.axpy(ops.feat_pe10(points, extra=hdr), noise, 0.02)           # the fp32 rows the forward saw
        grads, _ = ops.ae_backward(Xn, params, g_out=(g_int.float() * torch.sign(pre)).contiguous(), noise=None, var=var, latent_act=act,
                                   sigmoid_out=sig_out, in_dim=in_dim, out_dim=out_dim, want=want, slab_rows=slab)
        return param_autograd.backward_result(4, ops.AE_PARAM_NAMES, params, grads)


class SGQueryFn(torch.autograd.Function):
    """Saves the lobes and the directions."""

    @staticmethod
    def forward(ctx, sgs, dirs):
        sgs, dirs = sgs.detach().float().contiguous(), dirs.detach().float().contiguous()
        ctx.save_for_backward(sgs, dirs)
        ctx.set_materialize_grads(False)
        return ops.sg_query(sgs, dirs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        sgs, dirs = ctx.saved_tensors
        if g is None or not ctx.needs_input_grad[0]:
            return None, None
        return ops.sg_query_backward(sgs, dirs, g.float().contiguous()), None


def sg_query(sgs, dirs):
    """query_indir_illum with a graph to the lobes: sgs [n,L,7], dirs [n,S,3] -> radiance [n,S,3]."""
    param_autograd.refuse_input_grad("SG query", sample_dirs=dirs)
    return SGQueryFn.apply(sgs, dirs)


def forward(net, points, hdr_shift, noise):
    """IndirctIllumNetwork.forward with a graph to the network's parameters, on the caller's stream: points [n,3], hdr_shift [n,1], noise
    [n,64] (already padded) -> (lgt_sgs [n,24,7], env_int [n,3]).  A Function runs only if its sub-network has a parameter that requires
    grad; the other half is today's forward."""
    param_autograd.refuse_input_grad("indirect-illumination network", points=points, hdr_shift=hdr_shift, noise=noise)
    points = points.detach().float().contiguous()
    hdr = hdr_shift.detach().float().contiguous() if net.use_hdr else None
    noise = noise.detach().float().contiguous()
    if any(p.requires_grad for p in net.lobe_layer.parameters()):
        sgs = LobeFn.apply(net, points, hdr, *lobe_params(net))
    else:
        with torch.no_grad():
            sgs = net._lobes(points, hdr)
    if any(p.requires_grad for p in net.integral_layer.parameters()):
        integ = IntegralFn.apply(net, points, hdr, noise, *ae_autograd.linear_params(net.integral_layer))
    else:
        with torch.no_grad():
            integ = net._integral(ops.feat_pe10(points, extra=hdr), noise)
    return sgs, integ
