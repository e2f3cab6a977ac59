"""Differentiable visibility network: a torch.autograd.Function around VisNetwork's forward kernel and rb_vt_vis_bwd.

Differentiable inputs: the ten nn.Linear tensors of ONE VisNetwork.  The points and the directions are constants: a tensor that requires grad
there raises NotImplementedError instead of receiving a silent zero.  The forward runs the module's own forward kernel under the current
precision policy (VisNetwork.logits_from_points) -- its logits are the forward-only path's, bit for bit.  The backward is ONE call into the
visibility-training library, which recomputes the encoding and every activation in fp64 from the fp32 coordinates and parameters;
ctx.needs_input_grad turns into NULL pointers."""
import torch

from . import ops

SLAB_ROWS = ops.VIS_SLAB_ROWS      # rows per slab of the backward (bounds its scratch independently of M); tests use small values
PART_ROWS = ops.VIS_PART_ROWS      # rows per partition of a weight gradient's row range inside a slab


def refuse_input_grad(**tensors):
    """points / directions are not differentiable on this path: say so instead of returning a zero gradient."""
    if not torch.is_grad_enabled():
        return
    for name, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise NotImplementedError(f"robir_amd visibility network has no gradient with respect to `{name}` (its HIP backward differentiates the "
                                      f"network parameters only: pass {name}.detach(), or differentiate the input on the reference's modules)")


def linear_params(net):
    """The ten parameter tensors in ops.VIS_PARAM_NAMES order."""
    return [t for i in range(5) for t in (net.vis_layer[2 * i].weight, net.vis_layer[2 * i].bias)]


class VisLogitsFn(torch.autograd.Function):
    """Saved through ctx.save_for_backward, and nothing else: the points, the directions and the parameters -- no activation, no output.
    Tensors never sit on ctx as plain attributes (output -> grad_fn -> ctx -> output would be a reference cycle that only the cyclic
    collector frees; autograd checks saved inputs for in-place changes -- an optimiser step between forward and backward is an error, not
    a silently stale gradient).  ctx keeps the module-independent scalars."""

    @staticmethod
    def forward(ctx, net, points, dirs, rep, *params):
        # autograd runs this with grad mode off: the module takes today's forward-only path and the ordinary kernel runs
        points, dirs = points.detach().float().contiguous(), dirs.detach().float().contiguous()
        logits = net.logits_from_points(points, dirs, rep)
        ctx.save_for_backward(points, dirs, *params)
        ctx.cfg = (int(rep), int(getattr(net, "_train_slab_rows", 0) or SLAB_ROWS), int(getattr(net, "_train_part_rows", 0) or 0))
        ctx.set_materialize_grads(False)
        return logits

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_logits):
        points, dirs, *params = ctx.saved_tensors
        rep, slab, part = ctx.cfg
        want = tuple(k for k, need in zip(ops.VIS_PARAM_NAMES, ctx.needs_input_grad[4:]) if need)
        if g_logits is None or not want:
            return (None,) * (4 + len(params))
        grads, _ = ops.vis_backward(points, dirs, rep, params, g_logits.float().contiguous(), want=want, slab_rows=slab,
                                    part_rows=part or min(slab, PART_ROWS))
        return (None, None, None, None, *(grads[k].to(p.dtype) if k in grads else None for k, p in zip(ops.VIS_PARAM_NAMES, params)))


def logits(net, points, dirs, rep=1):
    """VisNetwork.logits_from_points with a graph to the network's parameters: points [M/rep,3], dirs [M,3] -> logits [M,2]."""
    refuse_input_grad(points=points, dirs=dirs)
    return VisLogitsFn.apply(net, points, dirs, int(rep), *linear_params(net))
