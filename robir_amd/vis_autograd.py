"""Differentiable visibility network: a torch.autograd.Function around VisNetwork's forward kernel and rb_vt_vis_bwd.

Differentiable inputs: the ten nn.Linear tensors of ONE VisNetwork.  The points and the directions are constants: a tensor that requires grad
there raises NotImplementedError instead of receiving a silent zero.  The forward runs the module's own forward kernel under the current
precision policy (VisNetwork.logits_from_points) -- its logits are the forward-only path's, bit for bit.  The backward is ONE call into the
visibility-training library, which recomputes the encoding and every activation in fp64 from the fp32 coordinates and parameters;
ctx.needs_input_grad turns into NULL pointers."""
import torch

from . import ops, param_autograd

SLAB_ROWS = ops.VIS_SLAB_ROWS      # rows per slab of the backward (bounds its scratch independently of M); tests use small values
PART_ROWS = ops.VIS_PART_ROWS      # rows per partition of a weight gradient's row range inside a slab


def linear_params(net):
    """The ten parameter tensors in ops.VIS_PARAM_NAMES order."""
    return [t for i in range(5) for t in (net.vis_layer[2 * i].weight, net.vis_layer[2 * i].bias)]


class VisLogitsFn(torch.autograd.Function):
    """Saves the points, the directions and the parameters (param_autograd: what is saved, and why that way)."""

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
        return param_autograd.backward_result(4, ops.VIS_PARAM_NAMES, params, grads)


def logits(net, points, dirs, rep=1):
    """VisNetwork.logits_from_points with a graph to the network's parameters: points [M/rep,3], dirs [M,3] -> logits [M,2]."""
    param_autograd.refuse_input_grad("visibility network", points=points, dirs=dirs)
    return VisLogitsFn.apply(net, points, dirs, int(rep), *linear_params(net))
