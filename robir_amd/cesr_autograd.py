"""Differentiable CESR networks: one torch.autograd.Function per head around SDFNetwork's forward kernels (kinds `shadow` and `normal`) and
rb_ct_cesr_bwd.

  * RawFn:  the raw output [M,2] / [M,3] (SDFNetwork.forward, _cesr, _cesr_points, eval_point_labels).
  * VisFn:  ops.softmax2(raw, 1), shadow_net's diffuse_vis [n * n_label] (SDFNetwork.diffuse_vis).
  * UnitFn: ops.normalize3(raw, 1e-4, 1), normal_net's unit normal [n,3] (SDFNetwork.unit_normal).

Each is differentiable in the 27 weight-norm tensors of ONE network.  The forward is the forward-only route that dispatch.cesr picks under
the current precision policy, followed by the head's own kernel -- the unmarked path's bits.  The backward is ONE call into the CESR-training
library on the caller's stream; the library recomputes the encoding, the folded weights, every activation and the head in fp64 from the fp32
inputs and parameters.  What the backward reads of the input: the points [n,3] where the forward took points; the caller's rows where it
took dense rows (kind codes 0 and 1 of ops.cesr_net); and for the (point features, label) form (code 2 on rows [n,64]) the first three
feature columns, which ARE the points (rb_feat_pe10's layout) -- the one-hot block is never read from memory.

The points / rows are constants: one that requires grad raises NotImplementedError instead of receiving a silent zero.
ctx.needs_input_grad turns into NULL pointers.  LinDiffCombineFn carries the graph through the hook's albedo recombination."""
import math

import torch

from . import ops, param_autograd

SLAB_ROWS = ops.CESR_SLAB_ROWS      # rows per slab of the backward (bounds its scratch independently of M); tests use small values
PART_ROWS = ops.CESR_PART_ROWS      # rows per partition of a weight gradient's row range inside a slab
HEADS = (lambda raw: raw, lambda raw: ops.softmax2(raw, 1), lambda raw: ops.normalize3(raw, 1e-4, 1))


def cesr_params(net):
    """The 27 parameter tensors of an SDFNetwork in ops.CESR_PARAM_NAMES order."""
    return [getattr(getattr(net, "lin%d" % l), w) for l in range(9) for w in ("weight_g", "weight_v", "bias")]


def _make(name, head, doc):
    class Fn(torch.autograd.Function):
        """Saves the backward's input (points or rows) and the parameters (param_autograd: what is saved, and why that way)."""

        @staticmethod
        def forward(ctx, net, x, M, code, n_label, points, *params):
            # autograd runs this with grad mode off: the ordinary kernels run
            out = HEADS[head](net._cesr_eval(x, M, code, n_label, points))
            ctx.save_for_backward(x[:, :3].contiguous() if code == 2 and not points else x, *params)
            ctx.cfg = (M, net.kind, n_label if code == 2 else 1, int(getattr(net, "_train_slab_rows", 0) or SLAB_ROWS),
                       int(getattr(net, "_train_part_rows", 0) or 0))
            ctx.set_materialize_grads(False)
            return out

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, g):
            x, *params = ctx.saved_tensors
            M, kind, n_label, slab, part = ctx.cfg
            want = tuple(k for k, need in zip(ops.CESR_PARAM_NAMES, ctx.needs_input_grad[6:]) if need)
            if g is None or not want:
                return (None,) * (6 + len(params))
            grads, _ = ops.cesr_backward(x, M, kind, params, g.float().contiguous(), head=head, n_label=n_label, want=want, slab_rows=slab,
                                         part_rows=part or min(slab, PART_ROWS))
            return param_autograd.backward_result(6, ops.CESR_PARAM_NAMES, params, grads)

    Fn.__name__ = Fn.__qualname__ = name
    Fn.__doc__ = doc + "  " + Fn.__doc__
    return Fn


RawFn = _make("RawFn", 0, "The raw output of shadow_net / normal_net.")
VisFn = _make("VisFn", 1, "shadow_net's class-1 probability, ops.softmax2(raw, 1).")
UnitFn = _make("UnitFn", 2, "normal_net's unit normal, ops.normalize3(raw, 1e-4, 1).")
_FNS = (RawFn, VisFn, UnitFn)


def apply(net, x, M, code, n_label, points, head):
    """SDFNetwork._cesr / _cesr_points of a marked, trainable network: ops.cesr_net's arguments (code 0 normal, 1 shadow dense rows, 2 shadow
    on (point, label) pairs), points: x holds points [n,3], else rows; head 0 raw, 1 softmax2(., 1), 2 normalize3(., 1e-4, 1)."""
    param_autograd.refuse_input_grad("CESR network", **{"points" if points else "rows": x})
    if (head == 1 and net.kind != "shadow") or (head == 2 and net.kind != "normal"):
        raise ValueError(f"head {head} does not belong to the {net.kind} network (1: shadow_net's softmax, 2: normal_net's unit vector)")
    return _FNS[head].apply(net, x.detach().float().contiguous(), int(M), int(code), int(n_label), bool(points), *cesr_params(net))


class LinDiffCombineFn(torch.autograd.Function):
    """rgb = diffuse * albedo / pi + specular (training/train_cesr.py:523-524): ops.lin_diff_combine's bits forward, the three element-wise
    products backward (plumbing)."""

    @staticmethod
    def forward(ctx, diffuse, albedo, spec):
        ctx.save_for_backward(diffuse, albedo)
        return ops.lin_diff_combine(diffuse, albedo, spec)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        diffuse, albedo = ctx.saved_tensors
        need = ctx.needs_input_grad
        return (g * albedo / math.pi if need[0] else None, g * diffuse / math.pi if need[1] else None, g if need[2] else None)


def lin_diff_combine(diffuse, albedo, spec):
    """ops.lin_diff_combine, with a graph when grad mode is on and an input requires grad."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (diffuse, albedo, spec)):
        return LinDiffCombineFn.apply(diffuse.float().contiguous(), albedo.float().contiguous(), spec.float().contiguous())
    return ops.lin_diff_combine(diffuse, albedo, spec)
