"""Test-side truth for the visibility network's backward: torch autograd of the oracle's formulas (robir_oracle.nets.vis_logits) on the CPU, in
float64 (the truth) or float32 (the yardstick: what PyTorch's own fp32 autograd achieves on the same inputs).  The encoding is evaluated in the
evaluation's dtype from the fp32 coordinates.  Shared by tests/test_vis_train_gpu.py, tools/gen_vis_grad_golden.py and
tools/prof_vis_backward.py."""
import torch

from robir_oracle import nets as on

NAMES = tuple(f"vis_layer.{2 * i}.{w}" for i in range(5) for w in ("weight", "bias"))
PREFIX = "visibility_network."


def vis_params(sd, prefix=PREFIX):
    """The ten tensors of the visibility network out of a state dict, keyed by NAMES."""
    return {k: torch.as_tensor(sd[prefix + k]) for k in NAMES}


def vis_forward(params, points, dirs, rep=1):
    """-> logits [M,2] in the dtype of `params`; points [M/rep,3] and dirs [M,3] are the fp32 coordinates."""
    dtype = next(iter(params.values())).dtype
    sd = {PREFIX + k: v for k, v in params.items()}
    p = points.detach().float().to(dtype).repeat_interleave(int(rep), 0)
    return on.vis_logits(sd, p, dirs.detach().float().to(dtype))


def leaves(params, dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}


def vis_grads(params, points, dirs, g_logits, rep=1, dtype=torch.float64):
    """Gradients of <g_logits, logits> for all ten tensors."""
    with torch.enable_grad():
        lv = leaves(params, dtype)
        loss = (torch.as_tensor(g_logits).to(dtype) * vis_forward(lv, points, dirs, rep)).sum()
        gr = torch.autograd.grad(loss, list(lv.values()))
    return dict(zip(lv, gr))


def loss_grads(params, points, dirs, loss_fn, rep=1, dtype=torch.float64):
    """(loss value, gradients) of loss_fn(logits) for all ten tensors."""
    with torch.enable_grad():
        lv = leaves(params, dtype)
        loss = loss_fn(vis_forward(lv, points, dirs, rep))
        gr = torch.autograd.grad(loss, list(lv.values()))
    return float(loss.detach()), dict(zip(lv, gr))
