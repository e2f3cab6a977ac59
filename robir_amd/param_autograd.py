"""What the parameter-only autograd Functions (ae_autograd.SparseAEFn, vis_autograd.VisLogitsFn) share.

Such a Function differentiates the nn.Linear tensors of ONE network through a HIP backward; every other input is a constant.  It saves through
ctx.save_for_backward, and nothing else: its inputs and the parameters -- no activation, no output.  Tensors never sit on ctx as plain
attributes (output -> grad_fn -> ctx -> output would be a reference cycle that only the cyclic collector frees; autograd checks saved inputs
for in-place changes -- an optimiser step between forward and backward is an error, not a silently stale gradient).  ctx keeps the
module-independent scalars."""
import torch


def refuse_input_grad(network, **tensors):
    """The inputs of `network` are not differentiable on this path: say so instead of returning a zero gradient."""
    if not torch.is_grad_enabled():
        return
    for name, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise NotImplementedError(f"robir_amd {network} has no gradient with respect to `{name}` (its HIP backward differentiates the "
                                      f"network parameters only: pass {name}.detach(), or differentiate the input on the reference's modules)")


def backward_result(n_other, names, params, grads):
    """What backward() returns: None for the n_other leading non-parameter inputs, then for each parameter (names / params in forward()'s
    order) its gradient from the name -> gradient dict in the parameter's dtype, or None where the dict has none."""
    return (*(None,) * n_other, *(grads[k].to(p.dtype) if k in grads else None for k, p in zip(names, params)))
