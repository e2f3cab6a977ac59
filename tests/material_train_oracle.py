"""Test-side truth for the spec auto-encoder's backward: torch autograd of the oracle's formulas (robir_oracle.nets.sparse_ae) on the CPU,
in float64 (the truth) or float32 (the yardstick: what PyTorch's own fp32 autograd achieves on the same inputs).  Shared by
tests/test_material_train_gpu.py, tools/gen_material_grad_golden.py and tools/prof_material_backward.py."""
import torch
import torch.nn.functional as F

from robir_oracle import nets as on

NAMES = tuple(f"brdf_encoder_layer.{2 * i}.{w}" for i in range(5) for w in ("weight", "bias")) \
    + tuple(f"brdf_decoder_layer.{2 * i}.{w}" for i in range(3) for w in ("weight", "bias"))
SPEC = on.MAT + "spec_brdf_encoder_layer"
ACTS = {0: torch.sigmoid, 1: F.softplus}


def ae_params(sd, prefix=SPEC):
    """The sixteen tensors of one auto-encoder out of a state dict, keyed by NAMES."""
    return {k: torch.as_tensor(sd[prefix + "." + k]) for k in NAMES}


def ae_forward(params, X, noise, var=None, latent_act=0, sigmoid_out=True, in_dim=63):
    """-> (out, out_xi, raw_latent) in the dtype of `params`; X [n,64] feature rows, of which the first in_dim are the network's input."""
    dtype = next(iter(params.values())).dtype
    sd = {"ae." + k: v for k, v in params.items()}
    x = X[:, :in_dim].to(dtype)
    v = None if var is None else var.to(dtype)
    nz = torch.zeros(x.shape[0], 32, dtype=dtype) if noise is None else noise.to(dtype)
    out, out_xi = on.sparse_ae(sd, "ae", x, nz, True, ACTS[latent_act], torch.sigmoid if sigmoid_out else None, var=v)
    raw = on._seq(sd, "ae.brdf_encoder_layer.", 5, x, lambda t: F.leaky_relu(t, 0.2))
    raw = raw * (1.0 - (v if v is not None else torch.zeros(32, dtype=dtype)))
    return out, out_xi, raw


def ae_grads(params, X, noise, g_out=None, g_out_xi=None, g_raw=None, dtype=torch.float64, **kw):
    """Gradients of <g_out, out> + <g_out_xi, out_xi> + <g_raw, raw_latent> for all sixteen tensors (zeros where the loss does not reach)."""
    with torch.enable_grad():
        leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
        out, out_xi, raw = ae_forward(leaves, X, noise, **kw)
        loss = 0
        for g, y in ((g_out, out), (g_out_xi, out_xi), (g_raw, raw)):
            if g is not None:
                loss = loss + (torch.as_tensor(g).to(dtype) * y).sum()
        gr = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    return {k: (torch.zeros_like(p) if g is None else g) for (k, p), g in zip(leaves.items(), gr)}
