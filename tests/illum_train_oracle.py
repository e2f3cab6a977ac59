"""Test-side truth for the indirect-illumination network's backward: torch autograd of the oracle's formulas (robir_oracle.nets.indirect_illum
and its sparse_ae) and of query_indir_illum (model/loss.py:128-141, restated here) on the CPU, in float64 (the truth) or float32 (the yardstick:
what PyTorch's own fp32 autograd achieves on the same inputs).  The lobe net's encoding is evaluated in the evaluation's dtype from the fp32
coordinates; the integral layer is evaluated on the fp32 perturbed rows the kernel saw (passed as `x` with zero noise).  Shared by
tests/test_illum_train_cpu.py, tests/test_illum_train_gpu.py, tools/gen_illum_grad_golden.py and tools/prof_illum_backward.py."""
import torch
import torch.nn.functional as F

from robir_oracle import nets as on

PREFIX = on.ILL
LOBE_NAMES = tuple(f"lobe_layer.{2 * i}.{w}" for i in range(5) for w in ("weight", "bias"))
AE_NAMES = tuple(f"brdf_encoder_layer.{2 * i}.{w}" for i in range(5) for w in ("weight", "bias")) \
    + tuple(f"brdf_decoder_layer.{2 * i}.{w}" for i in range(3) for w in ("weight", "bias"))
INT_NAMES = tuple("integral_layer." + k for k in AE_NAMES)
NAMES = LOBE_NAMES + INT_NAMES          # the 26 tensors, IndirctIllumNetwork.named_parameters()'s names


def illum_params(sd, prefix=PREFIX):
    """The 26 tensors of the indirect-illumination network out of a state dict, keyed by NAMES."""
    return {k: torch.as_tensor(sd[prefix + k]) for k in NAMES}


def leaves(params, dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}


def _dtype(params):
    return next(iter(params.values())).dtype


def _sd(params):
    return {PREFIX + k: v for k, v in params.items()}


def lobes_forward(params, points, hdr):
    """-> lgt_sgs [n,24,7] in the dtype of `params`; points [n,3] and hdr [n,1] (None: the no_hdr net) are the fp32 inputs."""
    dtype = _dtype(params)
    pts = points.detach().float().to(dtype)
    feat = on.pe(pts, 10) if hdr is None else torch.cat([on.pe(pts, 10), hdr.detach().float().to(dtype).reshape(-1, 1)], -1)
    out = on._seq(_sd(params), PREFIX + "lobe_layer.", 5, feat, torch.relu).reshape(-1, 24, 6)
    ab = torch.sigmoid(out[..., :2])
    theta, phi = ab[..., :1] * 2 * torch.pi, ab[..., 1:2] * torch.pi
    lobes = torch.cat([torch.cos(theta) * torch.sin(phi), torch.sin(theta) * torch.sin(phi), torch.cos(phi)], -1)
    return torch.cat([lobes, torch.sigmoid(out[..., 2:3]) * 30 + 0.1, torch.relu(out[..., 3:])], -1)


def integral_forward(params, rows, var=None):
    """-> env_int [n,3]: |second output| of the oracle's sparse_ae on the fp32 perturbed rows [n, in_dim] the kernel saw (zero noise)."""
    dtype = _dtype(params)
    x = rows.detach().float().to(dtype)
    v = torch.zeros(32, dtype=dtype, device=x.device) if var is None else torch.as_tensor(var).to(x)      # zeros on x's device: x (1 - 0) = x
    _, rnd = on.sparse_ae(_sd(params), PREFIX + "integral_layer", x, torch.zeros_like(x), False, F.softplus, None, v)
    return rnd.abs()


def both_forward(params, points, hdr, noise):
    """on.indirect_illum itself (encoding and perturbation in the dtype of `params`): what the reference fixture is compared with."""
    dtype = _dtype(params)
    return on.indirect_illum(_sd(params), points.detach().to(dtype), None if hdr is None else hdr.detach().to(dtype).reshape(-1, 1),
                             noise.detach().to(dtype))


def query(sgs, dirs):
    """query_indir_illum (model/loss.py:128-141) in plain torch: sgs [n,L,7], dirs [n,S,3] -> [n,S,3] in the dtype of sgs."""
    sgs = sgs[:, None]                                    # [n,1,L,7]
    d = dirs.to(sgs.dtype)[:, :, None]                    # [n,S,1,3]
    lobes = sgs[..., :3] / torch.norm(sgs[..., :3], dim=-1, keepdim=True)
    return (sgs[..., -3:] * torch.exp(sgs[..., 3:4] * ((d * lobes).sum(-1, keepdim=True) - 1.0))).sum(2)


def grads_of(loss_fn, params, dtype, names=None):
    """(loss value, dict name -> gradient) of loss_fn(leaves) for `names` (default: every leaf the loss reaches is required)."""
    with torch.enable_grad():
        lv = leaves(params, dtype)
        loss = loss_fn(lv)
        keys = list(names or lv)
        gr = torch.autograd.grad(loss, [lv[k] for k in keys])
    return float(loss.detach()), dict(zip(keys, gr))


def query_grads(sgs, dirs, g, dtype):
    """(radiance, d <g, radiance> / d sgs) of the plain-torch query in `dtype` from the fp32 inputs."""
    with torch.enable_grad():
        x = sgs.detach().float().to(dtype).requires_grad_(True)
        rad = query(x, dirs.detach().float().to(dtype))
        gs, = torch.autograd.grad((rad * g.detach().float().to(dtype)).sum(), x)
    return rad.detach(), gs


def radiance_loss(sgs_all, int_all, trace, points_mask, anneal_t=0.0, loss_type="L1"):
    """model/loss.py:156-171 on tensors, in the dtype of sgs_all: sgs_all [N,24,7], int_all [N,3], trace: trace_radiance [N,S,3],
    sample_dirs [n,S,3], indir_mask [N,S], gt_integral [N,3]."""
    dist = F.l1_loss if loss_type == "L1" else F.mse_loss
    dt = sgs_all.dtype
    pred = query(sgs_all[points_mask], trace["sample_dirs"].to(dt))
    loss = dist(pred[trace["indir_mask"][points_mask]], trace["trace_radiance"].to(dt)[trace["indir_mask"]] + anneal_t)
    return loss + dist(int_all[points_mask], trace["gt_integral"].to(dt)[points_mask])
