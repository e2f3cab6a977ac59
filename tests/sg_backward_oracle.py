"""The oracle's shading formulas (oracle/robir_oracle/sg.py) with both sampled visibilities INJECTED as tensors, so that PyTorch autograd can
differentiate them in any dtype: the float64 truth and the fp32 yardstick of tests/test_sg_backward_gpu.py and of
tools/gen_sg_grad_golden.py.  Nothing here is sampled or drawn; the composition is render_with_sg's (sg.py), line for line."""
import math

import torch

from robir_oracle import sg

GRAD_NAMES = ("lgt", "f0", "rough", "albedo", "metallic", "bvis", "light_vis", "indir_integral")


def shade(normal, view, lgt, f0, rough, albedo, bvis, light_vis=None, metallic=None, indir_integral=None, lin_diff=False):
    """-> (spec [n,3], diff [n,3]).  lgt [M,7] or [n,M,7]; f0: one element; rough [n]; bvis [n]; light_vis [n,M] | None (comp_vis=False);
    metallic [n] | None; indir_integral [n,3] | None."""
    n = normal.shape[0]
    if lgt.dim() == 2:
        lgt = lgt.unsqueeze(0).expand(n, lgt.shape[0], 7)
    M = lgt.shape[1]
    l_lobe = lgt[..., :3] / (lgt[..., :3].norm(dim=-1, keepdim=True) + sg.TINY)
    l_lam = lgt[..., 3:4].abs()
    l_mu0 = lgt[..., -3:].abs()
    nrm = normal.unsqueeze(-2).expand(n, M, 3)
    vw = view.unsqueeze(-2).expand(n, M, 3)
    f0e = f0.reshape(1, 1, 1).expand(n, M, 3)
    met = metallic.reshape(n, 1) if metallic is not None else None
    spec = sg._specular(None, nrm, vw, f0e, rough.reshape(n, 1), albedo, met, l_lobe, l_lam, l_mu0, None, None, False, light_vis is not None,
                        False, bvis=bvis)
    l_mu_d = l_mu0 * light_vis.unsqueeze(-1) if light_vis is not None else l_mu0
    dmu = l_mu_d if lin_diff else l_mu_d * (albedo / math.pi).unsqueeze(-2)
    p_lobe, p_lam, p_mu = sg.sg_product(nrm, sg.LAMBDA_COS, sg.MU_COS, l_lobe, l_lam, dmu)
    diff = p_mu * sg.hemisphere_int(p_lam, (p_lobe * nrm).sum(-1, keepdim=True)) \
        - dmu * sg.ALPHA_COS * sg.hemisphere_int(l_lam, (l_lobe * nrm).sum(-1, keepdim=True))
    diff = diff.sum(-2).clamp(min=0.0)
    if indir_integral is not None:
        diff = indir_integral if lin_diff else indir_integral * (albedo / math.pi)
    return spec, diff


def grads(inputs, g_spec, g_diff, dtype):
    """Autograd of <g_spec, spec> + <g_diff, diff> in `dtype` on the CPU.  inputs: dict of numpy / tensors with the keys of shade()'s
    arguments (None = absent).  -> (dict name -> gradient tensor for every differentiable input present, spec, diff)."""
    t = {k: (None if v is None else torch.as_tensor(v).detach().cpu().to(dtype)) for k, v in inputs.items() if k != "lin_diff"}
    leaves = {k: t[k].clone().requires_grad_(True) for k in GRAD_NAMES if t.get(k) is not None}
    with torch.enable_grad():
        spec, diff = shade(t["normal"], t["view"], leaves["lgt"], leaves["f0"], leaves["rough"], leaves["albedo"], leaves["bvis"],
                           light_vis=leaves.get("light_vis"), metallic=leaves.get("metallic"), indir_integral=leaves.get("indir_integral"),
                           lin_diff=bool(inputs.get("lin_diff", False)))
        loss = (spec * torch.as_tensor(g_spec).cpu().to(dtype)).sum() + (diff * torch.as_tensor(g_diff).cpu().to(dtype)).sum()
        gs = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    out = {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(leaves, gs)}
    return out, spec.detach(), diff.detach()
