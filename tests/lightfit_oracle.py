"""The oracle of the light-SG fit (robir_amd/lightfit.py, librobir_hip_lightfit.so): a PyTorch-CPU restatement of the three formulas of
model/sg_render.py:26-42, the MSE of envmaps/fit_envmap_with_sg.py:53, a torch.optim.Adam loop and a numpy float64 area resize.

Every function takes the fp32 inputs the kernels take and evaluates in `dtype`: torch.float64 is the reference of the tests, torch.float32 the
yardstick e_torch of the parity rule: e_kernel <= max(2 e_torch, 1e-5)."""
import math

import numpy as np
import torch


def envmap_dirs(H, W, upper_hemi=False):
    """compute_envmap's grid (sg_render.py:9-23) as the fp32 tensor [H W, 3] the kernels read."""
    phi, theta = torch.meshgrid([torch.linspace(0.0, math.pi / 2.0 if upper_hemi else math.pi, H),
                                 torch.linspace(1.0 * math.pi, -1.0 * math.pi, W)], indexing="ij")
    return torch.stack([torch.cos(theta) * torch.sin(phi), torch.sin(theta) * torch.sin(phi), torch.cos(phi)], -1).reshape(-1, 3)


def envmap(lgt, dirs):
    """rgb [n,3] = sum_k |mu_k| exp(|lambda_k| (d . l_k / |l_k| - 1)), in the dtype of its arguments; no epsilon in the norm."""
    axis = lgt[:, :3] / torch.norm(lgt[:, :3], dim=-1, keepdim=True)
    lam, mu = torch.abs(lgt[:, 3:4]), torch.abs(lgt[:, 4:])
    c = (dirs[:, None, :] * axis[None, :, :]).sum(-1, keepdim=True)
    return (mu[None] * torch.exp(lam[None] * (c - 1.0))).sum(1)


def backward(lgt, dirs, g_rgb, dtype=torch.float64):
    """autograd's d <g_rgb, envmap> / d lgt -> [M,7] in dtype."""
    p = lgt.detach().to(dtype).clone().requires_grad_()
    with torch.enable_grad():
        (envmap(p, dirs.to(dtype)) * g_rgb.to(dtype)).sum().backward()
    return p.grad.detach()


def loss_and_grad(lgt, dirs, target, dtype=torch.float64):
    p = lgt.detach().to(dtype).clone().requires_grad_()
    with torch.enable_grad():
        loss = ((envmap(p, dirs.to(dtype)) - target.to(dtype)) ** 2).mean()
        loss.backward()
    return float(loss.detach()), p.grad.detach()


def fit(init, dirs, target, steps, dtype=torch.float64, lr=1e-2):
    """The reference's loop (fit_envmap_with_sg.py:41,50-55) -> parameters, exp_avg, exp_avg_sq (dtype) and the loss before each update."""
    with torch.enable_grad():
        p = torch.nn.Parameter(init.detach().to(dtype).clone())
        opt = torch.optim.Adam([p], lr=lr)
        d, t = dirs.to(dtype), target.to(dtype)
        losses = []
        for _ in range(steps):
            opt.zero_grad()
            loss = ((envmap(p, d) - t) ** 2).mean()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    st = opt.state[p]
    return p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), np.asarray(losses, dtype=np.float64)


def init_light_sgs(M, seed):
    """fit_envmap_with_sg.py:37-38 from a CPU generator."""
    sg = torch.randn(M, 7, generator=torch.Generator().manual_seed(seed))
    sg[:, 3:4] *= 100.0
    return sg


def _overlap(n_src, n_dst):
    """[n_dst, n_src] float64: the share of source pixel j in destination pixel i's footprint [i n_src / n_dst, (i + 1) n_src / n_dst),
    rows summing to 1; the overlaps are integers in units of 1 / n_dst of a source pixel."""
    i = np.arange(n_dst, dtype=np.int64)[:, None]
    j = np.arange(n_src, dtype=np.int64)[None, :]
    ov = np.minimum((i + 1) * n_src, (j + 1) * n_dst) - np.maximum(i * n_src, j * n_dst)
    return np.maximum(ov, 0).astype(np.float64) / float(n_src)


def area_resize(img, H, W):
    """Coverage-weighted mean (cv2.INTER_AREA when shrinking) of img [H0, W0, 3] in float64 -> [H, W, 3] float64."""
    img = np.asarray(img, dtype=np.float64)
    H0, W0 = img.shape[:2]
    assert H <= H0 and W <= W0
    return np.einsum("yj,jqc,xq->yxc", _overlap(H0, H), img, _overlap(W0, W))


# The smallest shapes at which the kernels can go wrong: name -> (H, W, M, Mt).  240 pixels are no multiple of a wave or of four waves and
# fewer than the workgroups of a full grid; 130 lobes are a second lobe tile with two live lobes; 64 / 65 lobes straddle a lane's second lobe.
CASES = {
    "1x1x1": (1, 1, 1, 8),
    "12x20x130": (12, 20, 130, 128),
    "16x32x8": (16, 32, 8, 8),
    "16x32x24": (16, 32, 24, 128),
    "16x32x64": (16, 32, 64, 128),
    "16x32x65": (16, 32, 65, 128),
    "signs": (16, 32, 8, 8),        # negative raw lambda and mu entries, one mu_raw exactly 0: the sign chain and the zero gradient at 0
    "norms": (16, 32, 8, 8),        # lobe axes of norm 0.3 and 40: the chain through the normalisation
}
TRAJECTORY_CASES = ("16x32x8", "16x32x24", "12x20x130")


def make_case(name, H=None, W=None, M=None, Mt=None):
    """fp32 CPU tensors of a case: lgt [M,7] (the reference's init from seed 5), dirs [H W, 3], target [H W, 3] = the float64 envmap of
    synth.synth_light_sgs(3, Mt, False) rounded to fp32, g_rgb [H W, 3] a random upstream."""
    from robir_amd import synth
    if name in CASES:
        H, W, M, Mt = CASES[name]
    lgt = init_light_sgs(M, 5)
    if name == "signs":
        lgt[::2, 3] *= -1.0
        lgt[1::3, 4:] *= -1.0
        lgt[0, 4] = -abs(float(lgt[0, 4]))
        lgt[2, 5] = 0.0
    if name == "norms":
        unit = lgt[:, :3] / lgt[:, :3].norm(dim=-1, keepdim=True)
        lgt[0::2, :3] = unit[0::2] * 0.3
        lgt[1::2, :3] = unit[1::2] * 40.0
    dirs = envmap_dirs(H, W)
    tgt_sg = torch.from_numpy(np.asarray(synth.synth_light_sgs(3, Mt, False))).double()
    target = envmap(tgt_sg, dirs.double()).float()
    g_rgb = torch.randn(H * W, 3, generator=torch.Generator().manual_seed(11))
    return dict(name=name, H=H, W=W, M=M, lgt=lgt.contiguous(), dirs=dirs.contiguous(), target=target.contiguous(), g_rgb=g_rgb.contiguous())
