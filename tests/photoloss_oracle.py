"""A torch restatement of the tone curves (model/color_correction.py:31-73,116-137) and of the image term of InvLoss.forward
(model/loss.py:31-42,97-110), written from the formulas.  Every function works in the dtype of its inputs: the tests run it in float64 (the
truth, differentiated by autograd) and in float32 (what PyTorch's own arithmetic achieves on the same inputs), both on the CPU.

Curves: 0 scale_aces, 1 warp_aces, 2 ln_space, 3 identity (ACESToneMapping's hdr_mode), 4 the loss's fallback x / (x + 1)."""
import torch

CURVES = (0, 1, 2, 3)
RATIONAL = 4
ROWS = (1, 85, 86, 257, 70001)


def aces_fn(x):
    """The ACES filmic fit as a ratio of two quadratics."""
    num = x * (2.51 * x + 0.03)
    den = x * (2.43 * x + 0.59) + 0.14
    return num / den


def aces_inv(y):
    """The root of aces_fn(x) = y that is 0 at y = 0: (2.51 - 2.43 y) x^2 - (0.59 y - 0.03) x - 0.14 y = 0."""
    a = 2.51 - 2.43 * y
    q = 0.59 * y - 0.03
    disc = q * q + 4 * a * 0.14 * y
    return (q + torch.sqrt(disc)) / (2 * a)


def make_shift(shift):
    return torch.clamp(shift, 1e-4, 1)


def curve_fn(x, t, curve):
    """hdr2ldr's curve on an already clamped shift."""
    if curve == 0:
        return aces_fn(x) / t ** 0.2
    if curve == 1:
        return aces_fn(aces_inv(0.73 * t) / 0.73 * x) / t
    if curve == 2:
        u = x * (0.5 + t) / 0.5
        return u / (1 + t * u)
    if curve == RATIONAL:
        return x / (x + 1)
    return x


def curve_inv(x, t, curve):
    """ldr2hdr's curve on an already clamped shift."""
    if curve == 0:
        return aces_inv(x * t ** 0.2)
    if curve == 1:
        return 0.73 * aces_inv(x * t) / aces_inv(0.73 * t)
    if curve == 2:
        y = x / (1 - t * x)
        return y * 0.5 / (0.5 + t)
    return x


def tonemap(x, shift, curve, inverse=False):
    """x [n,3]; shift [1] or [n] (raw: clamped here, as make_shift does); -> [n,3]."""
    t = make_shift(shift).reshape(-1, 1)
    return curve_inv(x, t, curve) if inverse else curve_fn(x, t, curve)


def image_loss(sg_rgb, indir_rgb, gt, net_mask, obj_mask, shift, curve, l2=False):
    """loss.py:97-110 + 31-42: sum over the rows of m = net_mask & obj_mask of dist(hdr2ldr(sg + indir), gt) / N."""
    x = sg_rgb if indir_rgb is None else sg_rgb + indir_rgb
    pred = tonemap(x, shift, curve) if shift is not None else curve_fn(x, None, curve)
    m = net_mask & obj_mask
    N = obj_mask.shape[0]
    if N == 0 or int(m.sum()) == 0:
        return (x.sum() * 0).to(x.dtype)
    d = pred[m] - gt[m]
    return ((d * d).sum() if l2 else d.abs().sum()) / float(N)


def as_input(adapt_illum):
    return torch.clamp(adapt_illum * 10 + 0.5, 0, 1).view(1, 1)


# ------------------------------------------------------------------------------------------------ inputs inside the curves' domains
def tonemap_case(n, curve, inverse, per_row, seed=0):
    """fp32 (x [n,3], shift [n] | [1], gy [n,3]).  hdr2ldr: x in [0, 8]; ldr2hdr curve 0 / 1: x t^0.2 resp. x t <= 0.95 (aces_inv is singular
    at 2.51 / 2.43); curve 2: x <= 0.9 with t <= 1; t in [0.05, 1]."""
    g = torch.Generator().manual_seed(1000 * curve + 100 * int(inverse) + 10 * int(per_row) + seed + n)
    t = 0.05 + 0.95 * torch.rand(n if per_row else 1, generator=g)
    u = torch.rand(n, 3, generator=g)
    if not inverse:
        x = 8.0 * u
    elif curve == 0:
        x = 0.95 * u / (t.reshape(-1, 1) ** 0.2)
    elif curve == 1:
        x = 0.95 * u / t.reshape(-1, 1)
    else:
        x = 0.9 * u
    gy = torch.randn(n, 3, generator=g)
    x, t = x.float(), t.float()
    tt = t.double().reshape(-1, 1)
    if inverse and curve in (0, 1):
        assert float((x.double() * (tt ** 0.2 if curve == 0 else tt)).max()) <= 0.951
    assert bool(torch.isfinite(tonemap(x.double(), t.double(), curve, inverse)).all())
    return x, t, gy.float()


def loss_case(n, curve, per_row, l2, seed=0, indir=True):
    """fp32 dict: sg_rgb, indir_rgb, gt [n,3], net_mask, obj_mask [n] bool, shift [n] | [1] (None for curves 3 / 4).  sg + indir in [0, 8];
    for L1 every |pred - gt| >= 1e-3 in float64 (gt is pushed away where it is not)."""
    g = torch.Generator().manual_seed(7000 + 1000 * curve + 100 * int(l2) + 10 * int(per_row) + seed + n)
    sg = 5.0 * torch.rand(n, 3, generator=g)
    ind = 3.0 * torch.rand(n, 3, generator=g) if indir else None
    gt = torch.rand(n, 3, generator=g)
    m1 = torch.rand(n, generator=g) < 0.8
    m2 = torch.rand(n, generator=g) < 0.8
    m1[0] = m2[0] = True                     # never an empty mask: n = 1 is one row INSIDE both masks
    shift = None
    if curve in (0, 1, 2):
        shift = (0.05 + 0.95 * torch.rand(n if per_row else 1, generator=g)).float()
    x64 = sg.double() + (ind.double() if indir else 0)
    pred = tonemap(x64, shift.double(), curve) if shift is not None else curve_fn(x64, None, curve)
    close = (pred - gt.double()).abs() < 2e-3
    gt = torch.where(close, (pred + 0.01).float(), gt)
    assert float((pred - gt.double()).abs().min()) >= 1e-3
    return dict(sg_rgb=sg.float(), indir_rgb=None if ind is None else ind.float(), gt=gt.float(), net_mask=m1, obj_mask=m2, shift=shift)


def tonemap_grads(x, shift, gy, curve, inverse, dtype):
    """(y, gx, gshift) of <gy, tonemap(x, shift)> by autograd in `dtype`."""
    with torch.enable_grad():
        xx = x.to(dtype).clone().requires_grad_(True)
        tt = shift.to(dtype).clone().requires_grad_(True)
        y = tonemap(xx, tt, curve, inverse)
        gx, gt = torch.autograd.grad((y * gy.to(dtype)).sum(), [xx, tt], allow_unused=True)
    return y.detach(), gx, torch.zeros_like(tt) if gt is None else gt


def loss_grads(case, curve, l2, dtype):
    """(loss, d sg_rgb, d indir_rgb or None, d shift or None) by autograd in `dtype`."""
    c = lambda t: None if t is None else t.to(dtype).clone().requires_grad_(True)
    with torch.enable_grad():
        sg, ind, sh = c(case["sg_rgb"]), c(case["indir_rgb"]), c(case["shift"])
        loss = image_loss(sg, ind, case["gt"].to(dtype), case["net_mask"], case["obj_mask"], sh, curve, l2)
        leaves = [t for t in (sg, ind, sh) if t is not None]
        gr = list(torch.autograd.grad(loss, leaves, allow_unused=True))
    gr = [torch.zeros_like(l) if g is None else g for g, l in zip(gr, leaves)]
    g_sg = gr.pop(0)
    g_ind = gr.pop(0) if ind is not None else None
    g_sh = gr.pop(0) if sh is not None else None
    return loss.detach(), g_sg, g_ind, g_sh
