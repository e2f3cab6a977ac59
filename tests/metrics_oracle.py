"""A float64 numpy restatement of the image metrics (include/robir_hip_metrics.h), written on the test side: the transfers,
the pair sums, the angular error, the albedo ratio (lsq and median) and SSIM in two forms that must agree to 1e-10 here -- the explicit valid
11 x 11 window, and scipy.ndimage.gaussian_filter(sigma=1.5, truncate=3.5) cropped by 5 (scikit-image's recipe).  Plus the seeded inputs the
CPU and GPU tests share."""
import numpy as np

NONE, CLIP, GAMMA22, GAMMA22_Q8 = 0, 1, 2, 3
TRANSFERS = (NONE, CLIP, GAMMA22, GAMMA22_Q8)
C1, C2 = 0.01 ** 2, 0.03 ** 2
TILE, ROWS = 16, 256          # RB_MT_SSIM_TILE, RB_MT_ROWS


def transfer(x, t):
    x = np.asarray(x, dtype=np.float64)
    if t == NONE:
        return x
    if t == CLIP:
        return np.clip(x, 0.0, 1.0)
    y = np.clip(np.maximum(x, 0.0) ** (1.0 / 2.2), 0.0, 1.0)
    return np.floor(255.0 * y) / 255.0 if t == GAMMA22_Q8 else y


def load_pair(pred, gt, t=NONE, scale=None):
    p = np.asarray(pred, dtype=np.float32).astype(np.float64)
    if scale is not None:
        p = p * np.asarray(scale, dtype=np.float32).astype(np.float64)
    return transfer(p, t), transfer(np.asarray(gt, dtype=np.float32).astype(np.float64), t)


def pair_stats(pred, gt, mask=None, t=NONE, scale=None):
    """pred, gt [V,P,C], mask [V,P] -> (count [V], sums [V,C,5]): sum d^2, |d|, p g, p^2, g^2 over the masked pixels."""
    p, g = load_pair(pred, gt, t, scale)
    V, P, C = p.shape
    m = np.ones((V, P), bool) if mask is None else np.asarray(mask).astype(bool)
    w = m[..., None].astype(np.float64)
    d = p - g
    sums = np.stack([(w * d * d).sum(1), (w * np.abs(d)).sum(1), (w * p * g).sum(1), (w * p * p).sum(1), (w * g * g).sum(1)], -1)
    return m.sum(1).astype(np.float64), sums


def angular_stats(a, b, mask=None):
    """a, b [V,P,3] -> (count [V], sum of angles in radians [V]); rows with a vector shorter than 1e-6 are left out."""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    la, lb = np.sqrt((a * a).sum(-1)), np.sqrt((b * b).sum(-1))
    ok = (la >= 1e-6) & (lb >= 1e-6)
    if mask is not None:
        ok &= np.asarray(mask).astype(bool)
    dot = ((a / np.where(ok, la, 1.0)[..., None]) * (b / np.where(ok, lb, 1.0)[..., None])).sum(-1)
    ang = np.where(ok, np.arccos(np.clip(dot, -1.0, 1.0)), 0.0)
    return ok.sum(1).astype(np.float64), ang.sum(1)


def ratio_lsq(pred, gt, mask=None):
    n, s = pair_stats(np.asarray(pred).reshape(1, -1, np.shape(pred)[-1]), np.asarray(gt).reshape(1, -1, np.shape(gt)[-1]),
                      None if mask is None else np.asarray(mask).reshape(1, -1))
    pg, pp = s[0, :, 2], s[0, :, 3]
    return np.where(pp > 0, pg / np.where(pp > 0, pp, 1.0), 1.0)


def ratio_median(pred, gt, mask=None):
    """The LOWER median (torch.median's choice) of gt / pred in float32 over the masked pixels with pred > 1e-6."""
    p, g = np.asarray(pred, np.float32).reshape(-1, np.shape(pred)[-1]), np.asarray(gt, np.float32).reshape(-1, np.shape(gt)[-1])
    keep = np.ones(p.shape[0], bool) if mask is None else np.asarray(mask).reshape(-1).astype(bool)
    out = np.ones(p.shape[1])
    for c in range(p.shape[1]):
        rows = keep & (p[:, c] > 1e-6)
        if rows.any():
            q = np.sort(g[rows, c] / p[rows, c])
            out[c] = q[(len(q) - 1) // 2]
    return out


def window():
    x = np.arange(-5, 6, dtype=np.float64)
    w = np.exp(-x * x / 4.5)
    return w / w.sum()


def _quotient(ux, uy, exx, eyy, exy):
    vx, vy, vxy = exx - ux * ux, eyy - uy * uy, exy - ux * uy
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def ssim_map_window(p, g):
    """p, g [H,W] float64 -> [H-10,W-10]: every valid 11 x 11 window written out."""
    w2 = np.outer(window(), window())
    H, W = p.shape
    from numpy.lib.stride_tricks import sliding_window_view
    f = lambda z: (sliding_window_view(z, (11, 11)) * w2).sum((-1, -2))
    return _quotient(f(p), f(g), f(p * p), f(g * g), f(p * g))


def ssim_map_scipy(p, g):
    """The same through scipy.ndimage.gaussian_filter(sigma=1.5, truncate=3.5), cropped by 5: the border handling never reaches the crop."""
    import scipy.ndimage as ndi
    f = lambda z: ndi.gaussian_filter(z, 1.5, truncate=3.5, mode="reflect")[5:-5, 5:-5]
    return _quotient(f(p), f(g), f(p * p), f(g * g), f(p * g))


def ssim(pred, gt, mask=None, t=NONE, scale=None, check=True):
    """pred, gt [V,H,W,C], mask [V,H,W] -> (count [V], sum [V], map [V,H-10,W-10,C] float64 with zeros at the windows that are not
    counted).  check: the two forms agree to 1e-10 on every entry."""
    p, g = load_pair(pred, gt, t, scale)
    V, H, W, C = p.shape
    out = np.zeros((V, H - 10, W - 10, C))
    for v in range(V):
        for c in range(C):
            out[v, :, :, c] = ssim_map_window(p[v, :, :, c], g[v, :, :, c])
            if check:
                other = ssim_map_scipy(p[v, :, :, c], g[v, :, :, c])
                assert np.abs(other - out[v, :, :, c]).max() <= 1e-10, np.abs(other - out[v, :, :, c]).max()
    m = np.ones((V, H - 10, W - 10), bool) if mask is None else np.asarray(mask).astype(bool)[:, 5:H - 5, 5:W - 5]
    out = out * m[..., None]
    return m.sum((1, 2)).astype(np.float64), out.sum((1, 2, 3)), out


def ssim_f32_torch(pred, gt):
    """The defect this library avoids: the fp32 PyTorch restatement (two conv2d, E[x^2] - mu^2 in fp32) of one [H,W,C] pair -> map."""
    import torch
    import torch.nn.functional as F
    w = torch.tensor(window(), dtype=torch.float32)
    a = torch.as_tensor(np.asarray(pred, np.float32)).permute(2, 0, 1)[:, None]
    b = torch.as_tensor(np.asarray(gt, np.float32)).permute(2, 0, 1)[:, None]
    f = lambda z: F.conv2d(F.conv2d(z, w.view(1, 1, 1, 11)), w.view(1, 1, 11, 1))
    ux, uy = f(a), f(b)
    s = _quotient(ux, uy, f(a * a), f(b * b), f(a * b))
    return s[:, 0].permute(1, 2, 0).numpy()


# ----------------------------------------------------------------------------------------- seeded inputs
def images(kind, V, H, W, C, seed=0):
    """(pred, gt) float32 [V,H,W,C]: "noise" uniform in [0,1); "smooth" a sine pattern and a noisy copy; "flat" the flat-bright pair -- mean
    0.9 with noise of amplitude 1e-3, where an fp32 variance cancels against C2."""
    rng = np.random.default_rng([seed, V, H, W, C, {"noise": 0, "smooth": 1, "flat": 2}[kind]])
    if kind == "noise":
        return rng.random((V, H, W, C), dtype=np.float32), rng.random((V, H, W, C), dtype=np.float32)
    if kind == "flat":
        mk = lambda: (np.full((V, H, W, C), 0.9, np.float32) + 1e-3 * rng.standard_normal((V, H, W, C)).astype(np.float32))
        return mk(), mk()
    yy, xx = np.mgrid[0:H, 0:W]
    a = (0.5 + 0.4 * np.sin(xx / 7.0) * np.cos(yy / 5.0))[None, ..., None].repeat(V, 0).repeat(C, -1).astype(np.float32)
    b = np.clip(a + 0.05 * rng.standard_normal(a.shape).astype(np.float32), 0, 1).astype(np.float32)
    return a, b


def masks(V, H, W, seed=0):
    """[V,H,W] bool, a different one per view: view 0 random; view 1 (if any) EMPTY; view 2 (if any) a single centre at (H//2, W//2).  With
    V == 1 the random one."""
    rng = np.random.default_rng([seed, V, H, W, 77])
    m = rng.random((V, H, W)) < 0.6
    if V > 1:
        m[1] = False
    if V > 2:
        m[2] = False
        m[2, H // 2, W // 2] = True
    return m


def rows(V, P, C, seed=0):
    """(pred, gt float32 [V,P,C] in [-0.2, 1.3), mask [V,P]) for the pair sums; the last view's mask is empty when V > 1."""
    rng = np.random.default_rng([seed, V, P, C, 5])
    p = (1.5 * rng.random((V, P, C), dtype=np.float32) - 0.2).astype(np.float32)
    g = (1.5 * rng.random((V, P, C), dtype=np.float32) - 0.2).astype(np.float32)
    m = rng.random((V, P)) < 0.7
    if V > 1:
        m[-1] = False
    return p, g, m


def normals(V, P, seed=0):
    """(a, b float32 [V,P,3], mask [V,P]): random directions of random length; every 7th row of a and every 11th of b is shorter than 1e-6
    (zeros, or 1e-7 long)."""
    rng = np.random.default_rng([seed, V, P, 9])
    a = rng.standard_normal((V, P, 3)).astype(np.float32)
    b = (a + 0.3 * rng.standard_normal((V, P, 3))).astype(np.float32)
    a[:, ::7] = 0.0
    b[:, ::11] = np.float32(1e-7) / np.sqrt(np.float32(3))
    return a, b, rng.random((V, P)) < 0.8


def rel(a, b):
    """max |a - b| / max(|b|, tiny) over the entries -- the plain relative error of a few sums of one sign (or exact zeros)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.where(a == b, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-300))))
