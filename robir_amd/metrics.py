"""Image metrics on the device (librobir_hip_metrics.so, include/robir_hip_metrics.h): MSE, MAE, PSNR, SSIM, the angular
error of two normal fields, the albedo ratio, and `evaluate_views`, the protocol of a relighting evaluation on the dict `render_view` returns.

Tensors are CUDA fp32.  An image argument is one of
    [H, W, C]       one view                              [P, C]      one view given as a pixel list
    [V, H, W, C]    V views                               [V, P, C]   V pixel lists -- pass views=True (a 3-D tensor is ONE image otherwise)
with 1 <= C <= 4; `mask` is a bool (or uint8) tensor of the same shape without the channel axis, or None for every pixel.
`transfer` ("none", "clip", "gamma22", "gamma22_q8", or the header's number) is applied on load to BOTH images, after the per-channel
`scale` [C] (a tensor, a sequence or None) has multiplied the prediction.  Every function returns a float64 tensor with one value per view.

The kernels leave fp64 sums per view; deriving a metric from them is float64 torch on V numbers.  There is no PyTorch fallback: a missing
library raises.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import ptr, stream_ptr

c_long, c_int = ctypes.c_long, ctypes.c_int
NONE, CLIP, GAMMA22, GAMMA22_Q8 = 0, 1, 2, 3
TRANSFERS = {"none": NONE, "clip": CLIP, "gamma22": GAMMA22, "gamma22_q8": GAMMA22_Q8}
SSIM_BORDER = 10          # the map of valid windows is (H - 10) x (W - 10)


def _transfer(t):
    if isinstance(t, str):
        if t.lower() not in TRANSFERS:
            raise ValueError(f"transfer {t!r}: one of {sorted(TRANSFERS)}")
        return TRANSFERS[t.lower()]
    return NONE if t is None else int(t)


def _f32(t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: a CUDA float32 tensor is needed, got {type(t).__name__}")
    if t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError(f"{what}: a CUDA float32 tensor is needed, got {t.dtype} on {t.device}")
    return t.contiguous()


def _scale(scale, C, dev):
    if scale is None:
        return None
    s = torch.as_tensor(scale, dtype=torch.float32).to(dev).reshape(-1).contiguous()
    if s.numel() == 1:
        s = s.expand(C).contiguous()
    if s.numel() != C:
        raise ValueError(f"scale has {s.numel()} values for {C} channels")
    return s


def _mask(mask, shape, dev):
    if mask is None:
        return None
    m = torch.as_tensor(mask).to(dev)
    if m.numel() != int(np.prod(shape)):
        raise ValueError(f"mask {tuple(m.shape)} does not match the images' {tuple(shape)}")
    return m.reshape(shape).to(torch.uint8).contiguous()


def _scratch(nbytes, dev):
    if nbytes < 0:
        raise _lib.RobirHipError("librobir_hip_metrics.so refused the sizes of the scratch query")
    return torch.empty(max(16, int(nbytes)), dtype=torch.uint8, device=dev)


def _as_rows(x, views, what):
    """-> [V, P, C]"""
    x = _f32(x, what)
    if x.dim() == 4:
        return x.reshape(x.shape[0], -1, x.shape[3])
    if x.dim() == 3:
        return x if views else x.reshape(1, -1, x.shape[2])
    if x.dim() == 2:
        return x.reshape(1, x.shape[0], x.shape[1])
    raise ValueError(f"{what}: [H,W,C], [V,H,W,C], [P,C] or (views=True) [V,P,C] expected, got {tuple(x.shape)}")


def _as_images(x, what):
    """-> [V, H, W, C]"""
    x = _f32(x, what)
    if x.dim() == 3:
        return x[None]
    if x.dim() == 4:
        return x
    raise ValueError(f"{what}: [H,W,C] or [V,H,W,C] expected, got {tuple(x.shape)}")


# ----------------------------------------------------------------------------------------- the three entry points
def pair_stats(pred, gt, mask=None, transfer=NONE, scale=None, views=False):
    """rb_mt_pair_stats -> (count [V], sums [V, C, 5]) float64: per view the masked pixel count and per channel
    sum d^2, sum |d|, sum p g, sum p^2, sum g^2 with p = T(scale pred), g = T(gt), d = p - g."""
    p, g = _as_rows(pred, views, "pred"), _as_rows(gt, views, "gt")
    if p.shape != g.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ")
    V, P, C = p.shape
    dev = p.device
    m, s = _mask(mask, (V, P), dev), _scale(scale, C, dev)
    stats = torch.zeros(V, 1 + 5 * C, dtype=torch.float64, device=dev)
    L = _lib.metrics()
    scratch = _scratch(L.rb_mt_pair_scratch_bytes(c_long(V), c_long(P), c_int(C)), dev)
    nz = lambda t: ptr(t) if t is not None and t.numel() else None
    _lib.call_metrics("rb_mt_pair_stats", nz(p), nz(g), c_long(V), c_long(P), c_int(C), nz(m), nz(s), c_int(_transfer(transfer)),
                      nz(stats), ptr(scratch), c_long(scratch.numel()), stream_ptr())
    return stats[:, 0], stats[:, 1:].reshape(V, C, 5)


def angular_stats(a, b, mask=None, views=False):
    """rb_mt_angular_stats -> (count [V], sum of angles in radians [V]) float64; rows with a vector shorter than 1e-6 are left out."""
    a, b = _as_rows(a, views, "a"), _as_rows(b, views, "b")
    if a.shape != b.shape or a.shape[2] != 3:
        raise ValueError(f"two [.., 3] fields of one shape expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    V, P, _ = a.shape
    dev = a.device
    m = _mask(mask, (V, P), dev)
    stats = torch.zeros(V, 2, dtype=torch.float64, device=dev)
    scratch = _scratch(_lib.metrics().rb_mt_angular_scratch_bytes(c_long(V), c_long(P)), dev)
    nz = lambda t: ptr(t) if t is not None and t.numel() else None
    _lib.call_metrics("rb_mt_angular_stats", nz(a), nz(b), c_long(V), c_long(P), nz(m), nz(stats), ptr(scratch), c_long(scratch.numel()),
                      stream_ptr())
    return stats[:, 0], stats[:, 1]


def ssim_stats(pred, gt, mask=None, transfer=NONE, scale=None, want_map=False):
    """rb_mt_ssim -> (count [V], sum [V]) float64 and the map [V, H - 10, W - 10, C] fp32 (None unless want_map)."""
    p, g = _as_images(pred, "pred"), _as_images(gt, "gt")
    if p.shape != g.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ")
    V, H, W, C = p.shape
    dev = p.device
    m, s = _mask(mask, (V, H, W), dev), _scale(scale, C, dev)
    stats = torch.zeros(V, 2, dtype=torch.float64, device=dev)
    out = torch.empty(V, max(H - SSIM_BORDER, 0), max(W - SSIM_BORDER, 0), C, dtype=torch.float32, device=dev) if want_map else None
    nbytes = _lib.metrics().rb_mt_ssim_scratch_bytes(c_long(V), c_long(H), c_long(W))
    scratch = torch.empty(max(16, int(nbytes)), dtype=torch.uint8, device=dev)      # a refused size is reported by the call below
    nz = lambda t: ptr(t) if t is not None and t.numel() else None
    _lib.call_metrics("rb_mt_ssim", nz(p), nz(g), c_long(V), c_long(H), c_long(W), c_int(C), nz(m), nz(s), c_int(_transfer(transfer)),
                      nz(stats), nz(out), ptr(scratch), c_long(scratch.numel()), stream_ptr())
    return stats[:, 0], stats[:, 1], out


# ----------------------------------------------------------------------------------------- the metrics (float64 torch on V numbers)
def mse(pred, gt, mask=None, transfer=NONE, scale=None, views=False):
    """Mean over the masked pixels and the channels of (p - g)^2; NaN for a view with an empty mask."""
    n, s = pair_stats(pred, gt, mask, transfer, scale, views)
    return s[:, :, 0].sum(1) / (n * s.shape[1])


def mae(pred, gt, mask=None, transfer=NONE, scale=None, views=False):
    """Mean over the masked pixels and the channels of |p - g|."""
    n, s = pair_stats(pred, gt, mask, transfer, scale, views)
    return s[:, :, 1].sum(1) / (n * s.shape[1])


def psnr(pred, gt, mask=None, transfer=NONE, scale=None, views=False):
    """-10 log10(sum_c sum d^2 / (C n)) for a data range of 1; identical images give inf."""
    return -10.0 * torch.log10(mse(pred, gt, mask, transfer, scale, views))


def ssim(pred, gt, mask=None, transfer=NONE, scale=None, return_map=False):
    """Mean SSIM over the channels and the valid windows whose centre is in the mask (NaN for a view with none).  return_map=True:
    (mean [V], map [V, H - 10, W - 10, C] fp32 with exact zeros at the windows that are not counted)."""
    n, s, out = ssim_stats(pred, gt, mask, transfer, scale, want_map=return_map)
    C = pred.shape[-1]
    mean = s / (n * C)
    return (mean, out) if return_map else mean


def normal_error_deg(pred, gt, mask=None, views=False):
    """Mean angle in degrees between the rows of two normal fields (neither needs unit length); rows where either is shorter than 1e-6
    -- the background of a render -- are left out."""
    n, s = angular_stats(pred, gt, mask, views)
    return s / n * (180.0 / math.pi)


def albedo_ratio(pred, gt, mask=None, mode="lsq"):
    """The per-channel factor that aligns a predicted albedo with the ground truth, over ALL given views together -> [C] fp32 on the
    device, ready for input['albedo_ratio'].
      "lsq"     sum p g / sum p^2 from one rb_mt_pair_stats call without a transfer; a channel with sum p^2 = 0 gives 1
      "median"  the median of gt / pred over the masked pixels with pred > 1e-6: torch.median on the device -- plumbing, not a kernel of
                this project (a device-side selection is out of scope); a channel without such a pixel gives 1"""
    p, g = _as_rows(pred, False, "pred"), _as_rows(gt, False, "gt")
    p, g = p.reshape(1, -1, p.shape[2]), g.reshape(1, -1, g.shape[2])
    if p.shape != g.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ")
    C = p.shape[2]
    if mode == "lsq":
        _, s = pair_stats(p, g, mask, NONE, None, views=True)
        pg, pp = s[0, :, 2], s[0, :, 3]
        return torch.where(pp > 0, pg / torch.where(pp > 0, pp, torch.ones_like(pp)), torch.ones_like(pp)).float()
    if mode != "median":
        raise ValueError(f"mode {mode!r}: 'lsq' or 'median'")
    m = _mask(mask, (1, p.shape[1]), p.device)
    keep = torch.ones(p.shape[1], dtype=torch.bool, device=p.device) if m is None else m[0].bool()
    out = torch.ones(C, dtype=torch.float32, device=p.device)
    for c in range(C):
        rows = keep & (p[0, :, c] > 1e-6)
        if bool(rows.any()):
            out[c] = torch.median(g[0, rows, c] / p[0, rows, c])
    return out


# ----------------------------------------------------------------------------------------- the protocol
_GT_ALIASES = {"rgb": ("rgb",), "albedo": ("albedo", "diffuse_albedo"), "roughness": ("roughness",), "normal": ("normal", "normals", "normal_map"),
               "mask": ("mask", "network_object_mask")}


def _first(d, names):
    for k in names:
        if k in d and d[k] is not None:
            return d[k]
    return None


def _dev_images(x, like, dev):
    """numpy or tensor, [H,W,C] / [V,H,W,C] / flat [N,C] -> fp32 [V,H,W,C] on dev; `like`: a [V,H,W,.] shape for flat inputs."""
    t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
    t = t.to(dev)
    if t.dtype != torch.bool:
        t = t.float()
    if t.dim() == 2 and like is not None:
        t = t.reshape(like[0], like[1], like[2], -1)
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4:
        raise ValueError(f"an image [H,W,C], a batch [V,H,W,C] or flat rows with a known image size expected, got {tuple(t.shape)}")
    return t.contiguous()


def evaluate_views(pred, gt, mask=None, transfer=GAMMA22, device=None):
    """The metrics of rendered views against ground truth.

    pred: the dict `render.render_view` returns (flat [N, .] tensors) or the arrays of the .npz `python -m robir_amd.render --out` writes
          ([H, W, .]), or a batch of those ([V, H, W, .]): sg_rgb, indir_rgb (optional), diffuse_albedo, roughness, normals / normal_map.
    gt:   any of rgb, albedo, roughness, normal, mask as [H, W, .] / [V, H, W, .] (a render's own names -- sg_rgb + indir_rgb,
          diffuse_albedo, normals, network_object_mask -- are understood too).  rgb and albedo are LINEAR, like the prediction.
    mask: [H, W] / [V, H, W] bool; None takes gt's mask, and every pixel where it has none.

    -> {"views": [one dict per view], "mean": {the means over the views}, "albedo_ratio": [3]} with the keys
         psnr, ssim                   of sg_rgb + indir_rgb against gt rgb, `transfer` (gamma 2.2) on both
         albedo_ratio                 albedo_ratio(diffuse_albedo, gt albedo, mask, "lsq") over all views together
         albedo_psnr, albedo_ssim     of the albedo scaled by that ratio, `transfer` on both
         roughness_mse                linear
         normal_mae_deg               mean angular error in degrees
    A key whose ground truth (or prediction) is absent is left out."""
    dev = torch.device(device) if device is not None else torch.device("cuda:0")
    g_rgb = _first(gt, _GT_ALIASES["rgb"])
    if g_rgb is None and "sg_rgb" in gt:
        g_rgb = np.asarray(_np(gt["sg_rgb"])) + (np.asarray(_np(gt["indir_rgb"])) if "indir_rgb" in gt else 0.0)
    truth = {"rgb": g_rgb, **{k: _first(gt, _GT_ALIASES[k]) for k in ("albedo", "roughness", "normal")}}
    if mask is None:
        mask = _first(gt, _GT_ALIASES["mask"])
    like = None
    for v in list(truth.values()) + [mask]:
        if v is not None and np.ndim(v) >= 3:
            like = _dev_images(v, None, dev).shape
            break
    if like is None and mask is not None and np.ndim(mask) == 2:
        like = (1,) + tuple(np.shape(mask))
    truth = {k: (None if v is None else _dev_images(v, like, dev)) for k, v in truth.items()}
    if like is None:
        raise ValueError("evaluate_views: the ground truth holds no image")
    V = like[0]
    m = None if mask is None else torch.as_tensor(np.asarray(_np(mask))).to(dev).reshape(V, like[1], like[2]).bool()
    per = {}
    ratio = None
    p_rgb = pred.get("sg_rgb")
    if truth["rgb"] is not None and p_rgb is not None:
        x = _dev_images(p_rgb, like, dev)
        if pred.get("indir_rgb") is not None:
            x = x + _dev_images(pred["indir_rgb"], like, dev)
        per["psnr"] = psnr(x, truth["rgb"], m, transfer)
        per["ssim"] = ssim(x, truth["rgb"], m, transfer)
    if truth["albedo"] is not None and pred.get("diffuse_albedo") is not None:
        a = _dev_images(pred["diffuse_albedo"], like, dev)
        ratio = albedo_ratio(a, truth["albedo"], m, "lsq")
        per["albedo_psnr"] = psnr(a, truth["albedo"], m, transfer, scale=ratio)
        per["albedo_ssim"] = ssim(a, truth["albedo"], m, transfer, scale=ratio)
    if truth["roughness"] is not None and pred.get("roughness") is not None:
        r, rg = _dev_images(pred["roughness"], like, dev), truth["roughness"]
        per["roughness_mse"] = mse(r[..., :1].contiguous(), rg[..., :1].contiguous(), m)
    p_n = _first(pred, ("normals", "normal_map", "normal"))
    if truth["normal"] is not None and p_n is not None:
        per["normal_mae_deg"] = normal_error_deg(_dev_images(p_n, like, dev), truth["normal"], m)
    per = {k: v.cpu() for k, v in per.items()}
    views = [{k: float(v[i]) for k, v in per.items()} for i in range(V)]
    res = {"views": views, "mean": {k: float(v.mean()) for k, v in per.items()}}
    if ratio is not None:
        res["albedo_ratio"] = [float(x) for x in ratio.cpu()]
        for d in views:
            d["albedo_ratio"] = res["albedo_ratio"]
    return res


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
