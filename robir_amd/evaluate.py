"""Scores rendered views against ground truth on the device (robir_amd/metrics.py): PSNR and SSIM of the image, the albedo
ratio, PSNR and SSIM of the aligned albedo, roughness MSE and the normal error in degrees, per view and averaged.

    python -m robir_amd.evaluate --pred view.npz [more.npz ...] --gt gt.npz|DIR --out metrics.json [--transfer gamma22_q8] [--ssim-maps DIR]

--pred   what `python -m robir_amd.render --out` writes, one file per view
--gt     an .npz with any of rgb, albedo, roughness, normal, mask ([H,W,.], or [V,H,W,.] for several predictions; a render's own .npz is
         understood too), or a directory of rgb_*.png|exr, albedo_*.png, normal_*.png, roughness_*.png, mask_*.png, matched to the
         predictions by sorted order.  The metrics apply the transfer to BOTH sides, so the readers return LINEAR colour: an 8-bit PNG level
         k of rgb / albedo (which holds x^(1/2.2), as `--png-dir` writes it) is read as the centre of its bin, ((k + 0.5) / 255)^2.2 -- under
         gamma22_q8 that gives back k / 255 exactly.  Roughness is k / 255, a normal 2 k / 255 - 1, a mask k >= 128; EXR is linear as it is.
--transfer   none | clip | gamma22 (default) | gamma22_q8 (what the PNG set holds)
--ssim-maps  also write ssim_<view>.png (and albedo_ssim_<view>.png), the SSIM map averaged over the channels

Nothing is downloaded and no dataset is required.
"""
import argparse
import glob
import json
import os

import numpy as np
import torch

KINDS = ("rgb", "albedo", "normal", "roughness", "mask")
KEYS = ("psnr", "ssim", "albedo_psnr", "albedo_ssim", "roughness_mse", "normal_mae_deg")


def read_png(path, kind):
    """One ground-truth PNG (PIL) -> float32 [H,W,C] (bool [H,W] for a mask), decoded as the module's text says."""
    from PIL import Image
    img = Image.open(path)
    a = np.asarray(img.convert("L") if kind in ("roughness", "mask") else img.convert("RGB"))
    if a.dtype != np.uint8:
        raise ValueError(f"{path}: an 8-bit PNG is needed, got {a.dtype}")
    k = a.astype(np.float64)
    if kind == "mask":
        return a >= 128
    if kind == "roughness":
        return (k / 255.0).astype(np.float32)[..., None]
    if kind == "normal":
        return (2.0 * k / 255.0 - 1.0).astype(np.float32)
    return (((k + 0.5) / 255.0) ** 2.2).astype(np.float32)


def read_gt_dir(path, n_views):
    """{kind: [V,H,W,C]} of the kinds the directory holds; every kind present needs one file per prediction."""
    from . import exr
    out = {}
    for kind in KINDS:
        files = sorted(glob.glob(os.path.join(path, kind + "_*.png")))
        if kind == "rgb":
            files = sorted(files + glob.glob(os.path.join(path, "rgb_*.exr")), key=lambda f: os.path.splitext(os.path.basename(f))[0])
        if not files:
            continue
        if len(files) != n_views:
            raise ValueError(f"{path}: {len(files)} {kind}_* files for {n_views} predictions")
        imgs = [exr.read_exr(f)[..., :3].astype(np.float32) if f.endswith(".exr") else read_png(f, kind) for f in files]
        out[kind] = np.stack(imgs)
    if not out:
        raise ValueError(f"{path}: no rgb_*, albedo_*, normal_*, roughness_* or mask_* file")
    return out


def read_gt(path, n_views):
    if os.path.isdir(path):
        return read_gt_dir(path, n_views)
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def read_preds(paths):
    """The .npz files of the views, stacked -> {key: [V,H,W,.]}; every file needs the first one's keys and size."""
    views = []
    for p in paths:
        with np.load(p, allow_pickle=False) as z:
            views.append({k: z[k] for k in z.files})
    keys = [k for k in views[0] if all(k in v and v[k].shape == views[0][k].shape for v in views)]
    if "sg_rgb" not in keys and "diffuse_albedo" not in keys:
        raise ValueError(f"{paths[0]}: not a file written by `python -m robir_amd.render --out` (no sg_rgb / diffuse_albedo of one size in every view)")
    return {k: np.stack([v[k] for v in views]) for k in keys}


def _batched(gt, n_views):
    """[H,W,.] entries of a one-view ground truth get their view axis."""
    out = {}
    for k, v in gt.items():
        v = np.asarray(v)
        if v.ndim == (2 if k == "mask" else 3):      # mask [H,W]; every other entry carries a channel axis
            v = v[None]
        out[k] = v
    return out


def table(res):
    keys = [k for k in KEYS if k in res["mean"]]
    rows = [["view"] + keys]
    for i, d in enumerate(res["views"]):
        rows.append([str(i)] + ["%.6g" % d[k] for k in keys])
    rows.append(["mean"] + ["%.6g" % res["mean"][k] for k in keys])
    width = [max(len(r[c]) for r in rows) for c in range(len(rows[0]))]
    lines = ["  ".join(x.rjust(w) for x, w in zip(r, width)) for r in rows]
    if "albedo_ratio" in res:
        lines.append("albedo_ratio " + " ".join("%.6g" % x for x in res["albedo_ratio"]))
    return "\n".join(lines)


def _json_number(x):
    """inf / nan are not JSON: written as the strings "inf", "-inf", "nan"."""
    if isinstance(x, float) and not np.isfinite(x):
        return "nan" if np.isnan(x) else ("inf" if x > 0 else "-inf")
    return x


def to_json(res, transfer, preds):
    clean = lambda d: {k: ([_json_number(x) for x in v] if isinstance(v, list) else _json_number(v)) for k, v in d.items()}
    out = {"transfer": transfer, "pred": list(preds), "views": [clean(d) for d in res["views"]], "mean": clean(res["mean"])}
    if "albedo_ratio" in res:
        out["albedo_ratio"] = res["albedo_ratio"]
    return out


def evaluate_files(preds, gt, transfer="gamma22", ssim_maps=None):
    """The CLI as a function -> (evaluate_views' result, the JSON document)."""
    from . import metrics, texture
    pred = read_preds(preds)
    truth = _batched(read_gt(gt, len(preds)), len(preds))
    res = metrics.evaluate_views(pred, truth, transfer=transfer)
    if ssim_maps:
        os.makedirs(ssim_maps, exist_ok=True)
        dev = torch.device("cuda:0")
        mask = metrics._first(truth, metrics._GT_ALIASES["mask"])
        V, H, W = pred["sg_rgb" if "sg_rgb" in pred else "diffuse_albedo"].shape[:3]
        m = None if mask is None else torch.from_numpy(np.asarray(mask)).to(dev).reshape(V, H, W)
        pairs = []
        g_rgb = truth.get("rgb")
        if g_rgb is None and "sg_rgb" in truth:
            g_rgb = truth["sg_rgb"] + truth.get("indir_rgb", 0.0)
        if g_rgb is not None and "sg_rgb" in pred:
            pairs.append(("ssim", pred["sg_rgb"] + pred.get("indir_rgb", 0.0), g_rgb, None))
        g_alb = metrics._first(truth, metrics._GT_ALIASES["albedo"])
        if g_alb is not None and "diffuse_albedo" in pred:
            pairs.append(("albedo_ssim", pred["diffuse_albedo"], g_alb, res.get("albedo_ratio")))
        for name, p, g, scale in pairs:
            to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
            _, maps = metrics.ssim(to(p), to(g), m, transfer, scale=scale, return_map=True)
            for i in range(V):
                texture.save_png(os.path.join(ssim_maps, f"{name}_{i}.png"), maps[i].mean(-1).clamp(0, 1).cpu().numpy())
    return res, to_json(res, transfer, preds)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pred", nargs="+", required=True)
    ap.add_argument("--gt", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--transfer", default="gamma22", choices=("none", "clip", "gamma22", "gamma22_q8"))
    ap.add_argument("--ssim-maps")
    a = ap.parse_args(argv)
    res, doc = evaluate_files(a.pred, a.gt, a.transfer, a.ssim_maps)
    print(table(res))
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
