"""numpy restatement of librobir_hip_texfit.so (include/robir_hip_texfit.h, robir_amd/csrc/texfit/texfit_math.h): the same operations in the
same order, one rounding each, so that with dtype float32 every kernel is reproduced BIT FOR BIT.  With dtype float64 the same rules are
the reference of the property tests (adjointness, grid_sample, torch.optim.Adam) and of the closed loop: an fp64 torch fit of a small
scene (sg_backward_oracle.shade + these taps + lazy Adam), independent of the kernels' rounding.  Also the uv cases and the scene shared by
the CPU and the GPU tests; meshes, cameras and the G-buffer come from meshrender_restatement, the atlas from texbake_restatement."""
import functools

import numpy as np

import meshrender_restatement as mr
import texbake_restatement as tr

F32, F64 = np.float32, np.float64


# ----------------------------------------------------------------------------------------- texfit_math.h
def taps(uv, R, filter=1, dtype=F32):
    """uv [n,2] -> (texel [n,4] int32, weight [n,4]) in the order nw, ne, sw, se; -1 / +0 outside the image."""
    uv = np.asarray(uv, dtype=dtype).reshape(-1, 2)
    u, v = uv[:, 0], uv[:, 1]
    n = u.shape[0]
    texel, weight = np.full((n, 4), -1, dtype=np.int32), np.zeros((n, 4), dtype=dtype)
    fr, half, one = dtype(R), dtype(0.5), dtype(1.0)
    with np.errstate(all="ignore"):
        if filter == 0:
            lim = dtype(R - 1)
            c = np.minimum(np.maximum(np.floor(u * fr), dtype(0.0)), lim)
            r = np.minimum(np.maximum(np.floor((one - v) * fr), dtype(0.0)), lim)
            c, r = np.nan_to_num(c, nan=0.0).astype(np.int64), np.nan_to_num(r, nan=0.0).astype(np.int64)
            texel[:, 0] = r * R + c
            weight[:, 0] = one
            return texel, weight
        x, y = u * fr - half, (one - v) * fr - half
        x0, y0 = np.floor(x), np.floor(y)
        wx1, wx0, wy1, wy0 = x - x0, (x0 + one) - x, y - y0, (y0 + one) - y
        w = (wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1)
        c0 = np.nan_to_num(np.clip(x0, -2.0, R + 1.0), nan=-2.0).astype(np.int64)
        r0 = np.nan_to_num(np.clip(y0, -2.0, R + 1.0), nan=-2.0).astype(np.int64)
    for k in range(4):
        c, r = c0 + (k & 1), r0 + (k >> 1)
        ok = (c >= 0) & (c < R) & (r >= 0) & (r < R)
        texel[:, k] = np.where(ok, r * R + c, -1)
        weight[:, k] = np.where(ok, w[k], dtype(0.0))
    return texel, weight


def fetch(planes, texel, weight, C=None, dtype=F32):
    """planes [R,R,Cs] -> [n,C] = ((a w0 + b w1) + c w2) + d w3; an absent tap's value is +0."""
    planes = np.asarray(planes, dtype=dtype)
    R, Cs = planes.shape[0], planes.shape[2]
    C = Cs if C is None else C
    flat = planes.reshape(R * R, Cs)[:, :C]
    ok = (texel >= 0) & (texel < R * R)
    val = np.where(ok[:, :, None], flat[np.clip(texel, 0, R * R - 1)], dtype(0.0)).astype(dtype)
    w = np.asarray(weight, dtype=dtype)[:, :, None]
    with np.errstate(all="ignore"):
        return (((val[:, 0] * w[:, 0] + val[:, 1] * w[:, 1]) + val[:, 2] * w[:, 2]) + val[:, 3] * w[:, 3]).astype(dtype)


def sort_pairs(texel, weight, R):
    """The (row, tap) pairs sorted by texel, stable; absent taps (key R^2) at the tail -> (pair_row [4n] int32, pair_weight [4n], seg_texel [T]
    int32, seg_start [T+1] int32)."""
    key = np.asarray(texel).reshape(-1).astype(np.int64)
    key = np.where(key < 0, R * R, key)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    seg_texel, first = np.unique(skey[skey < R * R], return_index=True)
    seg_start = np.concatenate([first, [int((skey < R * R).sum())]]).astype(np.int32)
    return (order // 4).astype(np.int32), np.asarray(weight).reshape(-1)[order].copy(), seg_texel.astype(np.int32), seg_start


def scatter(pair_row, pair_weight, seg_start, g_tex, dtype=F32):
    """grad [T,C]: per segment the fp64 sum of weight * g_tex[row] in ascending pair order, rounded once to `dtype`; a row outside [0, n) is
    passed over."""
    g = np.asarray(g_tex)
    n, C = g.shape
    P, T = len(pair_row), len(seg_start) - 1
    grad = np.zeros((T, C), dtype=dtype)
    for s in range(T):
        p0, p1 = max(int(seg_start[s]), 0), min(int(seg_start[s + 1]), P)
        rows = np.asarray(pair_row[p0:p1]).astype(np.int64)
        ok = (rows >= 0) & (rows < n)
        if not ok.any():
            continue
        prod = np.asarray(pair_weight[p0:p1])[ok].astype(F64)[:, None] * g[rows[ok]].astype(F64)
        grad[s] = (np.cumsum(np.concatenate([np.zeros((1, C)), prod]), axis=0)[-1]).astype(dtype)         # sequential, from +0
    return grad


def dense(seg_texel, grad, R):
    out = np.zeros((R * R, grad.shape[1]), dtype=grad.dtype)
    out[np.asarray(seg_texel).astype(np.int64)] = grad
    return out.reshape(R, R, -1)


def adam(planes, m, v, seg_texel, grad, lr, lo, hi, beta1, beta2, eps, t, dtype=F32):
    """One lazy Adam step IN PLACE on planes [R,R,Cs] (its first C channels), m, v [R,R,C] at the texels seg_texel [T]; grad [T,C]; lr, lo,
    hi [C]; t: the step number.  fp64 from the `dtype` inputs, every stored value rounded once; a texel outside [0, R^2) is skipped."""
    R, Cs = planes.shape[0], planes.shape[2]
    C = grad.shape[1]
    tex = np.asarray(seg_texel).astype(np.int64)
    ok = (tex >= 0) & (tex < R * R)
    idx, g = tex[ok], np.asarray(grad)[ok].astype(F64)
    P, M, V = planes.reshape(R * R, Cs), m.reshape(R * R, C), v.reshape(R * R, C)
    lr, lo, hi = (np.asarray(a, dtype=F64)[None, :] for a in (lr, lo, hi))
    bc1, bc2 = 1.0 - float(beta1) ** int(t), 1.0 - float(beta2) ** int(t)
    m1 = (beta1 * M[idx].astype(F64) + (1.0 - beta1) * g).astype(dtype)
    v1 = (beta2 * V[idx].astype(F64) + (1.0 - beta2) * (g * g)).astype(dtype)
    with np.errstate(all="ignore"):
        step = lr * (m1.astype(F64) / bc1) / (np.sqrt(v1.astype(F64) / bc2) + eps)
        p1 = np.fmin(np.fmax(P[idx, :C].astype(F64) - step, lo), hi).astype(dtype)
    M[idx], V[idx] = m1, v1
    P[idx, :C] = p1


# ----------------------------------------------------------------------------------------- uv cases
def tap_uvs(R, seed=5):
    """uv [n,2] float32, n >= 257: the G-buffer case's uvs, texel centres (weights exactly 1, 0, 0, 0), u or v = 0 and 1 (taps outside the
    image), uv outside [0, 1], NaN, and random ones."""
    rng = np.random.default_rng(seed)
    verts, faces, uv, planes, vn = mr.gbuffer_case()
    from robir_amd import synth
    _, _, K = synth.synth_camera(13, 21)
    pose = mr.rotated_pose()
    face_id, bary, _ = mr.raster(mr.project(verts, mr.pose_inverse(pose), K), faces, 13, 21)
    hit = np.nonzero(face_id.reshape(-1) >= 0)[0]
    rows = [mr.gbuffer(face_id, bary, faces, verts, uv, pose[:3, 3], index=hit)["uv"]]
    centres = [((c + 0.5) / R, 1.0 - (r + 0.5) / R) for r in range(min(R, 4)) for c in range(min(R, 4))] + [((R - 0.5) / R, 0.5 / R)]
    border = [(0.0, 0.3), (1.0, 0.3), (0.3, 0.0), (0.3, 1.0), (0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0)]
    outside = [(-0.2, 0.5), (1.4, 0.5), (0.5, -3.0), (0.5, 2.5), (-1e9, 0.5), (0.5, 1e30), (1.0 + 0.4 / R, 0.5), (-0.4 / R, -0.4 / R),
               (np.inf, 0.5), (0.5, -np.inf)]
    nan = [(np.nan, 0.5), (0.5, np.nan), (np.nan, np.nan)]
    rows += [np.array(centres + border + outside + nan, dtype=F32), rng.uniform(-0.1, 1.1, (300, 2)).astype(F32)]
    return np.concatenate(rows).astype(F32)


SEGMENTS = (1, 63, 64, 65, 300, 1, 2, 5, 1)          # pairs per segment: one pair, around a wave's width, a long one; first and last short


def scatter_case(C, n=131, tail=7, seed=9):
    """A pair list built directly -> (pair_row [P] int32, pair_weight [P], seg_start [T+1] int32, g_tex [n,C]): the segments of SEGMENTS,
    rows ascending inside a segment as after the stable sort, a few rows outside [0, n) inside the segments (they contribute nothing) and
    `tail` pairs beyond seg_start[T] whose rows are far out of range (never read).  n is no multiple of 64 and P <= 4 n."""
    rng = np.random.default_rng(seed + C)
    rows = [np.sort(rng.integers(0, n, k)) for k in SEGMENTS]
    rows[4][[3, 77, 150]] = (-1, n, 2 ** 30)
    rows[1][10] = -5
    pair_row = np.concatenate(rows + [np.full(tail, 2 ** 30)]).astype(np.int32)
    pair_weight = rng.uniform(0.0, 1.0, pair_row.size).astype(F32)
    seg_start = np.concatenate([[0], np.cumsum(SEGMENTS)]).astype(np.int32)
    assert pair_row.size <= 4 * n and n % 64
    return pair_row, pair_weight, seg_start, rng.normal(size=(n, C)).astype(F32)


def adam_case(Cs, C, T, t, R=8, seed=21):
    """-> dict: planes [R,R,Cs], m, v [R,R,C], seg_texel [T] (no texel twice, two entries out of range when T > 4), grad [T,C], lr, lo, hi [C],
    beta1, beta2, eps, t.  The step size is large enough for both clamps to act; t = 1 starts from zero moments."""
    rng = np.random.default_rng(seed + 7 * Cs + C + T + t)
    planes = rng.uniform(0.0, 1.0, (R, R, Cs)).astype(F32)
    m = (rng.normal(size=(R, R, C)) * 1e-2 * (t > 1)).astype(F32)
    v = (rng.uniform(0.0, 1e-3, (R, R, C)) * (t > 1)).astype(F32)
    seg_texel = np.sort(rng.choice(R * R, T, replace=False)).astype(np.int32)
    if T > 4:
        seg_texel[0], seg_texel[-1] = -1, R * R
    grad = (rng.normal(size=(T, C)) * 1e-2).astype(F32)
    lr = np.linspace(0.3, 0.05, C)
    return dict(planes=planes, m=m, v=v, seg_texel=seg_texel, grad=grad, lr=lr, lo=np.full(C, 0.25), hi=np.linspace(0.7, 0.9, C),
                beta1=0.9, beta2=0.999, eps=1e-8, t=t)


ADAM_CASES = ((8, 4, 37, 1), (8, 4, 37, 1000), (8, 4, 1, 1), (4, 4, 64, 1000), (16, 16, 5, 3), (1, 1, 64, 1))       # (Cs, C, T, t)


# ----------------------------------------------------------------------------------------- the closed loop's scene
LOOP = dict(R=64, H=32, W=32, views=4, steps=50, lr=0.02, betas=(0.9, 0.999), eps=1e-8, lo=(0.0, 0.0, 0.0, 0.02), hi=(1.0, 1.0, 1.0, 1.0),
            cull=1, lobes=16, noise=0.2, seed=11)
ANGLES = ((0.37, -0.52, 0.21), (-0.45, 0.9, 0.1), (0.2, 2.3, -0.3), (-0.3, -2.0, 0.15))       # four cameras around the ball


@functools.lru_cache(maxsize=None)
def loop_scene():
    """An 80-face icosphere with the per-face atlas at R = 64, four rotated cameras at 32 x 32 (cull = 1), a 16-lobe light, a smooth truth
    atlas and the start: the truth plus uniform +-0.2 noise on albedo and roughness, clipped to [0.05, 0.95].  Geometry rows come from the
    fp32 restatement of the rasteriser and the G-buffer, which the device reproduces bit for bit.  Computed once; never modified."""
    from robir_amd import synth
    L = LOOP
    R, H, W = L["R"], L["H"], L["W"]
    v, f = mr.icosphere(1)
    uv = tr.atlas_uv(80, R)
    vn = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)
    _, _, K = synth.synth_camera(H, W)
    poses = np.stack([mr.rotated_pose(angles=a) for a in ANGLES])
    rr, cc = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    s, t = rr / R * 2 * np.pi, cc / R * 2 * np.pi
    truth = np.zeros((R, R, 8), dtype=F32)
    truth[..., 0] = 0.5 + 0.3 * np.sin(s) * np.cos(t)
    truth[..., 1] = 0.5 + 0.3 * np.cos(2 * s + 0.5)
    truth[..., 2] = 0.5 + 0.3 * np.sin(t + 1.0) * np.sin(s)
    truth[..., 3] = 0.5 + 0.3 * np.cos(s - t)
    rng = np.random.default_rng(L["seed"])
    start = truth.copy()
    start[..., :4] = np.clip(truth[..., :4] + rng.uniform(-L["noise"], L["noise"], (R, R, 4)), 0.05, 0.95).astype(F32)
    rows = []
    for pose in poses:
        face_id, bary, _ = mr.raster(mr.project(v, mr.pose_inverse(pose), K), f, H, W, cull=L["cull"])
        idx = np.nonzero(face_id.reshape(-1) >= 0)[0]
        g = mr.gbuffer(face_id, bary, f, v, uv, pose[:3, 3], vnormals=vn, index=idx)
        rows.append(dict(idx=idx, **g))
    light = synth.synth_light_sgs(0, L["lobes"]).astype(F32)
    return dict(v=v, f=f, uv=uv, vn=vn, K=K, poses=poses, truth=truth, start=start, rows=rows, light=light)


def loop_rows(scene):
    """The rows of all views concatenated in view order -> dict of float32 arrays: normal, view_dir [n,3], uv [n,2]."""
    return {k: np.concatenate([r[k] for r in scene["rows"]]) for k in ("normal", "view_dir", "uv")}


def fit_loop64(scene, target, rows=None, steps=None):
    """The fit in float64 torch on the CPU (rows: normal, view_dir [n,3], uv [n,2] of the hit rows, default loop_rows): fetch by these taps,
    sg_backward_oracle.shade (direct shading: no visibility), pred = x / (x + 1),
    loss = sum (pred - target)^2 / n, autograd to the fetched albedo and roughness, the transpose into a dense gradient, lazy Adam with the
    clamp on the touched texels.  target [n,3]: the colours at the hit rows.  -> (loss history [steps], planes [R,R,8] float64, touched
    [R,R] bool)."""
    import torch

    import sg_backward_oracle as sbo
    L = LOOP
    R, steps = L["R"], L["steps"] if steps is None else steps
    rows = loop_rows(scene) if rows is None else rows
    texel, weight = taps(rows["uv"], R, 1, dtype=F64)
    n = texel.shape[0]
    ok = torch.from_numpy(texel >= 0)
    tex_i = torch.from_numpy(np.clip(texel, 0, R * R - 1).astype(np.int64))
    w = torch.from_numpy(weight) * ok
    nrm, vd = torch.from_numpy(rows["normal"]).double(), torch.from_numpy(rows["view_dir"]).double()
    lgt, f0 = torch.from_numpy(scene["light"]).double(), torch.tensor([0.02], dtype=torch.float64)
    gt = torch.as_tensor(target).double().reshape(n, 3)
    planes = torch.from_numpy(scene["start"].astype(F64)).reshape(R * R, 8).clone()
    touched = torch.zeros(R * R, dtype=torch.bool)
    touched[tex_i[ok]] = True
    m, v2 = torch.zeros(R * R, 4, dtype=torch.float64), torch.zeros(R * R, 4, dtype=torch.float64)
    lo, hi = torch.tensor(L["lo"], dtype=torch.float64), torch.tensor(L["hi"], dtype=torch.float64)
    b1, b2 = L["betas"]
    hist = []
    for t in range(1, steps + 1):
        tex = (planes[tex_i, :4] * w[:, :, None]).sum(1)
        alb, rough = tex[:, :3].clone().requires_grad_(True), tex[:, 3].clone().requires_grad_(True)
        with torch.enable_grad():
            spec, diff = sbo.shade(nrm, vd, lgt, f0, rough, alb, torch.ones(n, dtype=torch.float64))
            x = spec + diff
            loss = ((x / (x + 1.0) - gt) ** 2).sum() / n
            g_alb, g_rough = torch.autograd.grad(loss, [alb, rough])
        hist.append(float(loss.detach()))
        g_tex = torch.cat([g_alb, g_rough[:, None]], 1)
        grad = torch.zeros(R * R, 4, dtype=torch.float64)
        grad.index_add_(0, tex_i.reshape(-1), (g_tex[:, None, :] * w[:, :, None]).reshape(-1, 4))
        mt = b1 * m[touched] + (1 - b1) * grad[touched]
        vt = b2 * v2[touched] + (1 - b2) * grad[touched] ** 2
        m[touched], v2[touched] = mt, vt
        step = L["lr"] * (mt / (1 - b1 ** t)) / (torch.sqrt(vt / (1 - b2 ** t)) + L["eps"])
        planes[touched, :4] = torch.minimum(torch.maximum(planes[touched, :4] - step, lo), hi)
    return hist, planes.reshape(R, R, 8).numpy(), touched.reshape(R, R).numpy()
