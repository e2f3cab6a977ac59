"""numpy fp32 restatement of librobir_hip_texbake.so (include/robir_hip_texbake.h, robir_amd/csrc/texbake/texbake_math.h): the same operations
in the same order, one rounding each, so that every kernel is reproduced BIT FOR BIT -- plus independently written float64 forms of the
dilation and the sampler, the atlas properties and the raster cases shared by the CPU and the GPU tests."""
import math

import numpy as np

F32 = np.float32
TILE = 8
HALF, ONE, ZERO = F32(0.5), F32(1.0), F32(0.0)


# ----------------------------------------------------------------------------------------- texbake_math.h
def edge_fn(ax, ay, bx, by, x, y):
    """(qx - px)(y - py) - (qy - py)(x - px) from the endpoint that sorts first by (x, then y), negated when a -> b names it backwards."""
    ax, ay, bx, by = F32(ax), F32(ay), F32(bx), F32(by)
    swap = bool(bx < ax or (bx == ax and by < ay))
    px, py, qx, qy = (bx, by, ax, ay) if swap else (ax, ay, bx, by)
    with np.errstate(all="ignore"):
        e = (qx - px) * (y - py) - (qy - py) * (x - px)
    return -e if swap else e


class Face:
    def __init__(self, uv, R):
        uv = np.asarray(uv, dtype=F32).reshape(3, 2)
        fr = F32(R)
        with np.errstate(all="ignore"):
            self.x = uv[:, 0] * fr
            self.y = (ONE - uv[:, 1]) * fr
            self.area = F32(edge_fn(self.x[0], self.y[0], self.x[1], self.y[1], self.x[2], self.y[2]))
        self.c0 = self.r0 = 0
        self.c1 = self.r1 = -1
        if not (self.area != 0 and np.isfinite(self.area)):
            return
        lim = F32(R - 1)
        c0, c1 = max(np.ceil(self.x.min() - HALF), ZERO), min(np.floor(self.x.max() - HALF), lim)
        r0, r1 = max(np.ceil(self.y.min() - HALF), ZERO), min(np.floor(self.y.max() - HALF), lim)
        if not (c0 <= c1 and r0 <= r1):
            return
        self.c0, self.c1, self.r0, self.r1 = int(c0), int(c1), int(r0), int(r1)

    @property
    def empty(self):
        return self.c0 > self.c1

    def tiles(self):
        """The tile indices ty * ntiles + tx of the texel box in row-major order, given ntiles by the caller."""
        if self.empty:
            return []
        return [(ty, tx) for ty in range(self.r0 // TILE, self.r1 // TILE + 1) for tx in range(self.c0 // TILE, self.c1 // TILE + 1)]

    def cover(self):
        """(rows, cols, covered [h,w] bool, b0 [h,w], b1 [h,w]) over the texel box."""
        rows, cols = np.arange(self.r0, self.r1 + 1), np.arange(self.c0, self.c1 + 1)
        x = (cols.astype(F32) + HALF)[None, :]
        y = (rows.astype(F32) + HALF)[:, None]
        X, Y = self.x, self.y
        with np.errstate(all="ignore"):
            e0 = edge_fn(X[1], Y[1], X[2], Y[2], x, y)
            e1 = edge_fn(X[2], Y[2], X[0], Y[0], x, y)
            e2 = edge_fn(X[0], Y[0], X[1], Y[1], x, y)
            s = ONE if self.area > 0 else F32(-1.0)
            cov = (s * e0 >= 0) & (s * e1 >= 0) & (s * e2 >= 0)
            b0, b1 = (e0 / self.area).astype(F32), (e1 / self.area).astype(F32)
        shape = (rows.size, cols.size)
        return rows, cols, np.broadcast_to(cov, shape), np.broadcast_to(b0, shape), np.broadcast_to(b1, shape)


def bin_counts(uv, R):
    return np.array([len(Face(t, R).tiles()) for t in np.asarray(uv, dtype=F32).reshape(-1, 3, 2)], dtype=np.int32)


def bin_pairs(uv, R):
    """(pair_tile, pair_face) in face order, a face's tiles row-major."""
    ntiles = (R + TILE - 1) // TILE
    pt, pf = [], []
    for f, t in enumerate(np.asarray(uv, dtype=F32).reshape(-1, 3, 2)):
        for ty, tx in Face(t, R).tiles():
            pt.append(ty * ntiles + tx)
            pf.append(f)
    return np.array(pt, dtype=np.int32), np.array(pf, dtype=np.int32)


def raster(uv, R):
    """-> (face_id [R,R] int32, bary [R,R,2] float32): faces in ascending index, the first that covers a texel centre owns it."""
    face_id = np.full((R, R), -1, dtype=np.int32)
    bary = np.zeros((R, R, 2), dtype=F32)
    for f, t in enumerate(np.asarray(uv, dtype=F32).reshape(-1, 3, 2)):
        face = Face(t, R)
        if face.empty:
            continue
        rows, cols, cov, b0, b1 = face.cover()
        box = (slice(rows[0], rows[-1] + 1), slice(cols[0], cols[-1] + 1))
        take = cov & (face_id[box] < 0)
        face_id[box][take] = f
        bary[box][..., 0][take] = b0[take]
        bary[box][..., 1][take] = b1[take]
    return face_id, bary


# ----------------------------------------------------------------------------------------- the atlas
def atlas_ncols(F):
    cells = (F + 1) // 2
    n = math.isqrt(cells)
    return max(1, n if n * n == cells else n + 1)


def atlas_cell(F, R):
    if F < 1:
        raise ValueError("an atlas needs at least one face")
    ncols = atlas_ncols(F)
    S = R // ncols
    if S < 6:
        raise ValueError(f"resolution {R} gives cells of {S} texels: the smallest resolution at which every face owns a texel is {6 * ncols}")
    return S


def atlas_uv(F, R):
    S, ncols = atlas_cell(F, R), atlas_ncols(F)
    f = np.arange(F)
    cell, odd = f >> 1, (f & 1).astype(bool)
    x0, y0, s = ((cell % ncols) * S).astype(F32), ((cell // ncols) * S).astype(F32), F32(S)
    uv = np.zeros((F, 3, 2), dtype=F32)
    for k in range(3):
        lx = np.where(odd, F32(3.5) if k == 1 else s - ONE, s - F32(3.5) if k == 1 else ONE).astype(F32)
        ly = np.where(odd, F32(3.5) if k == 2 else s - ONE, s - F32(3.5) if k == 2 else ONE).astype(F32)
        uv[:, k, 0] = (x0 + lx) / F32(R)
        uv[:, k, 1] = ONE - (y0 + ly) / F32(R)
    return uv


def owners(uv, R):
    """[R,R] int: how many faces cover each texel centre (the ownership count behind face_id)."""
    n = np.zeros((R, R), dtype=np.int32)
    for t in np.asarray(uv, dtype=F32).reshape(-1, 3, 2):
        face = Face(t, R)
        if not face.empty:
            rows, cols, cov, _, _ = face.cover()
            n[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1] += cov
    return n


def gutter_is_clean(face_id):
    """No uncovered texel is 8-adjacent to covered texels of two different faces."""
    fid = np.asarray(face_id).astype(np.int64)
    H, W = fid.shape
    pad = np.full((H + 2, W + 2), -1, dtype=np.int64)
    pad[1:-1, 1:-1] = fid
    big = np.iinfo(np.int64).max
    lo, hi = np.full((H, W), big), np.full((H, W), -1, dtype=np.int64)
    for dr in range(3):
        for dc in range(3):
            if (dr, dc) != (1, 1):
                nb = pad[dr:dr + H, dc:dc + W]
                lo = np.where(nb >= 0, np.minimum(lo, nb), lo)
                hi = np.maximum(hi, nb)
    return not bool(((fid < 0) & (hi >= 0) & (lo != hi)).any())


# ----------------------------------------------------------------------------------------- interpolation, dilation
def interp(face_id, bary, faces, attr, index=None):
    fid, b = np.asarray(face_id).reshape(-1), np.asarray(bary, dtype=F32).reshape(-1, 2)
    attr, faces = np.asarray(attr, dtype=F32), np.asarray(faces).reshape(-1, 3)
    if index is not None:
        fid, b = fid[index], b[index]
    ok = fid >= 0
    v = faces[np.where(ok, fid, 0)] if faces.shape[0] else np.zeros((fid.size, 3), dtype=np.int64)
    b0, b1 = b[:, 0:1], b[:, 1:2]
    with np.errstate(all="ignore"):
        b2 = (ONE - b0) - b1
        out = (b0 * attr[v[:, 0]] + b1 * attr[v[:, 1]]) + b2 * attr[v[:, 2]] if attr.shape[0] else np.zeros((fid.size, attr.shape[1]), F32)
    out = np.where(ok[:, None], out, ZERO).astype(F32)
    return out if index is not None else out.reshape(*np.asarray(face_id).shape, attr.shape[1])


def dilate(image, mask):
    """One ring, fp32: -> (image', mask' uint8)."""
    img, m = np.asarray(image, dtype=F32), np.asarray(mask) != 0
    H, W, C = img.shape
    pi = np.zeros((H + 2, W + 2, C), dtype=F32)
    pm = np.zeros((H + 2, W + 2), dtype=bool)
    pi[1:-1, 1:-1], pm[1:-1, 1:-1] = img, m
    total, count = np.zeros((H, W, C), dtype=F32), np.zeros((H, W), dtype=np.int32)
    with np.errstate(all="ignore"):
        for dr in range(3):
            for dc in range(3):
                if (dr, dc) == (1, 1):
                    continue
                nm = pm[dr:dr + H, dc:dc + W]
                total = total + np.where(nm[..., None], pi[dr:dr + H, dc:dc + W], ZERO)
                count = count + nm
        grow = ~m & (count > 0)
        mean = total / np.maximum(count, 1).astype(F32)[..., None]
    out = np.where(grow[..., None], mean, img).astype(F32)
    mo = np.where(m, np.asarray(mask).astype(np.uint8), grow.astype(np.uint8)).astype(np.uint8)
    return out, mo


def dilate64(image, mask):
    """The same ring written texel by texel in float64 (the independent form)."""
    img, m = np.asarray(image, dtype=np.float64), np.asarray(mask) != 0
    H, W, _ = img.shape
    out, mo = img.copy(), m.copy()
    for r in range(H):
        for c in range(W):
            if m[r, c]:
                continue
            nb = [img[rr, cc] for rr in (r - 1, r, r + 1) for cc in (c - 1, c, c + 1)
                  if (rr, cc) != (r, c) and 0 <= rr < H and 0 <= cc < W and m[rr, cc]]
            if nb:
                out[r, c] = np.sum(nb, axis=0) / len(nb)
                mo[r, c] = True
    return out, mo


# ----------------------------------------------------------------------------------------- the sampler
def _fetch(img, x, y, dt):
    """grid_sample, bilinear, zeros padding, align_corners=False, at texel coordinates: img [R,R,C], x, y [n] of dtype dt."""
    R = img.shape[0]
    one = dt(1.0)
    x0, y0 = np.floor(x), np.floor(y)
    wx1, wx0, wy1, wy0 = x - x0, (x0 + one) - x, y - y0, (y0 + one) - y
    c0, r0 = np.clip(x0, -2, R + 1).astype(np.int64), np.clip(y0, -2, R + 1).astype(np.int64)
    pad = np.zeros((R + 4, R + 4, img.shape[2]), dtype=dt)
    pad[2:R + 2, 2:R + 2] = img
    g = lambda r, c: pad[np.clip(r + 2, 0, R + 3), np.clip(c + 2, 0, R + 3)]
    w = lambda a: a[:, None]
    return ((g(r0, c0) * w(wx0 * wy0) + g(r0, c0 + 1) * w(wx1 * wy0)) + g(r0 + 1, c0) * w(wx0 * wy1)) + g(r0 + 1, c0 + 1) * w(wx1 * wy1)


def _unit(v, dt):
    n = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return v / np.maximum(n, dt(1e-4))[:, None]


def sample(position, normal, mask, uv, scale=1.0, dt=F32):
    """rb_tb_sample in dtype dt: fp32 = the kernel bit for bit; float64 = the reference for the parity rule (inputs stay the fp32 values).
    Returns x, normal, object_mask, tangent_u, tangent_v and the fetched mask value."""
    pos, nrm, msk = (np.asarray(a, dtype=F32).astype(dt) for a in (position, normal, mask))
    uv = np.asarray(uv, dtype=F32).astype(dt)
    R = pos.shape[0]
    fr, half, one, d = dt(R), dt(0.5), dt(1.0), dt(F32(0.001))
    u, v = uv[:, 0], uv[:, 1]
    tx, ty = u * fr - half, (one - v) * fr - half
    txu, tyv = (u + d) * fr - half, (one - (v + d)) * fr - half
    p = _fetch(pos, tx, ty, dt)
    m = _fetch(msk[..., None], tx, ty, dt)[:, 0]
    return {"x": p * dt(F32(scale)), "normal": _unit(_fetch(nrm, tx, ty, dt), dt), "object_mask": m > dt(F32(0.1)),
            "tangent_u": _unit(_fetch(pos, tx, tyv, dt) - p, dt), "tangent_v": _unit(_fetch(pos, txu, ty, dt) - p, dt), "mask_value": m}


def sample_torch(position, normal, mask, uv, scale=1.0, dtype=None):
    """TexSampler.sample as the reference writes it (model/texture_model.py:135-160) on PyTorch's CPU grid_sample, with this project's UV
    convention (v up: grid y = 1 - 2 v) and scale: the independent form (float64) and the e_torch yardstick (float32)."""
    import torch
    import torch.nn.functional as Fn
    dtype = dtype or torch.float32
    chw = lambda a: torch.as_tensor(np.asarray(a, dtype=F32)).to(dtype).permute(2, 0, 1)[None]
    vert, norm = chw(position), chw(normal)
    msk = torch.as_tensor(np.asarray(mask, dtype=F32)).to(dtype)[None, None]
    uv = torch.as_tensor(np.asarray(uv, dtype=F32)).to(dtype)
    d = torch.tensor(float(F32(0.001)), dtype=dtype)

    def fetch(img, u, v):
        grid = torch.stack([u * 2 - 1, 1 - v * 2], -1).reshape(1, 1, -1, 2)
        return Fn.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False).reshape(img.shape[1], -1).permute(1, 0)

    unit = lambda t: t / torch.clamp(torch.norm(t, dim=-1, keepdim=True), min=1e-4)
    u, v = uv[:, 0], uv[:, 1]
    p = fetch(vert, u, v)
    m = fetch(msk, u, v).reshape(-1)
    out = {"x": p * float(F32(scale)), "normal": unit(fetch(norm, u, v)), "object_mask": m > float(F32(0.1)),
           "tangent_u": unit(fetch(vert, u, v + d) - p), "tangent_v": unit(fetch(vert, u + d, v) - p), "mask_value": m}
    return {k: t.numpy() for k, t in out.items()}


# ----------------------------------------------------------------------------------------- the raster cases
def _uv_of_texels(pts, R):
    """Texel-space points (x right, y down) -> uv float32."""
    p = np.asarray(pts, dtype=np.float64)
    return np.stack([p[..., 0] / R, 1.0 - p[..., 1] / R], -1).astype(F32)


def fan(variant):
    """(vt [10,2], faces_vt [9,3], R = 64): nine triangles (hub, rim k, rim k + 1) around a hub; face k names the shared edge rim k+1 -> hub,
    face k + 1 names it hub -> rim k+1."""
    R = 64
    k = np.arange(9)
    if variant == "irrational":
        ang = 2 * np.pi * k / 9 + 0.1 * np.sqrt(2.0) + 0.05 * np.sin(k * np.sqrt(3.0))
        hub = np.array([32.0 + np.sqrt(2.0) / 3, 32.0 - np.pi / 7])
        rim = hub + (27.0 + np.sqrt(5.0) * np.cos(k * np.e))[:, None] * np.stack([np.cos(ang), np.sin(ang)], -1)
    else:                                  # the hub on a texel centre, every rim corner on a half-texel lattice point
        ang = 2 * np.pi * k / 9 + 0.2
        hub = np.array([32.5, 32.5])
        rim = np.round(2 * (hub + 28.0 * np.stack([np.cos(ang), np.sin(ang)], -1))) / 2
    vt = _uv_of_texels(np.concatenate([hub[None], rim]), R)
    faces = np.stack([np.zeros(9, dtype=np.int64), 1 + k, 1 + (k + 1) % 9], -1).astype(np.int32)
    return vt, faces, R


def fan_interior(vt, R, margin=1e-2):
    """[R,R] bool in float64: texel centres inside the fan's union and more than `margin` texels from its outer boundary."""
    x, y = vt[:, 0].astype(np.float64) * R, (1.0 - vt[:, 1].astype(np.float64)) * R
    rim = np.stack([x[1:], y[1:]], -1)
    c = np.arange(R) + 0.5
    px, py = np.meshgrid(c, c)
    inside = np.zeros((R, R), dtype=bool)
    dist = np.full((R, R), np.inf)
    for k in range(9):
        a, b = rim[k], rim[(k + 1) % 9]
        tri = [(x[0], y[0]), tuple(a), tuple(b)]
        e = [(q[0] - p[0]) * (py - p[1]) - (q[1] - p[1]) * (px - p[0]) for p, q in zip(tri, tri[1:] + tri[:1])]
        inside |= (np.minimum.reduce(e) >= 0) | (np.maximum.reduce(e) <= 0)
        ab = b - a
        t = np.clip(((px - a[0]) * ab[0] + (py - a[1]) * ab[1]) / (ab @ ab), 0.0, 1.0)
        dist = np.minimum(dist, np.hypot(px - (a[0] + t * ab[0]), py - (a[1] + t * ab[1])))
    return inside & (dist > margin)


def raster_cases():
    """name -> (uv [F,3,2] float32, R)."""
    rng = np.random.default_rng(7)
    cases = {}
    q = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=F32)
    cases["quad_diagonal"] = (q[[[0, 1, 2], [0, 2, 3]]], 16)                      # the diagonal passes through texel centres
    cases["tiles_r20"] = (np.concatenate([_uv_of_texels([[[2.2, 1.3], [8.0, 2.1], [3.1, 7.6]]], 20),          # box ends on a tile boundary
                                          np.array([[[0.02, 0.03], [0.97, 0.05], [0.5, 0.98]]], dtype=F32),       # spans all tiles
                                          np.array([[[-0.3, 0.2], [0.3, -0.4], [0.25, 0.3]]], dtype=F32)]), 20)   # partly outside
    good = np.array([[0.1, 0.15], [0.9, 0.2], [0.45, 0.85]], dtype=F32)
    cases["degenerate_first"] = (np.stack([np.array([[0.2, 0.2], [0.5, 0.5], [0.8, 0.8]], dtype=F32),             # zero area
                                           np.array([[0.1, 0.1], [np.nan, 0.3], [0.4, 0.9]], dtype=F32),          # a NaN corner
                                           np.array([[0.3, 0.3], [0.3, 0.3], [0.3, 0.3]], dtype=F32),             # a point
                                           good]), 16)
    cases["good_alone"] = (good[None], 16)
    cases["slivers"] = (_uv_of_texels([[[1.2, 3.6], [14.7, 3.7], [8.1, 3.9]], [[1.1, 1.2], [14.2, 14.3], [14.25, 14.3]]], 16), 16)
    cases["overlap"] = (np.array([[[0.3, 0.3], [0.9, 0.35], [0.6, 0.9]], [[0.1, 0.1], [0.8, 0.2], [0.4, 0.8]],
                                  [[0.05, 0.5], [0.95, 0.05], [0.7, 0.95]]], dtype=F32), 24)
    ang = rng.uniform(0, 2 * np.pi, (200, 1)) + np.array([0.0, 2.1, 4.2]) + rng.uniform(-0.3, 0.3, (200, 3))     # rings around (4, 4) that grow
    pts = 4.0 + (0.6 + 3.2 * np.arange(200) / 199.0)[:, None, None] * np.stack([np.cos(ang), np.sin(ang)], -1)
    cases["crowded_tile"] = (_uv_of_texels(pts, 16), 16)                          # 200 faces in the 8 x 8 tile (0, 0)
    cases["no_faces"] = (np.zeros((0, 3, 2), dtype=F32), 16)
    for variant in ("irrational", "half_texel"):
        vt, faces, R = fan(variant)
        cases["fan_" + variant] = (vt[faces], R)
    return cases


ATLAS_CASES = ((1, 8), (2, 8), (3, 16), (7, 32), (200, 96), (200, 128))
