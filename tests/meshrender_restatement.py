"""numpy restatement of librobir_hip_raster.so (include/robir_hip_raster.h, robir_amd/csrc/raster/raster_math.h): the same operations in the
same order, one rounding each, so that with dtype float32 every kernel is reproduced BIT FOR BIT.  With dtype float64 the same rule is
the reference path of the end-to-end test: rasteriser and G-buffer in double precision, independent of the kernels' rounding.  Also the
meshes, cameras and cases shared by the CPU and the GPU tests."""
import numpy as np

F32 = np.float32
TILE = 8
NEAR = 1e-4


# ----------------------------------------------------------------------------------------- raster_math.h
def project(vertices, pose_inv, K, dtype=F32):
    """vertices [V,3] -> screen [V,4] = (u, v, w, zc)."""
    x, P, K = np.asarray(vertices, dtype=dtype).reshape(-1, 3), np.asarray(pose_inv, dtype=dtype), np.asarray(K, dtype=dtype)
    with np.errstate(all="ignore"):
        row = [((P[i, 0] * x[:, 0] + P[i, 1] * x[:, 1]) + P[i, 2] * x[:, 2]) + P[i, 3] for i in range(3)]
        zc = -row[2]
        qx, qy = row[0] / zc, -row[1] / zc
        u = (K[0, 0] * qx + K[0, 1] * qy) + K[0, 2]
        v = (K[1, 0] * qx + K[1, 1] * qy) + K[1, 2]
        w = dtype(1.0) / zc
    return np.stack([u, v, w, zc], -1).astype(dtype)


class Face:
    """One face ready for its pixels: s [3,4], the corners' (u, v, w, zc)."""

    def __init__(self, s, H, W, near=NEAR, cull=0, dtype=F32):
        s = np.asarray(s, dtype=dtype).reshape(3, 4)
        self.dtype, self.s = dtype, s
        self.px, self.py, self.qx, self.qy, self.sg = (np.zeros(3, dtype=dtype) for _ in range(5))
        for k in range(3):
            a, b = s[(k + 1) % 3], s[(k + 2) % 3]
            swap = bool(b[0] < a[0] or (b[0] == a[0] and b[1] < a[1]))
            p, q = (b, a) if swap else (a, b)
            self.px[k], self.py[k], self.qx[k], self.qy[k], self.sg[k] = p[0], p[1], q[0], q[1], -1.0 if swap else 1.0
        self.w = s[:, 2].copy()
        with np.errstate(all="ignore"):
            self.area = dtype(self.edge(2, s[2, 0], s[2, 1]))
        self.c0 = self.r0 = 0
        self.c1 = self.r1 = -1
        near = dtype(F32(near))
        for k in range(3):
            if not s[k, 3] > near:
                return
            if not np.isfinite(s[k, :3]).all():
                return
        if not (self.area != 0 and np.isfinite(self.area)):
            return
        if (cull == 1 and self.area < 0) or (cull == 2 and self.area > 0):
            return
        zero = dtype(0.0)
        c0, c1 = max(np.ceil(s[:, 0].min()), zero), min(np.floor(s[:, 0].max()), dtype(W - 1))
        r0, r1 = max(np.ceil(s[:, 1].min()), zero), min(np.floor(s[:, 1].max()), dtype(H - 1))
        if not (c0 <= c1 and r0 <= r1):
            return
        self.c0, self.c1, self.r0, self.r1 = int(c0), int(c1), int(r0), int(r1)

    def edge(self, k, x, y):
        return self.sg[k] * ((self.qx[k] - self.px[k]) * (y - self.py[k]) - (self.qy[k] - self.py[k]) * (x - self.px[k]))

    @property
    def empty(self):
        return self.c0 > self.c1

    def tiles(self):
        if self.empty:
            return []
        return [(ty, tx) for ty in range(self.r0 // TILE, self.r1 // TILE + 1) for tx in range(self.c0 // TILE, self.c1 // TILE + 1)]

    def sample(self):
        """(rows, cols, covered [h,w], d [h,w], b0 [h,w], b1 [h,w]) over the pixel box."""
        dt = self.dtype
        rows, cols = np.arange(self.r0, self.r1 + 1), np.arange(self.c0, self.c1 + 1)
        x, y = cols.astype(dt)[None, :], rows.astype(dt)[:, None]
        with np.errstate(all="ignore"):
            e0, e1, e2 = self.edge(0, x, y), self.edge(1, x, y), self.edge(2, x, y)
            s = dt(1.0) if self.area > 0 else dt(-1.0)
            cov = (s * e0 >= 0) & (s * e1 >= 0) & (s * e2 >= 0)
            l0, l1 = e0 / self.area, e1 / self.area
            l2 = (dt(1.0) - l0) - l1
            t0, t1 = l0 * self.w[0], l1 * self.w[1]
            d = (t0 + t1) + l2 * self.w[2]
            b0, b1 = t0 / d, t1 / d
        return rows, cols, cov, d.astype(dt), b0.astype(dt), b1.astype(dt)


def _faces(screen, faces, H, W, near, cull, dtype):
    screen, faces = np.asarray(screen, dtype=dtype).reshape(-1, 4), np.asarray(faces).reshape(-1, 3)
    V = screen.shape[0]
    nan = np.full((3, 4), np.nan, dtype=dtype)
    for f, idx in enumerate(faces):
        ok = all(0 <= int(i) < V for i in idx)
        yield f, Face(screen[idx] if ok else nan, H, W, near, cull, dtype)


def bin_counts(screen, faces, H, W, near=NEAR, cull=0):
    return np.array([len(face.tiles()) for _, face in _faces(screen, faces, H, W, near, cull, F32)], dtype=np.int32)


def bin_pairs(screen, faces, H, W, near=NEAR, cull=0):
    """(pair_tile, pair_face) in face order, a face's tiles row-major."""
    ntx = (W + TILE - 1) // TILE
    pt, pf = [], []
    for f, face in _faces(screen, faces, H, W, near, cull, F32):
        for ty, tx in face.tiles():
            pt.append(ty * ntx + tx)
            pf.append(f)
    return np.array(pt, dtype=np.int32), np.array(pf, dtype=np.int32)


def raster(screen, faces, H, W, near=NEAR, cull=0, dtype=F32):
    """-> (face_id [H,W] int32, bary [H,W,2], depth [H,W]): faces in ascending index, the largest d > 0 wins, an equal d stays."""
    face_id = np.full((H, W), -1, dtype=np.int32)
    bary, best = np.zeros((H, W, 2), dtype=dtype), np.zeros((H, W), dtype=dtype)
    for f, face in _faces(screen, faces, H, W, near, cull, dtype):
        if face.empty:
            continue
        rows, cols, cov, d, b0, b1 = face.sample()
        box = (slice(rows[0], rows[-1] + 1), slice(cols[0], cols[-1] + 1))
        with np.errstate(all="ignore"):
            take = cov & (d > best[box])
        face_id[box][take] = f
        best[box][take] = d[take]
        bary[box][..., 0][take] = b0[take]
        bary[box][..., 1][take] = b1[take]
    with np.errstate(all="ignore"):
        depth = np.where(face_id >= 0, dtype(1.0) / best, dtype(0.0)).astype(dtype)
    return face_id, bary, depth


def _unit(v, dtype):
    with np.errstate(all="ignore"):
        n = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        return (v / np.maximum(n, dtype(1e-12))[:, None]).astype(dtype)


def fetch_nearest(planes, u, v, dtype=F32):
    R = planes.shape[0]
    fr, lim = dtype(R), dtype(R - 1)
    with np.errstate(all="ignore"):
        c = np.minimum(np.maximum(np.floor(u * fr), dtype(0.0)), lim)
        r = np.minimum(np.maximum(np.floor((dtype(1.0) - v) * fr), dtype(0.0)), lim)
    c, r = np.nan_to_num(c, nan=0.0).astype(np.int64), np.nan_to_num(r, nan=0.0).astype(np.int64)
    return planes[r, c]


def fetch_bilinear(planes, u, v, dtype=F32):
    """rb_tb_sample's fetch: x = u R - 0.5, y = (1 - v) R - 0.5, zero padding, products added in the order nw, ne, sw, se."""
    R, C = planes.shape[0], planes.shape[2]
    fr, half, one = dtype(R), dtype(0.5), dtype(1.0)
    with np.errstate(all="ignore"):
        x, y = u * fr - half, (one - v) * fr - half
        x0, y0 = np.floor(x), np.floor(y)
        wx1, wx0, wy1, wy0 = x - x0, (x0 + one) - x, y - y0, (y0 + one) - y
        nw, ne, sw, se = wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1
        c0 = np.nan_to_num(np.clip(x0, -2.0, R + 1.0), nan=-2.0).astype(np.int64)
        r0 = np.nan_to_num(np.clip(y0, -2.0, R + 1.0), nan=-2.0).astype(np.int64)

        def tap(r, c):
            ok = (r >= 0) & (r < R) & (c >= 0) & (c < R)
            val = planes[np.clip(r, 0, R - 1), np.clip(c, 0, R - 1)]
            return np.where(ok[:, None], val, dtype(0.0)).astype(dtype)

        a, b, c, d = tap(r0, c0), tap(r0, c0 + 1), tap(r0 + 1, c0), tap(r0 + 1, c0 + 1)
        return (((a * nw[:, None] + b * ne[:, None]) + c * sw[:, None]) + d * se[:, None]).astype(dtype)


def gbuffer(face_id, bary, faces, vertices, uv, cam, planes=None, filter=1, vnormals=None, index=None, dtype=F32):
    """-> dict position [n,3], uv [n,2], view_dir [n,3], tex [n,C], normal [n,3]; zeros on rows without a valid face."""
    fid = np.asarray(face_id).reshape(-1)
    bar = np.asarray(bary, dtype=dtype).reshape(-1, 2)
    faces, vertices = np.asarray(faces).reshape(-1, 3).astype(np.int64), np.asarray(vertices, dtype=dtype).reshape(-1, 3)
    uv, cam = np.asarray(uv, dtype=dtype).reshape(-1, 3, 2), np.asarray(cam, dtype=dtype).reshape(3)
    t = np.arange(fid.size) if index is None else np.asarray(index).astype(np.int64)
    n, F, V = t.size, faces.shape[0], vertices.shape[0]
    tin = (t >= 0) & (t < fid.size)
    f = np.where(tin, fid[np.clip(t, 0, fid.size - 1)], -1)
    ok = (f >= 0) & (f < F)
    fc = np.clip(f, 0, max(F - 1, 0))
    vi = faces[fc] if F else np.zeros((n, 3), dtype=np.int64)
    ok &= ((vi >= 0) & (vi < V)).all(-1)
    vi = np.clip(vi, 0, max(V - 1, 0))
    b = bar[np.clip(t, 0, fid.size - 1)]
    one = dtype(1.0)
    with np.errstate(all="ignore"):
        b0, b1 = b[:, 0:1], b[:, 1:2]
        b2 = (one - b0) - b1
        mix = lambda A, B, C: ((b0 * A + b1 * B) + b2 * C).astype(dtype)
        pos = mix(vertices[vi[:, 0]], vertices[vi[:, 1]], vertices[vi[:, 2]])
        q = mix(uv[fc, 0], uv[fc, 1], uv[fc, 2])
        vd = _unit((cam[None, :] - pos).astype(dtype), dtype)
    z = lambda a: np.where(ok[:, None], a, dtype(0.0)).astype(dtype)
    out = {"position": z(pos), "uv": z(q), "view_dir": z(vd)}
    if planes is not None:
        planes = np.asarray(planes, dtype=dtype)
        out["tex"] = z((fetch_nearest if filter == 0 else fetch_bilinear)(planes, q[:, 0], q[:, 1], dtype))
    if vnormals is not None:
        vn = np.asarray(vnormals, dtype=dtype).reshape(-1, 3)
        with np.errstate(all="ignore"):
            out["normal"] = z(_unit(mix(vn[vi[:, 0]], vn[vi[:, 1]], vn[vi[:, 2]]), dtype))
    return out


# ----------------------------------------------------------------------------------------- meshes, cameras, rays
def icosphere(subdivisions, radius=0.25):
    """(vertices [V,3] float32, faces [F,3] int32), outward winding (counter-clockwise seen from outside): 20 * 4^subdivisions faces."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(int(subdivisions)):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius).astype(F32), np.asarray(f, dtype=np.int32)


def rotated_pose(distance=0.9, angles=(0.37, -0.52, 0.21), offset=(0.03, -0.02, 0.0)):
    """A camera-to-world pose that is not axis-aligned: synth_camera's (identity rotation, centre on +z) turned about x, y and z, the camera
    still facing the origin up to `offset` (in camera units, so the object is off the image centre)."""
    ax, ay, az = angles
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    R = Rz @ Ry @ Rx
    pose = np.eye(4)
    pose[:3, :3] = R
    pose[:3, 3] = R @ (np.array([0.0, 0.0, distance]) + np.asarray(offset, dtype=np.float64))
    return pose.astype(F32)


def pose_inverse(pose):
    """As robir_amd/observe.py forms it (torch.inverse of the 4 x 4 matrix), here through numpy in double, rounded once to float32."""
    p = np.eye(4)
    p[:3, :4] = np.asarray(pose, dtype=np.float64)[:3, :4]
    return np.linalg.inv(p).astype(F32)


def pixel_rays(pose, K, H, W):
    """float64: (cam [3], unnormalised world directions [H,W,3] of the pixels' sample points (u, v) = (c, r), scaled so that the component
    along the viewing axis is 1: a point at distance `depth` along the axis is cam + depth * ray)."""
    pose, K = np.asarray(pose, dtype=np.float64), np.asarray(K, dtype=np.float64)
    c, r = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    yl = (r - K[1, 2]) / K[1, 1]
    xl = (c - K[0, 2] - K[0, 1] * yl) / K[0, 0]
    local = np.stack([xl, -yl, -np.ones_like(xl)], -1)
    return pose[:3, 3].copy(), local @ pose[:3, :3].T


def ray_ball(cam, rays, radius):
    """(hit [..] bool, t [..]: the first intersection of cam + t ray with the ball of `radius` about the origin; rays unnormalised)."""
    a = (rays * rays).sum(-1)
    b = 2.0 * (rays * cam).sum(-1)
    c = float((cam * cam).sum()) - radius * radius
    disc = b * b - 4.0 * a * c
    hit = disc > 0
    t = (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2.0 * a)
    return hit & (t > 0), t


# ----------------------------------------------------------------------------------------- cases shared by the CPU and the GPU tests
def ortho_screen(points):
    """Screen vertices given directly: points [V,3] = (u, v, zc) -> [V,4] = (u, v, 1 / zc, zc) in float32 (NaN / non-positive zc pass)."""
    p = np.asarray(points, dtype=F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([p[:, 0], p[:, 1], F32(1.0) / p[:, 2], p[:, 2]], -1).astype(F32)


def raster_cases():
    """name -> (screen [V,4], faces [F,3], H, W): the shapes at which the rasteriser can go wrong, all small."""
    rng = np.random.default_rng(7)
    cases = {}
    # 200 small triangles at different depths inside one tile (rows / columns 8 .. 15 of a 13 x 21 image): four batches of 64, depth
    # order across batches; the deepest-last and nearest-last orders both occur
    n = 200
    ctr = rng.uniform(8.5, 14.5, (n, 1, 2))
    ctr[:, :, 1] = rng.uniform(8.2, 12.4, (n, 1))
    tri = ctr + rng.uniform(-2.5, 2.5, (n, 3, 2))
    z = rng.uniform(0.5, 3.0, (n, 3, 1))
    cases["tile200"] = (ortho_screen(np.concatenate([tri, z], -1).reshape(-1, 3)), np.arange(3 * n, dtype=np.int32).reshape(n, 3), 13, 21)
    # two coincident faces (the lower index wins), then a nearer one over part of them
    q = [(2, 2, 1.0), (11, 3, 1.5), (4, 10, 2.0)]
    cases["coincident"] = (ortho_screen(q + q + [(3, 3, 0.9), (8, 3, 0.9), (3, 8, 0.9)]),
                           np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], dtype=np.int32), 13, 21)
    # a shared edge through pixel centres (integer screen coordinates), the two faces named with opposite windings of the edge
    sq = [(2, 1, 1.0), (12, 1, 1.3), (12, 11, 1.1), (2, 11, 0.8)]
    cases["shared_edge"] = (ortho_screen(sq), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32), 13, 21)
    cases["shared_edge_mixed"] = (ortho_screen(sq), np.array([[0, 1, 2], [2, 3, 0]], dtype=np.int32), 13, 21)
    # partly off-screen, wholly off-screen, behind the camera (one corner / all corners), NaN, zero area, an index out of range
    v = [(-5, -4, 1.0), (9, 3, 1.0), (2, 16, 1.0),            # partly off
         (30, 30, 1.0), (40, 30, 1.0), (30, 44, 1.0),         # wholly off
         (1, 1, -1.0), (9, 2, 1.0), (3, 9, 1.0),              # one corner behind
         (1, 1, -1.0), (9, 2, -2.0), (3, 9, -0.5),            # all behind
         (np.nan, 1, 1.0), (9, 2, 1.0), (3, 9, 1.0),          # NaN coordinate
         (4, 4, 1.0), (6, 6, 1.0), (8, 8, 1.0),               # zero area
         (15, 2, 2.0), (20, 2, 2.0), (15, 9, 2.0),            # an ordinary face at the right border
         (1, 1, 5e-5), (9, 2, 1.0), (3, 9, 1.0),              # a corner inside the near plane
         (14, 5, np.inf), (20, 6, 1.0), (16, 12, 1.0)]        # zc = inf: w = 0, finite -- drawn
    f = [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 13, 14], [15, 16, 17], [18, 19, 20], [21, 22, 23], [24, 25, 26], [0, 1, 99]]
    cases["edge_cases"] = (ortho_screen(v), np.array(f, dtype=np.int32), 13, 21)
    # both windings side by side, for cull
    cases["windings"] = (ortho_screen([(1, 1, 1.0), (9, 1, 1.0), (1, 9, 1.0), (11, 2, 1.0), (11, 10, 1.0), (19, 2, 1.0)]),
                         np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32), 13, 21)
    return cases


def gbuffer_case(H=13, W=21, R=8, C=8, seed=3):
    """A small scene for the G-buffer: screen, faces, vertices, per-corner uv (texel centres among them), planes [R,R,C], vertex normals."""
    rng = np.random.default_rng(seed)
    verts = np.array([(-0.3, -0.2, 0.0), (0.3, -0.25, 0.05), (0.0, 0.3, -0.05), (0.35, 0.3, 0.1)], dtype=F32)
    faces = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32)
    centre = lambda c, r: ((c + 0.5) / R, 1.0 - (r + 0.5) / R)
    uv = np.array([[centre(1, 1), centre(6, 2), centre(3, 6)], [(0.02, 0.98), (1.0, 0.0), (0.55, 0.45)]], dtype=F32)
    planes = rng.uniform(0.05, 1.0, (R, R, C)).astype(F32)
    vn = rng.normal(size=(4, 3)).astype(F32)
    return verts, faces, uv, planes, vn
