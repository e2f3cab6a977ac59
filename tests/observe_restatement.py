"""numpy restatement of librobir_hip_observe.so (include/robir_hip_observe.h, robir_amd/csrc/observe/observe_math.h): the same operations in
the same order, in float32 (what the kernels and the host build must reproduce bit for bit) or, with dt=np.float64, the form the accuracy
bounds are measured against.  Next to it, the reference's own lines (model/focus_sampler.py: F.normalize, the two matrix products,
F.grid_sample(align_corners=True); training/tex_module.py: torch.sort and the gathers) restated on PyTorch-CPU, and the seeded cases that
the CPU tests, the GPU tests and tools/check_observe_host.py share.

Conventions: x [N,3]; cam_loc [M,3], pose_inv [M,4,4], K [M,3,3]; images [M,H,W,C], masks [M,H,W]; a pixel position is (u, v) with u along
the W columns.  Every sum is associated from the left.
"""
import functools
import itertools

import numpy as np
import torch
import torch.nn.functional as F


# ----------------------------------------------------------------------------------------- the kernels' arithmetic
def project(x, cam_loc, pose_inv, K, dt=np.float32):
    """-> view_dir [M,N,3], uv [M,N,2], z [M,N]."""
    x, c, P, K = (np.asarray(a, dtype=dt) for a in (x, cam_loc, pose_inv, K))
    d = [x[None, :, k] - c[:, None, k] for k in range(3)]
    length = np.maximum(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), dt(1e-12))
    dirs = [d[k] / length for k in range(3)]
    p = [dirs[k] + c[:, None, k] for k in range(3)]
    row = [((P[:, i, 0, None] * p[0] + P[:, i, 1, None] * p[1]) + P[:, i, 2, None] * p[2]) + P[:, i, 3, None] for i in range(3)]
    z = -row[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        zz = np.where(z != 0, z, dt(1e-5))
        q = [row[0] / zz, -(row[1] / zz), -(row[2] / zz)]
        uv = [(K[:, i, 0, None] * q[0] + K[:, i, 1, None] * q[1]) + K[:, i, 2, None] * q[2] for i in range(2)]
    return np.stack(dirs, -1), np.stack(uv, -1), z


def pixel_position(uv, H, W, dt=np.float32):
    """grid_sample's round trip: g = u / W 2 - 1, ix = ((g + 1) / 2) (W - 1) -> (ix, iy)."""
    u, v = np.asarray(uv[..., 0], dtype=dt), np.asarray(uv[..., 1], dtype=dt)
    gx, gy = u / dt(W) * dt(2) - dt(1), v / dt(H) * dt(2) - dt(1)
    return ((gx + dt(1)) / dt(2)) * dt(W - 1), ((gy + dt(1)) / dt(2)) * dt(H - 1)


def fetch(images, uv, dt=np.float32):
    """images [M,H,W,C], uv [M,N,2] -> [M,N,C]: bilinear, zeros padding, align_corners=True, taps added nw, ne, sw, se."""
    img = np.asarray(images, dtype=dt)
    M, H, W, C = img.shape
    with np.errstate(invalid="ignore"):
        x, y = pixel_position(uv, H, W, dt)
        x0, y0 = np.floor(x), np.floor(y)
        wx1, wx0, wy1, wy0 = x - x0, (x0 + dt(1)) - x, y - y0, (y0 + dt(1)) - y
        nw, ne, sw, se = wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1
        c0 = np.fmin(np.fmax(x0, dt(-2)), dt(W) + dt(1)).astype(np.int64)
        r0 = np.fmin(np.fmax(y0, dt(-2)), dt(H) + dt(1)).astype(np.int64)
        cam = np.arange(M)[:, None]

        def tap(r, c):
            ok = (r >= 0) & (r < H) & (c >= 0) & (c < W)
            val = img[cam, np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)]
            return np.where(ok[..., None], val, dt(0))
        a, b, c, d = tap(r0, c0), tap(r0, c0 + 1), tap(r0 + 1, c0), tap(r0 + 1, c0 + 1)
        return ((a * nw[..., None] + b * ne[..., None]) + c * sw[..., None]) + d * se[..., None]


def scatter(x, cam_loc, pose_inv, K, images, masks=None, dt=np.float32):
    """rb_ob_scatter -> dict(uv [M,N,2], view_dir [M,N,3], rgb [M,N,C], valid [M,N] uint8, z [M,N], mask_value [M,N] or None)."""
    dirs, uv, z = project(x, cam_loc, pose_inv, K, dt)
    M, H, W, _ = np.shape(images)
    rgb = fetch(images, uv, dt)
    with np.errstate(invalid="ignore"):
        ok = (uv[..., 0] >= 0) & (uv[..., 0] < dt(W)) & (uv[..., 1] >= 0) & (uv[..., 1] < dt(H)) & (z > 0)
        mv = None
        if masks is not None:
            mv = fetch(np.asarray(masks)[..., None], uv, dt)[..., 0]
            ok = ok & (mv > dt(0.5))
    return {"uv": uv, "view_dir": dirs, "rgb": rgb, "valid": ok.astype(np.uint8), "z": z, "mask_value": mv}


def select(vis, draws, n_obs):
    """rb_ob_select -> (index [n_obs,N] int32, count [N] int32): the n_obs largest keys vis + 0.01 draws, ties to the lower camera."""
    vis, draws = np.asarray(vis), np.asarray(draws, dtype=np.float32)
    M, N = vis.shape
    keys = (vis != 0).astype(np.float32) + np.float32(0.01) * draws
    order = np.argsort(-keys, axis=0, kind="stable")[:n_obs].astype(np.int32)
    index = np.full((n_obs, N), -1, dtype=np.int32)
    index[:order.shape[0]] = order
    return index, (vis != 0).sum(0).astype(np.int32)


def gather(index, sc):
    """rb_ob_gather from a scatter() result: its rows (index[k][n], n); zeros where the index is negative."""
    index = np.asarray(index)
    n = np.arange(index.shape[1])[None]
    out = {}
    for k in ("uv", "view_dir", "rgb", "valid"):
        rows = sc[k][np.clip(index, 0, None), n]
        out[k] = np.where((index >= 0).reshape(index.shape + (1,) * (rows.ndim - 2)), rows, rows.dtype.type(0))
    return out


def accumulate(x, normals, cam_loc, pose_inv, K, images, vis, dt=np.float32):
    """rb_ob_accumulate -> dict(weight [N], mean [N,C], var [N,C], count [N] int32)."""
    dirs, uv, _ = project(x, cam_loc, pose_inv, K, dt)
    rgb = fetch(images, uv, dt)
    nr = np.asarray(normals, dtype=dt)
    M, N, C = rgb.shape
    sw, s1, s2, cnt = np.zeros(N, dt), np.zeros((N, C), dt), np.zeros((N, C), dt), np.zeros(N, np.int32)
    for m in range(M):
        w = np.maximum(-((nr[:, 0] * dirs[m, :, 0] + nr[:, 1] * dirs[m, :, 1]) + nr[:, 2] * dirs[m, :, 2]), dt(0))
        use = (np.asarray(vis)[m] != 0) & (w > 0)
        wc = w[:, None] * rgb[m]
        sw = np.where(use, sw + w, sw)
        s1 = np.where(use[:, None], s1 + wc, s1)
        s2 = np.where(use[:, None], s2 + wc * rgb[m], s2)
        cnt = cnt + use.astype(np.int32)
    some = sw > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(some[:, None], s1 / sw[:, None], dt(0))
        var = np.where(some[:, None], np.maximum(s2 / sw[:, None] - mean * mean, dt(0)), dt(0))
    return {"weight": np.where(some, sw, dt(0)), "mean": mean, "var": var, "count": np.where(some, cnt, 0).astype(np.int32)}


# ----------------------------------------------------------------------------------------- the reference's lines on PyTorch-CPU
def scatter_torch(x, cam_loc, pose_inv, K, images, masks=None, dtype=torch.float32):
    """inv_camera_params + sample_images + sample_masks + the uv_valid test as the reference writes them, with ONE change: uv is divided by
    and compared with (W, H) where the reference has (H, W) -- identical for the square images it is compared on, and the form the library
    builds for the others.  No z > 0 term (the reference has none)."""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    x, c, pinv, K, img = t(x), t(cam_loc), t(pose_inv), t(K), t(images)
    M, H, W, _ = img.shape
    locations = x[None].expand(M, -1, -1)
    ray_dirs = F.normalize(locations - c[:, None, :], dim=-1)
    norm_inv = pinv @ torch.cat([ray_dirs + c[:, None, :], torch.ones_like(ray_dirs[..., -1:])], -1).permute(0, 2, 1)
    z_pos = -norm_inv[:, 2:3, :]
    ppc_inv = norm_inv / torch.where(z_pos != 0, z_pos, 1e-5 * torch.ones_like(z_pos))
    ppc_inv[:, 1:3, :] *= -1
    uv = (K @ ppc_inv[:, :3, :]).permute(0, 2, 1)[..., :2]
    size = torch.tensor([W, H]).to(dtype)
    grid = (uv[:, None] / size) * 2 - 1
    rgb = F.grid_sample(img.permute(0, 3, 1, 2), grid, align_corners=True).permute(0, 2, 3, 1)[:, 0]
    valid = torch.logical_and(uv >= 0, uv < size).prod(-1).bool()
    mv = None
    if masks is not None:
        mv = F.grid_sample(t(masks)[:, None], grid, align_corners=True).permute(0, 2, 3, 1)[:, 0, :, 0]
        valid = valid & (mv > 0.5)
    return {"uv": uv.numpy(), "view_dir": ray_dirs.numpy(), "rgb": rgb.numpy(), "valid": valid.numpy().astype(np.uint8),
            "z": z_pos[:, 0].numpy(), "mask_value": None if mv is None else mv.numpy()}


def accumulate_torch(sc, normals, vis, dtype=torch.float32):
    """The weighted statistics of rb_ob_accumulate as one would write them on the [M,N,.] tensors of scatter_sample (sc: a scatter_torch
    result): w = clamp(-(n . view_dir), 0) over the visible pairs, sums over the camera axis."""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    dirs, rgb, nr = t(sc["view_dir"]), t(sc["rgb"]), t(normals)
    w = torch.clamp(-(nr[None] * dirs).sum(-1), min=0) * torch.as_tensor(np.asarray(vis) != 0).to(dtype)
    sw = w.sum(0)
    some = sw > 0
    den = torch.where(some, sw, torch.ones_like(sw))[:, None]
    mean = (w[..., None] * rgb).sum(0) / den
    var = torch.clamp((w[..., None] * rgb * rgb).sum(0) / den - mean * mean, min=0)
    z = torch.zeros_like(mean)
    return {"weight": sw.numpy(), "mean": torch.where(some[:, None], mean, z).numpy(), "var": torch.where(some[:, None], var, z).numpy(),
            "count": (w > 0).sum(0).numpy().astype(np.int32)}


def recast_torch(uv, pose, K, dtype=torch.float32):
    """utils/rend_util.py get_camera_params: pixel positions uv [M,N,2] of cameras pose [M,4,4] (camera-to-world), K [M,3,3] -> unit ray
    directions [M,N,3] (zero skew)."""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    uv, pose, K = t(uv), t(pose), t(K)
    fx, fy, cx, cy, sk = (K[:, i, j, None] for i, j in ((0, 0), (1, 1), (0, 2), (1, 2), (0, 1)))
    z = torch.ones_like(uv[..., 0])
    x_lift = (uv[..., 0] - cx + cy * sk / fy - sk * uv[..., 1] / fy) / fx * z
    y_lift = (uv[..., 1] - cy) / fy * z
    cam = torch.stack([x_lift, -y_lift, -z, torch.ones_like(z)], -1).permute(0, 2, 1)
    world = torch.bmm(pose, cam).permute(0, 2, 1)[:, :, :3]
    return F.normalize(world - pose[:, None, :3, 3], dim=2).numpy()


def select_torch(vis, draws, n_obs):
    """tex_module.py:50: torch.sort(obs_mask + rand 0.01, dim=0, descending=True), the first n_obs rows of the index."""
    keys = torch.as_tensor(np.asarray(vis) != 0).float() + torch.as_tensor(np.asarray(draws, dtype=np.float32)) * 0.01
    return torch.sort(keys, dim=0, descending=True)[1][:n_obs].numpy().astype(np.int32)


def sorted_torch(x, surface_mask, obs_rgb, obs_dirs, obs_mask, cam_pos, n_obs, rand):
    """tex_module.py:35-59, sample_observations_sorted, from the line after its sample_observations call: obs_rgb, obs_dirs [M,Ns,3],
    obs_mask [M,Ns] bool and cam_pos [M,3] are what that call returned for the Ns points of surface_mask, rand [M,Ns] stands for its
    rand_like.  n_obs = 1.  -> (rgb, dirs [N,3], mask [N], pos [N,3], the narrowed surface_mask)."""
    t = lambda a: torch.as_tensor(np.asarray(a))
    x, surface_mask, obs_rgb, obs_dirs, obs_mask, obs_pos = t(x), t(surface_mask).clone(), t(obs_rgb), t(obs_dirs), t(obs_mask), t(cam_pos)
    all_obs_rgb, all_obs_dirs = torch.ones_like(x), torch.ones_like(x)
    all_obs_mask, all_obs_pos = torch.zeros_like(x[..., 0]), torch.zeros_like(x)
    obs_pos = obs_pos[:, None, :].expand(-1, obs_mask.shape[1], -1)
    selected = obs_mask.sum(0) >= n_obs
    surface_mask[surface_mask.clone()] = selected
    obs_rgb, obs_dirs, obs_mask, obs_pos = obs_rgb[:, selected], obs_dirs[:, selected], obs_mask[:, selected].float(), obs_pos[:, selected]
    _, idx = torch.sort(obs_mask + t(rand)[:, selected] * 0.01, dim=0, descending=True)
    take = lambda a: a.gather(0, idx[..., None].expand(-1, -1, 3))[:n_obs]
    all_obs_rgb[surface_mask] = take(obs_rgb)
    all_obs_dirs[surface_mask] = take(obs_dirs)
    all_obs_mask[surface_mask] = 1
    all_obs_pos[surface_mask] = take(obs_pos)
    return all_obs_rgb.numpy(), all_obs_dirs.numpy(), all_obs_mask.numpy(), all_obs_pos.numpy(), surface_mask.numpy()


# ----------------------------------------------------------------------------------------- the cases
SIZES = ((32, 32), (24, 40))          # (H, W): the non-square pair tells (H, W) from (W, H)
BEHIND = 3                            # the camera of the five that stands inside the ball of points


def look_at(position):
    """Camera-to-world pose [4,4] float64 of a camera at `position` looking at the origin: columns right, up, back, position (the camera
    looks along its -z, y up: utils/rend_util.py lift)."""
    c = np.asarray(position, dtype=np.float64)
    back = c / np.linalg.norm(c)
    right = np.cross([0.0, 0.0, 1.0], back)
    right /= np.linalg.norm(right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, np.cross(back, right), back, c
    return pose


def cameras(M, H, W, seed=0):
    """M look-at cameras at distance 4 around the origin with per-camera K; of five, camera BEHIND stands at distance 0.3, inside the ball
    of points, so that some points lie behind it.  -> pose, pose_inv [M,4,4], cam_loc [M,3], K [M,3,3], float32."""
    rng = np.random.default_rng(1000 + 10 * seed + M)
    pose, K = np.zeros((M, 4, 4)), np.zeros((M, 3, 3))
    for m in range(M):
        d = rng.normal(size=3)
        d[2] = 0.5 * d[2]                                              # keep away from the world's up axis
        inside = M == 5 and m == BEHIND
        pose[m] = look_at(d / np.linalg.norm(d) * (0.3 if inside else 4.0))
        # from distance 4 the ball of radius 0.6 is a little larger than the image; the camera inside it has a wide angle, so that the
        # mirrored projections of points behind it land in the image (where the reference would take them for valid)
        focal = min(H, W) * (0.4 if inside else rng.uniform(3.5, 4.5))
        K[m] = [[focal, 0, 0.5 * W + rng.uniform(-1, 1)], [0, focal * rng.uniform(0.97, 1.03), 0.5 * H + rng.uniform(-1, 1)], [0, 0, 1]]
    pose = pose.astype(np.float32)
    pose_inv = np.linalg.inv(pose.astype(np.float64)).astype(np.float32)
    return pose, pose_inv, np.ascontiguousarray(pose[:, :3, 3]), K.astype(np.float32)


class Case:
    """One seeded case: x, normals [N,3]; pose, pose_inv, cam_loc, K; images [M,H,W,3], masks [M,H,W] (a disc of radius 0.45 min(H, W) with
    a soft edge); occluded [M,N] (a random pattern that stands for the secondary cast) and draws [M,N] (a scaled permutation: all keys
    differ)."""

    def __init__(self, M, N, H, W, content):
        self.M, self.N, self.H, self.W, self.content = M, N, H, W, content
        self.name = f"M{M}_N{N}_{H}x{W}_{content}"
        rng = np.random.default_rng(7 + 13 * M + N + 101 * H + (content == "affine"))
        self.pose, self.pose_inv, self.cam_loc, self.K = cameras(M, H, W)
        p = rng.normal(size=(N, 3))
        self.x = (p / np.maximum(np.linalg.norm(p, axis=1, keepdims=True), 1e-9) * 0.6 * rng.uniform(size=(N, 1)) ** (1 / 3)).astype(np.float32)
        nr = rng.normal(size=(N, 3))
        self.normals = (nr / np.maximum(np.linalg.norm(nr, axis=1, keepdims=True), 1e-9)).astype(np.float32)
        py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        if content == "affine":
            self.images = np.stack([np.stack([px / W, py / H, np.full((H, W), m / M)], -1) for m in range(M)]).astype(np.float32)
        else:
            self.images = rng.uniform(size=(M, H, W, 3)).astype(np.float32)
        r = np.hypot(px - 0.5 * (W - 1), py - 0.5 * (H - 1))
        self.masks = np.broadcast_to(np.clip(0.45 * min(H, W) - r + 0.5, 0, 1), (M, H, W)).astype(np.float32).copy()
        self.occluded = rng.uniform(size=(M, N)) < 0.35
        self.draws = ((rng.permutation(M * N).reshape(M, N) + 0.5) / max(M * N, 1)).astype(np.float32)

    def cams(self):
        return self.cam_loc, self.pose_inv, self.K

    @functools.lru_cache(maxsize=None)
    def scatter(self, dt=np.float32, masks=True):
        """The restatement's scatter of this case -- computed once, shared, never modified."""
        return scatter(self.x, *self.cams(), self.images, self.masks if masks else None, dt)

    @functools.lru_cache(maxsize=None)
    def scatter_torch(self, dtype=torch.float32):
        return scatter_torch(self.x, *self.cams(), self.images, self.masks, dtype)

    @functools.lru_cache(maxsize=None)
    def vis(self):
        """valid (fp32 restatement) and not occluded, uint8 [M,N]."""
        return (self.scatter()["valid"].astype(bool) & ~self.occluded).astype(np.uint8)

    def excluded(self):
        """Pairs that may be left out of the valid comparison against float64: the float64 uv within 1e-3 pixels of an image border (u or
        v of 0, W or H), or the float64 mask sample within 1e-4 of 0.5."""
        s = self.scatter(np.float64)
        u, v = s["uv"][..., 0], s["uv"][..., 1]
        near = lambda a, b: np.abs(a - b) <= 1e-3
        return near(u, 0) | near(u, self.W) | near(v, 0) | near(v, self.H) | (np.abs(s["mask_value"] - 0.5) <= 1e-4)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case over M in {1, 5}, N in {0, 1, 300}, the two image sizes and the two image contents."""
    out = {}
    for M, N, (H, W), content in itertools.product((1, 5), (0, 1, 300), SIZES, ("random", "affine")):
        c = Case(M, N, H, W, content)
        out[c.name] = c
    return out


N_OBS = (1, 3)


def rel_err64(a, b):
    """max |a - b| / (|b| + mean |b|): the project's distance (tests/conftest.py rel_err), on numpy arrays; 0 for empty ones."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float((np.abs(a - b) / (np.abs(b) + np.abs(b).mean() + 1e-30)).max())
