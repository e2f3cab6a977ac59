"""Multi-view observations of surface points on the device: which training views see a point, along which direction, with what pixel colour.

Counterpart of the reference's model/focus_sampler.py (inv_camera_params, FocusSampler) and training/tex_module.py (TexSpaceSampler), the
piece between a TexSampler (robir_amd/texture.py), which draws surface points from the baked maps, and the renderer's `points` / `dirs` /
`tex_uv` input form.  The arithmetic runs in librobir_hip_observe.so (include/robir_hip_observe.h); the secondary cast that
decides occlusion goes through the model's own octree_ray_tracer.  Everything here runs under no_grad.

Names, parameter order and defaults are the reference's; keyword-only extras (`camera=`, `draws=`, `all_views=`, `chunk=`) pin what the
reference draws at random or widen it.  Three departures from the reference, all documented in DESIGN 4.10:
  - u is divided by and compared with the image width and v with its height (the reference uses (H, W) in that order for (u, v));
  - a point behind a camera is not valid for that camera (the reference projects it mirrored into the image);
  - sample_observations returns the colours of the camera it chose ([1,N,3]); the reference returns those of all M cameras, of which
    sample_observations_sorted then reads camera 0 whatever camera was chosen.
"""
import torch

from . import ops

# visible_views forms uv, view_dir, rgb and valid for all M cameras of the points it is given: 33 bytes per (camera, point) pair.  The
# chunked callers (observed_color, the all_views selection) size their chunks so that these temporaries stay under this many bytes.
SCATTER_BYTES = 256 << 20
PAIR_BYTES = 33


def inv_camera_params(locations, pose_inv, cam_loc, intrinsics):
    """locations [M,N,3] (or [N,3], shared by the cameras), pose_inv [M,4,4], cam_loc [M,3], intrinsics [M,3,3] -> (uv [M,N,2], ray_dirs
    [M,N,3]): the pixel position at which camera m sees the point and the unit direction from the camera to it."""
    M = cam_loc.shape[0]
    K = intrinsics[:, :3, :3].float().contiguous()
    pinv, c = pose_inv.float().contiguous(), cam_loc.float().contiguous()
    blank = torch.zeros(1, 2, 2, 1, device=c.device)          # the projection needs no image: a 2 x 2 one, never looked at
    if locations.dim() == 2 or M == 1 or locations.stride(0) == 0:
        x = (locations if locations.dim() == 2 else locations[0]).float().contiguous()
        uv, dirs, _, _ = ops.ob_scatter(x, c, pinv, K, blank.expand(M, 2, 2, 1).contiguous())
        return uv, dirs
    out = [ops.ob_scatter(locations[m].float().contiguous(), c[m:m + 1], pinv[m:m + 1], K[m:m + 1], blank) for m in range(M)]
    return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])


class FocusSampler:
    """The reference's FocusSampler (model/focus_sampler.py:33-101) on device tensors: images [M,H,W,3] (or [M,H*W,3] with img_res), masks
    [M,H,W] (or [M,H*W]; an empty tensor or None: no masks), poses [M,4,4] camera-to-world, intrinsics [M,3,3].  Images are held as
    [M,H,W,3] float32 and masks as [M,H,W] float32 on the device of `poses`."""

    def __init__(self, images, masks, poses, intrinsics, img_res=None):
        dev = poses.device
        M = self.n_cameras = len(images)
        H, W = (images[0].shape[0], images[0].shape[1]) if img_res is None else (int(img_res[0]), int(img_res[1]))
        p = torch.eye(4, device=dev).repeat(M, 1, 1).float()
        p[:, :3, :4] = poses[:, :3, :4].float()
        self.pose_inv = torch.inverse(p).float().contiguous()
        self.cam_loc = poses[:, :3, 3].float().contiguous()
        self.images = torch.as_tensor(images).to(dev).float().reshape(M, H, W, -1).contiguous()
        if self.images.shape[-1] != 3:
            raise ValueError(f"FocusSampler: images must have 3 channels, got {tuple(self.images.shape)}")
        self.masks = None
        if masks is not None and torch.as_tensor(masks).numel() > 0:
            self.masks = torch.as_tensor(masks).to(dev).float().reshape(M, H, W).contiguous()
        self.intrinsics = intrinsics[:, :3, :3].to(dev).float().contiguous()
        self.img_size = torch.tensor([H, W], device=dev).float()          # the reference's attribute: (H, W)

    def cameras(self, sl=None):
        """(cam_loc, pose_inv, intrinsics, images, masks) of all cameras or of the slice `sl` of them."""
        t = (self.cam_loc, self.pose_inv, self.intrinsics, self.images, self.masks)
        return t if sl is None else tuple(None if a is None else a[sl].contiguous() for a in t)

    def sample_images(self, uv):
        """uv [M,N,2] pixel positions -> colours [M,N,3]."""
        return ops.ob_fetch(self.images, uv.float().contiguous())

    def sample_masks(self, uv):
        """uv [M,N,2] -> [M,N,1] bool: the mask sample > 0.5 (all true without masks)."""
        if self.masks is None:
            return torch.ones(*uv.shape[:2], 1, dtype=torch.bool, device=uv.device)
        return ops.ob_fetch(self.masks[..., None], uv.float().contiguous()) > 0.5

    def scatter(self, x, sl=None):
        """x [N,3] -> uv [M,N,2], view_dir [M,N,3], rgb [M,N,3], valid [M,N] uint8, for all cameras or the slice `sl`."""
        c, pinv, K, images, masks = self.cameras(sl)
        return ops.ob_scatter(x.float().contiguous(), c, pinv, K, images, masks)

    def scatter_sample(self, x):
        """x [N,3] -> ({"object_mask" [M,N] bool, "uv" [M,N,2], "view_dir" [M,N,3]}, {"rgb" [M,N,3]}).  A NaN uv is never valid, so the
        reference's NaN check cannot trigger and no host read is made."""
        assert len(x.shape) == 2
        uv, view_dir, rgb, valid = self.scatter(x)
        return {"object_mask": valid.bool(), "uv": uv, "view_dir": view_dir}, {"rgb": rgb}


def _cast_valid(model, x, normals, view_dir, valid, offset):
    """vis [M,N] bool: valid pairs whose ray from x + offset n towards the camera hits nothing.  The valid pairs are compacted and cast as
    ONE batch; no ray is cast for the others."""
    M, N = valid.shape
    vis = torch.zeros(M * N, dtype=torch.bool, device=x.device)
    idx = valid.reshape(-1).nonzero()[:, 0]
    if idx.numel() == 0:
        return vis.reshape(M, N)
    n = idx % N
    origins = (x[n] + normals[n] * offset).contiguous()
    dirs = (-view_dir.reshape(-1, 3)[idx]).contiguous()
    with torch.no_grad():
        _, hit, _ = model.octree_ray_tracer(sdf=None, cam_loc=origins, object_mask=None, ray_directions=dirs[:, None, :])
    vis[idx] = ~hit.reshape(-1)
    return vis.reshape(M, N)


def visible_views(model, focus, x, normals, offset=0.005, *, cameras=None, scatter=None):
    """vis [M,N] bool: camera m sees point x[n] -- the pair is valid (inside the image, on the mask, in front of the camera) and the
    segment from x + offset n to the camera is free (any hit of model.octree_ray_tracer counts as occluded, training/tex_module.py:24-32).
    cameras: a slice of the cameras (then M is its length).  scatter: the (uv, view_dir, rgb, valid) of these points, if at hand."""
    x, normals = x.float().contiguous(), normals.float().contiguous()
    _, view_dir, _, valid = focus.scatter(x, cameras) if scatter is None else scatter
    return _cast_valid(model, x, normals, view_dir, valid, offset)


def _chunk_points(M, chunk=None):
    if chunk is not None:
        return max(1, int(chunk))
    return max(256, SCATTER_BYTES // (PAIR_BYTES * M) // 256 * 256)


def _visible_chunked(model, focus, x, normals, offset, chunk):
    """visible_views as uint8 [M,N], N in chunks: only the mask itself has M N entries."""
    M, N = focus.n_cameras, x.shape[0]
    vis = torch.zeros(M, N, dtype=torch.uint8, device=x.device)
    step = _chunk_points(M, chunk)
    for i in range(0, N, step):
        vis[:, i:i + step] = visible_views(model, focus, x[i:i + step], normals[i:i + step], offset).to(torch.uint8)
    return vis


def observed_color(model, focus, x, normals, *, offset=0.005, chunk=None):
    """The colour the training views observe at surface points x [N,3] with normals [N,3]: (mean [N,3], var [N,3], weight [N], count [N]
    int32) over the cameras that see the point (visible_views), weighted by w = max(-n . view_dir, 0); var = max(sum(w rgb^2) / sum(w) -
    mean^2, 0); zeros where no camera contributes.  N is walked in chunks of `chunk` points (default: so that visible_views' temporaries
    stay under SCATTER_BYTES = 256 MiB, i.e. 33 M chunk bytes): per chunk the mask vis [M,chunk] is all that has M x chunk entries on
    top of them, and the statistics come from one fused kernel that writes nothing of that size."""
    x, normals = x.float().contiguous(), normals.float().contiguous()
    N, dev = x.shape[0], x.device
    mean, var = torch.zeros(N, 3, device=dev), torch.zeros(N, 3, device=dev)
    weight, count = torch.zeros(N, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
    c, pinv, K, images, _ = focus.cameras()
    step = _chunk_points(focus.n_cameras, chunk)
    for i in range(0, N, step):
        xs, ns = x[i:i + step].contiguous(), normals[i:i + step].contiguous()
        vis = visible_views(model, focus, xs, ns, offset).to(torch.uint8).contiguous()
        weight[i:i + step], mean[i:i + step], var[i:i + step], count[i:i + step] = ops.ob_accumulate(xs, ns, c, pinv, K, images, vis)
    return mean, var, weight, count


class TexSpaceSampler:
    """The reference's TexSpaceSampler (training/tex_module.py): batches of surface points drawn in texture space, each with a training
    view that sees it.  TexSpaceSampler(model, tex_sampler, focus_sampler) -- or TexSpaceSampler(trainer) with an object that has .model,
    .tex_sampler and .focus_sampler, the reference's single argument."""

    def __init__(self, model, tex_sampler=None, focus_sampler=None):
        if tex_sampler is None and focus_sampler is None and hasattr(model, "model"):
            model, tex_sampler, focus_sampler = model.model, model.tex_sampler, model.focus_sampler
        if tex_sampler is None or focus_sampler is None:
            raise TypeError("TexSpaceSampler(model, tex_sampler, focus_sampler), or TexSpaceSampler(trainer) with those three attributes")
        self.model, self.tex_sampler, self.focus_sampler = model, tex_sampler, focus_sampler

    def sample_observations(self, x, normals, *, camera=None):
        """x, normals [N,3] -> (rgb [1,N,3], cam_dir [1,N,3], vis_mask [1,N] bool, cam_pos [1,3]) of ONE camera, drawn with torch.randint
        unless given; the projection, the fetch and the cast run for that camera alone."""
        fs = self.focus_sampler
        m = int(torch.randint(fs.n_cameras, [])) if camera is None else int(camera)
        if not 0 <= m < fs.n_cameras:
            raise ValueError(f"sample_observations: camera {m} of {fs.n_cameras}")
        x, normals = x.float().contiguous(), normals.float().contiguous()
        sc = fs.scatter(x, slice(m, m + 1))
        vis = visible_views(self.model, fs, x, normals, scatter=sc)
        return sc[2], sc[1], vis, fs.cam_loc[m:m + 1]

    def sample_observations_sorted(self, x, surface_mask, n_obs=1, normals=None, *, camera=None, all_views=False, draws=None):
        """x [N,3], surface_mask [N] bool, normals [N,3] -> (rgb, dirs [N,3], mask [N] float, cam_pos [N,3]): ones / zeros outside the
        selected points as in the reference.  surface_mask is narrowed IN PLACE to the points with at least n_obs visible views (the
        reference does the same).  With n_obs > 1 the three [N,3] outputs become [n_obs,N,3], the best view first.
        all_views=False: one camera (`camera`, random unless given), the reference's behaviour.  all_views=True: the n_obs views with the
        largest keys vis + 0.01 draws among ALL cameras (draws [M,Ns] over the Ns surface points, torch.rand unless given), chosen by
        rb_ob_select from the mask alone; colours and directions are computed for the chosen n_obs rows only."""
        if normals is None:
            raise TypeError("sample_observations_sorted: normals are needed for the secondary cast")
        if not 1 <= int(n_obs) <= ops.OB_MAX_OBS:
            raise ValueError(f"sample_observations_sorted: n_obs = {n_obs} outside 1 .. {ops.OB_MAX_OBS}")
        n_obs, fs, dev = int(n_obs), self.focus_sampler, x.device
        lead = () if n_obs == 1 else (n_obs,)
        all_rgb, all_dirs = torch.ones(*lead, *x.shape, device=dev), torch.ones(*lead, *x.shape, device=dev)
        all_mask, all_pos = torch.zeros(x.shape[0], device=dev), torch.zeros(*lead, *x.shape, device=dev)
        xs, ns = x[surface_mask].float().contiguous(), normals[surface_mask].float().contiguous()
        if all_views:
            vis = _visible_chunked(self.model, fs, xs, ns, 0.005, None)
            cams = fs.cameras()
        else:
            m = int(torch.randint(fs.n_cameras, [])) if camera is None else int(camera)
            vis = visible_views(self.model, fs, xs, ns, cameras=slice(m, m + 1)).to(torch.uint8).contiguous()
            cams = fs.cameras(slice(m, m + 1))
        if draws is None:
            draws = torch.rand(vis.shape, device=dev)
        index, count = ops.ob_select(vis, draws.float().contiguous(), n_obs)
        selected = count >= n_obs
        surface_mask[surface_mask.clone()] = selected
        index = index[:, selected].contiguous()
        _, dirs, rgb, _ = ops.ob_gather(index, xs[selected].contiguous(), *cams)
        pos = cams[0][index.long()]
        sq = (lambda t: t[0]) if n_obs == 1 else (lambda t: t)
        all_rgb[..., surface_mask, :] = sq(rgb)
        all_dirs[..., surface_mask, :] = sq(dirs)
        all_pos[..., surface_mask, :] = sq(pos)
        all_mask[surface_mask] = 1
        return all_rgb, all_dirs, all_mask, all_pos

    def data_batch(self, n, **kw):
        """n points drawn by the TexSampler -> (new_inputs, normal, obs_rgb): new_inputs = {"points": the cameras' centres, "dirs": the
        directions from them to the points, "object_mask", "tex_uv"}, each with a leading batch axis, is the renderer's second input
        form: model(new_inputs, trainstage=...) renders the points as seen from their views."""
        tex_input = self.tex_sampler.sample(n)
        x, surface_mask, normal = tex_input["x"], tex_input["object_mask"], tex_input["normal"]
        obs_rgb, obs_dirs, obs_mask, obs_pos = self.sample_observations_sorted(x, surface_mask, normals=normal, **kw)
        new_inputs = {"points": obs_pos[None], "dirs": obs_dirs[None], "object_mask": obs_mask.bool()[None], "tex_uv": tex_input["uv"][None]}
        return new_inputs, normal, obs_rgb

    def simple_data_batch(self, model_inputs):
        n = model_inputs["uv"].shape[1]
        tex_input = self.tex_sampler.sample(n)
        return {"points": tex_input["x"], "normals": tex_input["normal"], "object_mask": tex_input["object_mask"].bool()}
