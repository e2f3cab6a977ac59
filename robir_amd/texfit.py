"""Fit the albedo and roughness planes of a baked asset to a set of views, through the mesh view, on the device.

robir_amd.texture bakes a point sample of the material network into a UV atlas; robir_amd.meshrender draws the asset.  What the bake loses
(chart borders, dilation, resolution) the exported asset keeps -- unless the texels themselves are fitted to the views the asset is meant to
reproduce.  This module closes that loop: the G-buffer's plane fetch is linearised once per batch of views (librobir_hip_texfit.so: the
four taps per hit row, include/robir_hip_texfit.h), a step fetches the four fit channels from the taps, shades the rows with
sg_render.render_with_all_sg under grad (rb_sg_shade / rb_sg_shade_bwd), takes training.photometric_loss against the target colours,
carries d loss / d (albedo, roughness) back onto the touched texels with the transpose of the fetch -- a gather over (row, tap) pairs sorted
by texel -- and moves those texels with a lazy Adam step.  Geometry, uv, the normal plane and the metallic plane stay frozen.

    python -m robir_amd.texfit --asset DIR (--views views.npz | --synthetic --n-views N --size S) [--light DIR]
        [--vis none|network|octree] --steps K --out DIR2

views.npz: images [M,H,W,3] (what the loss compares the tone-mapped view with), poses [M,4,4] camera-to-world, intrinsics [M,3,3] and,
optionally, masks [M,H,W].
"""
import argparse
import json
import os
import shutil

import numpy as np
import torch

from . import meshrender, ops

FIT_CHANNELS = 4          # albedo | roughness: the leading planes of meshrender.PLANES
LO = (0.0, 0.0, 0.0, 0.02)
HI = (1.0, 1.0, 1.0, 1.0)


# ----------------------------------------------------------------------------------------- the transpose's pair list
def sort_pairs(tap_texel, tap_weight, R):
    """The (row, tap) pairs of tf_taps sorted by texel with a stable sort (pairs of one texel stay in ascending 4 row + tap order; absent
    taps get the key R^2 and sort to the tail) -> (pair_row [4n] int32, pair_weight [4n], seg_texel [T] int32, seg_start [T+1] int32).
    One host read: T."""
    dev, n = tap_texel.device, tap_texel.shape[0]
    key = tap_texel.reshape(-1).to(torch.int64)
    key = torch.where(key < 0, torch.full_like(key, R * R), key)
    skey, order = torch.sort(key, stable=True)
    pair_row = (order // 4).to(torch.int32).contiguous()
    pair_weight = tap_weight.reshape(-1)[order].contiguous()
    texels, counts = torch.unique_consecutive(skey, return_counts=True)
    T = int((texels < R * R).sum()) if n else 0          # the single sync
    seg_start = torch.zeros(T + 1, dtype=torch.int32, device=dev)
    if T:
        seg_start[1:] = torch.cumsum(counts[:T], 0).to(torch.int32)
    return pair_row, pair_weight, texels[:T].to(torch.int32).contiguous(), seg_start


class _Fetch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, planes, uv, filter):
        R = planes.shape[0]
        texel, weight = ops.tf_taps(uv, R, filter)
        ctx.save_for_backward(texel, weight)
        ctx.shape = tuple(planes.shape)
        return ops.tf_fetch(planes.float().contiguous(), texel, weight)

    @staticmethod
    def backward(ctx, g_tex):
        texel, weight = ctx.saved_tensors
        R, _, C = ctx.shape
        pair_row, pair_weight, seg_texel, seg_start = sort_pairs(texel, weight, R)
        dense = torch.zeros(R * R, C, dtype=torch.float32, device=g_tex.device)
        dense[seg_texel.long()] = ops.tf_scatter(pair_row, pair_weight, seg_start, g_tex.float().contiguous())
        return dense.reshape(R, R, C), None, None


def fetch(planes, uv, filter=1):
    """planes [R,R,C] at uv [n,2] (v up) -> [n,C]: the mesh view's plane fetch (filter 1: bilinear with zero padding, 0: the containing
    texel) with a graph to `planes`, for callers who want autograd through the atlas with an optimiser of their own.  The backward is the
    transpose as a gather into a dense [R,R,C] gradient; the same inputs give the same bytes on every run.  uv is frozen."""
    if isinstance(uv, torch.Tensor) and uv.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("texfit.fetch: uv requires grad, but the fetch has no gradient to uv (geometry and uv are frozen)")
    return _Fetch.apply(planes, uv, int(filter))


# ----------------------------------------------------------------------------------------- views
def orbit_poses(pose, n):
    """pose [4,4] (camera-to-world, numpy) -> [n,4,4] float32: the pose turned about the world's y axis by 2 pi k / n, k = 0 .. n - 1."""
    pose = np.asarray(pose, dtype=np.float64)
    out = np.zeros((int(n), 4, 4), dtype=np.float32)
    for k in range(int(n)):
        a = 2.0 * np.pi * k / int(n)
        turn = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
        out[k] = (turn @ pose).astype(np.float32)
    return out


def _views(views, dev):
    """-> (images [M,H,W,3], masks [M,H,W] or None, poses: a list of M camera-to-world matrices or None, pose_inv / cam_loc or None, K [M,3,3])"""
    from . import observe
    if isinstance(views, observe.FocusSampler):
        return views.images.to(dev), views.masks, None, (views.pose_inv.to(dev), views.cam_loc.to(dev)), views.intrinsics.to(dev)
    t = lambda a: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(dev).float().contiguous()
    images, poses, K = t(views["images"]), t(views["poses"]), t(views["intrinsics"])
    if images.dim() != 4 or images.shape[-1] != 3 or poses.shape[0] != images.shape[0] or K.shape[0] != images.shape[0]:
        raise ValueError(f"texfit: images [M,H,W,3], poses [M,4,4], intrinsics [M,3,3] expected, got {tuple(images.shape)}, "
                         f"{tuple(poses.shape)}, {tuple(K.shape)}")
    masks = views.get("masks")
    masks = t(masks) if masks is not None and torch.as_tensor(np.asarray(masks) if not torch.is_tensor(masks) else masks).numel() else None
    return images, masks, poses, None, K[:, :3, :3].contiguous()


class ViewBatch:
    """Everything about a batch of views that does not depend on the fitted texels, built once: per view the asset is projected, rasterised
    and its G-buffer formed for the hit rows exactly as render_mesh does (meshrender.view_rows); the rows of all views are concatenated in
    view order.  points, normal, view_dir [n,3], uv [n,2], frozen [n,Cs]: the view's own fetch of every plane (metallic and the normal
    plane are read from it); views and pixels: per view its index and the flat hit pixels [n_v] int64; starts [V+1]: the row range of each
    view; target [n,3] and obj_mask [n]; tap_texel / tap_weight [n,4] and the transpose's sorted pair list (sort_pairs); T touched texels."""

    def __init__(self, asset, images, masks, poses, cameras, K, index, filter=1, near=1e-4, cull=0):
        a, dev = asset, asset.planes.device
        H, W = images.shape[1], images.shape[2]
        rows, self.views, self.pixels = [], list(index), []
        for v in self.views:
            if poses is not None:
                face_id, _, _, idx, g = meshrender.view_rows(a, poses[v], K[v], H, W, filter, near, cull)
            else:         # a FocusSampler holds the inverse poses it formed itself
                face_id, _, _, idx, g = _view_rows_inv(a, cameras[0][v], cameras[1][v], K[v], H, W, filter, near, cull)
            rows.append(g)
            self.pixels.append(idx)
        cat = lambda k: torch.cat([g[k] for g in rows], 0).contiguous()
        self.points, self.view_dir, self.uv, self.frozen = cat("position"), cat("view_dir"), cat("uv"), cat("tex")
        if a.has_normal:
            self.normal = meshrender._unit(self.frozen[:, 5:8])
        elif rows and "normal" in rows[0]:
            self.normal = cat("normal")
        else:
            raise ValueError("texfit: the asset has neither a normal plane nor vertex normals")
        counts = [int(p.numel()) for p in self.pixels]
        self.starts = [0] + [int(c) for c in np.cumsum(counts)]
        self.n = int(self.starts[-1])
        self.target = torch.cat([images[v].reshape(-1, 3)[p] for v, p in zip(self.views, self.pixels)], 0).contiguous()
        if masks is not None:
            self.obj_mask = torch.cat([masks[v].reshape(-1)[p] > 0.5 for v, p in zip(self.views, self.pixels)], 0).contiguous()
        else:
            self.obj_mask = torch.ones(self.n, dtype=torch.bool, device=dev)
        self.net_mask = torch.ones(self.n, dtype=torch.bool, device=dev)
        R = a.planes.shape[0]
        self.tap_texel, self.tap_weight = ops.tf_taps(self.uv, R, filter)
        self.pair_row, self.pair_weight, self.seg_texel, self.seg_start = sort_pairs(self.tap_texel, self.tap_weight, R)
        self.T = int(self.seg_texel.numel())


def _view_rows_inv(a, pinv, cam, K, H, W, filter, near, cull):
    with torch.no_grad():
        screen = ops.rs_project(a.vertices, pinv.contiguous(), K[:3, :3].contiguous())
        face_id, bary, depth = meshrender.rasterize_screen(screen, a.faces, H, W, near, cull)
        hit = face_id.reshape(-1) >= 0
        idx = hit.nonzero()[:, 0].contiguous()
        g = meshrender.gbuffer(face_id, bary, a.vertices, a.faces, a.uv, cam.contiguous(), a.planes, filter,
                               None if a.has_normal else a.vnormals, idx)
    return face_id, depth, hit, idx, g


# ----------------------------------------------------------------------------------------- the fit
class AtlasFit:
    """Fits planes[..., 0:4] (albedo | roughness) of a baked asset to `views` through the mesh view.

    asset: what meshrender.load_asset accepts (a directory written by TextureSet.export, a TextureSet, a MeshAsset); its planes are copied.
    views: an observe.FocusSampler or a dict with images [M,H,W,3], poses [M,4,4], intrinsics [M,3,3] and optionally masks [M,H,W].  The
    images are what the tone-mapped view is compared with (training.photometric_loss): LDR for tone=None (the reference's x / (x + 1)) or
    an ACESToneMapping, HDR for tone="identity".
    light / model: as render_mesh (a light overrides the model's).  vis: "none" -- direct SG shading; "network" / "octree": the model's
    visibility network / its octree tracer and its indirect-illumination network, as render_mesh -- the sampled light visibility, the
    sampled specular visibility and the indirect term are computed once per batch of views under no_grad and reused: they enter the colour
    linearly and carry no gradient here.
    batch: views per step (default: all of them, one cached ViewBatch); with a smaller batch the views are taken in turn and their batches
    are cached as they are first used.  lr: one value or one per channel; lo / hi: the clamp per channel (albedo [0, 1], roughness
    [0.02, 1]).  Adam is lazy: a texel that no row of the step's batch reads is not touched and its moments do not decay."""

    def __init__(self, asset, views, light=None, model=None, vis="none", tone=None, loss_type="L1", batch=None, lr=0.01,
                 betas=(0.9, 0.999), eps=1e-8, lo=LO, hi=HI, filter=1, near=1e-4, cull=0):
        if vis not in ("none", "network", "octree"):
            raise ValueError(f"AtlasFit: vis = {vis!r}, expected 'none', 'network' or 'octree'")
        if vis != "none" and model is None:
            raise ValueError(f"AtlasFit: vis = {vis!r} needs the model's visibility and indirect-illumination networks")
        if model is None and light is None:
            raise ValueError("AtlasFit: give a model or a light (a directory with sg_128.npy, or [M,7] light SGs)")
        if loss_type not in ("L1", "L2"):
            raise ValueError(f"AtlasFit: unknown loss_type {loss_type!r} (L1 | L2)")
        dev = next(model.parameters()).device if model is not None else (light.device if torch.is_tensor(light) else torch.device("cuda:0"))
        src = meshrender.load_asset(asset, dev)
        self.asset_dir = asset if isinstance(asset, str) else None
        self.asset = meshrender.MeshAsset(src.vertices, src.faces, src.uv, src.planes.clone().contiguous(), src.has_normal, src.vnormals)
        self.start_planes = src.planes
        self.planes = self.asset.planes
        R = self.planes.shape[0]
        self.images, self.masks, self.poses, self.cameras, self.K = _views(views, dev)
        self.M = self.images.shape[0]
        self.model, self.light = model, light
        self.lgt, self.f0 = meshrender.light_and_f0(model, light, dev)
        if tone == "identity":
            from . import nets
            tone = nets.ACESToneMapping(hdr_mode=3).to(dev)
        self.tone, self.loss_type, self.vis = tone, loss_type, vis
        per = lambda x: [float(x)] * FIT_CHANNELS if np.ndim(x) == 0 else [float(y) for y in x]
        self.lr, self.lo, self.hi = per(lr), per(lo), per(hi)
        if not (len(self.lr) == len(self.lo) == len(self.hi) == FIT_CHANNELS):
            raise ValueError(f"AtlasFit: lr, lo, hi take one value or {FIT_CHANNELS} (albedo rgb, roughness)")
        self.betas, self.eps, self.filter, self.near, self.cull = (float(betas[0]), float(betas[1])), float(eps), int(filter), near, cull
        self.batch = self.M if batch is None else max(1, min(int(batch), self.M))
        self.adam_m = torch.zeros(R, R, FIT_CHANNELS, dtype=torch.float32, device=dev)
        self.adam_v = torch.zeros_like(self.adam_m)
        self.touched = torch.zeros(R * R, dtype=torch.bool, device=dev)
        self.t, self.loss_hist, self._batches = 0, [], {}

    # -- batches
    def view_batch(self, index):
        key = tuple(int(v) for v in index)
        if key not in self._batches:
            self._batches[key] = ViewBatch(self.asset, self.images, self.masks, self.poses, self.cameras, self.K, key, self.filter, self.near,
                                           self.cull)
            self.touched[self._batches[key].seg_texel.long()] = True
        return self._batches[key]

    def _next_batch(self):
        first = (self.t * self.batch) % self.M
        return self.view_batch([(first + k) % self.M for k in range(self.batch)])

    # -- one step
    def _constants(self, b):
        """vis != "none": the sampled light visibility [n,M], the sampled specular visibility [n] and the indirect term [n,3] of a batch,
        computed ONCE under no_grad with the materials the planes hold at that moment and reused by every later step: they enter the
        colour linearly and carry no gradient here."""
        from . import sg_render
        from .octree_tracing import OctreeVisModel
        vm = self.model.visibility_network if self.vis == "network" else OctreeVisModel(self.model.octree_ray_tracer)
        with torch.no_grad():
            tex = ops.tf_fetch(self.planes, b.tap_texel, b.tap_weight, FIT_CHANNELS)
            alb, rough = tex[:, 0:3].contiguous(), tex[:, 3:4].contiguous()
            dev, L = tex.device, self.lgt.shape[0]
            b.light_vis = sg_render._diffuse_vis_core(b.points, b.normal, vm, self.lgt, sg_render._rand((1, L, 32), dev),
                                                      sg_render._rand((1, L, 32), dev), 1.0, False, None, 1, None)
            b.bvis = sg_render._specular_vis_core(b.points, b.normal, b.view_dir, vm, rough.reshape(-1).contiguous(),
                                                  sg_render._rand((b.n, 8), dev), sg_render._rand((b.n, 8), dev), True, False, False, None, 1)
            b.indir = meshrender.shade_rows(b.points, b.normal, b.view_dir, alb, rough, model=self.model, light=self.light,
                                            vis=self.vis)["indir_rgb"].float().contiguous()

    def _shade(self, b, albedo, roughness):
        from . import sg_autograd, sg_render
        if self.vis != "none":
            if b.n and getattr(b, "light_vis", None) is None:
                self._constants(b)
            rgb = sg_autograd.sg_shade(b.normal, b.view_dir, self.lgt, self.f0, roughness.reshape(-1), albedo, b.bvis, light_vis=b.light_vis,
                                       metallic=None, indir_integral=None, lin_diff=False)[0]
            return {"sg_rgb": rgb, "indir_rgb": b.indir}
        return sg_render.render_with_all_sg(points=b.points, normal=b.normal, viewdirs=b.view_dir, lgtSGs=self.lgt, specular_reflectance=self.f0,
                                            roughness=roughness, diffuse_albedo=albedo, indir_integral=None, indir_lgtSGs=None, VisModel=None,
                                            testing=True, metallic=None, draws={})

    def forward(self, index=None):
        """The view of the current planes on the rows of a batch (default: all views), without a graph -> dict: sg_rgb, diffuse_albedo [n,3],
        roughness [n,1], batch (the ViewBatch: pixel indices, targets)."""
        b = self.view_batch(range(self.M) if index is None else index)
        with torch.no_grad():
            tex = ops.tf_fetch(self.planes, b.tap_texel, b.tap_weight, FIT_CHANNELS)
            alb, rough = tex[:, 0:3].contiguous(), tex[:, 3:4].contiguous()
            out = {"diffuse_albedo": alb, "roughness": rough, "batch": b}
            r = self._shade(b, alb, rough) if b.n else {"sg_rgb": torch.zeros(0, 3, device=tex.device)}
            out["sg_rgb"] = r["sg_rgb"]
            out["indir_rgb"] = r["indir_rgb"] if self.vis != "none" and b.n else torch.zeros_like(out["sg_rgb"])
        return out

    def step(self):
        """One step on the next batch of views -> the loss before the update (a float)."""
        from . import training
        b = self._next_batch()
        if b.n == 0 or b.T == 0:
            self.t += 1
            self.loss_hist.append(0.0)
            return 0.0
        with torch.no_grad():
            tex = ops.tf_fetch(self.planes, b.tap_texel, b.tap_weight, FIT_CHANNELS)
        alb = tex[:, 0:3].contiguous().requires_grad_(True)
        rough = tex[:, 3:4].contiguous().requires_grad_(True)
        with torch.enable_grad():
            r = self._shade(b, alb, rough)
            loss = training.photometric_loss(r["sg_rgb"], r.get("indir_rgb") if self.vis != "none" else None, b.target, b.net_mask, b.obj_mask, tone=self.tone, loss_type=self.loss_type)
            loss.backward()
        with torch.no_grad():
            g_tex = torch.cat([alb.grad, rough.grad.reshape(-1, 1)], 1).contiguous()
            grad = ops.tf_scatter(b.pair_row, b.pair_weight, b.seg_start, g_tex)
            self.t += 1
            ops.tf_adam(self.planes, self.adam_m, self.adam_v, b.seg_texel, grad, self.lr, self.lo, self.hi, self.betas[0], self.betas[1],
                        self.eps, self.t)
        value = float(loss.detach())
        self.loss_hist.append(value)
        return value

    def run(self, steps):
        """`steps` steps -> the loss history so far: loss_hist[i] is the loss before step i's update."""
        for _ in range(int(steps)):
            self.step()
        return list(self.loss_hist)

    # -- results
    def touched_fraction(self):
        return float(self.touched.float().mean())

    def ldr(self, sg_rgb):
        """The tone curve of the loss on shaded rows [n,3]."""
        with torch.no_grad():
            if self.tone is None:
                return sg_rgb / (sg_rgb + 1.0)
            return self.tone.hdr2ldr(sg_rgb, self.tone.as_input().detach())

    def psnr(self):
        """PSNR (robir_amd.metrics, data range 1) of the tone-mapped mesh view against the targets over the hit rows of all views."""
        from . import metrics
        f = self.forward()
        if f["batch"].n == 0:
            return float("nan")
        return float(metrics.psnr(self.ldr(f["sg_rgb"] + f["indir_rgb"]).float().contiguous(), f["batch"].target)[0])

    def result(self):
        """-> a MeshAsset with the refined planes (a copy)."""
        a = self.asset
        return meshrender.MeshAsset(a.vertices, a.faces, a.uv, self.planes.clone(), a.has_normal, a.vnormals)

    def settings(self):
        return {"vis": self.vis, "loss_type": self.loss_type, "tone": None if self.tone is None else type(self.tone).__name__ +
                f"(curve {self.tone._curve})", "batch": self.batch, "views": self.M, "lr": self.lr, "betas": list(self.betas), "eps": self.eps,
                "lo": self.lo, "hi": self.hi, "filter": self.filter, "resolution": int(self.planes.shape[0]), "steps": self.t}

    def save(self, out_dir, extra=None):
        """Writes the refined asset: mesh.obj / mesh.mtl copied and maps.npz with every key of the input (albedo and roughness replaced) when
        the asset came from a directory -- otherwise maps.npz holds the four material planes and the OBJ is written from the asset --,
        albedo.png and roughness.png rewritten, fit.json with the settings, the loss history and the touched-texel fraction -> out_dir."""
        from . import mesh as _mesh, texture
        os.makedirs(out_dir, exist_ok=True)
        p = self.planes.detach().cpu().numpy()
        alb, rough = np.ascontiguousarray(p[..., 0:3]), np.ascontiguousarray(p[..., 3])
        if self.asset_dir is not None:
            for name in os.listdir(self.asset_dir):
                if name not in ("maps.npz", "albedo.png", "roughness.png", "fit.json") and os.path.isfile(os.path.join(self.asset_dir, name)):
                    shutil.copyfile(os.path.join(self.asset_dir, name), os.path.join(out_dir, name))
            with np.load(os.path.join(self.asset_dir, "maps.npz"), allow_pickle=False) as z:
                maps = {k: z[k] for k in z.files}
        else:
            a = self.asset
            maps = {"metallic": p[..., 4].copy(), "uv": a.uv.cpu().numpy()}
            if a.has_normal:
                maps["normal"] = p[..., 5:8].copy()
            texture.save_obj(os.path.join(out_dir, "mesh.obj"), a.vertices, a.faces, a.uv, a.vnormals, mtl="mesh.mtl")
            with open(os.path.join(out_dir, "mesh.mtl"), "w") as f:
                f.write("# robir_amd.texfit\nnewmtl baked\nKa 0 0 0\nKd 1 1 1\nKs 0 0 0\nillum 2\nmap_Kd albedo.png\nmap_Pr roughness.png\n")
        maps["albedo"] = alb.reshape(np.shape(maps["albedo"])) if "albedo" in maps else alb
        maps["roughness"] = rough.reshape(np.shape(maps["roughness"])) if "roughness" in maps else rough
        np.savez(os.path.join(out_dir, "maps.npz"), **maps)
        texture.save_png(os.path.join(out_dir, "albedo.png"), _mesh._srgb(alb.astype(np.float64)))
        texture.save_png(os.path.join(out_dir, "roughness.png"), rough)
        doc = {"settings": self.settings(), "loss_hist": list(self.loss_hist), "touched_fraction": self.touched_fraction()}
        doc.update(extra or {})
        with open(os.path.join(out_dir, "fit.json"), "w") as f:
            json.dump(doc, f, indent=1)
        return out_dir


# ----------------------------------------------------------------------------------------- command line
def synthetic_views(model, n_views, size):
    """Targets for --synthetic: render.render_view of the model from orbit_poses of synth_camera's pose -> the dict AtlasFit takes; the images
    are the tone-mapped prediction where the view hits the object, masks the hit pixels."""
    from . import render, synth
    uv, pose, K = synth.synth_camera(size, size)
    poses = orbit_poses(pose, n_views)
    shift = model.gamma.hdr_shift.as_input().detach()
    images, masks = [], []
    for k in range(int(n_views)):
        out = render.render_view(model, uv, poses[k], K)
        hit = out["network_object_mask"].reshape(-1)
        images.append(model.gamma.hdr_shift.hdr2ldr(out["sg_rgb"] + out["indir_rgb"], shift).reshape(size, size, 3).float())
        masks.append(hit.reshape(size, size).float())
    return {"images": torch.stack(images), "masks": torch.stack(masks), "poses": torch.from_numpy(poses),
            "intrinsics": torch.from_numpy(K)[None].repeat(int(n_views), 1, 1)}


def main(argv=None):
    ap = argparse.ArgumentParser(description="Fit the albedo and roughness planes of a baked mesh to views through the mesh renderer on the GPU.")
    ap.add_argument("--asset", required=True, help="directory written by robir_amd.texture (mesh.obj, maps.npz)")
    ap.add_argument("--views", help="views.npz: images [M,H,W,3], poses [M,4,4], intrinsics [M,3,3], optionally masks [M,H,W]")
    ap.add_argument("--synthetic", action="store_true", help="the synthetic model of robir_amd.synth renders the targets")
    ap.add_argument("--n-views", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--light", help="directory holding sg_128.npy: shade under this light instead of the model's")
    ap.add_argument("--vis", default="none", choices=("none", "network", "octree"))
    ap.add_argument("--loss", default="L1", choices=("L1", "L2"))
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--batch", type=int)
    ap.add_argument("--filter", type=int, default=1, choices=(0, 1))
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    if bool(a.views) == bool(a.synthetic):
        ap.error("give --views or --synthetic")
    if a.views and not a.light:
        ap.error("--views needs --light (the light the asset is shaded under)")
    dev = torch.device("cuda:0")
    model = tone = None
    if a.synthetic:
        from . import renderer
        model = renderer.build_synthetic_model(dev)          # with its octrees: the targets are ray traced
        views = synthetic_views(model, a.n_views, a.size)
        tone = model.gamma.hdr_shift
    else:
        with np.load(a.views, allow_pickle=False) as z:
            views = {k: z[k] for k in z.files}
    fit = AtlasFit(a.asset, views, light=a.light, model=model, vis=a.vis, tone=tone, loss_type=a.loss, batch=a.batch, lr=a.lr, filter=a.filter)
    before = fit.psnr()
    fit.run(a.steps)
    after = fit.psnr()
    fit.save(a.out, extra={"psnr_before": before, "psnr_after": after})
    print(f"wrote {a.out}: {a.steps} steps, loss {fit.loss_hist[0] if fit.loss_hist else float('nan'):.6g} -> "
          f"{fit.loss_hist[-1] if fit.loss_hist else float('nan'):.6g}, PSNR {before:.2f} -> {after:.2f} dB, "
          f"{100 * fit.touched_fraction():.1f} % of the texels touched")


if __name__ == "__main__":
    main()
