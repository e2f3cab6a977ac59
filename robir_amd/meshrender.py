"""A view of the baked mesh on the device: what does this OBJ with these maps look like from a camera, under the model's or another light.

The asset chain (robir_amd.mesh -> robir_amd.texture) ends in mesh.obj / maps.npz; this module draws them.  The vertices are projected, the
faces binned into 8 x 8-pixel tiles and rasterised with a depth test and perspective-correct weights, and a G-buffer (position, uv, view
direction, a fetch of the baked planes) is formed for the hit pixels -- HIP kernels of librobir_hip_raster.so (include/robir_hip_raster.h,
DESIGN 4.13).  The hit rows are shaded by the existing sg_render.render_with_all_sg, and the result carries robir_amd.render's keys, so
`python -m robir_amd.evaluate --pred meshview.npz --gt neuralview.npz` scores the round trip neural view -> mesh + atlas -> view.

    python -m robir_amd.meshrender --asset DIR --synthetic --size 800 --out view.npz                       (direct SG shading, --vis none)
    python -m robir_amd.meshrender --asset DIR --neus-ckpt logs/.../200000.tar --stage-ckpt exps/.../latest.pth \
        --cameras data/hotdog/transforms_test.json --index 0 --size 800 [--light envmaps/envmap6] [--vis network|octree] --out view.npz

Conventions: the renderer's camera (looks along -z, y up; pose is camera-to-world, 4 x 4 or the 7-vector form); the sample point of pixel
(row r, column c) is (u, v) = (c, r), the integer uv grid of synth.synth_camera / render.blender_camera.  No clipping: a face with a corner
behind the near plane is skipped whole, so a camera INSIDE the object is out of scope.  Everything here runs under no_grad; robir_amd.texfit
takes the gradient of this view with respect to the albedo and roughness texels and fits them to target views.
"""
import argparse
import os

import numpy as np
import torch

from . import ops

PLANES = (("albedo", 3), ("roughness", 1), ("metallic", 1), ("normal", 3))       # the stack the G-buffer fetches, in this order
KEYS = ("sg_rgb", "indir_rgb", "diffuse_albedo", "roughness", "metallic", "vis_shadow", "normal_map", "normals", "network_object_mask",
        "bg_rgb", "depth")


# ----------------------------------------------------------------------------------------- projection, rasteriser, G-buffer
def pose_inverse(pose):
    """pose (camera-to-world, [4,4], [3,4] or the 7-vector (quaternion | centre) form) -> (pose_inv [4,4], cam_loc [3]), the inverse formed
    as robir_amd/observe.py forms it: the upper 3 x 4 block in an identity, torch.inverse."""
    pose = ops.pose_matrix(pose) if pose.dim() == 1 else pose
    p = torch.eye(4, device=pose.device)
    p[:3, :4] = pose[:3, :4].float()
    return torch.inverse(p).float().contiguous(), p[:3, 3].contiguous()


def project_vertices(vertices, pose, K):
    """vertices [V,3] -> screen [V,4] = (u, v, 1 / zc, zc): the pixel position at which the camera sees the vertex and its depth along the
    viewing axis (positive in front of the camera)."""
    pinv, _ = pose_inverse(pose.to(vertices.device))
    return ops.rs_project(vertices, pinv, K[:3, :3].to(vertices.device))


def rasterize_screen(screen, faces, H, W, near=1e-4, cull=0):
    """screen [V,4] of project_vertices -> (face_id [H,W] int32, -1 where empty, bary [H,W,2], depth [H,W]).  One host read (the number of
    (tile, face) pairs) sits between the count and the emit kernels; the prefix sum and the stable sort by tile are torch's."""
    H, W = int(H), int(W)
    faces = faces.to(torch.int32).contiguous()
    dev, F = screen.device, faces.shape[0]
    ntiles = ((W + ops.RS_TILE - 1) // ops.RS_TILE) * ((H + ops.RS_TILE - 1) // ops.RS_TILE)
    empty = lambda: ops.rs_raster(screen, faces, H, W, near, cull, torch.zeros(ntiles + 1, dtype=torch.int32, device=dev),
                                  torch.zeros(0, dtype=torch.int32, device=dev))
    if F == 0:
        return empty()
    counts = ops.rs_bin_count(screen, faces, H, W, near, cull)
    incl = torch.cumsum(counts.to(torch.int64), 0)
    P = int(incl[-1])                                            # the single sync
    if P >= 2 ** 31:
        raise ValueError(f"rasterize: {P} (tile, face) pairs do not fit 32-bit indices")
    if P == 0:
        return empty()
    pair_tile, pair_face = ops.rs_bin_emit(screen, faces, H, W, near, cull, (incl - counts).contiguous(), P)
    tiles, order = torch.sort(pair_tile, stable=True)            # faces stay ascending inside a tile
    pair_face = pair_face[order].contiguous()
    tile_start = torch.searchsorted(tiles, torch.arange(ntiles + 1, dtype=torch.int32, device=dev)).to(torch.int32)
    return ops.rs_raster(screen, faces, H, W, near, cull, tile_start, pair_face)


def rasterize(vertices, faces, pose, K, H, W, near=1e-4, cull=0):
    """The mesh as the camera (pose, K) sees it on the H x W pixel grid -> (face_id [H,W] int32, -1 where empty; bary [H,W,2]: the
    perspective-correct weights of corners 0 and 1; depth [H,W]: the distance along the viewing axis, 0 where empty).  The nearest face
    wins, an equal depth goes to the lowest face index.  cull: 0 none, 1 drops faces of negative screen area, 2 those of positive area.  A
    face with a corner closer than `near` is skipped whole (no clipping): a camera inside the object is out of scope."""
    with torch.no_grad():
        return rasterize_screen(project_vertices(ops._f32(vertices), pose, K), faces, H, W, near, cull)


def gbuffer(face_id, bary, vertices, faces, uv, cam_loc, planes=None, filter=1, vnormals=None, index=None):
    """The G-buffer of a rasterised view -> {"position" [n,3], "uv" [n,2], "view_dir" [n,3] (unit, from the point to the camera), "tex" [n,C]
    (the plane stack planes [R,R,C] at uv; filter 0: the containing texel, 1: texture.TexSampler's bilinear) and "normal" [n,3] (the
    interpolated, normalised vertex normals vnormals [V,3])}, the last two only when their input is given.  index None: all H W pixels in
    row-major order (zeros where empty); index [n] int64: those flat pixels only -- the hit rows, like the renderer."""
    with torch.no_grad():
        p, q, vd, tex, nrm = ops.rs_gbuffer(face_id, bary, faces.to(torch.int32).contiguous(), vertices, uv, cam_loc, planes, filter, vnormals,
                                            index)
    out = {"position": p, "uv": q, "view_dir": vd}
    if tex is not None:
        out["tex"] = tex
    if nrm is not None:
        out["normal"] = nrm
    return out


# ----------------------------------------------------------------------------------------- the asset
class MeshAsset:
    """What a view needs of a bake, on one device: vertices [V,3], faces [F,3] int32, uv [F,3,2] per face corner, planes [R,R,8] = albedo |
    roughness | metallic | normal (PLANES), has_normal (False: the normal channels are zero and vnormals [V,3] serve instead)."""

    def __init__(self, vertices, faces, uv, planes, has_normal=True, vnormals=None):
        self.vertices, self.faces, self.uv, self.planes = vertices, faces, uv, planes
        self.has_normal, self.vnormals = has_normal, vnormals


def stack_planes(maps, device):
    """{"albedo" [R,R,3], "roughness" [R,R], "metallic" [R,R], "normal" [R,R,3] (optional)} of tensors or arrays -> ([R,R,8], has_normal)."""
    to = lambda a: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device).float()
    alb = to(maps["albedo"])
    R = alb.shape[0]
    has_normal = "normal" in maps and maps["normal"] is not None
    parts = [alb.reshape(R, R, 3), to(maps["roughness"]).reshape(R, R, 1), to(maps["metallic"]).reshape(R, R, 1),
             to(maps["normal"]).reshape(R, R, 3) if has_normal else torch.zeros(R, R, 3, device=device)]
    return torch.cat(parts, -1).contiguous(), has_normal


def load_asset(asset, device="cuda"):
    """A texture.TextureSet, a MeshAsset or a directory written by TextureSet.export (mesh.obj with v / vt / f v/vt, maps.npz) -> MeshAsset."""
    from . import texture
    dev = torch.device(device)
    if isinstance(asset, MeshAsset):
        return asset
    if isinstance(asset, texture.TextureSet):
        planes, has_normal = stack_planes(asset.planes(), dev)
        return MeshAsset(ops._f32(asset.mesh.vertices.to(dev)), asset.mesh.faces.to(dev).to(torch.int32).contiguous(), ops._f32(asset.uv.to(dev)),
                         planes, has_normal, asset.mesh.normals)
    o = texture.load_obj(os.path.join(asset, "mesh.obj"))
    if "vt" not in o or "faces_vt" not in o:
        raise ValueError(f"{asset}/mesh.obj carries no texture coordinates")
    with np.load(os.path.join(asset, "maps.npz"), allow_pickle=False) as z:
        planes, has_normal = stack_planes({k: z[k] for k in ("albedo", "roughness", "metallic", "normal") if k in z.files}, dev)
    uv = torch.from_numpy(o["vt"][o["faces_vt"].astype(np.int64)]).to(dev).contiguous()
    vn = torch.from_numpy(o["vn"]).to(dev) if "vn" in o and o["vn"].shape == o["vertices"].shape else None
    return MeshAsset(torch.from_numpy(o["vertices"]).to(dev), torch.from_numpy(o["faces"]).to(dev), uv, planes, has_normal, vn)


def load_light(path, device="cuda"):
    """`<path>/sg_128.npy`, the light SGs EnvmapMaterialNetwork.load_light reads -> [M,7] on the device."""
    return torch.from_numpy(np.load(os.path.join(path, "sg_128.npy"))).float().to(device).contiguous()


# ----------------------------------------------------------------------------------------- the view
def _unit(v):
    return (v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)).contiguous()


def _rows(draws, idx, n_pixels):
    """A draw with one row per pixel of the image is narrowed to the hit rows (the renderer takes one row per hit)."""
    return {k: (v[idx].contiguous() if torch.is_tensor(v) and v.dim() >= 2 and v.shape[0] == n_pixels and k not in ("dvis_theta", "dvis_phi")
                else v) for k, v in (draws or {}).items()}


def light_and_f0(model, light, dev):
    """(light SGs [M,7], specular_reflectance) a view is shaded under: those of `light` ([M,7] or a directory with sg_128.npy; it overrides
    the model's) or of `model`; f0 = 0.02 without a model.  Detached: constants of whoever shades with them."""
    with torch.no_grad():
        if light is not None:
            lgt = light.to(dev).float().contiguous() if torch.is_tensor(light) else load_light(light, dev)
        else:
            mn = model.envmap_material_network
            lgt = (mn.restrict_lobes_upper(mn.lgtSGs) if mn.upper_hemi else mn.lgtSGs).detach()
        f0 = model.envmap_material_network.specular_reflectance.detach().abs() if model is not None else torch.full((1, 1), 0.02, device=dev)
    return lgt, f0


def shade_rows(points, normal, view_dir, albedo, roughness, model=None, light=None, vis="none", draws=None):
    """sg_render.render_with_all_sg on n surface rows with materials given per row (points, normal, view_dir, albedo [n,3], roughness [n,1]),
    under the lights and specular_reflectance of `model` or of `light` ([M,7] or a directory with sg_128.npy; it overrides the model's) ->
    render_with_all_sg's dict (sg_rgb, indir_rgb, vis_shadow, ...).  vis as in render_mesh; draws: one row per row of `points`."""
    from . import sg_render
    dev, n = points.device, points.shape[0]
    d = draws or {}
    with torch.no_grad():
        lgt, f0 = light_and_f0(model, light, dev)
        indir_sgs = indir_int = vis_model = None
        if vis != "none":
            from .octree_tracing import OctreeVisModel
            vis_model = model.visibility_network if vis == "network" else OctreeVisModel(model.octree_ray_tracer)
            shift = model.gamma.hdr_shift.as_input().detach()
            indir_sgs, integral = model.indirect_illum_network(points, shift.expand(n, 1).contiguous(), noise=d.get("illum_randn"))
            indir_int = ops.abs_scale(integral, 2 * np.pi, take_abs=False)
        return sg_render.render_with_all_sg(points=points, normal=normal, viewdirs=view_dir, lgtSGs=lgt, specular_reflectance=f0,
                                            roughness=roughness, diffuse_albedo=albedo, indir_integral=indir_int, indir_lgtSGs=indir_sgs,
                                            VisModel=vis_model, testing=bool(getattr(model, "testing", True)), metallic=None, draws=d)


def view_rows(a, pose, K, H, W, filter=1, near=1e-4, cull=0):
    """The per-view setup that render_mesh and robir_amd.texfit share: the MeshAsset `a` projected, rasterised and its G-buffer formed for the
    hit rows -> (face_id [H,W] int32, depth [H,W], hit [H W] bool, idx [n] int64: the flat hit pixels, g: gbuffer's dict for those rows --
    position, uv, view_dir, tex from all of a.planes, and normal from the vertex normals for an asset without a normal plane)."""
    with torch.no_grad():
        pinv, cam = pose_inverse(pose)
        screen = ops.rs_project(a.vertices, pinv, K[:3, :3])
        face_id, bary, depth = rasterize_screen(screen, a.faces, H, W, near, cull)
        hit = face_id.reshape(-1) >= 0
        idx = hit.nonzero()[:, 0].contiguous()
        g = gbuffer(face_id, bary, a.vertices, a.faces, a.uv, cam, a.planes, filter, None if a.has_normal else a.vnormals, idx)
    return face_id, depth, hit, idx, g


def render_mesh(asset, pose, K, H, W, model=None, light=None, vis="none", filter=1, draws=None, near=1e-4, cull=0):
    """The view of a baked asset from the camera (pose, K) on the H x W pixel grid -> dict of [H W, .] tensors with robir_amd.render's keys:
    sg_rgb, indir_rgb, diffuse_albedo, roughness, metallic, vis_shadow, normals, normal_map, network_object_mask, bg_rgb, depth (and
    points, uv, face_id; pred_rgb with a model).  Rows outside the mesh hold ones as the renderer's do (indir_rgb and depth: zeros).

    asset: a texture.TextureSet, a MeshAsset or a directory written by TextureSet.export.  Materials come from the G-buffer: the planes
    fetched at the interpolated uv (filter 1: bilinear, 0: the containing texel); the normal is the fetched plane renormalised (the
    interpolated vertex normal for an asset without a normal plane).  Shading is sg_render.render_with_all_sg on the hit rows, with the
    lights and specular_reflectance of `model` (an IDRNetwork) or of `light` (a directory with sg_128.npy, or [M,7]; it overrides the model's).
      vis="none":     VisModel=None, no indirect term -- direct SG shading, what a standard PBR viewer shows; needs no model;
      vis="network":  the model's visibility network and its indirect-illumination network, as forward('Material');
      vis="octree":   OctreeVisModel on the model's octree tracer instead of the network.
    draws: synth.pbr_draws' dict; a per-row draw may also hold one row per PIXEL ([H W, .]) and is then narrowed to the hit rows."""
    from . import sg_render
    if vis not in ("none", "network", "octree"):
        raise ValueError(f"render_mesh: vis = {vis!r}, expected 'none', 'network' or 'octree'")
    if vis != "none" and model is None:
        raise ValueError(f"render_mesh: vis = {vis!r} needs the model's visibility and indirect-illumination networks")
    if model is None and light is None:
        raise ValueError("render_mesh: give a model or a light (a directory with sg_128.npy, or [M,7] light SGs)")
    dev = next(model.parameters()).device if model is not None else (light.device if torch.is_tensor(light) else torch.device("cuda:0"))
    a = load_asset(asset, dev)
    H, W = int(H), int(W)
    N = H * W
    pose, K = torch.as_tensor(pose).to(dev).float(), torch.as_tensor(K).to(dev).float()
    with torch.no_grad():
        face_id, depth, hit, idx, g = view_rows(a, pose, K, H, W, filter, near, cull)
        n = idx.numel()
        out = {k: torch.ones(N, 3, device=dev) for k in ("sg_rgb", "diffuse_albedo", "roughness", "vis_shadow", "normals", "normal_map",
                                                         "bg_rgb", "points")}
        out.update(metallic=torch.ones(N, 1, device=dev), indir_rgb=torch.zeros(N, 3, device=dev), network_object_mask=hit,
                   depth=depth.reshape(N, 1), face_id=face_id.reshape(N, 1), uv=torch.zeros(N, 2, device=dev))
        if model is not None and model.envmap_material_network.envmap is not None:
            uv_px = torch.stack(torch.meshgrid(torch.arange(W, device=dev), torch.arange(H, device=dev), indexing="xy"), -1).reshape(N, 2).float()
            p44 = torch.eye(4, device=dev)
            p44[:3, :4] = (ops.pose_matrix(pose) if pose.dim() == 1 else pose)[:3, :4]
            out["bg_rgb"] = sg_render.render_envmap(model.envmap_material_network.envmap, ops.camera_rays(p44.contiguous(), K[:3, :3].contiguous(), uv_px))
        if n == 0:
            return out
        tex = g["tex"]
        alb, rough, metal = tex[:, 0:3].contiguous(), tex[:, 3:4].contiguous(), tex[:, 4:5].contiguous()
        if a.has_normal:
            nrm = _unit(tex[:, 5:8])
        elif "normal" in g:
            nrm = g["normal"]
        else:
            raise ValueError("render_mesh: the asset has neither a normal plane nor vertex normals")
        pts, vd = g["position"], g["view_dir"]
        r = shade_rows(pts, nrm, vd, alb, rough, model=model, light=light, vis=vis, draws=_rows(draws, idx, N))
        for k, v in (("sg_rgb", r["sg_rgb"]), ("indir_rgb", r["indir_rgb"]), ("vis_shadow", r["vis_shadow"]), ("diffuse_albedo", alb),
                     ("roughness", rough.expand(n, 3)), ("metallic", metal), ("normals", nrm), ("normal_map", nrm), ("points", pts),
                     ("uv", g["uv"])):
            out[k][idx] = v.float()
        if model is not None:
            shift = model.gamma.hdr_shift.as_input().detach()
            pred = model.gamma.hdr_shift.hdr2ldr(out["sg_rgb"] + out["indir_rgb"], shift)
            out["pred_rgb"] = torch.where(hit[:, None], pred, out["bg_rgb"])
    return out


# ----------------------------------------------------------------------------------------- command line
def main(argv=None):
    ap = argparse.ArgumentParser(description="Render a baked mesh (mesh.obj + maps.npz of robir_amd.texture) from a camera on the GPU.")
    ap.add_argument("--asset", required=True, help="directory written by robir_amd.texture (mesh.obj, maps.npz)")
    ap.add_argument("--synthetic", action="store_true", help="the synthetic weights and camera of robir_amd.synth")
    ap.add_argument("--neus-ckpt")
    ap.add_argument("--stage-ckpt")
    ap.add_argument("--cameras", help="a transforms_*.json; without it the synthetic camera")
    ap.add_argument("--index", type=int, default=0)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--light", help="directory holding sg_128.npy: shade under this light instead of the model's")
    ap.add_argument("--vis", default="none", choices=("none", "network", "octree"))
    ap.add_argument("--filter", type=int, default=1, choices=(0, 1), help="0: the containing texel, 1: bilinear")
    ap.add_argument("--cull", type=int, default=0, choices=(0, 1, 2))
    ap.add_argument("--out", required=True)
    ap.add_argument("--png-dir", help="also write the PNG set of robir_amd.render into this directory")
    a = ap.parse_args(argv)
    if not a.synthetic and not a.neus_ckpt and not a.light:
        ap.error("give --synthetic, --neus-ckpt or, for --vis none, --light")
    from . import render, renderer, synth
    dev = torch.device("cuda:0")
    H = W = a.size
    model = None
    if a.synthetic:
        model = renderer.build_synthetic_model(dev, build_octrees=a.vis == "octree")
    elif a.neus_ckpt:
        import warnings
        with warnings.catch_warnings():          # the NeuS checkpoint is loaded explicitly on the next lines
            warnings.simplefilter("ignore", RuntimeWarning)
            model = renderer.IDRNetwork(renderer.hotdog_conf())
        from .nets import load_neus_checkpoint
        load_neus_checkpoint(model.implicit_network.neus_model, a.neus_ckpt)
        if a.stage_ckpt:
            render.load_stage_checkpoint(model, a.stage_ckpt)
        model = model.to(dev).eval()
        if a.vis == "octree":
            model.octree_ray_tracer.generate(None)
    _, pose, K = render.blender_camera(a.cameras, a.index, H, W) if a.cameras else synth.synth_camera(H, W)
    if model is not None and a.light:
        model.envmap_material_network.load_light(a.light)
    out = render_mesh(a.asset, torch.from_numpy(pose), torch.from_numpy(K), H, W, model=model,
                      light=None if model is not None else a.light, vis=a.vis, filter=a.filter, cull=a.cull)
    np.savez_compressed(a.out, **{k: v.detach().cpu().numpy().reshape(H, W, -1) for k, v in out.items()})
    print("wrote", a.out, "hit fraction %.3f" % float(out["network_object_mask"].float().mean()))
    if a.png_dir:
        names = render.save_relight_images(out, H, W, a.png_dir, str(a.index), "relit" if a.light else "origin")
        print("wrote", ", ".join("%s_%d.png" % (n, a.index) for n in names), "to", a.png_dir)


if __name__ == "__main__":
    main()
