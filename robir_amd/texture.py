"""Materials of the learned scene baked into a UV texture atlas on the device, written as a textured OBJ.

Counterpart of the reference's model/texture_model.py (gen_uv_map, erode_map, get_vert_norm_mask_maps, TexSampler), model/rasterizor.py (the
OpenGL pass that draws vertex attributes into UV space) and scripts/tex_extract.py (albedo.png / roughness.png / normal.png beside an OBJ).
Here the UV-space rasteriser, the interpolation, the dilation and the sampler are HIP kernels (librobir_hip_texbake.so,
include/robir_hip_texbake.h): no GL context, no xatlas.  The default unwrap is a closed-form atlas with one right triangle per
face (atlas_uv); a mesh that carries its own UVs (load_obj, `uv=`) goes through the same rasteriser.  Everything runs under no_grad in
eval mode.

    python -m robir_amd.texture --synthetic [--scene nonconvex] --mesh-resolution 256 --resolution 4096 --out DIR
    python -m robir_amd.texture --neus-ckpt logs/.../200000.tar [--stage-ckpt exps/.../latest.pth] [--obj user.obj] --out DIR
    ... --views views.npz        also bakes what the training views observe (observed.png; robir_amd/observe.py)

Conventions: images are [R,R,C] with row 0 at the top; a UV pair is in OBJ convention (v up): texel space is x = u R, y = (1 - v) R.
"""
import argparse
import os
import struct
import time
import zlib

import numpy as np
import torch

from . import mesh as _mesh
from . import ops

CHUNK = 1 << 18
FILES = ("mesh.obj", "mesh.mtl", "albedo.png", "roughness.png", "metallic.png", "normal.png", "maps.npz")
OBSERVED_FILE = "observed.png"          # written next to FILES once bake_observations has run
OBSERVED_PLANES = ("observed", "observed_var", "observed_count")


# ----------------------------------------------------------------------------------------- atlas, rasteriser, interpolation, dilation
def atlas_uv(n_faces, resolution, device="cuda"):
    """uv [F,3,2] of the per-triangle atlas: face f in cell f >> 1 of a grid of ceil(sqrt(ceil(F / 2))) columns, half f & 1, each cell
    resolution // ncols texels wide (include/robir_hip_texbake.h).  ValueError below 6 texels per cell, naming the smallest resolution."""
    return ops.tb_atlas_uv(n_faces, resolution, torch.device(device))


def _corner_uv(uv, faces_vt=None):
    if faces_vt is not None:
        vt = ops._f32(uv)
        if vt.dim() != 2 or vt.shape[1] != 2 or faces_vt.dim() != 2 or faces_vt.shape[1] != 3:
            raise ValueError(f"rasterize_uv: vt must be [Vt,2] and faces_vt [F,3], got {tuple(vt.shape)}, {tuple(faces_vt.shape)}")
        idx = faces_vt.to(device=vt.device, dtype=torch.int64)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= vt.shape[0]):
            raise ValueError("rasterize_uv: faces_vt indexes outside vt")
        return vt[idx].contiguous()
    return ops._tb_uv(uv)


def rasterize_uv(uv, resolution, faces_vt=None):
    """uv [F,3,2] per face corner -- or (vt [Vt,2], faces_vt [F,3]), an OBJ's indexed form -- -> (face_id [R,R] int32, -1 where empty,
    bary [R,R,2]: the weights of corners 0 and 1).  The first face in index order that covers a texel centre owns it; one host read (the
    number of (tile, face) pairs) sits between the count and the emit kernels."""
    R = int(resolution)
    if not 1 <= R <= ops.TB_MAX_RESOLUTION:
        raise ValueError(f"rasterize_uv: resolution {R} outside 1 .. {ops.TB_MAX_RESOLUTION}")
    uv = _corner_uv(uv, faces_vt)
    dev, F = uv.device, uv.shape[0]
    ntiles = (R + ops.TB_TILE - 1) // ops.TB_TILE
    counts = ops.tb_bin_count(uv, R)
    incl = torch.cumsum(counts.to(torch.int64), 0)
    P = int(incl[-1]) if F else 0                                # the single sync
    if P >= 2 ** 31:
        raise ValueError(f"rasterize_uv: {P} (tile, face) pairs do not fit 32-bit indices")
    if P == 0:
        tile_start = torch.zeros(ntiles * ntiles + 1, dtype=torch.int32, device=dev)
        return ops.tb_raster(uv, R, tile_start, torch.zeros(0, dtype=torch.int32, device=dev))
    pair_tile, pair_face = ops.tb_bin_emit(uv, R, (incl - counts).contiguous(), P)
    tiles, order = torch.sort(pair_tile, stable=True)            # faces stay ascending inside a tile
    pair_face = pair_face[order].contiguous()
    tile_start = torch.searchsorted(tiles, torch.arange(ntiles * ntiles + 1, dtype=torch.int32, device=dev)).to(torch.int32)
    return ops.tb_raster(uv, R, tile_start, pair_face)


def interpolate(face_id, bary, faces, attr, index=None):
    """sum_k b_k attr[faces[face_id][k]] per texel: attr [V,C] -> [R,R,C], zeros where empty (the reference's render_texture).  index [n]
    int64 flat texel indices: -> [n,C] for those texels only."""
    return ops.tb_interp(face_id, bary, faces.to(torch.int32), attr, index)


def dilate(image, mask, rings=1):
    """`rings` steps of the reference's erode_map: image [H,W,C] or [H,W], mask [H,W] (non-zero = covered) -> (image', mask' uint8).  An
    uncovered texel with a covered 8-neighbour becomes the mean of its covered neighbours and counts as covered in the next ring.  The
    reference's get_vert_norm_mask_maps is dilate(position | normal, mask, 2) with dilate(mask, mask, 1)'s mask."""
    flat = image.dim() == 2
    img = ops._f32(image[..., None] if flat else image)
    m = (mask != 0).to(torch.uint8).contiguous()
    for _ in range(int(rings)):
        img, m = ops.tb_dilate(img, m)
    return (img[..., 0] if flat else img), m


# ----------------------------------------------------------------------------------------- the bake
class TextureSet:
    """The baked planes, float32 on the device: albedo [R,R,3], roughness [R,R], metallic [R,R], normal [R,R,3] (unit SDF gradient, object
    space), position [R,R,3], all dilated `rings` times; mask [R,R] (1 where a face covers the texel centre, before dilation); face_id
    [R,R] int32; uv [F,3,2] and the mesh they belong to.  After bake_observations also observed [R,R,3] (the mean colour the training views
    see), observed_var [R,R,3] and observed_count [R,R] (the number of contributing views), dilated like the others."""

    def __init__(self, mesh, uv, face_id, bary, albedo, roughness, metallic, normal, position, mask):
        self.mesh, self.uv, self.face_id, self.bary = mesh, uv, face_id, bary
        self.albedo, self.roughness, self.metallic, self.normal, self.position, self.mask = albedo, roughness, metallic, normal, position, mask
        self.observed = self.observed_var = self.observed_count = None
        self.rings = 4
        self.stats = {}

    @property
    def resolution(self):
        return self.face_id.shape[0]

    def planes(self):
        return {k: getattr(self, k) for k in ("albedo", "roughness", "metallic", "normal", "position", "mask")}

    def sampler(self, scale=1.0):
        """A TexSampler on the baked position and normal with the mask grown by one ring, the reference's composition."""
        return TexSampler(self.position, self.normal, dilate(self.mask, self.mask, 1)[1].float(), scale)

    def observed_planes(self):
        """The planes of bake_observations; empty before it has run."""
        return {k: getattr(self, k) for k in OBSERVED_PLANES if getattr(self, k) is not None}

    def bake_observations(self, model, focus, rings=None, chunk=None):
        """Adds the planes observed, observed_var [R,R,3] and observed_count [R,R]: at every covered texel, the mean and the variance of the
        colours that the training views of `focus` (robir_amd.observe.FocusSampler) see at the texel's baked position, weighted by
        max(-n . view_dir, 0) with the baked normal, over the views that model.octree_ray_tracer finds unoccluded
        (robir_amd.observe.observed_color); dilated `rings` times (default: as many as the bake's other planes).  -> self."""
        from . import observe
        R = self.resolution
        rings = self.rings if rings is None else int(rings)
        covered = self.mask.reshape(-1) > 0
        idx = torch.nonzero(covered).reshape(-1)
        dev = self.position.device
        with torch.no_grad():
            x, n = self.position.reshape(-1, 3)[idx].contiguous(), self.normal.reshape(-1, 3)[idx].contiguous()
            mean, var, _, count = observe.observed_color(model, focus, x, n, chunk=chunk)
            planes = {"observed": torch.zeros(R * R, 3, device=dev), "observed_var": torch.zeros(R * R, 3, device=dev),
                      "observed_count": torch.zeros(R * R, 1, device=dev)}
            planes["observed"][idx], planes["observed_var"][idx], planes["observed_count"][idx] = mean, var, count.float()[:, None]
            mask8 = covered.reshape(R, R).to(torch.uint8)
            for k, v in planes.items():
                img = dilate(v.reshape(R, R, -1), mask8, rings)[0]
                setattr(self, k, img[..., 0].contiguous() if img.shape[-1] == 1 else img)
        self.stats["observed_fraction"] = float((count > 0).float().mean()) if idx.numel() else 0.0
        return self

    def export(self, out_dir):
        """mesh.obj (v / vn / vt / f v/vt/vn), mesh.mtl, albedo.png (sRGB), roughness.png, metallic.png, normal.png (n 0.5 + 0.5; linear) and
        maps.npz (the float planes, face_id and uv, lossless) -> the list of paths.  After bake_observations also observed.png (sRGB), and
        maps.npz holds the three observed planes too; without it nothing else is written and nothing differs."""
        os.makedirs(out_dir, exist_ok=True)
        p = {k: v.detach().cpu().numpy() for k, v in self.planes().items()}
        extra = []
        if self.observed is not None:
            p.update({k: v.detach().cpu().numpy() for k, v in self.observed_planes().items()})
            save_png(os.path.join(out_dir, OBSERVED_FILE), _mesh._srgb(p["observed"].astype(np.float64)))
            extra = [OBSERVED_FILE]
        save_png(os.path.join(out_dir, "albedo.png"), _mesh._srgb(p["albedo"].astype(np.float64)))
        save_png(os.path.join(out_dir, "roughness.png"), p["roughness"])
        save_png(os.path.join(out_dir, "metallic.png"), p["metallic"])
        save_png(os.path.join(out_dir, "normal.png"), p["normal"].astype(np.float64) * 0.5 + 0.5)
        np.savez(os.path.join(out_dir, "maps.npz"), face_id=self.face_id.cpu().numpy(), uv=self.uv.cpu().numpy(), **p)
        save_obj(os.path.join(out_dir, "mesh.obj"), self.mesh.vertices, self.mesh.faces, self.uv, self.mesh.normals, mtl="mesh.mtl")
        with open(os.path.join(out_dir, "mesh.mtl"), "w") as f:
            f.write("# robir_amd.texture\nnewmtl baked\nKa 0 0 0\nKd 1 1 1\nKs 0 0 0\nillum 2\nmap_Kd albedo.png\nmap_Pr roughness.png\n"
                    "map_Pm metallic.png\n# object-space normal map (n * 0.5 + 0.5, linear): normal.png\n")
        return [os.path.join(out_dir, n) for n in FILES + tuple(extra)]


def _newton_step(src, x, f, g, halvings=4):
    """One damped Newton step onto the zero set: x - t f grad f / |grad f|^2 with t = 1, halved (up to `halvings` times, for the points concerned
    only) while the step does not bring |f| down; a point that no t improves stays where it is.  On a coarse mesh of a non-convex surface the
    plain step of mesh.vertex_attributes can throw a texel's point far off the surface where |grad f| is small; this one never raises |f|."""
    step = f[:, None] * g / (g * g).sum(-1, keepdim=True).clamp_min(1e-20)
    x1 = (x - step).contiguous()
    f1, g1 = src.value_grad(x1)
    bad = ~(f1.abs() <= f.abs())                                     # NaN counts as not improved
    t = 1.0
    for _ in range(int(halvings)):
        idx = torch.nonzero(bad).reshape(-1)
        if idx.numel() == 0:
            return x1, f1, g1
        t *= 0.5
        xs = (x[idx] - t * step[idx]).contiguous()
        fs, gs = src.value_grad(xs)
        ok = fs.abs() < f[idx].abs()
        sel = idx[ok]
        x1[sel], f1[sel], g1[sel] = xs[ok], fs[ok], gs[ok]
        bad[sel] = False
    idx = torch.nonzero(bad).reshape(-1)
    x1[idx], f1[idx], g1[idx] = x[idx], f[idx], g[idx]
    return x1, f1, g1


def bake(model, mesh, resolution=2048, project=1, rings=4, uv=None):
    """Bake an IDRNetwork's materials onto `mesh` (robir_amd.mesh.Mesh: vertices, faces) -> TextureSet.

    The mesh is rasterised into its UVs (uv [F,3,2] per face corner; None: atlas_uv).  The covered texels, in row-major order and in chunks of
    2^18, get their interpolated position, `project` Newton steps x <- x - f grad f / |grad f|^2 onto the SDF's zero set (damped: a step
    that does not bring |f| down is halved, _newton_step), the unit SDF gradient there as the normal (not the interpolated vertex normal) and mesh.bake_materials at the projected point.  Every plane is then
    dilated `rings` times over the chart borders."""
    src = _mesh._Source(model)
    if src.net is None or src.materials_net is None:
        raise TypeError("bake: needs an IDRNetwork (an SDF network and an envmap_material_network)")
    R = int(resolution)
    verts, faces = ops._f32(mesh.vertices), mesh.faces.to(torch.int32).contiguous()
    dev, F = verts.device, faces.shape[0]
    sync = (lambda: torch.cuda.synchronize(dev)) if dev.type == "cuda" else (lambda: None)
    with torch.no_grad():
        sync()
        t0 = time.perf_counter()
        uv = atlas_uv(F, R, dev) if uv is None else _corner_uv(uv.to(dev))
        if uv.shape[0] != F:
            raise ValueError(f"bake: {uv.shape[0]} UV triangles for {F} faces")
        face_id, bary = rasterize_uv(uv, R)
        sync()
        t1 = time.perf_counter()
        covered = face_id.reshape(-1) >= 0
        idx = torch.nonzero(covered).reshape(-1).contiguous()          # row-major
        planes = {"albedo": torch.zeros(R * R, 3, device=dev), "roughness": torch.zeros(R * R, 1, device=dev),
                  "metallic": torch.zeros(R * R, 1, device=dev), "normal": torch.zeros(R * R, 3, device=dev),
                  "position": torch.zeros(R * R, 3, device=dev)}
        for i in range(0, idx.numel(), CHUNK):
            sel = idx[i:i + CHUNK].contiguous()
            x = interpolate(face_id, bary, faces, verts, sel)
            f, g = src.value_grad(x)
            for _ in range(int(project)):
                x, f, g = _newton_step(src, x, f, g)
            m = _mesh.bake_materials(src.materials_net, x)
            planes["position"][sel] = x
            planes["normal"][sel] = g / g.norm(dim=-1, keepdim=True).clamp_min(1e-20)
            for k in ("albedo", "roughness", "metallic"):
                planes[k][sel] = m[k]
        sync()
        t2 = time.perf_counter()
        mask8 = covered.reshape(R, R).to(torch.uint8)
        out = {}
        for k, v in planes.items():
            img = dilate(v.reshape(R, R, -1), mask8, rings)[0]
            out[k] = img[..., 0].contiguous() if img.shape[-1] == 1 else img
        sync()
        t3 = time.perf_counter()
    ts = TextureSet(mesh, uv, face_id, bary, mask=mask8.float(), **out)
    ts.rings = int(rings)
    ncols = int(np.ceil(np.sqrt((F + 1) // 2))) if F else 0
    ts.stats = {"covered_fraction": idx.numel() / float(R * R), "cell": R // ncols if ncols else 0, "raster_s": t1 - t0, "bake_s": t2 - t1,
                "dilate_s": t3 - t2}
    return ts


# ----------------------------------------------------------------------------------------- the surface sampler
class TexSampler:
    """The reference's TexSampler (model/texture_model.py:127-160) on maps made here: position, normal [R,R,3] and mask [R,R] on the device.
    sample(n) draws n uniform UVs (or takes uv [n,2], mesh / OBJ convention) and returns the reference's keys.  `scale` multiplies the
    positions: the reference hard-codes 0.5 for its NeuS-unit meshes; a mesh extracted from an IDRNetwork is in stage-2 units already."""

    def __init__(self, position, normal, mask, scale=1.0):
        self.position, self.normal, self.mask, self.scale = ops._f32(position), ops._f32(normal), ops._f32(mask), float(scale)
        self.resolution = self.position.shape[0]

    def sample(self, n, uv=None):
        if uv is None:
            uv = torch.rand(int(n), 2, device=self.position.device)
        uv = ops._f32(uv.to(self.position.device)).reshape(-1, 2)
        x, nrm, om, tu, tv = ops.tb_sample(self.position, self.normal, self.mask, uv, self.scale)
        return {"uv": uv, "x": x, "normal": nrm, "object_mask": om.bool(), "tangent_u": tu, "tangent_v": tv}


# ----------------------------------------------------------------------------------------- PNG, OBJ
def png_bytes(image):
    """8-bit PNG (grey [H,W] / [H,W,1] or RGB [H,W,3]) of a float image in [0,1] (rounded to the nearest of 255 levels) or a uint8 one."""
    a = np.asarray(image)
    if a.dtype != np.uint8:
        a = np.round(np.clip(np.nan_to_num(a.astype(np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[..., 0]
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.size == 0:
        raise ValueError(f"save_png: image must be [H,W], [H,W,1] or [H,W,3], got {a.shape}")
    H, W = a.shape[:2]
    rows = np.concatenate([np.zeros((H, 1), np.uint8), np.ascontiguousarray(a).reshape(H, -1)], axis=1)      # filter type 0 per scanline
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if a.ndim == 3 else 0, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def save_png(path, image):
    with open(path, "wb") as f:
        f.write(png_bytes(image))


def save_obj(path, vertices, faces, uv, normals=None, mtl=None):
    """v, vt (one per face corner, uv [F,3,2]), vn (per vertex, when given) and f v/vt[/vn], 1-based; floats with 9 significant digits, which
    read back to the same float32."""
    v, f = _mesh._np(vertices, np.float32).reshape(-1, 3), _mesh._np(faces, np.int64).reshape(-1, 3)
    t, n = _mesh._np(uv, np.float32).reshape(-1, 2), _mesh._np(normals, np.float32)
    if t.shape[0] != 3 * f.shape[0]:
        raise ValueError("save_obj: uv must be [F,3,2]")
    lines = ["# robir_amd.texture"]
    if mtl:
        lines += [f"mtllib {mtl}", "usemtl baked"]
    lines += ["v %.9g %.9g %.9g" % tuple(r) for r in v.tolist()]
    lines += ["vt %.9g %.9g" % tuple(r) for r in t.tolist()]
    if n is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(r) for r in n.reshape(-1, 3).tolist()]
    vt = np.arange(1, 3 * f.shape[0] + 1).reshape(-1, 3)
    fmt = "f %d/%d/%d %d/%d/%d %d/%d/%d" if n is not None else "f %d/%d %d/%d %d/%d"
    for a, b in zip((f + 1).tolist(), vt.tolist()):
        lines.append(fmt % ((a[0], b[0], a[0], a[1], b[1], a[1], a[2], b[2], a[2]) if n is not None else (a[0], b[0], a[1], b[1], a[2], b[2])))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def load_obj(path):
    """v / vt / vn / f of a triangle OBJ -> dict of numpy arrays: vertices [V,3], faces [F,3] int32 and, when present, vt [Vt,2], faces_vt
    [F,3], vn [Vn,3], faces_vn [F,3] (0-based; negative OBJ indices are resolved).  Other statements are ignored."""
    v, vt, vn, fv, ft, fn = [], [], [], [], [], []
    with open(path) as fh:
        for ln in fh:
            w = ln.split()
            if not w or w[0].startswith("#"):
                continue
            if w[0] == "v":
                v.append([float(s) for s in w[1:4]])
            elif w[0] == "vt":
                vt.append([float(s) for s in w[1:3]])
            elif w[0] == "vn":
                vn.append([float(s) for s in w[1:4]])
            elif w[0] == "f":
                if len(w) != 4:
                    raise ValueError(f"{path}: only triangles are supported: {ln.strip()}")
                for s in w[1:]:
                    parts = (s.split("/") + ["", ""])[:3]
                    for dst, part, size in ((fv, parts[0], len(v)), (ft, parts[1], len(vt)), (fn, parts[2], len(vn))):
                        if part:
                            i = int(part)
                            dst.append(i - 1 if i > 0 else size + i)
    F = len(fv) // 3
    out = {"vertices": np.asarray(v, dtype=np.float32).reshape(-1, 3), "faces": np.asarray(fv, dtype=np.int32).reshape(F, 3)}
    if vt:
        out["vt"] = np.asarray(vt, dtype=np.float32).reshape(-1, 2)
    if vn:
        out["vn"] = np.asarray(vn, dtype=np.float32).reshape(-1, 3)
    for key, idx in (("faces_vt", ft), ("faces_vn", fn)):
        if idx:
            if len(idx) != 3 * F:
                raise ValueError(f"{path}: some face corners lack a {key[6:]} index")
            out[key] = np.asarray(idx, dtype=np.int32).reshape(F, 3)
    return out


# ----------------------------------------------------------------------------------------- command line
def main(argv=None):
    ap = argparse.ArgumentParser(description="Bake albedo / roughness / metallic / normal textures of the learned scene on the GPU.")
    ap.add_argument("--synthetic", action="store_true", help="the synthetic weights of robir_amd.synth instead of checkpoints")
    ap.add_argument("--scene", default="sphere", choices=("sphere", "nonconvex"))
    ap.add_argument("--neus-ckpt")
    ap.add_argument("--stage-ckpt")
    ap.add_argument("--obj", help="a triangle mesh with its own UVs (v / vt / f v/vt) instead of the extracted mesh and the atlas")
    ap.add_argument("--mesh-resolution", type=int, default=256, help="lattice points per axis of the extraction")
    ap.add_argument("--resolution", type=int, default=4096, help="texels per side")
    ap.add_argument("--project", type=int, default=1, help="Newton steps of every texel's point onto the SDF's zero set")
    ap.add_argument("--rings", type=int, default=4, help="dilation rings over the chart borders")
    ap.add_argument("--views", help="an .npz with images [M,H,W,3], masks [M,H,W] (may be empty), poses [M,4,4] camera-to-world and intrinsics "
                                    "[M,3,3]: also bake the colour these views observe (" + OBSERVED_FILE + ")")
    ap.add_argument("--out", required=True, help="directory of " + ", ".join(FILES))
    a = ap.parse_args(argv)
    if not a.synthetic and not a.neus_ckpt:
        ap.error("give --synthetic or --neus-ckpt")
    from . import renderer
    dev = torch.device("cuda:0")
    if a.synthetic:
        model = renderer.build_synthetic_model(dev, build_octrees=bool(a.views), scene=a.scene)
    else:
        import warnings
        with warnings.catch_warnings():          # the NeuS checkpoint is loaded explicitly on the next lines
            warnings.simplefilter("ignore", RuntimeWarning)
            model = renderer.IDRNetwork(renderer.hotdog_conf())
        from .nets import load_neus_checkpoint
        from .render import load_stage_checkpoint
        load_neus_checkpoint(model.implicit_network.neus_model, a.neus_ckpt)
        if a.stage_ckpt:
            load_stage_checkpoint(model, a.stage_ckpt)
        model = model.to(dev).eval()
    t0 = time.perf_counter()
    uv = None
    if a.obj:
        o = load_obj(a.obj)
        if "vt" not in o or "faces_vt" not in o:
            ap.error(f"{a.obj} carries no texture coordinates")
        vn = torch.from_numpy(o["vn"]).to(dev) if "vn" in o and o["vn"].shape == o["vertices"].shape else None
        m = _mesh.Mesh(torch.from_numpy(o["vertices"]).to(dev), torch.from_numpy(o["faces"]).to(dev), vn)
        uv = _corner_uv(torch.from_numpy(o["vt"]).to(dev), torch.from_numpy(o["faces_vt"]).to(dev))
    else:
        m = _mesh.extract_mesh(model, resolution=a.mesh_resolution, device=dev)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    ts = bake(model, m, a.resolution, a.project, a.rings, uv)
    if a.views:
        from . import observe
        z = np.load(a.views)
        missing = [k for k in ("images", "masks", "poses", "intrinsics") if k not in z]
        if missing:
            ap.error(f"{a.views} lacks the arrays {missing}")
        if model.octree_ray_tracer.sdf_octree is None:
            model.octree_ray_tracer.generate(None)
        as_dev = lambda k: torch.from_numpy(np.ascontiguousarray(z[k], dtype=np.float32)).to(dev)
        ts.bake_observations(model, observe.FocusSampler(as_dev("images"), as_dev("masks"), as_dev("poses"), as_dev("intrinsics")))
        torch.cuda.synchronize(dev)
    t2 = time.perf_counter()
    ts.export(a.out)
    t3 = time.perf_counter()
    s = ts.stats
    print(f"V {m.vertices.shape[0]} F {m.faces.shape[0]} cell {s['cell'] if uv is None else 0} covered fraction {s['covered_fraction']:.4f} "
          f"mesh {t1 - t0:.3f} s raster {s['raster_s']:.3f} s bake {s['bake_s']:.3f} s dilate {s['dilate_s']:.3f} s "
          f"(bake() {t2 - t1:.3f} s) export {t3 - t2:.3f} s -> {a.out}")


if __name__ == "__main__":
    main()
