"""Surface of the learned SDF as an indexed triangle mesh, extracted on the device, with per-vertex normals and baked materials.

Counterpart of the reference's neus/optimization/extraction.py:12-49 (extract_fields / extract_geometry / extract_mesh: 512^3 SDF values
copied to the host in 64^3 blocks, mcubes + trimesh on the CPU; confs_sg/env_path.py names the result meshes/mesh_{iter:06d}.ply) and the
starting point of its texture scripts.  Here the lattice is filled block-sparsely with the exact-threshold SDF kernels, the isosurface is
extracted by marching tetrahedra (robir_amd/csrc/mesh.hip; conventions and output order in include/robir_hip.h), vertex attributes come
from the existing network kernels, and the result is written as a binary PLY.  Everything runs under no_grad in eval mode.

    python -m robir_amd.mesh --synthetic [--scene nonconvex] --resolution 256 --out mesh.ply [--materials] [--refine 1] [--dense]
    python -m robir_amd.mesh --neus-ckpt logs/.../200000.tar [--stage-ckpt exps/.../latest.pth] --resolution 512 --out mesh_200000.ply
"""
import argparse
import time

import numpy as np
import torch

from . import ops

BLOCK = 8
# Default Lipschitz bound of the block culling: 1.5 x the largest |grad sdf| measured on the synthetic scenes' lattices, rounded up
# (profiles/mesh_times.md; 2.0 would not cover 1.5 x the `nonconvex` scene's maximum).
LIP = 2.5


# ----------------------------------------------------------------------------------------- isosurface of a lattice
def marching_tets(field, xs, ys, zs, threshold=0.0):
    """field [nx,ny,nz] float32 on the device (z fastest), axis coordinates xs, ys, zs -> (verts [V,3] float32, faces [F,3] int32).
    Inside = field < threshold; triangles wind so that their normal points towards increasing field.  Vertices are ordered by owner
    lattice vertex then edge slot, faces by cell, tetrahedron, triangle: the same field gives the same bytes.  One host read (the two
    totals) sits between the count and the emit kernels."""
    if field.dim() != 3 or min(field.shape) < 2:
        raise ValueError(f"marching_tets: field must be [nx,ny,nz] with every extent >= 2, got {tuple(field.shape)}")
    field = field.float().contiguous()
    dev = field.device
    xs, ys, zs = (torch.as_tensor(a, dtype=torch.float32, device=dev).contiguous() for a in (xs, ys, zs))
    if (xs.numel(), ys.numel(), zs.numel()) != tuple(field.shape):
        raise ValueError("marching_tets: axis coordinates do not match the field's shape")
    if not bool(torch.isfinite(field).all()):
        raise ValueError("marching_tets: the field holds non-finite values")
    iso = float(threshold)
    counts = ops.mesh_count(field, iso)
    incl = torch.cumsum(counts.to(torch.int64), 0)
    V, F = (int(v) for v in incl[-1].tolist())                  # the single sync
    if V >= 2 ** 31 or F >= 2 ** 31:
        raise ValueError(f"marching_tets: {V} vertices / {F} faces do not fit 32-bit indices")
    if V == 0 or F == 0:
        return (torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev))
    base = (incl - counts).t().contiguous()                     # [2,G] exclusive prefixes
    verts, vbase = ops.mesh_emit_vertices(field, xs, ys, zs, iso, base[0], V)
    faces = ops.mesh_emit_faces(field, iso, base[1], vbase, V, F)
    return verts, faces


def _axis_blocks(x, B):
    """Per block of an axis: centre coordinate (midpoint of first and last vertex), extent in cells, and the axis' largest spacing."""
    n = x.numel()
    i0 = torch.arange(0, n, B, device=x.device)
    i1 = torch.clamp(i0 + B, max=n) - 1
    h = float((x[1:] - x[:-1]).abs().max())
    return 0.5 * (x[i0] + x[i1]), (i1 - i0).to(torch.float32), h, (i1 - i0 + 1)


def fill_lattice(fn, xs, ys, zs, threshold=0.0, lip=LIP, block=BLOCK, chunk=1 << 18):
    """Evaluate fn ([M,3] device points -> [M] values) on the lattice xs x ys x zs, block-sparsely: -> (field [nx,ny,nz], fraction).

    The lattice is cut into blocks of `block` vertices per axis.  fn is evaluated at every block's centre; a block with
    |f_c - threshold| > lip * r, r^2 = sum_axis ((extent_in_cells/2 + 1) h_axis)^2 -- the distance from the centre to the farthest point
    of any cell touching the block -- cannot contain or touch a crossing edge of a `lip`-Lipschitz field, and all of its vertices are
    set to f_c: every lattice vertex keeps the side of the threshold it is on, every crossing edge keeps both of its true values, so
    marching_tets gives the dense mesh bit for bit.  `fraction` = lattice vertices evaluated exactly / all lattice vertices (the centre
    evaluations, one per block, are not counted).  lip=None: dense evaluation."""
    xs, ys, zs = (a.float().contiguous() for a in (xs, ys, zs))
    dev = xs.device
    nx, ny, nz = xs.numel(), ys.numel(), zs.numel()
    if min(nx, ny, nz) < 2:
        raise ValueError("fill_lattice: every axis needs at least 2 lattice points")
    B = int(block)
    field = torch.empty(nx, ny, nz, dtype=torch.float32, device=dev)
    (cx, ex, hx, mx), (cy, ey, hy, my), (cz, ez, hz, mz) = (_axis_blocks(a, B) for a in (xs, ys, zs))
    nb = cx.numel() * cy.numel() * cz.numel()
    ids = torch.arange(nb, dtype=torch.int32, device=dev)
    if lip is None:
        active = ids
        evaluated = nx * ny * nz
    else:
        centres = torch.stack(torch.meshgrid(cx, cy, cz, indexing="ij"), -1).reshape(-1, 3).contiguous()
        fc = torch.cat([fn(centres[i:i + chunk]).reshape(-1).float() for i in range(0, nb, chunk)])
        r = torch.sqrt(((ex / 2 + 1) * hx)[:, None, None] ** 2 + ((ey / 2 + 1) * hy)[None, :, None] ** 2
                       + ((ez / 2 + 1) * hz)[None, None, :] ** 2).reshape(-1)
        culled = (fc - float(threshold)).abs() > float(lip) * r          # NaN compares false: such a block is evaluated
        size = (mx[:, None, None] * my[None, :, None] * mz[None, None, :]).reshape(-1)
        active, idle = ids[~culled], ids[culled]
        evaluated = int(size[~culled].sum())
        ops.mesh_block_fill(idle, B, fc[culled].contiguous(), field)
    per = max(1, chunk // B ** 3)
    for i in range(0, active.numel(), per):
        blk = active[i:i + per].contiguous()
        vals = fn(ops.mesh_block_points(blk, B, xs, ys, zs)).reshape(-1).float()
        ops.mesh_block_store(blk, B, vals, field)
    return field, evaluated / float(nx * ny * nz)


# ----------------------------------------------------------------------------------------- models
class _Source:
    """value(x) [M] and, for the networks, value_grad(x) ([M], [M,3]) in the units of the points; materials(x) for an IDRNetwork."""

    def __init__(self, model):
        from . import nets
        self.net, self.fn, self.materials_net, self.radius = None, None, None, None
        self.in_scale, self.out_scale = 1.0, 1.0
        if isinstance(model, nets.SDFNetwork):
            self.net = model
        elif isinstance(model, nets.ImplicitNetworkMy):
            self.net, self.in_scale, self.out_scale, self.radius = model.neus_model.sdf_network, 2.0, 0.5, 1.0
        elif hasattr(model, "implicit_network") and hasattr(model, "envmap_material_network"):        # IDRNetwork
            self.net, self.in_scale, self.out_scale = model.implicit_network.neus_model.sdf_network, 2.0, 0.5
            self.radius = float(getattr(model, "object_bounding_sphere", 1.0))
            self.materials_net = model.envmap_material_network
        elif callable(model):
            self.fn = model
        else:
            raise TypeError(f"extract_mesh: {type(model).__name__} is neither an SDF network, an IDRNetwork nor a callable")

    def value(self, x):
        if self.net is None:
            return self.fn(x).reshape(-1)
        # the library-grade softplus path of the octree build: these values feed sign decisions
        return self.net.eval_points(x.contiguous(), self.in_scale, self.out_scale, full=False, precise=True)[0].reshape(-1)

    def value_grad(self, x):
        v, g = self.net.eval_points(x.contiguous(), self.in_scale, self.out_scale, full=False, grad=True, precise=True)
        return v.reshape(-1), g


class Mesh:
    """vertices [V,3] float32, faces [F,3] int32 and optional per-vertex normals [V,3], albedo [V,3], roughness [V,1], metallic [V,1]
    (None when not requested), as torch tensors on the device that produced them."""

    def __init__(self, vertices, faces, normals=None, albedo=None, roughness=None, metallic=None):
        self.vertices, self.faces, self.normals = vertices, faces, normals
        self.albedo, self.roughness, self.metallic = albedo, roughness, metallic
        self.stats = {}

    def export(self, path):
        save_ply(path, self.vertices, self.faces, self.normals, self.albedo, self.roughness, self.metallic)
        return path


def vertex_attributes(src, verts, threshold=0.0, refine=0, normals=True, materials=False, chunk=1 << 18):
    """(verts after `refine` Newton steps x <- x - (f - threshold) grad f / |grad f|^2, unit normals | None, material dict | None),
    chunked through the existing value + gradient and material kernels."""
    V = verts.shape[0]
    if (refine or normals) and src.net is None:
        if refine:
            raise ValueError("extract_mesh: refine needs a network (a plain callable has no gradient path)")
        normals = False
    out_v, out_n = [], []
    mats = {"albedo": [], "roughness": [], "metallic": []}
    if materials and src.materials_net is None:
        raise ValueError("extract_mesh: materials=True needs an IDRNetwork (envmap_material_network)")
    for i in range(0, V, chunk):
        x = verts[i:i + chunk].contiguous()
        if refine or normals:
            f, g = src.value_grad(x)
            for _ in range(int(refine)):
                x = (x - (f - float(threshold))[:, None] * g / (g * g).sum(-1, keepdim=True).clamp_min(1e-20)).contiguous()
                f, g = src.value_grad(x)
            if normals:
                out_n.append(g / g.norm(dim=-1, keepdim=True).clamp_min(1e-20))
        out_v.append(x)
        if materials:
            m = bake_materials(src.materials_net, x)
            for k in mats:
                mats[k].append(m[k])
    cat = lambda parts, w: torch.cat(parts) if parts else torch.zeros(0, w, dtype=torch.float32, device=verts.device)
    return (cat(out_v, 3), cat(out_n, 3) if normals else None,
            {k: cat(v, 3 if k == "albedo" else 1) for k, v in mats.items()} if materials else None)


def bake_materials(material_net, x):
    """albedo [n,3], roughness [n,1], metallic [n,1] of EnvmapMaterialNetwork.forward at the points x: the clean outputs, which do not
    depend on the perturbation draws (zeros are passed so that nothing is drawn)."""
    n = x.shape[0]
    noise = {"spec": torch.zeros(n, 32, device=x.device), "normal": torch.zeros(n, 60, device=x.device)}
    m = material_net(x, train_spec=True, noise=noise)
    return {"albedo": m["sg_diffuse_albedo"].reshape(n, 3), "roughness": m["sg_roughness"].reshape(n, 1),
            "metallic": m["sg_metallic"].reshape(n, 1)}


def _extract(src, bound_min, bound_max, resolution, threshold, lip, refine, normals, materials, device):
    res = int(resolution)
    lo = [float(v) for v in torch.as_tensor(bound_min).reshape(-1).tolist()]
    hi = [float(v) for v in torch.as_tensor(bound_max).reshape(-1).tolist()]
    # the reference's sample points (extraction.py:14-16)
    xs, ys, zs = (torch.linspace(lo[i], hi[i], res, dtype=torch.float32, device=device) for i in range(3))
    sync = (lambda: torch.cuda.synchronize(device)) if torch.device(device).type == "cuda" else (lambda: None)
    with torch.no_grad():
        sync()
        t0 = time.perf_counter()
        field, frac = fill_lattice(src.value, xs, ys, zs, threshold, lip)
        sync()
        t1 = time.perf_counter()
        verts, faces = marching_tets(field, xs, ys, zs, threshold)
        sync()
        t2 = time.perf_counter()
        del field
        verts, nrm, mats = vertex_attributes(src, verts, threshold, refine, normals, materials)
        sync()
        t3 = time.perf_counter()
    mesh = Mesh(verts, faces, nrm, **(mats or {}))
    mesh.stats = {"evaluated_fraction": frac, "fill_s": t1 - t0, "mesh_s": t2 - t1, "attributes_s": t3 - t2}
    return mesh


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func, *, lip=LIP):
    """extraction.py:30-40 with the reference's parameter order: -> (vertices [V,3] float32, triangles [F,3] int32) as numpy arrays in
    world units.  query_func: an SDFNetwork, an ImplicitNetworkMy / IDRNetwork or any callable on [M,3] device points.  The reference
    hands mcubes the NEGATED distance of an ISDF model; here the distance itself is contoured, so triangles face outward."""
    src = _Source(query_func)
    dev = next(src.net.parameters()).device if src.net is not None else torch.as_tensor(bound_min).device
    if dev.type != "cuda":
        dev = torch.device("cuda")
    m = _extract(src, bound_min, bound_max, resolution, threshold, lip, 0, False, False, dev)
    return m.vertices.cpu().numpy(), m.faces.cpu().numpy()


def extract_mesh(model, bbox=1.5, resolution=512, threshold=0.0, device='cuda', *, lip=LIP, refine=0, normals=True, materials=False):
    """extraction.py:43-49: the surface `model` = threshold inside the origin-centred box of half size `bbox`, on `resolution` lattice
    points per axis -> Mesh.  model: an SDFNetwork (NeuS units), an ImplicitNetworkMy / IDRNetwork (stage-2 units: sdf(x) =
    net(2x)/2; with bbox left at its default the box is the bounding sphere's cube) or any callable returning an SDF.
    lip: Lipschitz bound of the field for the block culling (None: dense); refine: Newton steps on the vertices; normals: unit SDF
    gradient (outward for an SDF; None for a plain callable); materials: albedo / roughness / metallic of an IDRNetwork's
    envmap_material_network at the vertices."""
    src = _Source(model)
    if src.radius is not None and bbox == 1.5:
        bbox = src.radius
    half = torch.as_tensor(bbox, dtype=torch.float32).reshape(-1)
    half = half.expand(3) if half.numel() == 1 else half
    return _extract(src, -half, half, resolution, threshold, lip, refine, normals, materials, torch.device(device))


# ----------------------------------------------------------------------------------------- PLY
def _srgb(x):
    x = np.clip(x, 0.0, 1.0)
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)


def _np(t, dtype):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t), dtype=dtype)


def ply_layout(V, F, normals=False, materials=False):
    """(header bytes, vertex dtype, face dtype) of the binary little-endian file save_ply writes."""
    props = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals:
        props += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if materials:
        props += [(n, "<f4") for n in ("albedo_r", "albedo_g", "albedo_b", "roughness", "metallic")]
        props += [(n, "u1") for n in ("red", "green", "blue")]
    lines = ["ply", "format binary_little_endian 1.0", "comment robir_amd.mesh", f"element vertex {V}"]
    lines += [f"property {'uchar' if t == 'u1' else 'float'} {n}" for n, t in props]
    lines += [f"element face {F}", "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii"), np.dtype(props), np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def save_ply(path, vertices, faces, normals=None, albedo=None, roughness=None, metallic=None):
    """Binary little-endian PLY: float x y z [nx ny nz] [albedo_r albedo_g albedo_b roughness metallic, uchar red green blue = the
    sRGB-encoded albedo], faces as `list uchar int`."""
    v, f = _np(vertices, np.float32).reshape(-1, 3), _np(faces, np.int32).reshape(-1, 3)
    n, a, r, m = _np(normals, np.float32), _np(albedo, np.float32), _np(roughness, np.float32), _np(metallic, np.float32)
    mats = a is not None
    if mats and (r is None or m is None):
        raise ValueError("save_ply: albedo, roughness and metallic go together")
    header, vdt, fdt = ply_layout(v.shape[0], f.shape[0], n is not None, mats)
    rec = np.zeros(v.shape[0], dtype=vdt)
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if n is not None:
        n = n.reshape(-1, 3)
        rec["nx"], rec["ny"], rec["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if mats:
        a = a.reshape(-1, 3)
        rec["albedo_r"], rec["albedo_g"], rec["albedo_b"] = a[:, 0], a[:, 1], a[:, 2]
        rec["roughness"], rec["metallic"] = r.reshape(-1), m.reshape(-1)
        c = np.round(_srgb(a.astype(np.float64)) * 255.0).astype(np.uint8)
        rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    frec = np.zeros(f.shape[0], dtype=fdt)
    frec["n"], frec["v"] = 3, f
    with open(path, "wb") as fh:
        fh.write(header)
        fh.write(rec.tobytes())
        fh.write(frec.tobytes())


def load_ply(path):
    """Reads the files save_ply writes -> dict of numpy arrays: vertices, faces and, when present, normals, albedo, roughness,
    metallic, rgb."""
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    V = F = None
    props, section = [], None
    for ln in lines[2:]:
        w = ln.split()
        if w[:2] == ["element", "vertex"]:
            V, section = int(w[2]), "vertex"
        elif w[:2] == ["element", "face"]:
            F, section = int(w[2]), "face"
        elif w[:1] == ["property"] and section == "vertex":
            if w[1] not in ("float", "uchar"):
                raise ValueError(f"{path}: unsupported vertex property type {w[1]}")
            props.append((w[2], "<f4" if w[1] == "float" else "u1"))
        elif w[:1] == ["property"] and section == "face" and w[1:4] != ["list", "uchar", "int"]:
            raise ValueError(f"{path}: unsupported face property {ln}")
    vdt, fdt = np.dtype(props), np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    if len(blob) != end + V * vdt.itemsize + F * fdt.itemsize:
        raise ValueError(f"{path}: {len(blob)} bytes, header predicts {end + V * vdt.itemsize + F * fdt.itemsize}")
    rec = np.frombuffer(blob, dtype=vdt, count=V, offset=end)
    frec = np.frombuffer(blob, dtype=fdt, count=F, offset=end + V * vdt.itemsize)
    if F and not (frec["n"] == 3).all():
        raise ValueError(f"{path}: only triangles are supported")
    names = [n for n, _ in props]
    col = lambda *ks: np.stack([rec[k] for k in ks], -1)
    out = {"vertices": col("x", "y", "z"), "faces": np.ascontiguousarray(frec["v"]).reshape(-1, 3)}
    if "nx" in names:
        out["normals"] = col("nx", "ny", "nz")
    if "albedo_r" in names:
        out.update(albedo=col("albedo_r", "albedo_g", "albedo_b"), roughness=col("roughness"), metallic=col("metallic"),
                   rgb=col("red", "green", "blue"))
    return out


# ----------------------------------------------------------------------------------------- command line
def main(argv=None):
    ap = argparse.ArgumentParser(description="Extract the SDF's zero set as a PLY mesh on the GPU (marching tetrahedra).")
    ap.add_argument("--synthetic", action="store_true", help="the synthetic weights of robir_amd.synth instead of checkpoints")
    ap.add_argument("--scene", default="sphere", choices=("sphere", "nonconvex"))
    ap.add_argument("--neus-ckpt")
    ap.add_argument("--stage-ckpt")
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--bbox", type=float, help="half size of the box (default: the model's bounding sphere)")
    ap.add_argument("--threshold", type=float, default=0.0)
    ap.add_argument("--lip", type=float, default=LIP, help="Lipschitz bound of the SDF used by the block culling")
    ap.add_argument("--dense", action="store_true", help="evaluate every lattice vertex (no culling)")
    ap.add_argument("--refine", type=int, default=0, help="Newton steps on the vertices")
    ap.add_argument("--materials", action="store_true", help="bake albedo / roughness / metallic per vertex")
    ap.add_argument("--no-normals", action="store_true")
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    if not a.synthetic and not a.neus_ckpt:
        ap.error("give --synthetic or --neus-ckpt")
    from . import renderer
    dev = torch.device("cuda:0")
    if a.synthetic:
        model = renderer.build_synthetic_model(dev, build_octrees=False, scene=a.scene)
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
    mesh = extract_mesh(model, bbox=1.5 if a.bbox is None else a.bbox, resolution=a.resolution, threshold=a.threshold, device=dev,
                        lip=None if a.dense else a.lip, refine=a.refine, normals=not a.no_normals, materials=a.materials)
    mesh.export(a.out)
    s = mesh.stats
    print(f"V {mesh.vertices.shape[0]} F {mesh.faces.shape[0]} evaluated fraction {s['evaluated_fraction']:.4f} "
          f"fill {s['fill_s']:.3f} s mesh {s['mesh_s']:.3f} s attributes {s['attributes_s']:.3f} s -> {a.out}")


if __name__ == "__main__":
    main()
