"""The end-to-end scene of the mesh view's test and of tools/measure_meshrender_caps.py: the synthetic model (seed 0), its surface extracted
at resolution 64 with one refinement step, the bake at 1024, the 64 x 64 synth_camera view with fixed draws, the neural forward('Material')
of that view, and the float64 path: rasteriser and G-buffer of tests/meshrender_restatement.py in double precision on the same mesh and
planes, shaded by the same existing call (meshrender.shade_rows -> sg_render.render_with_all_sg).  The distance of that path from the neural
forward is discretisation alone (mesh, atlas, dilation) and does not involve the new kernels."""
import numpy as np
import torch

import meshrender_restatement as mr

H = W = 64
MESH_RESOLUTION, ATLAS_RESOLUTION, REFINE = 64, 1024, 1
FIELDS = ("diffuse_albedo", "roughness", "normals", "sg_rgb")
PER_ROW = ("illum_randn", "spec_randn", "normal_randn", "svis_theta_dir", "svis_phi_dir", "svis_theta_ind", "svis_phi_ind")


def pixel_draws(dev):
    """synth.pbr_draws with one row per PIXEL: a view narrows the per-row draws to its own hit rows, so the same pixel gets the same draw in
    the neural and in the mesh view whatever their hit masks."""
    from robir_amd import synth
    return {k: torch.from_numpy(v).to(dev) for k, v in synth.pbr_draws(0, H * W).items()}


def rows_of(draws, idx):
    return {k: (v[idx].contiguous() if k in PER_ROW else v) for k, v in draws.items()}


def build(dev):
    """-> dict: model, mesh, ts (the TextureSet), pose, K (numpy), draws, neural (forward('Material') of the view, [H W, .] tensors)."""
    from robir_amd import mesh, renderer, synth, texture
    model = renderer.build_synthetic_model(dev, seed=0)
    m = mesh.extract_mesh(model, resolution=MESH_RESOLUTION, device=dev, refine=REFINE)
    ts = texture.bake(model, m, resolution=ATLAS_RESOLUTION)
    uv, pose, K = synth.synth_camera(H, W)
    draws = pixel_draws(dev)
    shift = model.gamma.hdr_shift.as_input().detach()
    inp = {"uv": torch.from_numpy(uv)[None].to(dev), "pose": torch.from_numpy(pose)[None].to(dev), "intrinsics": torch.from_numpy(K)[None].to(dev),
           "object_mask": torch.ones(1, H * W, dtype=torch.bool, device=dev), "hdr_shift": shift.expand(H * W, 1).contiguous()}
    first = model(inp, trainstage="Material", train_spec=True, draws={k: v for k, v in draws.items() if k not in PER_ROW})
    idx = first["network_object_mask"].reshape(-1).nonzero()[:, 0]
    neural = model(inp, trainstage="Material", train_spec=True, draws=rows_of(draws, idx))
    neural = {k: v for k, v in neural.items() if torch.is_tensor(v)}
    assert torch.equal(neural["network_object_mask"], first["network_object_mask"])
    return dict(model=model, mesh=m, ts=ts, pose=pose, K=K, draws=draws, neural=neural)


def boundary(mask):
    """[H,W] bool -> [H,W] bool: pixels whose 8-neighbourhood (the pixel included, the image border repeated) holds both a hit and a miss."""
    m = np.pad(np.asarray(mask, dtype=bool), 1, mode="edge")
    stack = np.stack([m[1 + dr:1 + dr + H, 1 + dc:1 + dc + W] for dr in (-1, 0, 1) for dc in (-1, 0, 1)])
    return stack.any(0) & ~stack.all(0)


def interior(mask):
    mask = np.asarray(mask, dtype=bool)
    return mask & ~boundary(mask)


def float64_view(scene, vis="network", filter=1):
    """The view through the float64 path -> dict of [H W, .] numpy arrays (FIELDS and network_object_mask), zeros outside the mesh."""
    from robir_amd import meshrender
    model, ts = scene["model"], scene["ts"]
    dev = ts.albedo.device
    a = meshrender.load_asset(ts, dev)
    v, f, uv = a.vertices.cpu().numpy(), a.faces.cpu().numpy(), a.uv.cpu().numpy()
    planes = a.planes.cpu().numpy().astype(np.float64)
    pose, K = scene["pose"], scene["K"]
    pinv = np.linalg.inv(np.asarray(pose, dtype=np.float64))
    screen = mr.project(v, pinv, K, dtype=np.float64)
    face_id, bary, _ = mr.raster(screen, f, H, W, dtype=np.float64)
    idx = np.nonzero(face_id.reshape(-1) >= 0)[0]
    g = mr.gbuffer(face_id, bary, f, v, uv, pose[:3, 3], planes, filter, None, idx, dtype=np.float64)
    tex = g["tex"]
    nrm = tex[:, 5:8] / np.maximum(np.linalg.norm(tex[:, 5:8], axis=-1, keepdims=True), 1e-12)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    idx_t = torch.from_numpy(idx).to(dev)
    r = meshrender.shade_rows(t(g["position"]), t(nrm), t(g["view_dir"]), t(tex[:, 0:3]), t(tex[:, 3:4]), model=model, vis=vis,
                              draws=rows_of(scene["draws"], idx_t))
    out = {k: np.zeros((H * W, 3)) for k in FIELDS}
    out["diffuse_albedo"][idx] = tex[:, 0:3]
    out["roughness"][idx] = np.repeat(tex[:, 3:4], 3, -1)
    out["normals"][idx] = nrm
    out["sg_rgb"][idx] = r["sg_rgb"].double().cpu().numpy()
    out["network_object_mask"] = face_id.reshape(-1) >= 0
    return out


def distances(view, neural, inner):
    """{field: max |view - neural| over the interior pixels} for FIELDS; view / neural: [H W, .] arrays or tensors."""
    num = lambda x: x.detach().double().cpu().numpy() if torch.is_tensor(x) else np.asarray(x, dtype=np.float64)
    sel = np.asarray(inner, dtype=bool).reshape(-1)
    return {k: float(np.abs(num(view[k]).reshape(H * W, -1)[sel] - num(neural[k]).reshape(H * W, -1)[sel]).max()) for k in FIELDS}
