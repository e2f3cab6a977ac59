#!/usr/bin/env python
"""Times the atlas fit on a view of the baked synthetic scene and writes the record profiles/texfit_times.md:

    python tools/prof_texfit.py [--size 800] [--mesh-res 256] [--resolution 4096] [--out profiles/texfit_times.md]

The scene is profiles/meshrender_times.md's: the synthetic model's surface extracted at --mesh-res, baked at --resolution, one --size x
--size view from synth_camera, direct SG shading (vis="none"), tone = None, L1.  The target is the view of the bake itself; the fit starts
from the bake with uniform +-0.1 noise on albedo and roughness.  HIP events around warm calls, the median of 10 after 3 warm-ups:
  cache     the ViewBatch: project, rasterise, G-buffer, rb_tf_taps, the stable sort of the 4 n pairs, the segments (one host read);
  fetch     rb_tf_fetch of the four fit channels;
  forward   sg_render.render_with_all_sg under grad (rb_sg_shade, the autograd path);
  loss      training.photometric_loss (rb_pl_image_loss: loss and d loss / d colour in one pass);
  backward  loss.backward(): rb_sg_shade_bwd;
  scatter   rb_tf_scatter;
  adam      rb_tf_adam on the touched texels;
  step      AtlasFit.step() as a whole, wall clock, with its host read of the loss;
and, like for like, the same gradient taken by index_add_ into a dense [R,R,4] plane followed by torch.optim.Adam over the whole plane.
Each new kernel's MINIMUM traffic is set beside the 6.3 TB/s streaming figure that the other profiles use."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robir_amd import mesh, meshrender, ops, renderer, synth, texfit, texture, training  # noqa: E402

STREAM_TBS, WARM, REPS = 6.3, 3, 10


def event_ms(fn):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts), out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--mesh-res", type=int, default=256)
    ap.add_argument("--resolution", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texfit_times.md"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    H = W = a.size
    with torch.no_grad():
        model = renderer.build_synthetic_model(dev, build_octrees=False)
        m = mesh.extract_mesh(model, resolution=a.mesh_res, device=dev)
        ts = texture.bake(model, m, resolution=a.resolution)
        asset = meshrender.load_asset(ts, dev)
        _, pose, K = synth.synth_camera(H, W)
        pose, K = torch.from_numpy(pose).to(dev), torch.from_numpy(K).to(dev)
        view = meshrender.render_mesh(asset, pose, K, H, W, model=model, vis="none")
        x = view["sg_rgb"]
        target = torch.where(view["network_object_mask"][:, None], x / (x + 1.0), torch.zeros_like(x)).reshape(1, H, W, 3)
        start = asset.planes.clone()
        gen = torch.Generator(device=dev).manual_seed(0)
        start[..., :4] = (start[..., :4] + (torch.rand(start[..., :4].shape, device=dev, generator=gen) - 0.5) * 0.2).clamp(0.02, 1.0)
        noisy = meshrender.MeshAsset(asset.vertices, asset.faces, asset.uv, start, asset.has_normal, asset.vnormals)
    views = {"images": target, "poses": pose[None], "intrinsics": K[None]}
    fit = texfit.AtlasFit(noisy, views, model=model, vis="none", tone=None, loss_type="L1", lr=0.01)
    R, C = fit.planes.shape[0], texfit.FIT_CHANNELS

    def cache():
        return texfit.ViewBatch(fit.asset, fit.images, fit.masks, fit.poses, fit.cameras, fit.K, (0,), fit.filter, fit.near, fit.cull)

    t_cache, b = event_ms(cache)
    n, T, P = b.n, b.T, 4 * b.n
    longest = int(torch.diff(b.seg_start.long()).max())
    with torch.no_grad():
        t_taps, _ = event_ms(lambda: ops.tf_taps(b.uv, R, 1))
        t_sort, _ = event_ms(lambda: texfit.sort_pairs(b.tap_texel, b.tap_weight, R))
        t_fetch, tex = event_ms(lambda: ops.tf_fetch(fit.planes, b.tap_texel, b.tap_weight, C))
    state = {}

    def forward():
        state["alb"] = tex[:, 0:3].contiguous().requires_grad_(True)
        state["rough"] = tex[:, 3:4].contiguous().requires_grad_(True)
        with torch.enable_grad():
            state["r"] = fit._shade(b, state["alb"], state["rough"])
        return state["r"]

    def loss():
        with torch.enable_grad():
            state["loss"] = training.photometric_loss(state["r"]["sg_rgb"], None, b.target, b.net_mask, b.obj_mask, tone=None, loss_type="L1")
        return state["loss"]

    def backward():
        state["alb"].grad = state["rough"].grad = None
        state["loss"].backward(retain_graph=True)

    t_forward, _ = event_ms(forward)
    t_loss, _ = event_ms(loss)
    t_backward, _ = event_ms(backward)
    with torch.no_grad():
        g_tex = torch.cat([state["alb"].grad, state["rough"].grad.reshape(-1, 1)], 1).contiguous()
        t_scatter, grad = event_ms(lambda: ops.tf_scatter(b.pair_row, b.pair_weight, b.seg_start, g_tex))
        planes, am, av = fit.planes.clone(), fit.adam_m.clone(), fit.adam_v.clone()
        t_adam, _ = event_ms(lambda: ops.tf_adam(planes, am, av, b.seg_texel, grad, fit.lr, fit.lo, fit.hi, 0.9, 0.999, 1e-8, 1))

        # like for like: the same gradient by index_add_ into a dense plane, then torch.optim.Adam over the whole plane
        ok = (b.tap_texel >= 0).reshape(-1)
        flat_texel = b.tap_texel.reshape(-1).long().clamp_min(0)
        contrib = lambda: (g_tex[:, None, :] * (b.tap_weight * (b.tap_texel >= 0))[:, :, None]).reshape(-1, C)
        dense_p = torch.nn.Parameter(fit.planes[..., :C].reshape(R * R, C).clone())
        opt = torch.optim.Adam([dense_p], lr=0.01)

        def dense_grad():
            d = torch.zeros(R * R, C, device=dev)
            d.index_add_(0, flat_texel, contrib())
            return d

        t_index_add, dgrad = event_ms(dense_grad)

        def dense_adam():
            dense_p.grad = dgrad
            opt.step()

        t_dense_adam, _ = event_ms(dense_adam)
        agree = float((dgrad[b.seg_texel.long()] - grad).abs().max() / grad.abs().max())

    def whole():
        torch.cuda.synchronize()
        t = time.perf_counter()
        fit.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for _ in range(WARM):
        whole()
    t_step = statistics.median(whole() for _ in range(REPS))

    traffic = {"taps": n * (8 + 32), "fetch": n * (32 + 4 * 16 + 16), "scatter": P * 8 + 4 * T + P * 16 + 16 * T, "adam": T * (4 + 16 + 6 * 16)}
    rows = [("cache build (ViewBatch), all of it", t_cache, None), ("  rb_tf_taps", t_taps, traffic["taps"]),
            ("  sort of the 4 n pairs + segments (torch, one host read)", t_sort, None), ("fetch (rb_tf_fetch, 4 channels)", t_fetch, traffic["fetch"]),
            ("shading forward under grad", t_forward, None), ("loss (rb_pl_image_loss)", t_loss, None), ("backward (rb_sg_shade_bwd)", t_backward, None),
            ("scatter (rb_tf_scatter)", t_scatter, traffic["scatter"]), ("adam (rb_tf_adam, touched texels)", t_adam, traffic["adam"]),
            ("AtlasFit.step(), wall clock", t_step, None), ("alternative: index_add_ into a dense [R,R,4] plane", t_index_add, None),
            ("alternative: torch.optim.Adam over the whole plane", t_dense_adam, R * R * C * 4 * 7)]
    lines = [f"# Atlas fit times (MI355X, synthetic sphere, {H} x {W} view, mesh lattice {a.mesh_res}^3, {R}^2 atlas)", "",
             "Written by `tools/prof_texfit.py`.  HIP events around warm calls, the median of 10 after 3 warm-ups; `AtlasFit.step()` is wall clock",
             "around synchronised calls and holds the host read of the loss.  TB/s = minimum traffic / time, to be read beside the 6.3 TB/s",
             "streaming figure.  The alternative rows take the same gradient with `index_add_` (atomics: the order of its sums is not fixed) and",
             "step every texel of the plane.", "",
             f"hit rows n = {n} of {H * W}, (row, tap) pairs P = {P}, touched texels T = {T} of {R * R} ({100.0 * T / (R * R):.2f} %), longest "
             f"segment = {longest} pairs, fit channels C = {C}.  The dense gradient and the gather agree to {agree:.1e} relative.", "",
             "Minimum traffic: taps 40 n; fetch n (32 + 16 C + 4 C); scatter 8 P + 4 T + 4 C P (a g_tex row per pair) + 4 C T; adam T (4 + 4 C + 24 C);",
             "dense Adam 28 R^2 C (parameter, gradient and two moments read, parameter and moments written).", "",
             "| stage | ms | minimum traffic, MB | TB/s |", "|---|---|---|---|"]
    for name, ms, by in rows:
        lines.append(f"| {name} | {ms:.3f} | {'' if by is None else '%.2f' % (by / 1e6)} | {'' if by is None else '%.3f' % (by / (ms * 1e-3) / 1e12)} |")
    lines += ["", f"Streaming figure for comparison: {STREAM_TBS} TB/s."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
