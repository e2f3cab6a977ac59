"""Where do the kernels' arithmetics sit relative to fp32?  Everything here is anchored on a FLOAT64 evaluation of the reference's formulas.

One Material chunk: the whole per-hit chain (indirect-illumination net -> NeuS normal -> material auto-encoders -> 128-lobe
light visibility through the visibility MLP -> BRDF-lobe visibility -> SG shading) evaluated on IDENTICAL surface points,
view directions and random draws by
  (r64)  the oracle in float64            -- the anchor: what the reference's formulas give without rounding noise,
  (o32)  the oracle in float32            -- the reference's own arithmetic (PyTorch CPU fp32),
  (k32)  the HIP kernels, f32-input MFMA  -- every MLP on v_mfma_f32_16x16x4_f32 (ROBIR_MLP_PRECISION=fp32),
  (kx6)  the HIP kernels, DEFAULT policy  -- ROBIR_PRECISION=exact: every fp32 operand carried exactly as three f16 pieces, six f16
                                             MFMA products per multiply-add, fp32 accumulation ("f16x6": the arithmetic bench.py's
                                             headline runs in and whose `dtype` claim -- not narrower than fp32 -- this file asserts),
  (kh3)  the HIP kernels, split precision -- ROBIR_PRECISION=split: (hi, lo) f16 pairs, 22-bit operands (the throughput policy).
Asserted per field for the DEFAULT: err(kx6 vs r64) <= X6_VS_K32 * err(k32 vs r64) + 2^-23 and <= X6_VS_O32 * err(o32 vs r64) + 2^-23
on the median and the 99th percentile (both factors are sampling allowances for quantiles of a few hundred entries of two fp32
evaluations that differ in summation order only -- NOT a representation floor: the three pieces ARE the fp32 operand);
test_per_net_error_budget asserts the same per network on 8192 rows with factor 1.0.
Asserted per field for split precision: err(kh3 vs r64) <= 1.25 * err(k32 vs r64) + F and <= 2 * err(o32 vs r64) + F, on the median and on the
99th percentile of the per-entry errors.  F = 16 * 2^-22 = 3.8e-6 is the representation floor of the split: an (hi, lo) half
pair carries 22 bits where fp32 carries 24, so a DIRECT network output (the NeuS normal: measured 2e-6 at p99 against 5e-7 for
the exact kernels) sits a few 2^-22 above fp32 while being 50x below the 1e-4 bar; every SHADING field (errors 1e-5..1e-3,
set by the conditioning of the SG formulas, not by the MLP arithmetic) must then be within 1.25x of the exact kernels.  The maximum is recorded but not compared: it is set by the handful of visibility samples that sit on the
n.d > 1e-6 cull (a 1e-7 change of the normal moves one sample in or out of a lobe's 32: 3e-2 of that lobe's visibility) and
those flip between ANY two evaluations that round differently -- they are counted instead.
All numbers go to gpurun_out/test_metrics.jsonl.
"""
import os

import numpy as np
import pytest
import torch

from conftest import err_entries, record_metric

pytestmark = pytest.mark.gpu

# sampling allowances of the chained test (quantiles over ~600 entries of fields whose error is set by a handful of ill-conditioned
# entries): two fp32 evaluations in different summation orders scatter around each other by this much -- the o32 / k32 columns do
X6_VS_K32 = 1.25
X6_VS_O32 = 2.0

FIELDS = ("sg_rgb", "indir_rgb", "sg_diffuse_rgb", "sg_specular_rgb", "indir_diffuse_rgb", "indir_specular_rgb",
          "vis_shadow", "diffuse_albedo", "roughness", "metallic", "normals", "normal_map")


def _oracle_chain(sd, pts, view, hdr, draws, dtype):
    """IDRNetwork.forward's per-hit part (implicit_differentiable_renderer.py:340-358,386-455) + the PBR hook."""
    from robir_oracle import nets as on, renderer as orend
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        c = lambda t: t.to(dtype)
        sdd = {k: (c(v) if v.is_floating_point() else v) for k, v in sd.items()}
        dr = {k: c(v) for k, v in draws.items()}
        sgs, integ = on.indirect_illum(sdd, c(pts), c(hdr), dr["illum_randn"])
        return orend.pbr_sg_render(sdd, c(pts), c(view), sgs, integ, dr, testing=True)
    finally:
        torch.set_default_dtype(old)


@pytest.mark.parametrize("seed,variance,sharp", [(0, 0.3, False), (3, 0.6, True)])
def test_chained_error_budget(monkeypatch, seed, variance, sharp):
    from robir_amd import precision, renderer, sg_render, synth
    from robir_oracle import nets as on
    dev = torch.device("cuda:0")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    model = renderer.build_synthetic_model(dev, seed=seed, variance=variance, sharp_light=sharp)
    sd = on.as_torch(synth.synth_state_dict(seed, variance=variance, sharp_light=sharp))
    # 256 pixels around the image centre of the 64x64 view: all but the principal-point ray (exactly axis-parallel: NaN in the
    # reference's slab test as well) hit the object
    uv, pose, K = synth.synth_camera(64, 64)
    sel = np.concatenate([np.arange(r * 64 + 24, r * 64 + 40) for r in range(24, 40)])
    inp = {"uv": torch.from_numpy(uv[sel]).to(dev)[None], "pose": torch.from_numpy(pose).to(dev)[None],
           "intrinsics": torch.from_numpy(K).to(dev)[None], "object_mask": torch.ones(1, 256, dtype=torch.bool, device=dev),
           "hdr_shift": torch.full((256, 1), 0.5, device=dev)}
    hit = model(inp, trainstage="Illum", draws={})["network_object_mask"].cpu()
    n_hit = int(hit.sum())
    assert n_hit >= 200        # the column and the row through the principal point are axis-parallel rays (no hit, like the reference)
    draws = {k: torch.from_numpy(v) for k, v in synth.pbr_draws(seed + 40, n_hit, chunk_id=9).items()}
    dd = {k: v.to(dev) for k, v in draws.items()}
    outs = {}
    for mode, vis in (("fp32", "fp32"), ("f16x6", "f16x6"), ("f16x3", "f16x3-auto")):
        monkeypatch.setenv("ROBIR_MLP_PRECISION", mode)
        monkeypatch.setattr(sg_render, "VIS_PRECISION", vis)
        outs[mode] = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in
                      model(inp, trainstage="Material", train_spec=True, draws=dd).items()}
    k32, kx6, kh3 = outs["fp32"], outs["f16x6"], outs["f16x3"]
    for o in (k32, kx6, kh3):
        assert torch.equal(o["network_object_mask"], hit)
        assert torch.equal(o["points"][hit], k32["points"][hit])       # the cast is geometry code: identical in every mode
    pts, view, hdr = k32["points"][hit], -k32["ray_dirs"][hit], inp["hdr_shift"].cpu()[hit]
    r64 = _oracle_chain(sd, pts, view, hdr, draws, torch.float64)
    o32 = _oracle_chain(sd, pts, view, hdr, draws, torch.float32)
    worst_ratio, worst_x6 = 0.0, 0.0
    ulp = 2.0 ** -23
    for f in FIELDS:
        ref = r64[f].expand(-1, 3) if (f == "roughness") else r64[f]
        o = o32[f].expand(-1, 3) if (f == "roughness") else o32[f]
        e = {"o32": err_entries(o, ref), "k32": err_entries(k32[f][hit], ref), "kx6": err_entries(kx6[f][hit], ref),
             "kh3": err_entries(kh3[f][hit], ref)}
        st = {}
        for name, v in e.items():
            st[name + "_p50"], st[name + "_p99"] = float(v.quantile(0.5)), float(v.quantile(0.99))
            st[name + "_max"], st[name + "_n_gt_1e-3"] = float(v.max()), int((v > 1e-3).sum())
        record_metric(f"chained_error_budget/seed{seed}/{f}", entries=int(e["kh3"].numel()), **st)
        print(f"{f:22s} " + "  ".join(f"{n}: p50 {st[n + '_p50']:.2e} p99 {st[n + '_p99']:.2e} max {st[n + '_max']:.2e} "
                                      f"n>1e-3 {st[n + '_n_gt_1e-3']}" for n in ("o32", "k32", "kx6", "kh3")))
        # ---- the DEFAULT policy (exact three-piece operands): an fp32 evaluation like the other two
        for q in ("_p50", "_p99"):
            assert st["kx6" + q] <= X6_VS_K32 * st["k32" + q] + ulp, ("f16x6 vs f32-input MFMA", f, q, st)
            assert st["kx6" + q] <= X6_VS_O32 * st["o32" + q] + ulp, ("f16x6 vs the reference's fp32", f, q, st)
            worst_x6 = max(worst_x6, st["kx6" + q] / (st["k32" + q] + ulp))
        assert st["kx6_n_gt_1e-3"] <= max(2 * st["o32_n_gt_1e-3"], st["k32_n_gt_1e-3"] + 3, 3), (f, st)       # cull flips, counted
        assert st["kx6_p99"] <= max(1e-4, 2.0 * st["o32_p99"]), (f, st)
        # ---- split precision
        slack = 16 * 2.0 ** -22
        for q in ("_p50", "_p99"):
            assert st["kh3" + q] <= 1.25 * st["k32" + q] + slack, (f, q, st)
            assert st["kh3" + q] <= 2.0 * st["o32" + q] + slack, (f, q, st)
            worst_ratio = max(worst_ratio, st["kh3" + q] / (st["k32" + q] + slack))
        # cull flips: the split-precision run may not have more large outliers than fp32 arithmetic itself produces
        assert st["kh3_n_gt_1e-3"] <= max(2 * st["o32_n_gt_1e-3"], st["k32_n_gt_1e-3"] + 3, 3), (f, st)
        # and the bulk sits at north_star's bar -- or where the reference's own fp32 arithmetic sits, for the SG terms that
        # are ill-conditioned in fp32 (lambda_trick / hemisphere_int cancel large exponentials: o32 itself is at 2e-4..1e-3)
        assert st["kh3_p99"] <= max(1e-4, 2.0 * st["o32_p99"]), (f, st)
    record_metric(f"chained_error_budget/seed{seed}/worst_ratio_h3_over_fp32mfma", ratio=worst_ratio)
    record_metric(f"chained_error_budget/seed{seed}/worst_ratio_x6_over_fp32mfma", ratio=worst_x6)
    # ROBIR_PRECISION=f16 (light-visibility MLP in plain f16, one product; every other net in split precision): NARROWER than fp32 --
    # measured against the same float64 anchor, printed and recorded (DESIGN.md quotes the table), held only to a sanity band: no parity claim
    assert precision.POLICIES["f16"] == ("f16x1", "f16x3")
    monkeypatch.setenv("ROBIR_MLP_PRECISION", "f16x3")
    monkeypatch.setattr(sg_render, "VIS_PRECISION", "f16x1")
    kf = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in model(inp, trainstage="Material", train_spec=True, draws=dd).items()}
    assert torch.equal(kf["network_object_mask"], hit)
    for f in FIELDS:
        ref = r64[f].expand(-1, 3) if (f == "roughness") else r64[f]
        v = err_entries(kf[f][hit], ref)
        st = dict(p50=float(v.quantile(0.5)), p99=float(v.quantile(0.99)), max=float(v.max()), n_gt_1e3=int((v > 1e-3).sum()))
        record_metric(f"f16_mode/seed{seed}/{f}", entries=int(v.numel()), **st)
        print(f"f16 mode {f:22s} p50 {st['p50']:.2e} p99 {st['p99']:.2e} max {st['max']:.2e} n>1e-3 {st['n_gt_1e3']}")
        assert st["p99"] <= 5e-2, (f, st)


def _scaled_vis_weights(sd_np, s):
    """Same visibility function, hidden activations of layer l larger by s^((l+1)/4) (the last hidden layer by s): a ReLU net
    is positively homogeneous, so scaling every hidden layer's weight by f = s^(1/4), its bias by f^(l+1), and the output
    layer's weight by 1/s leaves the logits unchanged.  (Spreading the factor keeps the WEIGHTS inside the range the
    split-precision packing accepts; the activations are what this test is about.)"""
    out = dict(sd_np)
    P = "visibility_network.vis_layer."
    f = float(s) ** 0.25
    for i, l in enumerate((0, 2, 4, 6)):
        out[P + f"{l}.weight"] = sd_np[P + f"{l}.weight"] * np.float32(f)
        out[P + f"{l}.bias"] = sd_np[P + f"{l}.bias"] * np.float32(f ** (i + 1))
    out[P + "8.weight"] = sd_np[P + "8.weight"] / np.float32(f ** 4)
    return out


def _max_hidden_activation(sd, p, d):
    from robir_oracle.encoding import pe
    h = torch.cat([pe(p, 10), pe(d, 10)], -1)
    m = 0.0
    for l in (0, 2, 4, 6):
        h = torch.relu(h @ sd[f"visibility_network.vis_layer.{l}.weight"].t() + sd[f"visibility_network.vis_layer.{l}.bias"])
        m = max(m, float(h.max()))
    return m


def test_activation_range_sentinel(monkeypatch):
    """Split-precision operands are (hi, lo) half pairs: beyond 65504 / lift they silently lose precision.  Every _h3 kernel
    tracks the largest hi half it consumed and reports through rb_range_check -> RobirHipError.  Stress weights with hidden
    activations ~1e3 must pass parity and raise nothing; activations ~2e5 must be reported (and the exact kernels, selected as
    the message says, still match the oracle)."""
    from robir_amd import nets, ops, sg_render, synth, _lib
    from robir_oracle import nets as on, sg as osg
    from conftest import rel_err
    dev = torch.device("cuda:0")
    base = synth.synth_state_dict(0, variance=0.3)
    g = torch.Generator().manual_seed(1)
    n = 96
    pts = torch.randn(n, 3, generator=g) * 0.2
    nrm = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    lgt = torch.from_numpy(base["envmap_material_network.lgtSGs"])
    u_t, u_p = torch.rand(128, 32, generator=g), torch.rand(128, 32, generator=g)
    ops.range_check(sync=True)                                       # start from a clean sentinel

    def scale_for(target):
        """s such that the largest hidden activation of the scaled net on these inputs is `target`."""
        lo, hi = 1.0, 1e12
        for _ in range(60):
            mid = (lo * hi) ** 0.5
            if _max_hidden_activation(on.as_torch(_scaled_vis_weights(base, mid)), pts, dirs) < target:
                lo = mid
            else:
                hi = mid
        return hi

    def run(s, mlp_mode, vis_mode):
        sdn = _scaled_vis_weights(base, s)
        sd = on.as_torch(sdn)
        v = nets.VisNetwork(10, 10, [256] * 4)
        v.load_state_dict({k[len("visibility_network."):]: torch.from_numpy(x) for k, x in sdn.items()
                           if k.startswith("visibility_network.")})
        v = v.to(dev).eval()
        monkeypatch.setenv("ROBIR_MLP_PRECISION", mlp_mode)
        monkeypatch.setattr(sg_render, "VIS_PRECISION", vis_mode)
        logits = v(pts.to(dev), dirs.to(dev)).cpu()
        lobes = torch.nn.functional.normalize(lgt[:, :3], dim=-1)
        vis = sg_render.get_diffuse_visibility(pts.to(dev), nrm.to(dev), v, lobes.to(dev), lgt[:, 3:4].abs().to(dev), nsamp=32,
                                               draws={"dvis_theta": u_t.to(dev), "dvis_phi": u_p.to(dev)}).cpu()
        ref_logits = on.vis_logits(sd, pts, dirs)
        ref_vis = osg.diffuse_visibility(pts, nrm, lambda p, d: on.vis_logits(sd, p, d), lobes, lgt[:, 3:4].abs(), u_t, u_p)
        return logits, vis, ref_logits, ref_vis

    s_ok = scale_for(1.0e3)                                          # hidden activations up to ~1e3
    logits, vis, ref_logits, ref_vis = run(s_ok, "f16x3", "f16x3-auto")
    ops.range_check(sync=True)                                       # nothing to report
    e1, e2 = rel_err(logits, ref_logits), rel_err(vis, ref_vis)
    record_metric("range_sentinel/act_1e3", scale=s_ok, logits=e1, light_vis=e2)
    assert e1 <= 1e-4 and e2 <= 1e-4, (e1, e2)
    s_bad = scale_for(2.0e5)                                         # beyond the f16 range of the hi halves
    run(s_bad, "f16x3", "f16x3-auto")
    with pytest.raises(_lib.RobirHipError, match="overflowed its activation range") as ei:
        ops.range_check(sync=True)
    assert "light-visibility" in str(ei.value) and "rb_vis_mlp_h3" in str(ei.value)
    ops.range_check(sync=True)                                       # reading clears the words
    run(s_bad, "f16x6", "f16x6")                                     # the exact-operand kernels carry the same f16 range on their leading piece
    with pytest.raises(_lib.RobirHipError, match="overflowed its activation range") as ei6:
        ops.range_check(sync=True)
    assert "light-visibility" in str(ei6.value) and "rb_vis_x6_points" in str(ei6.value)
    ops.range_check(sync=True)
    logits, vis, ref_logits, ref_vis = run(s_bad, "fp32", "fp32")    # the remedy the message names
    ops.range_check(sync=True)
    e1, e2 = rel_err(logits, ref_logits), rel_err(vis, ref_vis)
    record_metric("range_sentinel/act_2e5_exact_kernels", logits=e1, light_vis=e2)
    assert e1 <= 1e-4 and e2 <= 1e-4, (e1, e2)


# ---------------------------------------------------------------------------------------------------------------------------------
# per network: the default (exact three-piece operand) kernels against float64, next to the f32-input-MFMA kernels and the reference's
# own fp32 arithmetic on the same inputs.  This is the evidence behind bench.py's dtype "f16x6 ... not narrower than fp32".
PER_NET_ROWS = 8192
# err(x6 vs r64) <= PER_NET_VS_K32 * err(k32 vs r64) + 2^-23   (median and 99th percentile of the per-entry errors, 8192 rows)
# err(x6 vs r64) <= PER_NET_VS_O32 * err(o32 vs r64) + 2^-23   (o32: PyTorch CPU fp32 = the reference's arithmetic)
PER_NET_VS_K32 = 1.0
PER_NET_VS_O32 = 1.0


def _f64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def _per_net_cases(dev, sd_np, x=None, n=PER_NET_ROWS, cesr_seed=0):
    """[(name, oracle(sd, dtype) -> tensor, {form: thunk -> device tensor})]: inputs are drawn once (fp32) and shared by every column.
    x: the points [n,3] (default: n stage-2 points around the object); n: the row count, a multiple of 8."""
    from robir_amd import ops, packing, synth
    from robir_oracle import nets as on
    from robir_oracle.encoding import pe
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(20260929)
    if x is None:
        x = (torch.rand(n, 3, generator=g) - 0.5) * 1.2                                  # stage-2 points around the object
    assert x.shape == (n, 3) and x.dtype == torch.float32 and n % 8 == 0
    view = F.normalize(torch.randn(n, 3, generator=g), dim=-1)
    nrm = F.normalize(torch.randn(n, 3, generator=g), dim=-1)
    hdr = torch.rand(n, 1, generator=g)
    xd, vd, nd, hd = x.to(dev), view.to(dev), nrm.to(dev), hdr.to(dev)
    b32, back = packing.pack_sdf(sd_np, dev, full=True), packing.pack_sdf_back(sd_np, dev)
    x6f = packing.pack_sdf_x6(sd_np, dev, full=True)
    back6 = packing.pack_sdf_back_x6(sd_np, dev) + (packing.pack_sdf_back_x6(sd_np, dev, two_tile=True)[0],)
    feat_d = ops.sdf_mlp_points(xd, n, b32, 1, 2.0, 0.5, 1.0)[0][:, 1:].contiguous()    # one fp32 feature tensor for the colour columns
    feat = feat_d.cpu()
    c32, c6 = packing.pack_color(sd_np, dev), packing.pack_color_x6(sd_np, dev)
    v32, v6 = packing.pack_vis(sd_np, dev), packing.pack_vis_x6(sd_np, dev)
    ill32, ill6 = packing.pack_illum(sd_np, dev), packing.pack_illum_x6(sd_np, dev)
    pre = "envmap_material_network.spec_brdf_encoder_layer"
    enc32, _ = packing.pack_sparse_ae(sd_np, pre, dev)
    enc6 = packing.pack_sparse_ae_encoder_x6(sd_np, pre, dev)
    cesr = synth.synth_cesr_nets(cesr_seed)
    no = {"net." + k: v for k, v in cesr["normal_net"].items()}
    sh = {"net." + k: v for k, v in cesr["shadow_net"].items()}
    no32, no6 = packing.pack_softplus512(no, "net.", 63, dev), packing.pack_softplus512_x6(no, "net.", 63, dev)
    sh32, sh6 = packing.pack_softplus512(sh, "net.", 191, dev), packing.pack_softplus512_x6(sh, "net.", 191, dev)
    no_t = {k: torch.from_numpy(v) for k, v in cesr["normal_net"].items()}
    sh_t = {k: torch.from_numpy(v) for k, v in cesr["shadow_net"].items()}
    nl, nsh = 8, n // 8                                                                  # shadow_net: n/8 points x 8 one-hot labels
    lrelu = lambda t: F.leaky_relu(t, 0.2)

    def two_forms(fn):
        """{one tile per wave, two tiles per wave} of the SDF kernels, whatever ops.sdf_two_tile would pick at this size."""
        def run(rows):
            old, ops.SDF_TWO_TILE_MIN_ROWS = ops.SDF_TWO_TILE_MIN_ROWS, rows
            try:
                return fn()
            finally:
                ops.SDF_TWO_TILE_MIN_ROWS = old
        return {"x6_one_tile": lambda: run(1 << 60), "x6_two_tile": lambda: run(0)}

    def shadow_oracle(sd, dt):
        p = x[:nsh].to(dt)
        rows = torch.cat([pe(p, 10)[:, None, :].expand(-1, nl, -1), torch.eye(128, dtype=dt)[None, :nl].expand(nsh, -1, -1)], -1)
        return on.softplus_net512({k: v.to(dt) for k, v in sh_t.items()}, rows.reshape(-1, 191))

    cases = [
        ("sdf_values_257", lambda sd, dt: on.implicit_forward(sd, x.to(dt)),
         dict(k32=lambda: ops.sdf_mlp_points(xd, n, b32, 1, 2.0, 0.5, 1.0)[0],
              **two_forms(lambda: ops.sdf_points_x6(xd, n, x6f, True, 2.0, 0.5)))),
        ("sdf_gradient", lambda sd, dt: on.implicit_gradient(sd, x.to(dt)),
         dict(k32=lambda: ops.sdf_value_grad_f32(xd, n, b32, back, 2.0, 0.5)[1],
              **two_forms(lambda: ops.sdf_value_grad_x6(xd, n, x6f, back6, 2.0, 0.5)[1]))),
        ("colour_rgb", lambda sd, dt: on.color_raw(sd, x.to(dt), nrm.to(dt), view.to(dt), feat.to(dt)),
         dict(k32=lambda: ops.color_mlp_points(xd, vd, nd, feat_d, c32),
              x6_one_tile=lambda: ops.color_x6_points(xd, vd, nd, feat_d, c6, two_tile=False),
              x6_two_tile=lambda: ops.color_x6_points(xd, vd, nd, feat_d, c6, two_tile=True))),
        ("visibility_logits", lambda sd, dt: on.vis_logits(sd, x.to(dt) * 0.5, view.to(dt)),
         dict(k32=lambda: ops.vis_mlp_points(xd * 0.5, vd, v32, 1), x6=lambda: ops.vis_x6_points(xd * 0.5, vd, v6, 1))),
        ("illum_lobe_net_512", lambda sd, dt: on._seq(sd, on.ILL + "lobe_layer.", 5, torch.cat([pe(x.to(dt) * 0.5, 10), hdr.to(dt)], -1), torch.relu),
         dict(k32=lambda: ops.wide_mlp_points(xd * 0.5, hd, ill32, False), x6=lambda: ops.wide_x6_points(xd * 0.5, hd, ill6, False))),
        ("spec_encoder_512", lambda sd, dt: on._seq(sd, pre + ".brdf_encoder_layer.", 5, pe(x.to(dt) * 0.5, 10), lrelu),
         dict(k32=lambda: ops.wide_mlp_points(xd * 0.5, None, enc32, True), x6=lambda: ops.wide_x6_points(xd * 0.5, None, enc6, True))),
        ("cesr_normal_net", lambda sd, dt: on.softplus_net512({k: v.to(dt) for k, v in no_t.items()}, pe(x.to(dt) * 0.5, 10)),
         dict(k32=lambda: ops.cesr_net_points(xd * 0.5, n, 0, no32), x6=lambda: ops.cesr_net_x6_points(xd * 0.5, n, 0, no6))),
        ("cesr_shadow_net", shadow_oracle,
         dict(k32=lambda: ops.cesr_net_points(xd[:nsh].contiguous(), nsh * nl, 2, sh32, nl),
              x6=lambda: ops.cesr_net_x6_points(xd[:nsh].contiguous(), nsh * nl, 2, sh6, nl))),
    ]
    return cases


@pytest.mark.parametrize("weights", ["init", "trained_like"])
def test_per_net_error_budget(weights):
    """Every network of the path, DEFAULT arithmetic (exact three-piece operands, "f16x6") against a float64 evaluation of the
    reference's formulas (model/neus_model.py:385-417 SDF net, :425-438 its input gradient, :535-560 colour net;
    model/implicit_differentiable_renderer.py:250-258 visibility MLP, :199-222 lobe net; model/sg_envmap_material.py:74-99 encoder;
    training/train_cesr.py:106-110 CESR nets) on identical fp32 inputs and weights:
        err(x6 vs r64)  <=  PER_NET_VS_K32 * err(f32-input-MFMA kernel vs r64) + 2^-23
        err(x6 vs r64)  <=  PER_NET_VS_O32 * err(PyTorch CPU fp32 vs r64)      + 2^-23
    on the median and on the 99th percentile of the per-entry errors |a-b| / (|b| + mean|b|); maxima are recorded.  Both forms of a
    kernel that has two (one / two tiles per wave) are held to it."""
    from robir_amd import ops, synth
    from robir_oracle import nets as on
    dev = torch.device("cuda:0")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    sd_np = synth.synth_state_dict(0, variance=0.3)
    if weights == "trained_like":
        import importlib
        sd_np = importlib.import_module("test_mlp_gpu")._trained_like(sd_np, 5)
    sd32 = on.as_torch(sd_np)
    sd64 = _f64(sd32)
    ulp = 2.0 ** -23
    ops.range_check(sync=True)
    table = []
    for name, oracle, forms in _per_net_cases(dev, sd_np):
        r64 = oracle(sd64, torch.float64)
        o32 = oracle(sd32, torch.float32)
        assert o32.dtype == torch.float32 and r64.dtype == torch.float64, name
        st = {}
        cols = {"o32": o32}
        for form, thunk in forms.items():
            cols[form] = thunk().cpu().reshape(r64.shape)
        for col, v in cols.items():
            e = err_entries(v, r64)
            st[col + "_p50"], st[col + "_p99"], st[col + "_max"] = float(e.quantile(0.5)), float(e.quantile(0.99)), float(e.max())
        record_metric(f"per_net_error_budget/{weights}/{name}", entries=int(r64.numel()), **st)
        line = f"{name:20s} " + "  ".join(f"{c}: p50 {st[c + '_p50']:.2e} p99 {st[c + '_p99']:.2e} max {st[c + '_max']:.2e}" for c in cols)
        print(line)
        table.append((name, st, [c for c in cols if c.startswith("x6")]))
    ops.range_check(sync=True)
    for name, st, x6cols in table:
        for c in x6cols:
            for q in ("_p50", "_p99"):
                assert st[c + q] <= PER_NET_VS_K32 * st["k32" + q] + ulp, (name, c, q, "vs f32-input MFMA", st)
                assert st[c + q] <= PER_NET_VS_O32 * st["o32" + q] + ulp, (name, c, q, "vs the reference's fp32", st)
            assert st[c + "_p99"] <= 1e-4 and st[c + "_max"] <= 1e-4 * 4, (name, c, st)      # and north_star's bar itself


# ---------------------------------------------------------------------------------------------------------------------------------
# the same rule over the OPERAND RANGE of the exact-operand kernels (tests/split_model.py states the windows, tests/test_split_cpu.py
# establishes them on paper): the ray-march input domain with its special points, more weight draws, and -- for the positively homogeneous
# nets -- hidden activations moved by exact powers of two up to the clamp's binade and down through the f16 subnormals.
DOMAIN_ROWS = 1024           # 2048 entries for the two-output nets: the 99th percentile is the ~20th largest entry


def _domain_points(n, seed):
    """n points: uniform in [-1.5, 1.5]^3 (the ray-march range; with in_scale = 2 the encoding's arguments reach 2^9 * 3 = 1536) and a block of
    special rows: the origin, -0.0, the eight +-1 corners, axis-aligned points, points with one coordinate of +-2^-30."""
    t = 2.0 ** -30
    special = [[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0]]
    special += [[a, b, c] for a in (-1.0, 1.0) for b in (-1.0, 1.0) for c in (-1.0, 1.0)]
    for axis in range(3):
        for v in (-1.5, -0.37, 0.5, 1.0):
            special.append([v if i == axis else 0.0 for i in range(3)])
        for v in (-t, t):
            special.append([v if i == axis else (0.3, -0.7, 0.45)[i] for i in range(3)])
    special = torch.tensor(special, dtype=torch.float32)
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n - special.shape[0], 3, generator=g) - 0.5) * 3.0
    return torch.cat([x, special])


def _quantiles(v, ref):
    e = err_entries(v, ref)
    return {"p50": float(e.quantile(0.5)), "p99": float(e.quantile(0.99)), "max": float(e.max())}


def _rule_violations(st, col):
    """the project's rule for column `col` of st[column][quantile] on the median and the 99th percentile; -> list of violations"""
    ulp, bad = 2.0 ** -23, []
    for q in ("p50", "p99"):
        if not st[col][q] <= PER_NET_VS_K32 * st["k32"][q] + ulp:
            bad.append((col, q, "vs f32-input MFMA", st[col][q], st["k32"][q]))
        if not st[col][q] <= PER_NET_VS_O32 * st["o32"][q] + ulp:
            bad.append((col, q, "vs the reference's fp32", st[col][q], st["o32"][q]))
    return bad


def _flat(st):
    return {f"{c}_{q}": v for c, d in st.items() for q, v in d.items()}


@pytest.mark.parametrize("weights", ["init", "trained_like"])
@pytest.mark.parametrize("seed", [0, 3, 11])
def test_per_net_error_budget_ray_march_domain(seed, weights):
    """test_per_net_error_budget's rule (same constants, same float64 anchor, all eight nets + the SDF gradient, both tile forms) on the input
    domain the ray march really covers -- points in [-1.5, 1.5]^3 plus the special rows of _domain_points -- and on three weight draws, each as
    drawn and trained-like.  DOMAIN_ROWS rows: the smallest count that keeps the 99th percentile over ~2000 entries for the two-output nets."""
    import importlib
    from robir_amd import ops, synth
    from robir_oracle import nets as on
    dev = torch.device("cuda:0")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    sd_np = synth.synth_state_dict(seed, variance=0.3)
    if weights == "trained_like":
        sd_np = importlib.import_module("test_mlp_gpu")._trained_like(sd_np, 5 + seed)
    sd32 = on.as_torch(sd_np)
    sd64 = _f64(sd32)
    x = _domain_points(DOMAIN_ROWS, 700 + seed)
    ops.range_check(sync=True)
    bad = []
    for name, oracle, forms in _per_net_cases(dev, sd_np, x=x, n=DOMAIN_ROWS, cesr_seed=seed):
        r64, o32 = oracle(sd64, torch.float64), oracle(sd32, torch.float32)
        assert o32.dtype == torch.float32 and r64.dtype == torch.float64, name
        st = {"o32": _quantiles(o32, r64)}
        for form, thunk in forms.items():
            st[form] = _quantiles(thunk().cpu().reshape(r64.shape), r64)
        record_metric(f"per_net_error_budget_domain/seed{seed}/{weights}/{name}", entries=int(r64.numel()), **_flat(st))
        print(f"{name:20s} " + "  ".join(f"{c}: p50 {d['p50']:.2e} p99 {d['p99']:.2e} max {d['max']:.2e}" for c, d in st.items()))
        for c in st:
            if c.startswith("x6"):
                bad += [(name,) + b for b in _rule_violations(st, c)]
                if not (st[c]["p99"] <= 1e-4 and st[c]["max"] <= 4e-4):
                    bad.append((name, c, "north_star's bar", st[c]["p99"], st[c]["max"]))
    ops.range_check(sync=True)
    assert not bad, bad


# ---- power-of-two regimes ----------------------------------------------------------------------------------------------------
# A ReLU / LeakyReLU net is positively homogeneous: the first layer's weight and every bias times 2^k moves ALL hidden activations by 2^k
# exactly (a power of two: no rounding in fp32 or float64 short of under- / overflow), and the outputs with them.  The error measure
# |a - b| / (|b| + mean|b|) does not see the factor, so the rule applies as it stands.  Regimes are named by where they put the float64
# oracle's hidden activations on the test's inputs:
#   hot        the LARGEST in [32752, 65504): the binade in which sx_split_pair's m piece relies on the round-toward-zero clamp; with k + 1 the
#              largest is >= 65504 and the range sentinel must report
#   bf8_edge   the MEDIAN non-zero magnitude in [2^-15, 2^-14): the lowest binade in which the bf8 copy of the third piece is still exact
#   cold       ... in [2^-17, 2^-16): h pieces are f16 subnormals, every piece still inside the exact window (>= 2^-23 but for the ~1 % of
#              activations more than 2^6 below the median, whose absolute error is <= 2^-47): INSIDE the six-product window, BELOW the bf8 form's
#   below      ... in [2^-27, 2^-26): below both windows; an operand is then off by <= 2^-47, ~2^-21 of the median: recorded, held to the 1e-4 bar
def _hidden_magnitudes(weights, h, act, stride=1):
    """float64 hidden activations of a 4-hidden-layer net on rows h: ([largest magnitude of each layer], [median non-zero magnitude of each
    layer, over every `stride`-th row])"""
    import torch.nn.functional as F
    mx, med = [], []
    for W, b in weights[:4]:
        h = act(F.linear(h, W.double(), b.double()))
        a = h.abs()
        mx.append(float(a.max()))
        a = a[::stride]
        med.append(float(a[a > 0].median()))
    return mx, med


def _k_into(value, lo):
    """the k with lo <= value 2^k < 2 lo"""
    import math
    k = math.floor(math.log2(lo / value))
    while value * 2.0 ** k < lo:
        k += 1
    while value * 2.0 ** k >= 2 * lo:
        k -= 1
    return k


def _regime_ks(mx, med):
    from split_model import BF8_L_EXACT_MIN
    return {"base": 0, "hot": _k_into(mx, 32752.0), "bf8_edge": _k_into(med, BF8_L_EXACT_MIN), "cold": _k_into(med, 2.0 ** -17),
            "below": _k_into(med, 2.0 ** -27)}


def _pow2_regime(sd_np, prefix, k, k3=None, head_k=0):
    """layers prefix + '0' .. '8' with the activations of hidden layers 0-2 moved by 2^k, those of hidden layer 3 by 2^k3 (default: k too) and
    the outputs by 2^(k3 + head_k): first weight times 2^k, layer 3's times 2^(k3 - k), the output layer's times 2^head_k, every bias by
    its layer's factor.  Powers of two: nothing is rounded."""
    k3 = k if k3 is None else k3
    out = dict(sd_np)
    for key, e in (("0.weight", k), ("0.bias", k), ("2.bias", k), ("4.bias", k), ("6.weight", k3 - k), ("6.bias", k3), ("8.weight", head_k),
                   ("8.bias", k3 + head_k)):
        out[prefix + key] = sd_np[prefix + key] * np.float32(2.0 ** e)
        assert np.array_equal(out[prefix + key].astype(np.float64), sd_np[prefix + key].astype(np.float64) * 2.0 ** e), (key, e)      # nothing flushed
    return out


def _homogeneous_nets(dev, x, view, hdr):
    """{name: (weight prefix, activation, feature rows (float64), sentinel's name for the kernel, k32 thunk(sd), x6 thunk(sd), oracle(sd, dtype))}"""
    from robir_amd import ops, packing
    from robir_oracle import nets as on
    from robir_oracle.encoding import pe
    import torch.nn.functional as F
    xd, vd, hd = x.to(dev), view.to(dev), hdr.to(dev)
    pre = "envmap_material_network.spec_brdf_encoder_layer"
    lrelu = lambda t: F.leaky_relu(t, 0.2)
    xh = x * 0.5
    return {
        "visibility_logits": (on.VIS, torch.relu, torch.cat([pe(xh.double(), 10), pe(view.double(), 10)], -1), "rb_vis_x6_points",
                              lambda sd: ops.vis_mlp_points(xd * 0.5, vd, packing.pack_vis(sd, dev), 1),
                              lambda sd: ops.vis_x6_points(xd * 0.5, vd, packing.pack_vis_x6(sd, dev), 1),
                              lambda sd, dt: on.vis_logits(sd, xh.to(dt), view.to(dt))),
        "illum_lobe_net_512": (on.ILL + "lobe_layer.", torch.relu, torch.cat([pe(xh.double(), 10), hdr.double()], -1), "rb_wide_x6",
                               lambda sd: ops.wide_mlp_points(xd * 0.5, hd, packing.pack_illum(sd, dev), False),
                               lambda sd: ops.wide_x6_points(xd * 0.5, hd, packing.pack_illum_x6(sd, dev), False),
                               lambda sd, dt: on._seq(sd, on.ILL + "lobe_layer.", 5, torch.cat([pe(xh.to(dt), 10), hdr.to(dt)], -1), torch.relu)),
        "spec_encoder_512": (pre + ".brdf_encoder_layer.", lrelu, pe(xh.double(), 10), "rb_wide_x6",
                             lambda sd: ops.wide_mlp_points(xd * 0.5, None, packing.pack_sparse_ae(sd, pre, dev)[0], True),
                             lambda sd: ops.wide_x6_points(xd * 0.5, None, packing.pack_sparse_ae_encoder_x6(sd, pre, dev), True),
                             lambda sd, dt: on._seq(sd, pre + ".brdf_encoder_layer.", 5, pe(xh.to(dt), 10), lrelu)),
    }


@pytest.mark.parametrize("net", ["visibility_logits", "illum_lobe_net_512", "spec_encoder_512"])
def test_error_budget_power_of_two_regimes(net):
    """The stand-alone six-product kernels of the positively homogeneous nets with their hidden activations moved by exact powers of two
    (regimes above).  Per regime: the f32-input-MFMA result is the base result times 2^k bit for bit (else fp32 itself under- or overflowed and
    the regime measures nothing); hot / bf8_edge / cold are inside the exact window: the rule holds and the sentinel stays silent; hot + 1 is
    reported by the sentinel with the kernel's name; below: the quantiles are recorded and held to the 1e-4 / 4e-4 bar, run-to-run bit-identical."""
    import torch.nn.functional as F
    from robir_amd import ops, synth, _lib
    from robir_oracle import nets as on
    dev = torch.device("cuda:0")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    sd_np = synth.synth_state_dict(0, variance=0.3)
    n = DOMAIN_ROWS
    g = torch.Generator().manual_seed(4242)
    x = _domain_points(n, 900)
    view = F.normalize(torch.randn(n, 3, generator=g), dim=-1)
    hdr = torch.rand(n, 1, generator=g)
    prefix, act, rows, kernel_name, k32_of, x6_of, oracle = _homogeneous_nets(dev, x, view, hdr)[net]
    base64 = _f64(on.as_torch(sd_np))
    mxs, meds = _hidden_magnitudes([(base64[prefix + "%d.weight" % (2 * i)], base64[prefix + "%d.bias" % (2 * i)]) for i in range(5)], rows, act)
    mx, med = max(mxs), float(np.median(meds))
    ks = _regime_ks(mx, med)
    assert 32752.0 <= mx * 2.0 ** ks["hot"] < 65504.0 and ks["hot"] > 0 > ks["bf8_edge"] > ks["cold"] > ks["below"], (mx, med, ks)
    ops.range_check(sync=True)
    k32_base, bad = None, []
    for regime, k in ks.items():
        sd = _pow2_regime(sd_np, prefix, k)
        sd32 = on.as_torch(sd)
        r64, o32 = oracle(_f64(sd32), torch.float64), oracle(sd32, torch.float32)
        k32 = k32_of(sd).cpu()
        if regime == "base":
            k32_base, r64_base = k32, r64
        assert torch.equal(k32, k32_base * 2.0 ** k), (net, regime, k, "fp32 itself left its range: the regime measures nothing")
        assert torch.equal(r64, r64_base * 2.0 ** k), (net, regime, k)
        a = x6_of(sd)
        ops.range_check(sync=True)                                   # every regime is inside the f16 range of the leading piece
        st = {"o32": _quantiles(o32, r64), "k32": _quantiles(k32, r64), "x6": _quantiles(a.cpu(), r64)}
        record_metric(f"pow2_regimes/{net}/{regime}", k=k, largest_hidden=mx * 2.0 ** k, median_hidden=med * 2.0 ** k, entries=int(r64.numel()), **_flat(st))
        print(f"{net} {regime:9s} k {k:4d}  " + "  ".join(f"{c}: p50 {d['p50']:.2e} p99 {d['p99']:.2e} max {d['max']:.2e}" for c, d in st.items()))
        if regime == "below":
            assert torch.equal(a, x6_of(sd)), (net, regime)
            if not (st["x6"]["p99"] <= 1e-4 and st["x6"]["max"] <= 4e-4):
                bad.append((regime, "bar", st["x6"]))
        else:
            bad += [(regime,) + b for b in _rule_violations(st, "x6")]
    x6_of(_pow2_regime(sd_np, prefix, ks["hot"] + 1))                # the largest activation is now in [65504, 131008): the tight side of the boundary
    with pytest.raises(_lib.RobirHipError, match="overflowed its activation range") as ei:
        ops.range_check(sync=True)
    assert kernel_name in str(ei.value), str(ei.value)
    ops.range_check(sync=True)                                       # reading cleared the words
    assert not bad, bad


def _head_split(k):
    """fused kernel: how 2^-k is taken back behind hidden layers 0-2 so that the logits stay those of the base weights: the output layer's
    weights take what keeps them inside the f16 range and the bf8 window (2^-6 .. 2^14), hidden layer 3's weights the rest.  -> (k3, head_k)"""
    k3 = min(max(k, -14), 6)
    return k3, -k3


def test_light_visibility_power_of_two_regimes(monkeypatch):
    """The fused light-visibility kernel through get_diffuse_visibility in the forms that ship -- f16x6-pt and f16x6-stream (bf8 weight layout: two
    of the six products from bf8 copies) and, when the legacy library loads, f16x6-1t (six f16 products) -- with the hidden activations of the
    visibility MLP moved by exact powers of two.  The visibility is a soft-max of the logits, which is NOT homogeneous, so here 2^-k is taken
    back (powers of two again, _head_split): the activations that enter the three 256 x 256 layers -- hidden layers 0-2 -- sit in the regime,
    the output layer's input at most 2^14 down / 2^6 up, and logits, visibilities and both oracles are those of the base weights bit for bit;
    so must the f32-input-MFMA kernel's be (the harness check).  Rule inside a form's window (six products: hot, bf8_edge, cold; bf8: hot,
    bf8_edge); in the first regime below it (six products: below; bf8: cold) the 1e-4 / 4e-4 bar, and run-to-run bit-identity wherever a form is
    below its window, every quantile recorded; hot + 1 is reported by the sentinel."""
    from robir_amd import _lib, nets, ops, sg_render, synth
    from robir_oracle import nets as on
    from robir_oracle.encoding import pe
    dev = torch.device("cuda:0")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    sd_np = {k: v for k, v in synth.synth_state_dict(0, variance=0.3).items() if k.startswith("visibility_network.")}
    g = np.random.Generator(np.random.PCG64(62))
    n, L, nsamp = 64, 128, 32
    pts = torch.from_numpy((g.standard_normal((n, 3)) * 0.25).astype(np.float32))
    nrm = torch.nn.functional.normalize(torch.from_numpy(g.standard_normal((n, 3)).astype(np.float32)), dim=-1)
    lgt = torch.from_numpy(synth.synth_light_sgs(3, L))
    lobe, lam = torch.nn.functional.normalize(lgt[:, :3], dim=-1), lgt[:, 3:4].abs()
    u = torch.from_numpy(g.random((2, L, nsamp), dtype=np.float32))
    draws = {"dvis_theta": u[0][None].to(dev), "dvis_phi": u[1][None].to(dev)}
    sd32 = on.as_torch(sd_np)
    sd64 = _f64(sd32)
    layers64 = [(sd64[on.VIS + "%d.weight" % (2 * i)], sd64[on.VIS + "%d.bias" % (2 * i)]) for i in range(5)]
    seen = []

    def vis64(p, d):              # the float64 oracle, noting the hidden activations of the pairs the kernels evaluate (the front-facing ones)
        seen.append(_hidden_magnitudes(layers64, torch.cat([pe(p.double(), 10), pe(d.double(), 10)], -1), torch.relu, stride=16))
        return on.vis_logits(sd64, p.double(), d.double())

    # identical fp32 inputs for every column: the sampled directions and lobe weights the kernels themselves are handed (ops.dvis_dirs, on the
    # device), the cull on them in fp32; the MLP, the soft-max and the lobe-weighted mean in float64 (r64) / PyTorch-CPU float32 (o32)
    lgt7 = torch.zeros(L, 7)
    lgt7[:, :3], lgt7[:, 3:4] = lobe, lam
    dirs, wdir, wsum = (t.cpu() for t in ops.dvis_dirs(lgt7.to(dev), draws["dvis_theta"], draws["dvis_phi"], 1.0, direct=True))
    dd = dirs.reshape(L * nsamp, 3)
    front = (nrm.unsqueeze(1) * dd.unsqueeze(0)).sum(-1) > 1e-6
    pi_, di_ = front.nonzero(as_tuple=True)

    def oracle(vis_fn, dt):
        vis = torch.zeros(n, L * nsamp, dtype=dt)
        vis[front] = torch.softmax(vis_fn(pts[pi_], dd[di_]), -1)[..., 1]
        return ((vis.reshape(n, L, nsamp) * wdir.reshape(1, L, nsamp).to(dt)).sum(-1) / wsum.reshape(1, L).to(dt)).t()

    r64, o32 = oracle(vis64, torch.float64), oracle(lambda p, d: on.vis_logits(sd32, p, d), torch.float32)
    assert r64.dtype == torch.float64 and o32.dtype == torch.float32 and r64.shape == (L, n)
    mx012, mx3 = max(max(s[0][:3]) for s in seen), max(s[0][3] for s in seen)
    med = float(np.median([m for s in seen for m in s[1][:3]]))
    largest = lambda k: max(mx012 * 2.0 ** k, mx3 * 2.0 ** _head_split(k)[0])      # noqa: E731
    ks = _regime_ks(mx012, med)
    assert 32752.0 <= largest(ks["hot"]) < 65504.0 <= mx012 * 2.0 ** (ks["hot"] + 1), (mx012, mx3, ks)
    assert ks["hot"] > 0 > ks["bf8_edge"] > ks["cold"] > ks["below"], (mx012, med, ks)
    forms = {"f16x6-pt": "bf8", "f16x6-stream": "bf8"}
    try:
        _lib.legacy()
        forms["f16x6-1t"] = "six"
    except Exception:
        pass
    # rule | the 1e-4 / 4e-4 bar (the first regime below a form's window) | recorded only: at a median of 2^-26.5 the bf8 copy of an
    # activation's third piece is off by up to BF8_BELOW_WINDOW_ABS_ERR = 2^-38 (tests/split_model.py), 2^-11.5 = 3.4e-4 of the operand: the
    # operand model itself puts this regime beyond the bar, so nothing is asserted on its error but that it repeats bit for bit
    window = {"six": ("base", "hot", "bf8_edge", "cold"), "bf8": ("base", "hot", "bf8_edge")}
    barred = {"six": ("below",), "bf8": ("cold",)}

    def run(k, mode):
        sd = _pow2_regime(sd_np, on.VIS, k, *_head_split(k))
        v = nets.VisNetwork(10, 10, [256] * 4)
        v.load_state_dict({key[len("visibility_network."):]: torch.from_numpy(w) for key, w in sd.items()})
        v = v.to(dev).eval()
        monkeypatch.setattr(sg_render, "VIS_PRECISION", mode)
        return sg_render.get_diffuse_visibility(pts.to(dev), nrm.to(dev), v, lobe.to(dev), lam.to(dev), nsamp=nsamp, draws=draws).cpu()

    ops.range_check(sync=True)
    k32_base, bad = None, []
    st0 = {"o32": _quantiles(o32, r64)}
    for regime, k in ks.items():
        k32 = run(k, "fp32")
        if regime == "base":
            k32_base = k32
        assert torch.equal(k32, k32_base), (regime, k, "fp32 itself left its range: the regime measures nothing")
        st = dict(st0, k32=_quantiles(k32, r64))
        for mode, kind in forms.items():
            a = run(k, mode)
            ops.range_check(sync=True)
            st[mode] = _quantiles(a, r64)
            if regime in window[kind]:
                bad += [(regime,) + b for b in _rule_violations(st, mode)]
            else:
                assert torch.equal(a, run(k, mode)), (regime, mode)
                assert bool(torch.isfinite(a).all()), (regime, mode)
                if regime in barred[kind] and not (st[mode]["p99"] <= 1e-4 and st[mode]["max"] <= 4e-4):
                    bad.append((regime, mode, "bar", st[mode]))
        record_metric(f"pow2_regimes/light_visibility/{regime}", k=k, largest_hidden=largest(k), median_hidden_0_2=med * 2.0 ** k,
                      entries=int(r64.numel()), **_flat(st))
        print(f"light visibility {regime:9s} k {k:4d}  " + "  ".join(f"{c}: p50 {d['p50']:.2e} p99 {d['p99']:.2e} max {d['max']:.2e}" for c, d in st.items()))
    for mode in forms:
        run(ks["hot"] + 1, mode)
        with pytest.raises(_lib.RobirHipError, match="overflowed its activation range") as ei:
            ops.range_check(sync=True)
        assert "light-visibility" in str(ei.value) and "rb_dvis_fused" in str(ei.value), (mode, str(ei.value))
        ops.range_check(sync=True)
    assert not bad, bad
