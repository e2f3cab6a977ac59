"""Trainable materials on the GPU: rb_train_ae_bwd (librobir_hip_train.so), robir_amd/ae_autograd.py and robir_amd/training.py.

The truth is float64 autograd of the oracle's formulas (robir_oracle.nets.sparse_ae through tests/material_train_oracle.py) on the CPU, fed
the same fp32 feature rows and noise the kernels saw; tests/golden/ae_grad.npz (tools/gen_material_grad_golden.py) pins that oracle on the
REFERENCE's own SparseAE.  The yardstick is test_sg_backward_gpu's rule: for every gradient tensor `e_kernel <= max(2 e_torch, 1e-5)`, e =
conftest.rel_err against float64, e_torch what PyTorch's fp32 autograd of the same formulas achieves on the same inputs.  Every pair is
recorded.  conftest wraps every test in no_grad: the tests enter torch.enable_grad() themselves."""
import gc
import weakref

import numpy as np
import pytest
import torch

import material_train_oracle as mto
import sg_backward_oracle as sbo
from conftest import record_metric, rel_err, load_golden

pytestmark = pytest.mark.gpu
FLOOR = 1e-5
MAT = "envmap_material_network."


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _weights(synth_weights, which):
    if which == "init":
        return synth_weights
    import importlib
    return importlib.import_module("test_mlp_gpu")._trained_like(synth_weights, 5)


def _material_net(dev, sd, train=True):
    from robir_amd import nets
    net = nets.EnvmapMaterialNetwork(multires=10, num_lgt_sgs=128, specular_albedo=0.05)
    net.load_state_dict({k[len(MAT):]: torch.as_tensor(v) for k, v in sd.items() if k.startswith(MAT)})
    net = net.to(dev)
    return net.train() if train else net.eval()


def assert_parity(tag, kernel, torch32, ref64):
    bad = []
    for k, r in ref64.items():
        r = torch.as_tensor(r)
        e_kernel = rel_err(kernel[k].reshape(r.shape), r)
        e_torch = rel_err(torch32[k].reshape(r.shape), r)
        record_metric(f"material_train/{tag}/{k}", e_kernel=e_kernel, e_torch=e_torch, max_abs_ref=float(r.abs().max()))
        print(f"{tag:44s} d {k:30s} e_kernel {e_kernel:.2e}  e_torch {e_torch:.2e}")
        if not e_kernel <= max(2.0 * e_torch, FLOOR):
            bad.append((k, e_kernel, e_torch))
    assert not bad, (tag, bad)


def _inputs(n, seed=0, var=False):
    g = torch.Generator().manual_seed(100 + seed)
    pts = torch.randn(n, 3, generator=g) * 0.5
    noise = torch.randn(n, 32, generator=g)
    ups = dict(g_out=torch.randn(n, 5, generator=g), g_out_xi=torch.randn(n, 5, generator=g), g_raw=torch.randn(n, 32, generator=g))
    v = torch.rand(32, generator=g) * 0.5 if var else None
    return pts, noise, ups, v


def _kernel(dev, params, X, noise, ups, **kw):
    """ops.ae_backward on device copies -> (dict of CPU gradients, stats)."""
    from robir_amd import ops
    D = lambda t: None if t is None else torch.as_tensor(t).float().to(dev).contiguous()
    opt = {k: D(kw.pop(k)) for k in ("var",) if k in kw}
    out, stats = ops.ae_backward(X, [D(params[k]) for k in mto.NAMES], D(ups.get("g_out")), D(ups.get("g_out_xi")), D(ups.get("g_raw")),
                                 noise=D(noise), **opt, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}, stats


def _features(dev, pts):
    from robir_amd import ops
    return ops.feat_pe10(pts.to(dev).contiguous())


_REF = {}


def _truth(key, params, X, noise, ups, **kw):
    """(float64 gradients, fp32 gradients) of the oracle, computed once per case and shared."""
    if key not in _REF:
        Xc = X.cpu()
        _REF[key] = (mto.ae_grads(params, Xc, noise, dtype=torch.float64, **ups, **kw), mto.ae_grads(params, Xc, noise, dtype=torch.float32, **ups, **kw))
    return _REF[key]


# ------------------------------------------------------------------------------------------------ 1. fails without the feature
def test_marked_network_trains(dev, synth_weights):
    from robir_amd import nets, sg_autograd, training
    net = _material_net(dev, synth_weights)
    pts, noise, _, _ = _inputs(64)
    pts = torch.nn.functional.normalize(pts, dim=-1).to(dev)
    nz = {"spec": noise.to(dev), "normal": torch.randn(64, 60, generator=torch.Generator().manual_seed(1)).to(dev)}
    with torch.enable_grad():
        with pytest.raises(nets.ForwardOnlyError):
            net(pts, train_spec=True, noise=nz)
        assert training.enable_material_training(net) is net
        out = net(pts, train_spec=True, noise=nz)
        for k in ("sg_diffuse_albedo", "sg_roughness", "sg_metallic", "random_xi_diffuse_albedo", "random_xi_roughness", "random_xi_metallic"):
            assert out[k].requires_grad, k
        assert not out["sg_normal_map"].requires_grad and not out["random_xi_normal"].requires_grad
        assert out["sg_lgtSGs"] is net.lgtSGs and out["sg_specular_reflectance"] is net.specular_reflectance
        raw = net.spec_brdf_encoder_layer.encode(_features(dev, pts)[:, :63])
        assert raw.requires_grad and tuple(raw.shape) == (64, 32)
        g = torch.Generator().manual_seed(2)
        view = torch.nn.functional.normalize(pts.cpu() + 0.5 * torch.randn(64, 3, generator=g), dim=-1).to(dev)
        rgb = sg_autograd.sg_shade(pts, view, out["sg_lgtSGs"], out["sg_specular_reflectance"].abs(), out["sg_roughness"], out["sg_diffuse_albedo"],
                                   torch.rand(64, generator=g).to(dev), light_vis=torch.rand(64, 128, generator=g).to(dev))[0]
        loss = rgb.abs().mean() + training.kl_sparsity(raw) + 0.1 * training.latent_smooth(out)
        loss.backward()
    for name, p in net.named_parameters():
        touched = name.startswith("spec_brdf_encoder_layer.") or name in ("lgtSGs", "specular_reflectance")
        assert (p.grad is not None) == touched, name
        if touched:
            assert tuple(p.grad.shape) == tuple(p.shape) and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
    # the values of the trainable path are the forward-only path's, bit for bit (conftest's no_grad is active here)
    ref = net(pts, train_spec=True, noise=nz)
    for k, v in ref.items():
        assert not v.requires_grad or k in ("sg_lgtSGs", "sg_specular_reflectance"), k
        assert torch.equal(out[k].detach(), v.detach()), k
    assert torch.equal(raw.detach(), net.spec_brdf_encoder_layer.encode(_features(dev, pts)[:, :63]))
    # train_spec=False: the reference's .detach(); unmarking restores the guard
    with torch.enable_grad():
        out = net(pts, train_spec=False, noise=nz)
        assert not out["sg_roughness"].requires_grad and not out["sg_diffuse_albedo"].requires_grad
        training.enable_material_training(net, on=False)
        with pytest.raises(nets.ForwardOnlyError):
            net(pts, train_spec=True, noise=nz)


# ------------------------------------------------------------------------------------------------ 2. kernel-level parity
@pytest.mark.parametrize("weights", ["init", "trained_like"])
@pytest.mark.parametrize("n,slab", [(1, None), (17, None), (257, None), (150, 64)])
def test_kernel_parity(dev, synth_weights, weights, n, slab):
    """n = 1: a single row; 17: one past a 16-row MFMA tile; 257: ragged 64-row block tiles; 150 with slab_rows 64: three slabs, the last ragged.
    Random normal upstream gradients on all three outputs; all sixteen gradients compared."""
    params = mto.ae_params(_weights(synth_weights, weights))
    pts, noise, ups, _ = _inputs(n, seed=n)
    X = _features(dev, pts)
    ref64, t32 = _truth(("full", weights, n), params, X, noise, ups)
    kernel, stats = _kernel(dev, params, X, noise, ups, slab_rows=slab)
    assert set(kernel) == set(mto.NAMES) and stats["encoder_pass"]
    assert tuple(kernel["brdf_encoder_layer.0.weight"].shape) == (512, 63)
    assert_parity(f"kernel/{weights}/n{n}" + (f"_slab{slab}" if slab else ""), kernel, t32, ref64)


@pytest.mark.parametrize("absent", ["g_out", "g_out_xi", "g_raw"])
def test_kernel_parity_with_an_upstream_absent(dev, synth_weights, absent):
    params = mto.ae_params(synth_weights)
    pts, noise, ups, _ = _inputs(17, seed=17)
    ups = {k: v for k, v in ups.items() if k != absent}
    X = _features(dev, pts)
    ref64, t32 = _truth(("absent", absent), params, X, noise, ups)
    kernel, _ = _kernel(dev, params, X, noise, ups)
    assert_parity(f"kernel/without_{absent}", kernel, t32, ref64)


@pytest.mark.parametrize("case", ["var", "no_out_act", "softplus_latent"])
def test_kernel_parity_variants(dev, synth_weights, case):
    """A non-zero `var`, out_act=None, and the softplus latent activation code."""
    params = mto.ae_params(synth_weights)
    pts, noise, ups, var = _inputs(150, seed=3, var=True)
    X = _features(dev, pts)
    okw = dict(var=var) if case == "var" else dict(sigmoid_out=False) if case == "no_out_act" else dict(latent_act=1)
    ref64, t32 = _truth(("variant", case), params, X, noise, ups, **okw)
    kernel, _ = _kernel(dev, params, X, noise, ups, slab_rows=64, **okw)
    assert_parity(f"kernel/{case}", kernel, t32, ref64)


def test_kernel_against_the_reference_fixture(dev, synth_weights):
    """tests/golden/ae_grad.npz: the REFERENCE's SparseAE differentiated in float64 on 32 rows; the oracle's recorded distance from it is
    <= 1e-10 and the kernel holds the rule against every stored piece."""
    fx = load_golden("ae_grad")
    params = mto.ae_params(synth_weights)
    pts, noise = torch.from_numpy(fx["points"]), torch.from_numpy(fx["noise"])
    ups = {k: torch.from_numpy(fx[k]) for k in ("g_out", "g_out_xi", "g_raw")}
    X = _features(dev, pts)
    kernel, _ = _kernel(dev, params, X, noise, ups)
    t32 = mto.ae_grads(params, X.cpu(), noise, dtype=torch.float32, **ups)

    def pieces(g, k):
        if g.dim() == 1:
            return {f"{k}.full": g}
        return {f"{k}.rows8": g[:8], f"{k}.cols8": g[:, :8], f"{k}.sum": g.double().sum(), f"{k}.fro": g.double().norm()}
    K, T, R = {}, {}, {}
    for k in mto.NAMES:
        K.update(pieces(kernel[k], k))
        T.update(pieces(t32[k], k))
    for key in K:
        assert float(fx["oracle_dist." + key]) <= 1e-10, key
        R[key] = torch.from_numpy(np.asarray(fx["grad." + key]))
    assert_parity("reference_fixture", K, T, R)


# ------------------------------------------------------------------------------------------------ 3. gradient subsets
def test_decoder_only_stops_at_the_latent(dev, synth_weights):
    params = mto.ae_params(synth_weights)
    pts, noise, ups, _ = _inputs(150, seed=5)
    X = _features(dev, pts)
    full, fs = _kernel(dev, params, X, noise, ups, slab_rows=64)
    dec = tuple(k for k in mto.NAMES if k.startswith("brdf_decoder_layer."))
    part, ps = _kernel(dev, params, X, noise, ups, slab_rows=64, want=dec)
    assert set(part) == set(dec) and len(dec) == 6
    assert fs["encoder_pass"] and not ps["encoder_pass"] and ps["launches"] < fs["launches"]
    for k in dec:
        assert torch.equal(part[k], full[k]), k
    one, os_ = _kernel(dev, params, X, noise, ups, slab_rows=64, want=("brdf_encoder_layer.4.bias",))
    assert set(one) == {"brdf_encoder_layer.4.bias"} and os_["encoder_pass"] and os_["launches"] < fs["launches"]
    assert torch.equal(one["brdf_encoder_layer.4.bias"], full["brdf_encoder_layer.4.bias"])
    # through autograd: frozen encoder parameters turn into NULL pointers
    from robir_amd import ae_autograd, training
    net = _material_net(dev, synth_weights)
    ae = training.enable_material_training(net).spec_brdf_encoder_layer
    for p in ae.brdf_encoder_layer.parameters():
        p.requires_grad_(False)
    with torch.enable_grad():
        out, out_xi, raw = ae_autograd.run_points(ae, pts.to(dev), noise.to(dev))
        ((out * ups["g_out"].to(dev)).sum() + (out_xi * ups["g_out_xi"].to(dev)).sum() + (raw * ups["g_raw"].to(dev)).sum()).backward()
    for name, p in ae.named_parameters():
        assert (p.grad is not None) == name.startswith("brdf_decoder_layer."), name
        if p.grad is not None:
            assert torch.equal(p.grad.cpu(), _kernel(dev, params, X, noise, ups, want=(name,))[0][name]), name


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_determinism_and_slab_independence(dev, synth_weights):
    params = mto.ae_params(synth_weights)
    pts, noise, ups, _ = _inputs(257, seed=257)
    X = _features(dev, pts)
    a, _ = _kernel(dev, params, X, noise, ups)
    b, _ = _kernel(dev, params, X, noise, ups)
    for k in mto.NAMES:
        assert torch.equal(a[k], b[k]), k
    c, _ = _kernel(dev, params, X, noise, ups, slab_rows=64)
    ref64, t32 = _truth(("full", "init", 257), params, X, noise, ups)
    assert_parity("kernel/init/n257_slab64", c, t32, ref64)


# ------------------------------------------------------------------------------------------------ 5. the stage-3 hook body
@pytest.fixture(scope="module")
def model(dev):
    from robir_amd import renderer
    m = renderer.build_synthetic_model(dev, seed=0, variance=0.3)
    m.deferred_chunks = 0
    return m


def test_stage3_hook_body_gradients_vs_oracle(dev, model, synth_weights):
    """PBRTrainRunner.get_sg_render (training/train_pbr.py:348-396) restated test-side as tests/test_runner_hooks_gpu.py does, on ~200 hit
    points of the 64 x 64 synthetic view, the material network marked and in training mode, everything else in eval().  Loss = L1 on sg_rgb +
    kl_sparsity + 0.1 latent_smooth; the gradients of the spec auto-encoder, lgtSGs and specular_reflectance from ONE backward() against the
    oracle in float64 with the HIP forward's own sampled visibilities and the draws injected."""
    from robir_amd import sg_render, synth, training
    uv, pose, K = synth.synth_camera(64, 64)
    sl = slice(1024, 2048)
    inp = {"uv": torch.from_numpy(uv[sl]).to(dev)[None], "pose": torch.from_numpy(pose).to(dev)[None], "intrinsics": torch.from_numpy(K).to(dev)[None],
           "object_mask": torch.ones(1, 1024, dtype=torch.bool, device=dev), "hdr_shift": torch.full((1024, 1), 0.5, device=dev)}
    model.eval()
    first = model(inp, trainstage="Material", train_spec=True)
    idx = first["network_object_mask"].nonzero()[:200, 0]
    n = int(idx.shape[0])
    assert 100 <= n <= 200
    points, view_dirs = first["points"][idx].contiguous(), (-first["ray_dirs"][idx]).contiguous()
    dr = {k: torch.from_numpy(v).to(dev) for k, v in synth.pbr_draws(7, n, chunk_id=1).items()}
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(9)).to(dev)
    indir_sgs, indir_int = model.indirect_illum_network(points, torch.full((n, 1), 0.5, device=dev), noise=dr["illum_randn"])
    mat_net = model.envmap_material_network
    try:
        mat_net.train()
        training.enable_material_training(model)
        v = view_dirs / (torch.norm(view_dirs, dim=-1, keepdim=True) + 1e-6)
        with torch.enable_grad():
            mat = mat_net(points, train_spec=True, noise={"spec": dr["spec_randn"], "normal": dr["normal_randn"]})
            nrm = mat["sg_normal_map"].detach()
            out = sg_render.render_with_all_sg(points=points.detach(), normal=nrm, viewdirs=v, lgtSGs=mat["sg_lgtSGs"],
                                               indir_integral=indir_int * 2 * np.pi, specular_reflectance=mat["sg_specular_reflectance"].abs(),
                                               roughness=mat["sg_roughness"], diffuse_albedo=mat["sg_diffuse_albedo"], indir_lgtSGs=indir_sgs,
                                               VisModel=model.visibility_network, fun_spec=False, lin_diff=False, testing=False, metallic=None,
                                               draws=dr)
            raw = mat_net.spec_brdf_encoder_layer.encode(_features(dev, points)[:, :63])
            loss = (out["sg_rgb"] - target).abs().mean() + training.kl_sparsity(raw) + 0.1 * training.latent_smooth(mat)
            loss.backward()
        ae = mat_net.spec_brdf_encoder_layer
        kernel = {k: p.grad.detach().cpu() for k, p in ae.named_parameters()}
        kernel["lgtSGs"], kernel["specular_reflectance"] = mat_net.lgtSGs.grad.cpu(), mat_net.specular_reflectance.grad.cpu()
        for name, p in mat_net.named_parameters():
            if name.startswith(("normal_decoder_layer.", "brdf_encoder_layer.")):
                assert p.grad is None, name
        # the HIP forward's sampled visibilities (constants of the backward)
        rough = mat["sg_roughness"].detach()
        bvis = sg_render.get_specular_visibility(points, nrm, v, model.visibility_network, None, None, nsamp=8, testing=False, inv=False,
                                                 roughness=rough, draws=(dr["svis_theta_dir"], dr["svis_phi_dir"])).cpu()
        lvis = sg_render._diffuse_vis_core(points, nrm, model.visibility_network, mat_net.lgtSGs.detach(), dr["dvis_theta"], dr["dvis_phi"], 1.0,
                                           False, None, 1, None).cpu()
        X = _features(dev, points).cpu()
    finally:
        training.enable_material_training(model, on=False)
        mat_net.zero_grad(set_to_none=True)
        model.eval()

    params = mto.ae_params(synth_weights)

    def oracle(dtype):
        c = lambda t: t.detach().cpu().to(dtype)
        with torch.enable_grad():
            leaves = {k: p.to(dtype).clone().requires_grad_(True) for k, p in params.items()}
            leaves["lgtSGs"] = torch.as_tensor(synth_weights[MAT + "lgtSGs"]).to(dtype).clone().requires_grad_(True)
            leaves["specular_reflectance"] = torch.as_tensor(synth_weights[MAT + "specular_reflectance"]).to(dtype).clone().requires_grad_(True)
            brdf, brdf_r, raw = mto.ae_forward({k: leaves[k] for k in mto.NAMES}, X, c(dr["spec_randn"]))
            m = {"sg_diffuse_albedo": brdf[:, :3], "sg_roughness": brdf[:, 3:4] * 0.9 + 0.09, "random_xi_diffuse_albedo": brdf_r[:, :3],
                 "random_xi_roughness": brdf_r[:, 3:4] * 0.9 + 0.09}
            spec, diff = sbo.shade(c(nrm), c(v), leaves["lgtSGs"], leaves["specular_reflectance"].abs(), m["sg_roughness"].reshape(-1),
                                   m["sg_diffuse_albedo"], c(bvis).reshape(-1), light_vis=c(lvis))
            loss = ((spec + diff) - c(target)).abs().mean() + training.kl_sparsity(raw) + 0.1 * training.latent_smooth(m)
            gr = torch.autograd.grad(loss, list(leaves.values()))
        return dict(zip(leaves, gr)), float(loss.detach())

    (ref64, l64), (t32, _) = oracle(torch.float64), oracle(torch.float32)
    record_metric("material_train/stage3/loss", hip=float(loss.detach()), oracle64=l64)
    assert all(float(g.abs().max()) > 0 for g in ref64.values())
    assert_parity("stage3_hook", kernel, t32, ref64)


# ------------------------------------------------------------------------------------------------ 6. a fit
def test_fit_descends_and_the_weight_cache_follows_the_optimiser(dev, synth_weights):
    """20 Adam steps (lr 5e-4) on 256 points towards the materials of a second seed's network.  The first step's gradient holds the rule, the
    loss after step 20 is below the loss at step 0, the trajectory is recorded beside the float64 oracle's.  The step-2 forward equals a fresh
    module loaded with the updated state dict, bit for bit: every packed blob of the marked path follows optimizer.step()."""
    from robir_amd import synth, training
    n, steps = 256, 20
    pts, noise, _, _ = _inputs(n, seed=6)
    pts = torch.nn.functional.normalize(pts, dim=-1)
    nz = {"spec": noise.to(dev), "normal": torch.zeros(n, 60, device=dev)}
    target_net = _material_net(dev, synth.synth_state_dict(1, variance=0.3), train=False)
    tgt = target_net(pts.to(dev), train_spec=True, noise=nz)
    tgt = torch.cat([tgt["sg_diffuse_albedo"], tgt["sg_roughness"], tgt["sg_metallic"]], -1)
    net = _material_net(dev, synth_weights)
    training.enable_material_training(net)
    ae = net.spec_brdf_encoder_layer
    opt = torch.optim.Adam(ae.parameters(), lr=5e-4)
    losses, g0 = [], None
    for step in range(steps + 1):
        if step == 2:
            fresh = _material_net(dev, {MAT + k: v.detach().cpu() for k, v in net.state_dict().items()}, train=False)
            a, b = net(pts.to(dev), train_spec=True, noise=nz), fresh(pts.to(dev), train_spec=True, noise=nz)      # no_grad (conftest)
            for k in a:
                assert torch.equal(a[k].detach(), b[k].detach()), k
        with torch.enable_grad():
            opt.zero_grad()
            out = net(pts.to(dev), train_spec=True, noise=nz)
            got = torch.cat([out["sg_diffuse_albedo"], out["sg_roughness"], out["sg_metallic"]], -1)
            loss = ((got - tgt) ** 2).mean() + 0.1 * training.latent_smooth(out)
            loss.backward()
        losses.append(float(loss.detach()))
        if g0 is None:
            g0 = {k: p.grad.detach().cpu().clone() for k, p in ae.named_parameters()}
        opt.step()

    X = _features(dev, pts).cpu()

    def oracle_fit(dtype, n_steps):
        leaves = {k: v.to(dtype).clone().requires_grad_(True) for k, v in mto.ae_params(synth_weights).items()}
        o = torch.optim.Adam(list(leaves.values()), lr=5e-4)
        ls, first = [], None
        for _ in range(n_steps + 1):
            with torch.enable_grad():
                o.zero_grad()
                brdf, brdf_r, _ = mto.ae_forward(leaves, X, noise)
                m = {"sg_diffuse_albedo": brdf[:, :3], "sg_roughness": brdf[:, 3:4] * 0.9 + 0.09, "random_xi_diffuse_albedo": brdf_r[:, :3],
                     "random_xi_roughness": brdf_r[:, 3:4] * 0.9 + 0.09}
                got = torch.cat([m["sg_diffuse_albedo"], m["sg_roughness"], brdf[:, 4:5] * 0.99 + 0.01], -1)
                loss = ((got - tgt.cpu().to(dtype)) ** 2).mean() + 0.1 * training.latent_smooth(m)
                loss.backward()
            ls.append(float(loss.detach()))
            if first is None:
                first = {k: p.grad.detach().clone() for k, p in leaves.items()}
            o.step()
        return ls, first

    l64, g64 = oracle_fit(torch.float64, steps)
    _, g32 = oracle_fit(torch.float32, 0)
    record_metric("material_train/fit", **{f"hip_{i}": v for i, v in enumerate(losses)}, **{f"oracle64_{i}": v for i, v in enumerate(l64)})
    print("material fit  HIP     ", " ".join(f"{v:.4e}" for v in losses))
    print("material fit  oracle64", " ".join(f"{v:.4e}" for v in l64))
    assert_parity("fit/first_step", g0, g32, g64)
    assert losses[-1] < losses[0]


# ------------------------------------------------------------------------------------------------ 7. refusals and lifetimes
def test_points_refuse_a_gradient(dev, synth_weights):
    from robir_amd import ae_autograd, training
    net = _material_net(dev, synth_weights)
    training.enable_material_training(net)
    pts, noise, _, _ = _inputs(8)
    with torch.enable_grad():
        p = pts.to(dev).requires_grad_()
        with pytest.raises(NotImplementedError, match="points"):
            net(p, train_spec=True, noise={"spec": noise.to(dev)})
        with pytest.raises(NotImplementedError, match="points"):
            ae_autograd.run_points(net.spec_brdf_encoder_layer, p, noise.to(dev))
    out = net(p, train_spec=True, noise={"spec": noise.to(dev)})          # grad mode off: today's forward, no refusal
    assert not out["sg_roughness"].requires_grad


def test_graph_is_freed_by_reference_counting(dev, synth_weights):
    """Only save_for_backward holds tensors: once the outputs and the loss are dropped -- with or without a backward() -- the allocation
    returns to its base with the cyclic collector disabled."""
    from robir_amd import training
    net = _material_net(dev, synth_weights)
    training.enable_material_training(net)
    pts, noise, _, _ = _inputs(2048, seed=8)
    pts, nz = pts.to(dev), {"spec": noise.to(dev), "normal": torch.zeros(2048, 60, device=dev)}
    net(pts, train_spec=True, noise=nz)                  # packed blobs and side streams exist before the base is read
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        for run_backward in (False, True):
            net.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            with torch.enable_grad():
                out = net(pts, train_spec=True, noise=nz)
                loss = out["sg_roughness"].sum() + training.latent_smooth(out)
                refs = [weakref.ref(out["sg_roughness"]), weakref.ref(loss)]
                assert torch.cuda.memory_allocated() > base
                if run_backward:
                    loss.backward()
            del out, loss
            assert all(r() is None for r in refs)
            net.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            assert torch.cuda.memory_allocated() == base, (run_backward, torch.cuda.memory_allocated() - base)
    finally:
        if was:
            gc.enable()
