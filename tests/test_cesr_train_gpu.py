"""Trainable CESR networks on the GPU: rb_ct_cesr_bwd (librobir_hip_cesrtrain.so), robir_amd/cesr_autograd.py, robir_amd/training.py and
renderer.CESRHook with marked shadow_net / normal_net.

The truth is float64 autograd of the oracle's formulas (robir_oracle.nets.softplus_net512 through tests/cesr_train_oracle.py) on the CPU, fed
the same fp32 inputs the kernels saw; tests/golden/cesr_grad.npz / cesr_grad_normal.npz (tools/gen_cesr_grad_golden.py) pin that oracle on the
REFERENCE's own SDFNetwork.  The yardstick is the project's rule: for every tensor `e_kernel <= max(2 e_torch, 1e-5)`, e = conftest.rel_err
against float64, e_torch what PyTorch's fp32 autograd of the same formulas achieves on the same inputs.  Every pair is recorded.  conftest wraps
every test in no_grad: the tests enter torch.enable_grad() themselves."""
import gc
import weakref

import numpy as np
import pytest
import torch

import cesr_train_oracle as cto
from conftest import record_metric, rel_err, load_golden

pytestmark = pytest.mark.gpu
FLOOR = 1e-5
HEADS = {"shadow": (0, 1), "normal": (0, 2)}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _weights(kind, which):
    """"init": robir_amd.synth.synth_cesr_nets(0); "perturbed": + 0.02 N(0,1) on every weight_v (seed fixed), so that no layer is near its
    initial structure and g no longer is 0.9 .. 1.1 |v|."""
    from robir_amd import synth
    sd = {k: torch.from_numpy(np.asarray(v)).clone() for k, v in synth.synth_cesr_nets(0)[kind + "_net"].items()}
    if which == "perturbed":
        g = torch.Generator().manual_seed(78)
        for k in sorted(sd):
            if k.endswith("weight_v"):
                sd[k] = sd[k] + 0.02 * torch.randn(sd[k].shape, generator=g)
    return sd


def _net(dev, kind, sd, train=True):
    from robir_amd import nets
    net = nets.SDFNetwork(191, 2, 512, 8, [4], 0) if kind == "shadow" else nets.SDFNetwork(63, 3, 512, 8, [4], 0)
    net.load_state_dict(sd)
    net = net.to(dev)
    return net.train() if train else net.eval()


def assert_parity(tag, kernel, torch32, ref64):
    bad = []
    for k, r in ref64.items():
        r = torch.as_tensor(r)
        e_kernel = rel_err(torch.as_tensor(kernel[k]).reshape(r.shape), r)
        e_torch = rel_err(torch.as_tensor(torch32[k]).reshape(r.shape), r)
        record_metric(f"cesr_train/{tag}/{k}", e_kernel=e_kernel, e_torch=e_torch, max_abs_ref=float(r.abs().max()))
        print(f"{tag:44s} d {k:16s} e_kernel {e_kernel:.2e}  e_torch {e_torch:.2e}")
        if not e_kernel <= max(2.0 * e_torch, FLOOR):
            bad.append((k, e_kernel, e_torch))
    assert not bad, (tag, bad)


def _inputs(kind, n_pts, n_label, seed):
    """Points and one upstream gradient per head, drawn in a fixed order."""
    g = torch.Generator().manual_seed(900 + seed)
    M = n_pts * n_label
    pts = torch.randn(n_pts, 3, generator=g) * 0.5
    return pts, {0: torch.randn(M, cto.DIMS[kind][1], generator=g), 1: torch.randn(M, generator=g), 2: torch.randn(M, 3, generator=g)}


def _kernel(dev, kind, params, x, g_out, head, n_label=1, **kw):
    """ops.cesr_backward on device copies -> (dict of CPU gradients, stats)."""
    from robir_amd import ops
    D = lambda t: torch.as_tensor(t).float().to(dev).contiguous()
    M = x.shape[0] * n_label if x.shape[1] == 3 else x.shape[0]
    out, stats = ops.cesr_backward(D(x), M, kind, [D(params[k]) for k in cto.NAMES], D(g_out), head=head, n_label=n_label, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}, stats


_REF = {}


def _truth(key, params, x, kind, g_out, n_label, head):
    """(float64 gradients, fp32 gradients) of <g_out, head(net(x))> for the 27 tensors, computed once per case and shared."""
    if key not in _REF:
        _REF[key] = tuple(cto.grads(params, x, kind, g_out, dt, n_label, head) for dt in (torch.float64, torch.float32))
    return _REF[key]


# ------------------------------------------------------------------------------------------------ 1. fails without the feature
@pytest.mark.parametrize("kind", ["shadow", "normal"])
def test_marked_network_trains(dev, kind):
    from robir_amd import nets, training
    net = _net(dev, kind, _weights(kind, "init"))
    pts, g = _inputs(kind, 6, 1, 1)
    pts = pts.to(dev)
    call = (lambda: net.eval_point_labels(pts, 8)) if kind == "shadow" else (lambda: net._cesr_points(pts, 6, 0))
    with torch.enable_grad():
        with pytest.raises(nets.ForwardOnlyError):
            call()
        assert training.enable_cesr_training(net) is net
        y = call()
        assert y.grad_fn is not None and tuple(y.shape) == ((48, 2) if kind == "shadow" else (6, 3))
        y.square().sum().backward()
    named = dict(net.named_parameters())
    assert set(named) == set(cto.NAMES)
    for name, p in named.items():
        assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape), name
        assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
    # the values of the trainable path are the forward-only path's, bit for bit (conftest's no_grad is active here)
    ref = call()
    assert not ref.requires_grad and torch.equal(y.detach(), ref)
    with torch.enable_grad():          # the head helpers and the dense-rows forward
        if kind == "shadow":
            v = net.diffuse_vis(pts, 8)
            rows = cto.rows_of_points(pts.cpu(), 8, kind, torch.float32).to(dev)
        else:
            v = net.unit_normal(pts)
            rows = cto.rows_of_points(pts.cpu(), 1, kind, torch.float32).to(dev)
        d = net(rows)
        assert v.grad_fn is not None and d.grad_fn is not None and tuple(d.shape) == tuple(ref.shape)
    training.enable_cesr_training(net, on=False)
    from robir_amd import ops
    assert torch.equal(call(), ref) and torch.equal(d.detach(), net(rows))
    assert torch.equal(v.detach(), ops.softmax2(ref, 1) if kind == "shadow" else ops.normalize3(ref, 1e-4, 1))


# ------------------------------------------------------------------------------------------------ 2. kernel-level parity
NORMAL_CASES = [(1, 64, 64), (15, 64, 16), (17, 64, 16), (65, 64, 64), (200, 64, 48)]
SHADOW_CASES = [(1, 128, 64, 64), (3, 128, 64, 48), (25, 8, 64, 48), (5, 128, 1024, 80)]


@pytest.mark.parametrize("weights", ["init", "perturbed"])
@pytest.mark.parametrize("M,slab,part", NORMAL_CASES)
def test_normal_kernel_parity(dev, weights, M, slab, part):
    """(1,64,64), (15,64,16), (17,64,16): the 16-row MFMA tile edge; (65,64,64): a second slab of one row; (200,64,48): a ragged last
    partition and a ragged last slab of 8 rows.  The points form; heads 0 (raw) and 2 (unit vector); all 27 gradients."""
    params = cto.cesr_params(_weights("normal", weights))
    pts, g = _inputs("normal", M, 1, M)
    for head in HEADS["normal"]:
        ref64, t32 = _truth(("normal", weights, M, head), params, pts, "normal", g[head], 1, head)
        kernel, stats = _kernel(dev, "normal", params, pts, g[head], head, slab_rows=slab, part_rows=part)
        assert set(kernel) == set(cto.NAMES) and stats["lowest_layer"] == 0 and stats["partitions"] == -(-min(M, slab) // part)
        assert tuple(kernel["lin0.weight_v"].shape) == (512, 63) and tuple(kernel["lin3.weight_v"].shape) == (449, 512)
        assert tuple(kernel["lin3.weight_g"].shape) == (449, 1) and tuple(kernel["lin8.weight_v"].shape) == (3, 512)
        assert_parity(f"normal/{weights}/head{head}/M{M}_slab{slab}_part{part}", kernel, t32, ref64)


@pytest.mark.parametrize("weights", ["init", "perturbed"])
@pytest.mark.parametrize("n,n_label,slab,part", SHADOW_CASES)
def test_shadow_kernel_parity(dev, weights, n, n_label, slab, part):
    """(1,128,64,64): one point across two slabs; (3,128,64,48): the point changes at slab edges, ragged partitions; (25,8,64,48): points
    changing inside partitions, labels that do not fill the 128 columns; (5,128,1024,80): a single ragged slab.  The points form (the one-hot
    block comes from the row index); heads 0 (raw) and 1 (softmax class 1); all 27 gradients."""
    params = cto.cesr_params(_weights("shadow", weights))
    pts, g = _inputs("shadow", n, n_label, 10 * n + n_label)
    M = n * n_label
    for head in HEADS["shadow"]:
        ref64, t32 = _truth(("shadow", weights, n, n_label, head), params, pts, "shadow", g[head], n_label, head)
        kernel, stats = _kernel(dev, "shadow", params, pts, g[head], head, n_label=n_label, slab_rows=slab, part_rows=part)
        assert set(kernel) == set(cto.NAMES) and stats["lowest_layer"] == 0 and stats["partitions"] == -(-min(M, slab) // part)
        assert tuple(kernel["lin0.weight_v"].shape) == (512, 191) and tuple(kernel["lin3.weight_v"].shape) == (321, 512)
        assert tuple(kernel["lin8.bias"].shape) == (2,)
        assert_parity(f"shadow/{weights}/head{head}/n{n}x{n_label}_slab{slab}_part{part}", kernel, t32, ref64)


@pytest.mark.parametrize("weights", ["init", "perturbed"])
def test_shadow_dense_form(dev, weights):
    """(200, 64, 48) with dense one-hot rows [PE10 | one-hot] in fp32 on the same points and labels as a points-form call.  The two forms do
    NOT share the encoding -- the dense rows are the caller's fp32 features, the points form encodes in fp64 from the coordinates -- so the
    bytes differ, and each is compared under the yardstick with the truth on its own inputs; the two agree to fp32 rounding of the features."""
    params = cto.cesr_params(_weights("shadow", weights))
    pts, g = _inputs("shadow", 25, 8, 258)
    rows = cto.rows_of_points(pts, 8, "shadow", torch.float32)
    assert tuple(rows.shape) == (200, 191)
    for head in HEADS["shadow"]:
        ref64, t32 = _truth(("shadow-dense", weights, head), params, rows, "shadow", g[head], 1, head)
        dense, stats = _kernel(dev, "shadow", params, rows, g[head], head, slab_rows=64, part_rows=48)
        assert stats["partitions"] == 2 and stats["lowest_layer"] == 0
        assert_parity(f"shadow-dense/{weights}/head{head}", dense, t32, ref64)
        padded, _ = _kernel(dev, "shadow", params, torch.nn.functional.pad(rows, (0, 1)), g[head], head, slab_rows=64, part_rows=48)
        assert all(torch.equal(dense[k], padded[k]) for k in cto.NAMES)          # ld = 192: the same rows, the same bytes
        points_form, _ = _kernel(dev, "shadow", params, pts, g[head], head, n_label=8, slab_rows=64, part_rows=48)
        worst = max(rel_err(dense[k], points_form[k]) for k in cto.NAMES)
        record_metric(f"cesr_train/shadow-dense/{weights}/head{head}/vs_points_form", worst=worst)
        assert worst <= 1e-4, worst          # the fp32 features' rounding (6e-8 per column) through nine layers; not equal bytes


# ------------------------------------------------------------------------------------------------ 3. gradient subsets
def test_subsets_stop_the_data_path(dev):
    params = cto.cesr_params(_weights("shadow", "init"))
    pts, g = _inputs("shadow", 25, 8, 258)
    ref64, t32 = _truth(("shadow", "init", 25, 8, 1), params, pts, "shadow", g[1], 8, 1)
    run = lambda **kw: _kernel(dev, "shadow", params, pts, g[1], 1, n_label=8, slab_rows=64, part_rows=48, **kw)
    full, fs = run()
    last = tuple(k for k in cto.NAMES if k.startswith("lin8."))
    top, ts = run(want=last)
    assert set(top) == set(last) and ts["lowest_layer"] == 8 and fs["lowest_layer"] == 0 and ts["launches"] < fs["launches"]
    upper = tuple(k for k in cto.NAMES if int(k[3]) >= 4)
    up, us = run(want=upper)
    assert set(up) == set(upper) and us["lowest_layer"] == 4 and ts["launches"] < us["launches"] < fs["launches"]
    assert_parity("subset/lin4_and_up", up, t32, {k: ref64[k] for k in upper})          # the skip layer's gradient among them
    biases = tuple(k for k in cto.NAMES if k.endswith(".bias"))
    bs, bst = run(want=biases)
    assert set(bs) == set(biases) and bst["lowest_layer"] == 0
    for sub in (top, up, bs):
        for k, v in sub.items():
            assert torch.equal(v, full[k]), k          # the same association whatever else is wanted
    # NULL entries leave their tensors untouched: through the module, frozen parameters keep .grad = None and the data path stops at lin4
    from robir_amd import training
    net = training.enable_cesr_training(_net(dev, "shadow", _weights("shadow", "init")))
    net._train_slab_rows, net._train_part_rows = 64, 48
    for name, p in net.named_parameters():
        p.requires_grad_(name in upper)
    with torch.enable_grad():
        (net.diffuse_vis(pts.to(dev), 8) * g[1].to(dev)).sum().backward()
    for name, p in net.named_parameters():
        assert (p.grad is not None) == (name in upper), name
        if name in upper:
            assert torch.equal(p.grad.cpu(), full[name]), name


# ------------------------------------------------------------------------------------------------ 4. weight norm
def test_weight_norm_scaling_and_orthogonality(dev):
    """weight_v of lin2 times 3: W = g v / |v| is unchanged (up to the fp32 rounding of 3 v), so the outputs agree under the forward's tolerance
    (1e-4, what tests/test_cesr_gpu.py asserts of the forward under every policy), the weight_v gradient is a third (the yardstick, against the float64 oracle on the scaled weights), the others are
    unchanged.  <dv, v> = 0 per output row: max over the rows of |<dv, v>| / (|dv| |v|), evaluated in float64, is held to 10 x the float64
    oracle's own value.  The kernel stores fp32, so the oracle's value is measured on its gradient in that storage format (rounded to fp32
    once, which is what an exact kernel returns); the unrounded float64 figure (~1e-17) is recorded next to it."""
    from robir_amd import training
    kind = "normal"
    sd = _weights(kind, "perturbed")
    sd3 = {k: (v * 3 if k == "lin2.weight_v" else v.clone()) for k, v in sd.items()}
    pts, g = _inputs(kind, 200, 1, 4)
    a, _ = _kernel(dev, kind, cto.cesr_params(sd), pts, g[0], 0, slab_rows=64, part_rows=48)
    b, _ = _kernel(dev, kind, cto.cesr_params(sd3), pts, g[0], 0, slab_rows=64, part_rows=48)
    ref64, t32 = _truth(("wn3",), cto.cesr_params(sd3), pts, kind, g[0], 1, 0)
    assert_parity("weight_norm/v_times_3", b, t32, ref64)
    assert_parity("weight_norm/third", {"lin2.weight_v": a["lin2.weight_v"] / 3}, {"lin2.weight_v": t32["lin2.weight_v"]},
                  {"lin2.weight_v": ref64["lin2.weight_v"]})
    ya, yb = (_net(dev, kind, s, train=False)._cesr_points(pts.to(dev), 200, 0).cpu() for s in (sd, sd3))
    assert rel_err(ya, yb) <= 1e-4
    ortho = lambda dv, v: float(((dv.double() * v.double()).sum(1).abs() / (dv.double().norm(dim=1) * v.double().norm(dim=1))).max())
    worst_k = worst_o = worst_o64 = 0.0
    for l in range(9):
        k = f"lin{l}.weight_v"
        worst_k = max(worst_k, ortho(b[k], sd3[k]))
        worst_o = max(worst_o, ortho(ref64[k].float(), sd3[k]))
        worst_o64 = max(worst_o64, ortho(ref64[k], sd3[k]))
    record_metric("cesr_train/weight_norm/orthogonality", kernel=worst_k, oracle64_stored_fp32=worst_o, oracle64=worst_o64)
    print(f"<dv, v> / (|dv| |v|): kernel {worst_k:.2e}, float64 oracle rounded to fp32 {worst_o:.2e}, float64 oracle {worst_o64:.2e}")
    assert worst_k <= 10 * worst_o, (worst_k, worst_o, worst_o64)


# ------------------------------------------------------------------------------------------------ 5. determinism
def test_determinism_and_other_partitions(dev):
    params = cto.cesr_params(_weights("shadow", "perturbed"))
    pts, g = _inputs("shadow", 25, 8, 258)
    ref64, t32 = _truth(("shadow", "perturbed", 25, 8, 1), params, pts, "shadow", g[1], 8, 1)
    a, _ = _kernel(dev, "shadow", params, pts, g[1], 1, n_label=8, slab_rows=64, part_rows=48)
    b, _ = _kernel(dev, "shadow", params, pts, g[1], 1, n_label=8, slab_rows=64, part_rows=48)
    assert all(torch.equal(a[k], b[k]) for k in cto.NAMES)
    c, cs = _kernel(dev, "shadow", params, pts, g[1], 1, n_label=8, slab_rows=128, part_rows=32)
    assert cs["partitions"] == 4
    assert_parity("determinism/other_partition", c, t32, ref64)


# ------------------------------------------------------------------------------------------------ 6. the reference fixture
@pytest.mark.parametrize("kind", ["shadow", "normal"])
def test_reference_fixture(dev, kind):
    """Autograd through the marked module (the dense-rows forward) on the fixture's inputs against the REFERENCE's float64 gradients, every
    stored piece under the yardstick; e_torch: fp32 autograd of the oracle on the same rows."""
    from robir_amd import training
    gold = load_golden("cesr_grad" if kind == "shadow" else "cesr_grad_normal")
    sd = _weights(kind, "init")
    net = training.enable_cesr_training(_net(dev, kind, sd))
    rows, g = torch.from_numpy(gold[kind + ".rows"]), torch.from_numpy(gold[kind + ".g_out"])
    with torch.enable_grad():
        (net(rows.to(dev)) * g.to(dev)).sum().backward()
    got = {k: p.grad.cpu() for k, p in net.named_parameters()}
    t32 = cto.grads(cto.cesr_params(sd), rows, kind, g, torch.float32)
    pieces = lambda k, t: ({"full": t} if not k.endswith("weight_v") else {"rows8": t[:8], "cols8": t[:, :8], "sum": t.sum(), "fro": t.norm()})
    K, T, R = {}, {}, {}
    for k in cto.NAMES:
        for part, v in pieces(k, got[k].double()).items():
            K[f"{k}.{part}"], T[f"{k}.{part}"] = v, pieces(k, t32[k].double())[part]
            R[f"{k}.{part}"] = torch.from_numpy(np.asarray(gold[f"{kind}.grad.{k}.{part}"]))
    assert_parity(f"fixture/{kind}", K, T, R)


# ------------------------------------------------------------------------------------------------ 7. the stage step through CESRHook
@pytest.fixture(scope="module")
def scene(dev):
    from robir_amd import renderer, synth
    m = renderer.build_synthetic_model(dev, seed=0, variance=0.3).eval()
    uv, pose, K = synth.synth_camera(64, 64)
    sl = slice(1024, 1280)          # 256 pixels of the middle rows: ~150 hit points x 128 labels through shadow_net
    inp = {"uv": torch.from_numpy(uv[sl]).to(dev)[None], "pose": torch.from_numpy(pose).to(dev)[None], "intrinsics": torch.from_numpy(K).to(dev)[None],
           "object_mask": torch.ones(1, 256, dtype=torch.bool, device=dev), "hdr_shift": torch.full((256, 1), 0.5, device=dev)}
    return m, inp


def test_stage_step_through_the_hook(dev, scene):
    from robir_amd import deferred, ops, renderer, synth, training
    from robir_amd.cesr_autograd import cesr_params
    m, inp = scene
    shadow = training.enable_cesr_training(_net(dev, "shadow", _weights("shadow", "init")))
    normal = training.enable_cesr_training(_net(dev, "normal", _weights("normal", "init")))
    m.get_sg_render = renderer.CESRHook(m, shadow, normal, is_training=True, cur_iter=2000, prefit="explore")
    try:
        m.eval()
        out0 = m(inp, trainstage="Material", lin_diff=True, train_spec=True)          # conftest's no_grad: forward-only, may be recorded
        hit = deferred.plain(out0["network_object_mask"]).clone()
        n_hit = int(hit.sum())
        assert 16 <= n_hit <= 256
        draws = {k: torch.from_numpy(v).to(dev) for k, v in synth.pbr_draws(0, n_hit, chunk_id=1, nsamp_diffuse=8).items()}
        target = (deferred.plain(out0["sg_rgb"])[hit] * 0.7 + 0.05).clone()
        run = lambda: m(inp, trainstage="Material", lin_diff=True, train_spec=True, draws=draws)

        def loss_of(out):
            return (out["sg_rgb"][hit] - target).abs().mean() + out["gradient_error"]
        # pass 1: the whole step; the hook's diffuse_vis is captured on its way
        seen = {}
        real_dv = shadow.diffuse_vis

        def capture(x, n_label=128):
            seen["x"], seen["dv"] = x, real_dv(x, n_label)
            return seen["dv"]
        shadow.diffuse_vis = capture
        with torch.enable_grad():
            out = run()
            assert not isinstance(out, deferred.ChunkOutputs) and m.__dict__.get("_pending") is None
            assert out["sg_rgb"].grad_fn is not None and out["gradient_error"].grad_fn is not None and out["normal_map"].grad_fn is not None
            loss = loss_of(out)
            loss.backward()
        loss1 = float(loss)
        g_shadow = {k: p.grad.clone() for k, p in shadow.named_parameters()}
        g_normal = {k: p.grad.cpu() for k, p in normal.named_parameters()}
        assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in list(g_shadow.values()) + list(g_normal.values()))
        # pass 2: the same step on a LEAF diffuse_vis of the same values -> the gradient the shading (and the KL term) returns on it ...
        leaf = seen["dv"].detach().clone().requires_grad_(True)
        shadow.diffuse_vis = lambda x, n_label=128: leaf
        with torch.enable_grad():
            loss_of(run()).backward()
        # ... fed to ops.cesr_backward: shadow_net's gradients, bit for bit
        x = seen["x"] if seen["x"].shape[1] == 3 else seen["x"][:, :3].contiguous()
        assert x.shape[0] == n_hit and leaf.grad is not None and float(leaf.grad.abs().max()) > 0
        direct, stats = ops.cesr_backward(x, n_hit * 128, "shadow", cesr_params(shadow), leaf.grad, head=1, n_label=128)
        assert stats["lowest_layer"] == 0
        for k in cto.NAMES:
            assert torch.equal(direct[k], g_shadow[k]), k
        shadow.diffuse_vis = real_dv
        # normal_net: only the consistency term ((normal_map - normal_new)^2).mean() reaches it (the shading takes normal_new detached)
        hp = out["points"][hit].detach().contiguous()
        nm = m.envmap_material_network(hp, train_spec=True, noise={"spec": draws["spec_randn"], "normal": draws["normal_randn"]})["sg_normal_map"].cpu()
        fn = lambda lv: ((nm.to(cto._dtype(lv)) - cto.forward(lv, hp.cpu(), "normal", 1, 2)) ** 2).mean()
        params_n = cto.cesr_params(_weights("normal", "init"))
        n64, n32 = (cto.grads_of(fn, params_n, dt)[1] for dt in (torch.float64, torch.float32))
        assert_parity("stage/normal_net", g_normal, n32, n64)
        # a few Adam steps lower the loss; the next forward sees the new weights
        before = m(inp, trainstage="Material", lin_diff=True, train_spec=True, draws=draws)["normal_map"][hit].clone()
        opt = torch.optim.Adam(list(shadow.parameters()) + list(normal.parameters()), lr=1e-4)
        losses = [loss1]
        for _ in range(4):
            opt.step()
            opt.zero_grad(set_to_none=True)
            with torch.enable_grad():
                loss = loss_of(run())
                loss.backward()
            losses.append(float(loss))
        record_metric("cesr_train/stage/losses", first=losses[0], last=losses[-1])
        print("stage losses", ["%.5f" % v for v in losses])
        assert losses[-1] < losses[0], losses
        after = m(inp, trainstage="Material", lin_diff=True, train_spec=True, draws=draws)["normal_map"][hit]
        assert not torch.equal(before, after)
        # without pinned draws: a chunk forward of a hook with a trainable net is never recorded; forward-only, it is
        with torch.enable_grad():
            live = m(inp, trainstage="Material", lin_diff=True, train_spec=True)
            assert not isinstance(live, deferred.ChunkOutputs) and m.__dict__.get("_pending") is None and live["gradient_error"].grad_fn is not None
        rec = m(inp, trainstage="Material", lin_diff=True, train_spec=True)
        assert isinstance(rec, deferred.ChunkOutputs)
        m.flush()
    finally:
        m.flush()
        del m.get_sg_render


# ------------------------------------------------------------------------------------------------ 8. refusals and lifetime
def test_inputs_that_require_grad_are_refused(dev):
    from robir_amd import training
    shadow = training.enable_cesr_training(_net(dev, "shadow", _weights("shadow", "init")))
    normal = training.enable_cesr_training(_net(dev, "normal", _weights("normal", "init")))
    pts = torch.zeros(4, 3, device=dev)
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match="points"):
            shadow.eval_point_labels(pts.clone().requires_grad_(), 8)
        with pytest.raises(NotImplementedError, match="points"):
            normal.unit_normal(pts.clone().requires_grad_())
        with pytest.raises(NotImplementedError, match="rows"):
            normal(torch.zeros(4, 63, device=dev, requires_grad=True))
        with pytest.raises(NotImplementedError, match="rows"):
            shadow(torch.zeros(4, 191, device=dev, requires_grad=True))
    assert all(p.grad is None for p in list(shadow.parameters()) + list(normal.parameters()))


def test_graph_is_freed_by_reference_counting(dev):
    """Only save_for_backward holds tensors: once the output and the loss are dropped -- with or without a backward() -- the weakrefs are dead
    and the allocation (graph, gradients' scratch) returns to its base with the cyclic collector disabled."""
    from robir_amd import training
    net = training.enable_cesr_training(_net(dev, "shadow", _weights("shadow", "init")))
    net._train_slab_rows, net._train_part_rows = 256, 64
    pts = (_inputs("shadow", 16, 1, 8)[0]).to(dev)
    net.diffuse_vis(pts, 128)                 # packed blobs exist before the base is read
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        for run_backward in (False, True):
            net.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            with torch.enable_grad():
                y = net.diffuse_vis(pts, 128)
                loss = y.square().mean()
                refs = [weakref.ref(y), weakref.ref(loss)]
                assert torch.cuda.memory_allocated() > base
                if run_backward:
                    loss.backward()
            del y, loss
            assert all(r() is None for r in refs)
            net.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            assert torch.cuda.memory_allocated() == base, (run_backward, torch.cuda.memory_allocated() - base)
    finally:
        if was:
            gc.enable()
