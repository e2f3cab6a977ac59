"""Trainable visibility on the GPU: rb_vt_vis_bwd (librobir_hip_vistrain.so), robir_amd/vis_autograd.py and robir_amd/training.py.

The truth is float64 autograd of the oracle's formulas (robir_oracle.nets.vis_logits through tests/vis_train_oracle.py) on the CPU, fed the
same fp32 coordinates the kernels saw; tests/golden/vis_grad.npz (tools/gen_vis_grad_golden.py) pins that oracle on the REFERENCE's own
VisNetwork.  The yardstick is test_sg_backward_gpu's rule: for every gradient tensor `e_kernel <= max(2 e_torch, 1e-5)`, e = conftest.rel_err
against float64, e_torch what PyTorch's fp32 autograd of the same formulas achieves on the same inputs.  Every pair is recorded.  conftest
wraps every test in no_grad: the tests enter torch.enable_grad() themselves."""
import gc
import weakref

import numpy as np
import pytest
import torch

import vis_train_oracle as vto
from conftest import record_metric, rel_err, load_golden

pytestmark = pytest.mark.gpu
FLOOR = 1e-5
VIS = vto.PREFIX
CE = torch.nn.CrossEntropyLoss()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _weights(synth_weights, which):
    """"init": the synthetic weights; "perturbed": + 0.02 N(0,1) on every matrix, so that no layer is near its initial structure."""
    sd = {k: torch.as_tensor(v).clone() for k, v in synth_weights.items() if k.startswith(VIS)}
    if which == "perturbed":
        g = torch.Generator().manual_seed(77)
        for k in sd:
            if sd[k].dim() == 2:
                sd[k] = sd[k] + 0.02 * torch.randn(sd[k].shape, generator=g)
    return sd


def _vis_net(dev, sd, train=True):
    from robir_amd import nets
    net = nets.VisNetwork(points_multires=10, dirs_multires=10, dims=[256] * 4)
    net.load_state_dict({k[len(VIS):]: torch.as_tensor(v) for k, v in sd.items() if k.startswith(VIS)})
    net = net.to(dev)
    return net.train() if train else net.eval()


def assert_parity(tag, kernel, torch32, ref64, err=None):
    bad = []
    for k, r in ref64.items():
        r = torch.as_tensor(r)
        e = (err or {}).get(k, rel_err)
        e_kernel = e(torch.as_tensor(kernel[k]).reshape(r.shape), r)
        e_torch = e(torch.as_tensor(torch32[k]).reshape(r.shape), r)
        record_metric(f"vis_train/{tag}/{k}", e_kernel=e_kernel, e_torch=e_torch, max_abs_ref=float(r.abs().max()))
        print(f"{tag:44s} d {k:30s} e_kernel {e_kernel:.2e}  e_torch {e_torch:.2e}")
        if not e_kernel <= max(2.0 * e_torch, FLOOR):
            bad.append((k, e_kernel, e_torch))
    assert not bad, (tag, bad)


def _inputs(M, rep, seed=0):
    g = torch.Generator().manual_seed(300 + seed)
    pts = torch.randn(M // rep, 3, generator=g) * 0.5
    dirs = torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=-1)
    return pts, dirs, torch.randn(M, 2, generator=g)


def _kernel(dev, params, pts, dirs, rep, g_logits, **kw):
    """ops.vis_backward on device copies -> (dict of CPU gradients, stats)."""
    from robir_amd import ops
    D = lambda t: torch.as_tensor(t).float().to(dev).contiguous()
    out, stats = ops.vis_backward(D(pts), D(dirs), rep, [D(params[k]) for k in vto.NAMES], D(g_logits), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}, stats


_REF = {}


def _truth(key, params, pts, dirs, rep, g_logits):
    """(float64 gradients, fp32 gradients) of the oracle, computed once per case and shared."""
    if key not in _REF:
        _REF[key] = (vto.vis_grads(params, pts, dirs, g_logits, rep, torch.float64), vto.vis_grads(params, pts, dirs, g_logits, rep, torch.float32))
    return _REF[key]


# ------------------------------------------------------------------------------------------------ 1. fails without the feature
def test_marked_network_trains(dev, synth_weights):
    from robir_amd import nets, training
    net = _vis_net(dev, _weights(synth_weights, "init"))
    pts, dirs, g = _inputs(64, 4)
    pts, dirs, g = pts.to(dev), dirs.to(dev), g.to(dev)
    with torch.enable_grad():
        with pytest.raises(nets.ForwardOnlyError):
            net.logits_from_points(pts, dirs, 4)
        assert training.enable_visibility_training(net) is net
        y = net.logits_from_points(pts, dirs, 4)
        y1 = net(pts.repeat_interleave(4, 0), dirs)
        assert y.grad_fn is not None and y1.grad_fn is not None and tuple(y.shape) == (64, 2)
        ((y * g).sum() + (y1 * g).sum()).backward()
    for name, p in net.named_parameters():
        assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape), name
        assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
    # the values of the trainable path are the forward-only path's, bit for bit (conftest's no_grad is active here; unmarked as well)
    training.enable_visibility_training(net, on=False)
    ref = net.logits_from_points(pts, dirs, 4)
    assert not ref.requires_grad and torch.equal(y.detach(), ref)
    assert torch.equal(y1.detach(), net(pts.repeat_interleave(4, 0), dirs))
    with torch.enable_grad():
        with pytest.raises(nets.ForwardOnlyError):
            net(pts.repeat_interleave(4, 0), dirs)


# ------------------------------------------------------------------------------------------------ 2. kernel-level parity
CASES = [(1, 1, 64, 64), (15, 1, 64, 16), (17, 1, 64, 16), (65, 1, 64, 64), (200, 8, 64, 48), (4144, 16, 1024, 80)]


@pytest.mark.parametrize("weights", ["init", "perturbed"])
@pytest.mark.parametrize("M,rep,slab,part", CASES)
def test_kernel_parity(dev, synth_weights, weights, M, rep, slab, part):
    """(1,1,64,64), (15,1,64,16), (17,1,64,16): the 16-row MFMA tile edge; (65,1,64,64): a second slab of one row; (200,8,64,48): points
    changing inside partitions, a ragged last partition, a ragged last slab of 8 rows; (4144,16,1024,80): five slabs, 13 partitions of
    which the last is ragged.  A random normal upstream gradient on the logits; all ten gradients compared."""
    params = vto.vis_params(_weights(synth_weights, weights))
    pts, dirs, g = _inputs(M, rep, seed=M)
    ref64, t32 = _truth((weights, M), params, pts, dirs, rep, g)
    kernel, stats = _kernel(dev, params, pts, dirs, rep, g, slab_rows=slab, part_rows=part)
    assert set(kernel) == set(vto.NAMES) and stats["lowest_layer"] == 0
    assert stats["partitions"] == -(-min(M, slab) // part) and stats["scratch_bytes"] > 0
    assert tuple(kernel["vis_layer.0.weight"].shape) == (256, 126) and tuple(kernel["vis_layer.8.weight"].shape) == (2, 256)
    assert_parity(f"kernel/{weights}/M{M}_rep{rep}_slab{slab}_part{part}", kernel, t32, ref64)


# ------------------------------------------------------------------------------------------------ 3. gradient subsets
def test_subsets_stop_the_data_path(dev, synth_weights):
    params = vto.vis_params(_weights(synth_weights, "init"))
    pts, dirs, g = _inputs(200, 8, seed=200)
    kw = dict(slab_rows=64, part_rows=48)
    full, fs = _kernel(dev, params, pts, dirs, 8, g, **kw)
    last = ("vis_layer.8.weight", "vis_layer.8.bias")
    part, ps = _kernel(dev, params, pts, dirs, 8, g, want=last, **kw)
    assert set(part) == set(last) and ps["lowest_layer"] == 4 and fs["lowest_layer"] == 0 and ps["launches"] < fs["launches"]
    biases = tuple(k for k in vto.NAMES if k.endswith(".bias"))
    bs, bst = _kernel(dev, params, pts, dirs, 8, g, want=biases, **kw)
    assert set(bs) == set(biases) and bst["lowest_layer"] == 0
    first = ("vis_layer.0.weight", "vis_layer.0.bias")
    l0, l0s = _kernel(dev, params, pts, dirs, 8, g, want=first, **kw)
    assert set(l0) == set(first) and l0s["lowest_layer"] == 0 and l0s["launches"] < fs["launches"]
    mid, ms = _kernel(dev, params, pts, dirs, 8, g, want=("vis_layer.4.bias",), **kw)
    assert ms["lowest_layer"] == 2
    for sub in (part, bs, l0, mid):
        for k, v in sub.items():
            assert torch.equal(v, full[k]), k
    none, ns = _kernel(dev, params, pts, dirs, 8, g, want=(), **kw)
    assert none == {} and ns["launches"] == 0 and ns["lowest_layer"] == 5
    # an upstream gradient with one zero column
    gz = g.clone()
    gz[:, 0] = 0
    ref64, t32 = _truth(("zero_column", 200), params, pts, dirs, 8, gz)
    kz, _ = _kernel(dev, params, pts, dirs, 8, gz, **kw)
    assert float(kz["vis_layer.8.weight"][0].abs().max()) == 0 and float(kz["vis_layer.8.bias"][0]) == 0
    assert_parity("kernel/zero_column", kz, t32, ref64)
    # through autograd: frozen parameters turn into NULL pointers
    from robir_amd import training
    net = training.enable_visibility_training(_vis_net(dev, _weights(synth_weights, "init")))
    net._train_slab_rows, net._train_part_rows = 64, 48
    for name, p in net.named_parameters():
        p.requires_grad_(name.startswith("vis_layer.8."))
    with torch.enable_grad():
        (net.logits_from_points(pts.to(dev), dirs.to(dev), 8) * g.to(dev)).sum().backward()
    for name, p in net.named_parameters():
        assert (p.grad is not None) == name.startswith("vis_layer.8."), name
        if p.grad is not None:
            assert torch.equal(p.grad.cpu(), full[name]), name


# ------------------------------------------------------------------------------------------------ 4. the reference fixture
def _sum_err(fro):
    """The error of a `sum` piece whose float64 truth is the rounding residue of an exact zero (the two rows of the last layer's weight
    gradient cancel under a cross-entropy loss: softmax - onehot sums to zero over the classes, the fixture holds 1.6e-15): rel_err's
    denominator |b| + mean |b| is that residue itself there, so the distance is taken relative to the tensor's Frobenius norm instead."""
    return lambda a, b: float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs() / fro)


def test_autograd_against_the_reference_fixture(dev, synth_weights):
    """tests/golden/vis_grad.npz: the REFERENCE's VisNetwork differentiated in float64 on 32 rows under nn.CrossEntropyLoss; the oracle's
    recorded distance from it is <= 1e-10 and VisLogitsFn + nn.CrossEntropyLoss holds the rule against every stored piece."""
    from robir_amd import training
    fx = load_golden("vis_grad")
    sd = _weights(synth_weights, "init")
    params = vto.vis_params(sd)
    pts, dirs, labels, rep = torch.from_numpy(fx["points"]), torch.from_numpy(fx["dirs"]), torch.from_numpy(fx["labels"]), int(fx["rep"])
    net = training.enable_visibility_training(_vis_net(dev, sd))
    with torch.enable_grad():
        loss = CE(net.logits_from_points(pts.to(dev), dirs.to(dev), rep), labels.to(dev))
        loss.backward()
    kernel = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    l32, t32 = vto.loss_grads(params, pts, dirs, lambda y: CE(y, labels), rep=rep, dtype=torch.float32)
    record_metric("vis_train/reference_fixture/loss", hip=float(loss), torch32=l32, reference64=float(fx["loss"]))
    assert abs(float(loss) - float(fx["loss"])) <= 1e-4 * float(fx["loss"])          # the forward kernel's own parity bound

    def pieces(g, k):
        if g.dim() == 1:
            return {f"{k}.full": g}
        return {f"{k}.rows8": g[:8], f"{k}.cols8": g[:, :8], f"{k}.sum": g.double().sum(), f"{k}.fro": g.double().norm()}
    K, T, R, err = {}, {}, {}, {}
    for k in vto.NAMES:
        K.update(pieces(kernel[k], k))
        T.update(pieces(t32[k], k))
    for key in K:
        assert float(fx["oracle_dist." + key]) <= 1e-10, key
        R[key] = torch.from_numpy(np.asarray(fx["grad." + key]))
        if key.endswith(".sum") and abs(float(R[key])) <= 1e-12 * float(fx["grad." + key[:-4] + ".fro"]):
            err[key] = _sum_err(float(fx["grad." + key[:-4] + ".fro"]))
    assert set(err) == {"vis_layer.8.weight.sum"}
    assert_parity("reference_fixture", K, T, R, err)


# ------------------------------------------------------------------------------------------------ 5. determinism
def test_determinism_and_partition_independence(dev, synth_weights):
    params = vto.vis_params(_weights(synth_weights, "perturbed"))
    pts, dirs, g = _inputs(4144, 16, seed=4144)
    runs = [_kernel(dev, params, pts, dirs, 16, g, slab_rows=1024, part_rows=80)[0] for _ in range(3)]
    for k in vto.NAMES:
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], runs[2][k]), k
    ref64, t32 = _truth(("perturbed", 4144), params, pts, dirs, 16, g)
    for slab, part in ((1024, 1024), (1024, 16), (4144, 80), (512, 80)):
        other, st = _kernel(dev, params, pts, dirs, 16, g, slab_rows=slab, part_rows=part)
        assert st["partitions"] == -(-min(4144, slab) // part)
        assert_parity(f"kernel/perturbed/M4144_slab{slab}_part{part}", other, t32, ref64)
    default, st = _kernel(dev, params, pts, dirs, 16, g)
    assert st["partitions"] == 5          # min(M, 16384) = 4144 rows in partitions of 1024
    assert_parity("kernel/perturbed/M4144_default", default, t32, ref64)


def test_more_partitions_than_one_launch_holds(dev, synth_weights):
    """One slab of 4100 one-row partitions: more than the 4096 that one weight-gradient launch takes (Z_GROUP of csrc/train/chain.h), so
    every layer's weight gradient is two launches, 4096 + 4 partitions, the second with part0 = 4096.  Launches: 1 encode + 4 forward +
    5 x (2 weight-gradient + 1 reduce) + 4 data-gradient + 5 finish = 29; at part_rows = 80 (52 partitions, one launch each) 24.  The
    partials are 4100 x 256 x 257 doubles: 2.2 GB of scratch."""
    params = vto.vis_params(_weights(synth_weights, "perturbed"))
    pts, dirs, g = _inputs(4100, 4, seed=4100)
    ref64, t32 = _truth(("perturbed", 4100), params, pts, dirs, 4, g)
    kw = dict(slab_rows=4100, part_rows=1)
    full, stats = _kernel(dev, params, pts, dirs, 4, g, **kw)
    assert stats["partitions"] == 4100 and stats["launches"] == 29 and stats["lowest_layer"] == 0
    assert _kernel(dev, params, pts, dirs, 4, g, slab_rows=4100, part_rows=80)[1]["launches"] == 24
    assert set(full) == set(vto.NAMES)
    assert_parity("kernel/perturbed/M4100_slab4100_part1", full, t32, ref64)
    last = ("vis_layer.8.weight", "vis_layer.8.bias")
    sub, ss = _kernel(dev, params, pts, dirs, 4, g, want=last, **kw)
    assert set(sub) == set(last) and ss["lowest_layer"] == 4 and ss["partitions"] == 4100
    for k in last:
        assert torch.equal(sub[k], full[k]), k


# ------------------------------------------------------------------------------------------------ 6. trace_radiance
@pytest.fixture(scope="module")
def model(dev):
    from robir_amd import renderer
    m = renderer.build_synthetic_model(dev, seed=0, variance=0.3)
    m.eval()
    return m


def _chunk_input(dev):
    from robir_amd import synth
    uv, pose, K = synth.synth_camera(64, 64)
    return {"uv": torch.from_numpy(uv[1024:2048]).to(dev)[None], "pose": torch.from_numpy(pose).to(dev)[None],
            "intrinsics": torch.from_numpy(K).to(dev)[None], "object_mask": torch.ones(1, 1024, dtype=torch.bool, device=dev),
            "hdr_shift": torch.full((1024, 1), 0.5, device=dev)}


@pytest.fixture(scope="module")
def traced(dev, model):
    """One 'Illum' chunk of the 64 x 64 synthetic view and its secondary rays with pinned draws (nsamp 4), everything in eval() / no_grad:
    the fixed batch of traced labels that tests 6-8 share.  Left unchanged."""
    NS = 4
    model.deferred_chunks = 0
    try:
        with torch.no_grad():
            out = model(_chunk_input(dev), trainstage="Illum")
            fwd = {k: out[k].detach().clone() for k in ("points", "hdr_shift", "network_object_mask", "normals")}
            n = int(fwd["network_object_mask"].sum())
            g = torch.Generator().manual_seed(21)
            draws = (torch.rand(n * NS, generator=g), torch.rand(n * NS, generator=g))
            tr = model.trace_radiance(fwd, nsamp=NS, draws=draws)
    finally:
        model.__dict__.pop("deferred_chunks", None)
    mask = fwd["network_object_mask"]
    idx = mask.nonzero()[:, 0]
    return {"fwd": fwd, "draws": draws, "nsamp": NS, "n": n, "mask": mask, "points": fwd["points"][idx].cpu(),
            "dirs": tr["sample_dirs"].reshape(-1, 3).cpu(), "labels": (~tr["gt_vis"][idx]).long().reshape(-1).cpu(),
            "pred_vis": tr["pred_vis"].clone(), "gt_vis": tr["gt_vis"].clone()}


def test_trace_radiance_pred_vis_trains(dev, model, traced, synth_weights):
    from robir_amd import deferred, training
    vis = model.visibility_network
    NS, n = traced["nsamp"], traced["n"]
    assert 100 <= n <= 1024 and 0 < int(traced["labels"].sum()) < n * NS
    try:
        vis.train()
        training.enable_visibility_training(model)
        with torch.enable_grad():
            tr = model.trace_radiance(traced["fwd"], nsamp=NS, draws=traced["draws"])
            assert tr["pred_vis"].requires_grad and torch.equal(tr["pred_vis"].detach(), traced["pred_vis"])
            assert torch.equal(tr["gt_vis"], traced["gt_vis"])
            loss = training.visibility_loss(tr["pred_vis"], tr["gt_vis"], traced["mask"])
            loss.backward()
        kernel = {k: p.grad.detach().cpu() for k, p in vis.named_parameters()}
        for name, p in model.named_parameters():
            assert (p.grad is not None) == name.startswith("visibility_network."), name
        params = vto.vis_params(_weights(synth_weights, "init"))
        fn = lambda y: CE(y, traced["labels"])
        l64, ref64 = vto.loss_grads(params, traced["points"], traced["dirs"], fn, rep=NS, dtype=torch.float64)
        l32, t32 = vto.loss_grads(params, traced["points"], traced["dirs"], fn, rep=NS, dtype=torch.float32)
        record_metric("vis_train/trace_radiance/loss", hip=float(loss), oracle64=l64, torch32=l32)
        assert abs(float(loss) - l64) <= 1e-4 * l64          # the forward kernel's own parity bound
        assert_parity("trace_radiance", kernel, t32, ref64)
        # a recorded chunk forward: with the mark the trace runs at once and carries a graph ...
        vis.zero_grad(set_to_none=True)
        model.deferred_chunks = 4
        out = model(_chunk_input(dev), trainstage="Illum")            # no_grad (conftest), model in eval(): recorded
        assert isinstance(out, deferred.ChunkOutputs) and out._q.result is None
        with torch.enable_grad():
            tr = model.trace_radiance(out, nsamp=NS)
        assert not isinstance(tr, deferred.TraceOutputs) and out._q.result is not None
        assert isinstance(tr["pred_vis"], torch.Tensor) and tr["pred_vis"].requires_grad and tr["pred_vis"].grad_fn is not None
        with torch.enable_grad():
            training.visibility_loss(tr["pred_vis"], tr["gt_vis"], out["network_object_mask"]).backward()
        assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in vis.parameters())
        # ... unmarked, the recorded path is still taken
        training.enable_visibility_training(model, on=False)
        vis.eval()
        out = model(_chunk_input(dev), trainstage="Illum")
        assert isinstance(out, deferred.ChunkOutputs) and out._q.result is None
        tr = model.trace_radiance(out, nsamp=NS)
        assert isinstance(tr, deferred.TraceOutputs) and out._q.result is None
        assert tuple(tr["pred_vis"].shape) == (1024, NS, 2)
    finally:
        training.enable_visibility_training(model, on=False)
        model.flush()
        model.__dict__.pop("deferred_chunks", None)
        model.zero_grad(set_to_none=True)
        model.eval()


# ------------------------------------------------------------------------------------------------ 7. a fit   8. the weight cache
def test_fit_descends_and_the_weight_cache_follows_the_optimiser(dev, model, traced, synth_weights):
    """30 Adam steps at the stage's lr = 5e-4 on one fixed batch of traced labels (128 surface points x 4 directions): the loss after the
    last step is below the first, the trajectory is recorded beside the float64 oracle's.  One SGD step's parameters match the oracle's step
    under the rule.  After an optimiser step the fused light-visibility kernel on a 16-point chunk and the no_grad logits equal those of a
    freshly built network loaded with the stepped state dict, bit for bit: every packed blob follows optimizer.step()."""
    from robir_amd import sg_render, training
    NS, P, steps = traced["nsamp"], 128, 30
    pts, dirs, labels = traced["points"][:P], traced["dirs"][:P * NS], traced["labels"][:P * NS]
    sd = _weights(synth_weights, "init")
    params = vto.vis_params(sd)
    fn = lambda y: CE(y, labels)
    pd, dd, ld = pts.to(dev), dirs.to(dev), labels.to(dev)

    # one SGD step
    net = training.enable_visibility_training(_vis_net(dev, sd))
    sgd = torch.optim.SGD(net.parameters(), lr=0.1)
    with torch.enable_grad():
        CE(net.logits_from_points(pd, dd, NS), ld).backward()
    sgd.step()
    stepped = {k: p.detach().cpu() for k, p in net.named_parameters()}

    def oracle_step(dtype):
        lv = vto.leaves(params, dtype)
        o = torch.optim.SGD(list(lv.values()), lr=0.1)
        with torch.enable_grad():
            fn(vto.vis_forward(lv, pts, dirs, NS)).backward()
        o.step()
        return {k: v.detach() for k, v in lv.items()}
    assert_parity("fit/sgd_step", stepped, oracle_step(torch.float32), oracle_step(torch.float64))

    # 8. the consumers of the weights see the step
    fresh = _vis_net(dev, {VIS + k: v for k, v in net.state_dict().items()}, train=False)
    lgt = torch.as_tensor(synth_weights["envmap_material_network.lgtSGs"]).to(dev)
    lobes, lambdas = torch.nn.functional.normalize(lgt[:, :3], dim=-1), lgt[:, 3:4].abs()
    g = torch.Generator().manual_seed(5)
    dr = {"dvis_theta": torch.rand(lgt.shape[0], 8, generator=g).to(dev), "dvis_phi": torch.rand(lgt.shape[0], 8, generator=g).to(dev)}
    idx = traced["mask"].nonzero()[:16, 0]
    p16, n16 = traced["fwd"]["points"][idx].contiguous(), traced["fwd"]["normals"][idx].contiguous()
    a = sg_render.get_diffuse_visibility(p16, n16, net, lobes, lambdas, nsamp=8, draws=dr)
    b = sg_render.get_diffuse_visibility(p16, n16, fresh, lobes, lambdas, nsamp=8, draws=dr)
    assert tuple(a.shape) == (lgt.shape[0], 16) and torch.equal(a, b) and float(a.min()) < float(a.max())
    assert torch.equal(net.logits_from_points(pd, dd, NS), fresh.logits_from_points(pd, dd, NS))           # no_grad (conftest)
    before = _vis_net(dev, sd, train=False)
    assert not torch.equal(net.logits_from_points(pd, dd, NS), before.logits_from_points(pd, dd, NS))

    # 7. the fit
    net = training.enable_visibility_training(_vis_net(dev, sd))
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    losses = []
    for _ in range(steps + 1):
        with torch.enable_grad():
            opt.zero_grad()
            loss = CE(net.logits_from_points(pd, dd, NS), ld)
            loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
    lv = vto.leaves(params, torch.float64)
    o = torch.optim.Adam(list(lv.values()), lr=5e-4)
    l64 = []
    for _ in range(steps + 1):
        with torch.enable_grad():
            o.zero_grad()
            loss = fn(vto.vis_forward(lv, pts, dirs, NS))
            loss.backward()
        l64.append(float(loss.detach()))
        o.step()
    record_metric("vis_train/fit", **{f"hip_{i}": v for i, v in enumerate(losses)}, **{f"oracle64_{i}": v for i, v in enumerate(l64)})
    print("visibility fit  HIP     ", " ".join(f"{v:.4e}" for v in losses))
    print("visibility fit  oracle64", " ".join(f"{v:.4e}" for v in l64))
    assert losses[-1] < losses[0]


# ------------------------------------------------------------------------------------------------ 9. refusals and lifetimes
def test_points_and_dirs_refuse_a_gradient(dev, synth_weights):
    from robir_amd import training, vis_autograd
    net = training.enable_visibility_training(_vis_net(dev, _weights(synth_weights, "init")))
    pts, dirs, _ = _inputs(8, 1)
    with torch.enable_grad():
        p, d = pts.to(dev).requires_grad_(), dirs.to(dev).requires_grad_()
        with pytest.raises(NotImplementedError, match="points"):
            net(p, dirs.to(dev))
        with pytest.raises(NotImplementedError, match="dirs"):
            net.logits_from_points(pts.to(dev), d)
        with pytest.raises(NotImplementedError, match="points"):
            vis_autograd.logits(net, p, dirs.to(dev))
    out = net(p, d)                                     # grad mode off: today's forward, no refusal
    assert not out.requires_grad


def test_graph_is_freed_by_reference_counting(dev, synth_weights):
    """Only save_for_backward holds tensors: once the logits and the loss are dropped -- with or without a backward() -- the weakrefs are dead
    and the allocation returns to its base with the cyclic collector disabled."""
    from robir_amd import training
    net = training.enable_visibility_training(_vis_net(dev, _weights(synth_weights, "init")))
    pts, dirs, _ = _inputs(2048, 8, seed=8)
    pts, dirs = pts.to(dev), dirs.to(dev)
    net.logits_from_points(pts, dirs, 8)                 # packed blobs exist before the base is read
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        for run_backward in (False, True):
            net.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            with torch.enable_grad():
                y = net.logits_from_points(pts, dirs, 8)
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
