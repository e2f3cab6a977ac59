"""Trainable indirect illumination on the GPU: rb_it_lobe_bwd / rb_it_sg_query / rb_it_sg_query_bwd (librobir_hip_illumtrain.so),
robir_amd/illum_autograd.py and robir_amd/training.py.

The truth is float64 autograd of the oracle's formulas (robir_oracle.nets.indirect_illum and the query, through tests/illum_train_oracle.py) on
the CPU, fed the same fp32 inputs the kernels saw; tests/golden/illum_grad.npz (tools/gen_illum_grad_golden.py) pins that oracle on the
REFERENCE's own IndirctIllumNetwork and query_indir_illum.  The yardstick is the project's rule: for every tensor
`e_kernel <= max(2 e_torch, 1e-5)`, e = conftest.rel_err against float64, e_torch what PyTorch's fp32 autograd of the same formulas achieves on
the same inputs.  Every pair is recorded.  conftest wraps every test in no_grad: the tests enter torch.enable_grad() themselves."""
import gc
import weakref

import numpy as np
import pytest
import torch

import illum_train_oracle as ito
from conftest import record_metric, rel_err, load_golden

pytestmark = pytest.mark.gpu
FLOOR = 1e-5
ILL = ito.PREFIX


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _weights(synth_weights, which, no_hdr=False):
    """"init": the synthetic weights; "perturbed": + 0.02 N(0,1) on every matrix, so that no layer is near its initial structure.
    no_hdr: the first weights lose their hdr column ([512,63])."""
    sd = {k: torch.as_tensor(v).clone() for k, v in synth_weights.items() if k.startswith(ILL)}
    if which == "perturbed":
        g = torch.Generator().manual_seed(77)
        for k in sd:
            if sd[k].dim() == 2:
                sd[k] = sd[k] + 0.02 * torch.randn(sd[k].shape, generator=g)
    if no_hdr:
        for k in ("lobe_layer.0.weight", "integral_layer.brdf_encoder_layer.0.weight"):
            sd[ILL + k] = sd[ILL + k][:, :63].contiguous()
    return sd


def _illum_net(dev, sd, train=True, no_hdr=False):
    from robir_amd import nets
    net = nets.IndirctIllumNetwork(multires=10, dims=[512] * 4, num_lgt_sgs=24, no_hdr=no_hdr)
    net.load_state_dict({k[len(ILL):]: torch.as_tensor(v) for k, v in sd.items() if k.startswith(ILL)})
    net = net.to(dev)
    return net.train() if train else net.eval()


def assert_parity(tag, kernel, torch32, ref64, err=None):
    bad = []
    for k, r in ref64.items():
        r = torch.as_tensor(r)
        e = (err or {}).get(k, rel_err)
        e_kernel = e(torch.as_tensor(kernel[k]).reshape(r.shape), r)
        e_torch = e(torch.as_tensor(torch32[k]).reshape(r.shape), r)
        record_metric(f"illum_train/{tag}/{k}", e_kernel=e_kernel, e_torch=e_torch, max_abs_ref=float(r.abs().max()))
        print(f"{tag:44s} d {k:46s} e_kernel {e_kernel:.2e}  e_torch {e_torch:.2e}")
        if not e_kernel <= max(2.0 * e_torch, FLOOR):
            bad.append((k, e_kernel, e_torch))
    assert not bad, (tag, bad)


def _inputs(n, seed=0):
    g = torch.Generator().manual_seed(500 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"points": r(n, 3) * 0.5, "hdr": torch.rand(n, 1, generator=g), "noise": r(n, 64), "g_sgs": r(n, 24, 7), "g_int": r(n, 3)}


def _lobe_kernel(dev, params, pts, hdr, g_sgs, **kw):
    """ops.illum_lobe_backward on device copies -> (dict of CPU gradients, stats)."""
    from robir_amd import ops
    D = lambda t: None if t is None else torch.as_tensor(t).float().to(dev).contiguous()
    out, stats = ops.illum_lobe_backward(D(pts), D(hdr), [D(params[k]) for k in ito.LOBE_NAMES], D(g_sgs), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}, stats


_REF = {}


def _lobe_truth(key, params, pts, hdr, g_sgs):
    """(float64 gradients, fp32 gradients) of <g_sgs, lgt_sgs> for the ten lobe tensors, computed once per case and shared."""
    if key not in _REF:
        fn = lambda lv: (g_sgs.to(ito._dtype(lv)) * ito.lobes_forward(lv, pts, hdr)).sum()
        _REF[key] = tuple(ito.grads_of(fn, params, dt, ito.LOBE_NAMES)[1] for dt in (torch.float64, torch.float32))
    return _REF[key]


def _rows(dev, pts, hdr, noise):
    """The fp32 perturbed rows the integral layer's kernels see, on the CPU."""
    from robir_amd import ops
    D = lambda t: None if t is None else t.float().to(dev).contiguous()
    return ops.axpy(ops.feat_pe10(D(pts), extra=D(hdr)), D(noise), 0.02).cpu()


# ------------------------------------------------------------------------------------------------ 1. fails without the feature
def test_marked_network_trains(dev, synth_weights):
    from robir_amd import nets, training
    sd = _weights(synth_weights, "init")
    net = _illum_net(dev, sd)
    x = {k: v.to(dev) for k, v in _inputs(48).items()}
    with torch.enable_grad():
        with pytest.raises(nets.ForwardOnlyError):
            net(x["points"], x["hdr"], noise=x["noise"])
        assert training.enable_illumination_training(net) is net
        sgs, integ = net(x["points"], x["hdr"], noise=x["noise"])
        assert sgs.grad_fn is not None and integ.grad_fn is not None
        assert tuple(sgs.shape) == (48, 24, 7) and tuple(integ.shape) == (48, 3)
        ((sgs * x["g_sgs"]).sum() + (integ * x["g_int"]).sum()).backward()
    named = dict(net.named_parameters())
    assert set(named) == set(ito.NAMES)
    for name, p in named.items():
        assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape), name
        assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
    # the values of the trainable path are the forward-only path's, bit for bit (conftest's no_grad is active here)
    ref_sgs, ref_int = net(x["points"], x["hdr"], noise=x["noise"])
    assert not ref_sgs.requires_grad and torch.equal(sgs.detach(), ref_sgs) and torch.equal(integ.detach(), ref_int)
    training.enable_illumination_training(net, on=False)
    u_sgs, u_int = net(x["points"], x["hdr"], noise=x["noise"])
    assert torch.equal(sgs.detach(), u_sgs) and torch.equal(integ.detach(), u_int)
    # one sub-network frozen: its Function does not run and its parameters get nothing
    for half in ("lobe_layer.", "integral_layer."):
        net = training.enable_illumination_training(_illum_net(dev, sd))
        for name, p in net.named_parameters():
            p.requires_grad_(name.startswith(half))
        with torch.enable_grad():
            s2, i2 = net(x["points"], x["hdr"], noise=x["noise"])
            assert (s2.grad_fn is not None) == (half == "lobe_layer.") and (i2.grad_fn is not None) == (half == "integral_layer.")
            (s2 if half == "lobe_layer." else i2).sum().backward()
        assert torch.equal(s2.detach(), ref_sgs) and torch.equal(i2.detach(), ref_int)
        for name, p in net.named_parameters():
            assert (p.grad is not None) == name.startswith(half), name


# ------------------------------------------------------------------------------------------------ 2. kernel-level parity
CASES = [(1, 64, 64), (15, 64, 16), (17, 64, 16), (65, 64, 64), (200, 64, 48), (1100, 256, 80)]


@pytest.mark.parametrize("weights", ["init", "perturbed"])
@pytest.mark.parametrize("n,slab,part", CASES)
def test_lobe_kernel_parity(dev, synth_weights, weights, n, slab, part):
    """(1,64,64), (15,64,16), (17,64,16): the 16-row MFMA tile edge; (65,64,64): a second slab of one row; (200,64,48): a ragged last
    partition and a ragged last slab of 8 rows; (1100,256,80): five slabs, four partitions of which the last is ragged.  A random normal
    upstream gradient on the decoded lobes; all ten gradients compared."""
    params = ito.illum_params(_weights(synth_weights, weights))
    x = _inputs(n, seed=n)
    ref64, t32 = _lobe_truth((weights, n), params, x["points"], x["hdr"], x["g_sgs"])
    kernel, stats = _lobe_kernel(dev, params, x["points"], x["hdr"], x["g_sgs"], slab_rows=slab, part_rows=part)
    assert set(kernel) == set(ito.LOBE_NAMES) and stats["lowest_layer"] == 0
    assert stats["partitions"] == -(-min(n, slab) // part) and stats["scratch_bytes"] > 0
    assert tuple(kernel["lobe_layer.0.weight"].shape) == (512, 64) and tuple(kernel["lobe_layer.8.weight"].shape) == (144, 512)
    assert tuple(kernel["lobe_layer.8.bias"].shape) == (144,)
    assert_parity(f"lobe/{weights}/n{n}_slab{slab}_part{part}", kernel, t32, ref64)


@pytest.mark.parametrize("weights", ["init", "perturbed"])
def test_lobe_kernel_parity_without_hdr(dev, synth_weights, weights):
    """(33,64,16) on a no_hdr net: hdr = None, W0 is [512,63]."""
    from robir_amd import training
    sd = _weights(synth_weights, weights, no_hdr=True)
    params = ito.illum_params(sd)
    x = _inputs(33, seed=33)
    ref64, t32 = _lobe_truth((weights, "no_hdr"), params, x["points"], None, x["g_sgs"])
    kernel, stats = _lobe_kernel(dev, params, x["points"], None, x["g_sgs"], slab_rows=64, part_rows=16)
    assert tuple(kernel["lobe_layer.0.weight"].shape) == (512, 63) and stats["partitions"] == 3 and stats["lowest_layer"] == 0
    assert_parity(f"lobe/{weights}/no_hdr_n33", kernel, t32, ref64)
    if weights == "init":          # through the module: the reference's 63-column noise
        net = training.enable_illumination_training(_illum_net(dev, sd, no_hdr=True))
        with torch.enable_grad():
            sgs, integ = net(x["points"].to(dev), x["hdr"].to(dev), noise=x["noise"][:, :63].to(dev))
            ((sgs * x["g_sgs"].to(dev)).sum() + (integ * x["g_int"].to(dev)).sum()).backward()
        got = {k: p.grad.cpu() for k, p in net.named_parameters()}
        assert_parity("lobe/init/no_hdr_module", got, t32, ref64)
        rows = _rows(dev, x["points"], None, torch.nn.functional.pad(x["noise"][:, :63], (0, 1)))[:, :63]
        fn = lambda lv: (x["g_int"].to(ito._dtype(lv)) * ito.integral_forward(lv, rows)).sum()
        i64, i32 = (ito.grads_of(fn, params, dt, ito.INT_NAMES)[1] for dt in (torch.float64, torch.float32))
        assert tuple(got["integral_layer.brdf_encoder_layer.0.weight"].shape) == (512, 63)
        assert_parity("integral/init/no_hdr_module", got, i32, i64)


# ------------------------------------------------------------------------------------------------ 3. gradient subsets
def test_subsets_stop_the_data_path(dev, synth_weights):
    params = ito.illum_params(_weights(synth_weights, "init"))
    x = _inputs(200, seed=200)
    run = lambda **kw: _lobe_kernel(dev, params, x["points"], x["hdr"], x["g_sgs"], slab_rows=64, part_rows=48, **kw)
    full, fs = run()
    last = ("lobe_layer.8.weight", "lobe_layer.8.bias")
    part, ps = run(want=last)
    assert set(part) == set(last) and ps["lowest_layer"] == 4 and fs["lowest_layer"] == 0 and ps["launches"] < fs["launches"]
    biases = tuple(k for k in ito.LOBE_NAMES if k.endswith(".bias"))
    bs, bst = run(want=biases)
    assert set(bs) == set(biases) and bst["lowest_layer"] == 0
    upper = tuple(k for k in ito.LOBE_NAMES if int(k.split(".")[1]) >= 4)
    up, us = run(want=upper)
    assert set(up) == set(upper) and us["lowest_layer"] == 2 and ps["launches"] < us["launches"] < fs["launches"]
    for sub in (part, bs, up):
        for k, v in sub.items():
            assert torch.equal(v, full[k]), k
    none, ns = run(want=())
    assert none == {} and ns["launches"] == 0 and ns["lowest_layer"] == 5


# ------------------------------------------------------------------------------------------------ 4. the SG query
def _query_inputs(n, S, L, seed):
    """Lobes of length 1.7 (the normalisation's gradient counts), some mu exactly 0, lambda at 0.1 and 30.1 among random ones, an upstream
    gradient zeroed on a random 40 % of the samples."""
    g = torch.Generator().manual_seed(900 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    axis = torch.nn.functional.normalize(r(n, L, 3), dim=-1) * 1.7
    lam = torch.rand(n, L, 1, generator=g) * 30 + 0.1
    lam[:, 0] = 0.1
    lam[:, L - 1] = 30.1
    mu = torch.relu(r(n, L, 3))
    assert bool((mu == 0).any()) or n * L < 4
    dirs = torch.nn.functional.normalize(r(n, S, 3), dim=-1)
    gr = r(n, S, 3) * (torch.rand(n, S, 1, generator=g) >= 0.4)
    return torch.cat([axis, lam, mu], -1), dirs, gr


@pytest.mark.parametrize("n,S,L", [(1, 1, 24), (3, 63, 24), (5, 64, 24), (2, 65, 24), (33, 16, 24), (7, 512, 24), (4, 40, 5)])
def test_sg_query_forward_and_reverse(dev, n, S, L):
    """S = 1, 63 | 64 | 65 (the wave edge), 512 (two samples per lane), 33 points (more than one workgroup per compute-unit row), L = 5."""
    from robir_amd import ops, training
    sgs, dirs, gr = _query_inputs(n, S, L, seed=S + L)
    (rad64, g64), (rad32, g32) = (ito.query_grads(sgs, dirs, gr, dt) for dt in (torch.float64, torch.float32))
    sd, dd, gd = sgs.to(dev), dirs.to(dev), gr.to(dev)
    rad, gs = ops.sg_query(sd, dd), ops.sg_query_backward(sd, dd, gd)
    assert tuple(rad.shape) == (n, S, 3) and tuple(gs.shape) == (n, L, 7)
    assert torch.equal(rad, ops.sg_query(sd, dd)) and torch.equal(gs, ops.sg_query_backward(sd, dd, gd))          # equal inputs, equal bytes
    tag = f"query/n{n}_S{S}_L{L}"
    assert_parity(tag, {"radiance": rad.cpu(), "g_sgs": gs.cpu()}, {"radiance": rad32, "g_sgs": g32}, {"radiance": rad64, "g_sgs": g64})
    pieces = lambda t: {"g_axis": t[..., :3], "g_lambda": t[..., 3], "g_mu": t[..., 4:]}
    assert_parity(tag, pieces(gs.cpu()), pieces(g32), pieces(g64))
    with torch.enable_grad():          # through autograd
        leaf = sd.clone().requires_grad_()
        out = training.query_indir_illum(leaf, dd)
        assert torch.equal(out.detach(), rad)
        (out * gd).sum().backward()
    assert torch.equal(leaf.grad, gs)


# ------------------------------------------------------------------------------------------------ 5. the integral layer
@pytest.mark.parametrize("n,var", [(1, False), (17, False), (65, True), (200, False)])
def test_integral_layer_through_its_function(dev, synth_weights, n, var):
    """One clean pass on the perturbed rows through rb_train_ae_bwd, slabs of 64 rows: one row, the tile edge, a second slab of one row,
    four slabs; a non-zero `var` in one case."""
    from robir_amd import training
    sd = _weights(synth_weights, "perturbed")
    params = ito.illum_params(sd)
    x = _inputs(n, seed=n + 1)
    net = training.enable_illumination_training(_illum_net(dev, sd))
    net.integral_layer._train_slab_rows = 64
    v = None
    if var:
        v = torch.rand(32, generator=torch.Generator().manual_seed(9)) * 0.5
        net.integral_layer.var = v.clone()
    for name, p in net.named_parameters():
        p.requires_grad_(name.startswith("integral_layer."))
    with torch.enable_grad():
        sgs, integ = net(x["points"].to(dev), x["hdr"].to(dev), noise=x["noise"].to(dev))
        assert sgs.grad_fn is None
        (integ * x["g_int"].to(dev)).sum().backward()
    got = {k: p.grad.cpu() for k, p in net.named_parameters() if p.grad is not None}
    assert set(got) == set(ito.INT_NAMES)
    rows = _rows(dev, x["points"], x["hdr"], x["noise"])
    fn = lambda lv: (x["g_int"].to(ito._dtype(lv)) * ito.integral_forward(lv, rows, v)).sum()
    (_, ref64), (_, t32) = (ito.grads_of(fn, params, dt, ito.INT_NAMES) for dt in (torch.float64, torch.float32))
    val64 = ito.integral_forward({k: p.double() for k, p in params.items()}, rows, v)
    assert rel_err(integ.detach().cpu(), val64) <= 1e-4          # the forward kernels' own parity bound
    assert_parity(f"integral/n{n}_var{int(var)}", got, t32, ref64)


# ------------------------------------------------------------------------------------------------ 6. the reference fixture
def test_autograd_against_the_reference_fixture(dev, synth_weights):
    """tests/golden/illum_grad.npz: the REFERENCE's IndirctIllumNetwork and query_indir_illum differentiated in float64 on 16 points x 8
    directions under the radiance loss; the oracle's recorded distance from it is <= 1e-12 and the HIP path holds the rule against every
    stored piece."""
    from robir_amd import training
    fx = load_golden("illum_grad")
    sd = _weights(synth_weights, "init")
    params = ito.illum_params(sd)
    T = lambda k: torch.from_numpy(np.asarray(fx[k]))
    n, t = T("points").shape[0], float(fx["anneal_t"])
    every = torch.ones(n, dtype=torch.bool)
    trace = {k: T(k) for k in ("sample_dirs", "indir_mask", "trace_radiance", "gt_integral")}
    net = training.enable_illumination_training(_illum_net(dev, sd))
    with torch.enable_grad():
        sgs, integ = net(T("points").to(dev), T("hdr_shift").to(dev), noise=T("noise").to(dev))
        loss = training.radiance_loss({"network_object_mask": every.to(dev), "indirect_sgs": sgs, "indir_integral": integ},
                                      {k: v.to(dev) for k, v in trace.items()}, anneal_t=t)
        loss.backward()
    kernel = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}

    def oracle_loss(lv):
        return ito.radiance_loss(*ito.both_forward(lv, T("points"), T("hdr_shift"), T("noise")), trace, every, t, "L1")
    l32, t32 = ito.grads_of(oracle_loss, params, torch.float32)
    record_metric("illum_train/reference_fixture/loss", hip=float(loss), torch32=l32, reference64=float(fx["loss"]))
    assert abs(float(loss) - float(fx["loss"])) <= 1e-4 * float(fx["loss"])          # the forward kernels' own parity bound

    def pieces(g, k):
        if g.dim() == 1:
            return {f"{k}.full": g}
        return {f"{k}.rows8": g[:8], f"{k}.cols8": g[:, :8], f"{k}.sum": g.double().sum(), f"{k}.fro": g.double().norm()}
    K, T32, R = {}, {}, {}
    for k in ito.NAMES:
        K.update(pieces(kernel[k], k))
        T32.update(pieces(t32[k], k))
    for key in K:
        assert float(fx["oracle_dist." + key]) <= 1e-12, key
        R[key] = torch.from_numpy(np.asarray(fx["grad." + key]))
    assert_parity("reference_fixture", K, T32, R)


# ------------------------------------------------------------------------------------------------ 7. stage level
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


def test_illum_stage_trains(dev, model):
    """One 'Illum' chunk of the 64 x 64 synthetic view (the 1024 pixels test_vis_train_gpu.py uses; nsamp 4, every draw pinned): the model in
    eval(), the illumination network in train() and marked.  Measured on an MI355X: 888 hit points, indir_mask keeps 17 % of the samples."""
    from robir_amd import deferred, synth, training
    NS = 4
    ill = model.indirect_illum_network
    inp = _chunk_input(dev)
    model.deferred_chunks = 0
    try:
        n = int(model(inp, trainstage="Illum")["network_object_mask"].sum())
        assert 100 <= n <= 1024
        dr = {k: torch.from_numpy(v).to(dev) for k, v in synth.pbr_draws(0, n, chunk_id=1).items()}
        ref = model(inp, trainstage="Illum", draws=dr)                        # no_grad (conftest)
        g = torch.Generator().manual_seed(21)
        tr = model.trace_radiance(ref, nsamp=NS, draws=(torch.rand(n * NS, generator=g), torch.rand(n * NS, generator=g)))
        mask = ref["network_object_mask"]
        kept = float(tr["indir_mask"][mask].float().mean())
        print(f"stage: n_hit {n}, indir_mask keeps {100 * kept:.1f} % of the samples")
        assert 0.05 <= kept <= 0.95
        assert not tr["trace_radiance"].requires_grad and not tr["gt_integral"].requires_grad
        ill.train()
        training.enable_illumination_training(model)
        with torch.enable_grad():
            out = model(inp, trainstage="Illum", draws=dr)
            assert out["indirect_sgs"].grad_fn is not None and out["indir_integral"].grad_fn is not None
            assert torch.equal(out["indirect_sgs"].detach(), ref["indirect_sgs"]) and torch.equal(out["indir_integral"].detach(), ref["indir_integral"])
            loss = training.radiance_loss(out, tr, anneal_t=0.05)
            loss.backward()
        for name, p in model.named_parameters():
            assert (p.grad is not None) == name.startswith("indirect_illum_network."), name
        kernel = {k[len(ILL):]: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}
        # the oracle on the same points, noise, directions, masks and targets
        idx = mask.nonzero()[:, 0]
        pts, hdr, noise = ref["points"][idx].cpu(), inp["hdr_shift"][idx].cpu(), dr["illum_randn"].cpu()
        rows = _rows(dev, pts, hdr, noise)
        params = {k: p.detach().cpu() for k, p in ill.named_parameters()}
        trace = {"sample_dirs": tr["sample_dirs"].cpu(), "indir_mask": tr["indir_mask"][idx].cpu(),
                 "trace_radiance": tr["trace_radiance"][idx].cpu(), "gt_integral": tr["gt_integral"][idx].cpu()}
        every = torch.ones(n, dtype=torch.bool)
        fn = lambda lv: ito.radiance_loss(ito.lobes_forward(lv, pts, hdr), ito.integral_forward(lv, rows), trace, every, 0.05, "L1")
        (l64, ref64), (l32, t32) = (ito.grads_of(fn, params, dt) for dt in (torch.float64, torch.float32))
        record_metric("illum_train/stage/loss", hip=float(loss), oracle64=l64, torch32=l32, n_hit=n, kept=kept)
        assert abs(float(loss) - l64) <= 1e-4 * l64          # the forward kernels' own parity bound
        assert_parity("stage", kernel, t32, ref64)
        # recording: with the mark the chunk forward runs at once, unmarked it is still recorded
        model.zero_grad(set_to_none=True)
        model.deferred_chunks = 4
        with torch.enable_grad():
            out = model(inp, trainstage="Illum")
        assert not isinstance(out, deferred.ChunkOutputs) and out["indirect_sgs"].grad_fn is not None
        training.enable_illumination_training(model, on=False)
        ill.eval()
        with torch.enable_grad():
            out = model(inp, trainstage="Illum")
        assert isinstance(out, deferred.ChunkOutputs) and out._q.result is None
    finally:
        training.enable_illumination_training(model, on=False)
        model.flush()
        model.__dict__.pop("deferred_chunks", None)
        model.zero_grad(set_to_none=True)
        model.eval()


# ------------------------------------------------------------------------------------------------ 8. determinism
def test_determinism_and_partition_independence(dev, synth_weights):
    params = ito.illum_params(_weights(synth_weights, "perturbed"))
    x = _inputs(1100, seed=1100)
    run = lambda **kw: _lobe_kernel(dev, params, x["points"], x["hdr"], x["g_sgs"], **kw)
    runs = [run(slab_rows=256, part_rows=80)[0] for _ in range(3)]
    for k in ito.LOBE_NAMES:
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], runs[2][k]), k
    ref64, t32 = _lobe_truth(("perturbed", 1100), params, x["points"], x["hdr"], x["g_sgs"])
    for slab, part in ((256, 256), (256, 16), (1100, 80), (128, 80)):
        other, st = run(slab_rows=slab, part_rows=part)
        assert st["partitions"] == -(-min(1100, slab) // part)
        assert_parity(f"lobe/perturbed/n1100_slab{slab}_part{part}", other, t32, ref64)
    default, st = run()
    assert st["partitions"] == 5          # min(n, 4096) = 1100 rows in partitions of 256
    assert_parity("lobe/perturbed/n1100_default", default, t32, ref64)


# ------------------------------------------------------------------------------------------------ 9. a fit and the weight cache
def test_fit_descends_and_the_weight_cache_follows_the_optimiser(dev, synth_weights):
    """128 points x 16 directions; the targets are the radiance and the integral of the perturbed weights.  One SGD step's parameters match
    the oracle's step under the rule; 30 Adam steps at the stage's lr = 5e-4 end below the first loss, the trajectory is recorded beside the
    float64 oracle's; after optimizer.step() the no_grad forward equals a freshly built network loaded with the stepped state dict, bit for
    bit: the packed blobs follow the optimiser."""
    from robir_amd import training
    P, S, steps = 128, 16, 30
    x = _inputs(P, seed=7)
    g = torch.Generator().manual_seed(8)
    dirs = torch.nn.functional.normalize(torch.randn(P, S, 3, generator=g), dim=-1)
    sd = _weights(synth_weights, "init")
    params = ito.illum_params(sd)
    pd, hd, nd, dd = x["points"].to(dev), x["hdr"].to(dev), x["noise"].to(dev), dirs.to(dev)
    target = _illum_net(dev, _weights(synth_weights, "perturbed"), train=False)
    t_sgs, t_int = target(pd, hd, noise=nd)
    from robir_amd import ops
    t_rad = ops.sg_query(t_sgs, dd)
    rows = _rows(dev, x["points"], x["hdr"], x["noise"])
    every = torch.ones(P, dtype=torch.bool)
    trace = {"sample_dirs": dirs, "indir_mask": torch.ones(P, S, dtype=torch.bool), "trace_radiance": t_rad.cpu(), "gt_integral": t_int.cpu()}
    trace_d = {k: v.to(dev) for k, v in trace.items()}

    def hip_loss(net):
        sgs, integ = net(pd, hd, noise=nd)
        return training.radiance_loss({"network_object_mask": every.to(dev), "indirect_sgs": sgs, "indir_integral": integ}, trace_d)
    oracle_loss = lambda lv: ito.radiance_loss(ito.lobes_forward(lv, x["points"], x["hdr"]), ito.integral_forward(lv, rows), trace, every)

    # one SGD step
    net = training.enable_illumination_training(_illum_net(dev, sd))
    sgd = torch.optim.SGD(net.parameters(), lr=0.1)
    with torch.enable_grad():
        hip_loss(net).backward()
    sgd.step()
    stepped = {k: p.detach().cpu() for k, p in net.named_parameters()}

    def oracle_step(dtype):
        lv = ito.leaves(params, dtype)
        o = torch.optim.SGD(list(lv.values()), lr=0.1)
        with torch.enable_grad():
            oracle_loss(lv).backward()
        o.step()
        return {k: v.detach() for k, v in lv.items()}
    assert_parity("fit/sgd_step", stepped, oracle_step(torch.float32), oracle_step(torch.float64))

    # the consumers of the weights see the step
    fresh = _illum_net(dev, {ILL + k: v for k, v in net.state_dict().items()}, train=False)
    a, b = net(pd, hd, noise=nd), fresh(pd, hd, noise=nd)                      # no_grad (conftest)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    before = _illum_net(dev, sd, train=False)(pd, hd, noise=nd)
    assert not torch.equal(a[0], before[0]) and not torch.equal(a[1], before[1])

    # the fit
    net = training.enable_illumination_training(_illum_net(dev, sd))
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    losses = []
    for _ in range(steps + 1):
        with torch.enable_grad():
            opt.zero_grad()
            loss = hip_loss(net)
            loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
    lv = ito.leaves(params, torch.float64)
    o = torch.optim.Adam(list(lv.values()), lr=5e-4)
    l64 = []
    for _ in range(steps + 1):
        with torch.enable_grad():
            o.zero_grad()
            loss = oracle_loss(lv)
            loss.backward()
        l64.append(float(loss.detach()))
        o.step()
    record_metric("illum_train/fit", **{f"hip_{i}": v for i, v in enumerate(losses)}, **{f"oracle64_{i}": v for i, v in enumerate(l64)})
    print("illumination fit  HIP     ", " ".join(f"{v:.4e}" for v in losses))
    print("illumination fit  oracle64", " ".join(f"{v:.4e}" for v in l64))
    assert losses[-1] < losses[0]


# ------------------------------------------------------------------------------------------------ 10. refusals and lifetimes
def test_query_refuses_a_gradient_for_the_directions(dev):
    from robir_amd import illum_autograd, training
    sgs, dirs, _ = _query_inputs(4, 8, 24, seed=1)
    sgs, dirs = sgs.to(dev), dirs.to(dev)
    with torch.enable_grad():
        d = dirs.clone().requires_grad_()
        with pytest.raises(NotImplementedError, match="sample_dirs"):
            training.query_indir_illum(sgs, d)
        with pytest.raises(NotImplementedError, match="sample_dirs"):
            illum_autograd.sg_query(sgs.clone().requires_grad_(), d)
    assert not training.query_indir_illum(sgs, d).requires_grad          # grad mode off: no refusal


def test_graph_is_freed_by_reference_counting(dev, synth_weights):
    """Only save_for_backward holds tensors: once the outputs and the loss are dropped -- with or without a backward() -- the weakrefs are
    dead and the allocation returns to its base with the cyclic collector disabled."""
    from robir_amd import training
    net = training.enable_illumination_training(_illum_net(dev, _weights(synth_weights, "init")))
    x = {k: v.to(dev) for k, v in _inputs(300, seed=3).items()}
    dirs = torch.nn.functional.normalize(torch.randn(300, 8, 3, generator=torch.Generator().manual_seed(4)), dim=-1).to(dev)
    net(x["points"], x["hdr"], noise=x["noise"])                 # packed blobs exist before the base is read
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        for run_backward in (False, True):
            net.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            with torch.enable_grad():
                sgs, integ = net(x["points"], x["hdr"], noise=x["noise"])
                rad = training.query_indir_illum(sgs, dirs)
                loss = rad.square().mean() + integ.square().mean()
                refs = [weakref.ref(t) for t in (sgs, integ, rad, loss)]
                assert torch.cuda.memory_allocated() > base
                if run_backward:
                    loss.backward()
            del sgs, integ, rad, loss
            assert all(r() is None for r in refs)
            net.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            assert torch.cuda.memory_allocated() == base, (run_backward, torch.cuda.memory_allocated() - base)
    finally:
        if was:
            gc.enable()
