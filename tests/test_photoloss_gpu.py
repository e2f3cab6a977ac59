"""The photometric loss on the GPU: rb_pl_tonemap_bwd / rb_pl_image_loss (librobir_hip_photoloss.so), robir_amd/tonemap_autograd.py,
robir_amd/loss.py and training.enable_tonemap_training / photometric_loss.

The truth is float64 autograd of tests/photoloss_oracle.py on the CPU, fed the same fp32 inputs.  The yardstick is the training tests'
rule: for every gradient tensor `e_kernel <= max(2 e_torch, 1e-5)`, e = conftest.rel_err against float64, e_torch what PyTorch's fp32
autograd of the same formulas achieves on the same inputs.  Every pair is recorded.  conftest wraps every test in no_grad: the tests enter
torch.enable_grad() themselves."""
import numpy as np
import pytest
import torch

import photoloss_oracle as plo
from conftest import record_metric, rel_err
from test_material_train_gpu import FLOOR

pytestmark = pytest.mark.gpu
CURVE_DIRS = [(c, inv) for c in plo.CURVES for inv in (False, True)] + [(plo.RATIONAL, False)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def assert_parity(tag, kernel, torch32, ref64):
    bad = []
    for k, r in ref64.items():
        r = torch.as_tensor(r)
        e_kernel = rel_err(kernel[k].reshape(r.shape), r)
        e_torch = rel_err(torch32[k].reshape(r.shape), r)
        record_metric(f"photoloss/{tag}/{k}", e_kernel=e_kernel, e_torch=e_torch, max_abs_ref=float(r.abs().max()))
        print(f"{tag:48s} {k:12s} e_kernel {e_kernel:.2e}  e_torch {e_torch:.2e}")
        if not e_kernel <= max(2.0 * e_torch, FLOOR):
            bad.append((k, e_kernel, e_torch))
    assert not bad, (tag, bad)


_REF = {}


def _tm_truth(n, curve, inverse, per_row):
    """The case and its (float64, float32) oracle gradients, computed once and shared."""
    key = ("tm", n, curve, inverse, per_row)
    if key not in _REF:
        x, t, gy = plo.tonemap_case(n, min(curve, 3), inverse, per_row)
        out = []
        for dt in (torch.float64, torch.float32):
            y, gx, gs = plo.tonemap_grads(x, t, gy, curve, inverse, dt)
            out.append({"y": y, "gx": gx, "gshift": gs})
        _REF[key] = (x, t, gy, out[0], out[1])
    return _REF[key]


def _loss_truth(n, curve, per_row, l2, indir=True):
    key = ("loss", n, curve, per_row, l2, indir)
    if key not in _REF:
        case = plo.loss_case(n, curve, per_row, l2, indir=indir)
        out = []
        for dt in (torch.float64, torch.float32):
            loss, g_sg, g_ind, g_sh = plo.loss_grads(case, curve, l2, dt)
            d = {"loss": loss, "g_rgb": g_sg}
            if g_sh is not None:
                d["g_shift"] = g_sh
            out.append(d)
        _REF[key] = (case, out[0], out[1])
    return _REF[key]


def _dev_case(case, dev):
    return {k: (None if v is None else v.to(dev)) for k, v in case.items()}


# ------------------------------------------------------------------------------------------------ 1. forward bits
@pytest.mark.parametrize("n", plo.ROWS)
def test_forward_bits_equal_ops_tonemap(dev, n):
    """photoloss_math.h's fp32 forward (rb_pl_tonemap) and a MARKED module's hdr2ldr / ldr2hdr equal ops.tonemap bit for bit, every curve and
    direction, shift per row and single."""
    from robir_amd import nets, ops, training
    for curve in plo.CURVES:
        tone = training.enable_tonemap_training(nets.ACESToneMapping(hdr_mode=curve if curve < 3 else 7).to(dev))
        for inverse in (False, True):
            for per_row in (False, True):
                x, t, _ = plo.tonemap_case(n, curve, inverse, per_row)
                x, t = x.to(dev), t.to(dev)
                want = ops.tonemap(x, t, int(inverse) + 16 * curve)
                assert torch.equal(ops.pl_tonemap(x, t, curve, int(inverse)), want), (curve, inverse, per_row)
                with torch.enable_grad():
                    xr = x.clone().requires_grad_(True)
                    got = (tone.ldr2hdr if inverse else tone.hdr2ldr)(xr, t)
                assert got.requires_grad and torch.equal(got.detach(), want), (curve, inverse, per_row)
                assert rel_err(want, plo.tonemap(x.cpu().double(), t.cpu().double(), curve, inverse)) <= 1e-5
    x = plo.tonemap_case(n, 3, False, False)[0].to(dev)
    assert torch.equal(ops.pl_tonemap(x, None, plo.RATIONAL), x / (x + 1))


# ------------------------------------------------------------------------------------------------ 2. the curves' backward
@pytest.mark.parametrize("per_row", [False, True], ids=["one_shift", "row_shift"])
@pytest.mark.parametrize("curve,inverse", CURVE_DIRS)
@pytest.mark.parametrize("n", plo.ROWS)
def test_tonemap_backward_parity(dev, n, curve, inverse, per_row):
    from robir_amd import ops
    x, t, gy, ref64, t32 = _tm_truth(n, curve, inverse, per_row)
    gx, gs = ops.pl_tonemap_backward(x.to(dev), t.to(dev), curve, int(inverse), gy.to(dev))
    want = {k: ref64[k] for k in ("gx", "gshift")}
    assert_parity(f"tonemap_bwd/c{curve}_{'inv' if inverse else 'fwd'}_{'row' if per_row else 'one'}/n{n}", {"gx": gx.cpu(), "gshift": gs.cpu()},
                  t32, want)
    # either gradient alone: the same bits
    only_x, none_s = ops.pl_tonemap_backward(x.to(dev), t.to(dev), curve, int(inverse), gy.to(dev), want_shift=False)
    none_x, only_s = ops.pl_tonemap_backward(x.to(dev), t.to(dev), curve, int(inverse), gy.to(dev), want_x=False)
    assert none_s is None and none_x is None and torch.equal(only_x, gx) and torch.equal(only_s, gs)


def test_tonemap_autograd_function(dev):
    """The Function through a marked module: gradients to x and to a raw_shift tensor equal the kernel's; a Python-float shift gives a graph
    to x alone; a gradient of the gradient raises."""
    from robir_amd import nets, ops, training
    tone = training.enable_tonemap_training(nets.ACESToneMapping(hdr_mode=0).to(dev))
    x, t, gy, _, _ = _tm_truth(257, 0, False, True)
    x, t, gy = x.to(dev), t.to(dev), gy.to(dev)
    with torch.enable_grad():
        xr, tr = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
        y = tone.hdr2ldr(xr, tr)
        gx, gt = torch.autograd.grad((y * gy).sum(), [xr, tr])
    kx, ks = ops.pl_tonemap_backward(x, t, 0, 0, gy)
    assert torch.equal(gx, kx) and torch.equal(gt, ks)
    with torch.enable_grad():
        xr = x.clone().requires_grad_(True)
        y = tone.hdr2ldr(xr, 0.01)
        assert y.requires_grad and torch.equal(y.detach(), ops.tonemap(x, torch.tensor([0.01], device=dev), 0))
        w = torch.ones_like(y).requires_grad_(True)                  # an upstream that requires grad: the second order is really asked for
        (g1,) = torch.autograd.grad((y * w).sum(), xr, create_graph=True)
        with pytest.raises(RuntimeError, match="once_differentiable|differentiated twice"):
            g1.sum().backward()
        # a shift alone that requires grad
        tr = t.clone().requires_grad_(True)
        y = tone.ldr2hdr(x * 0.1, tr)
        assert y.requires_grad
        (gt2,) = torch.autograd.grad(y.sum(), tr)
        assert tuple(gt2.shape) == tuple(t.shape) and float(gt2.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 3. the fused loss
@pytest.mark.parametrize("l2", [False, True], ids=["L1", "L2"])
@pytest.mark.parametrize("per_row", [False, True], ids=["one_shift", "row_shift"])
@pytest.mark.parametrize("curve", plo.CURVES + (plo.RATIONAL,))
@pytest.mark.parametrize("n", plo.ROWS)
def test_image_loss_parity(dev, n, curve, per_row, l2):
    from robir_amd import ops
    case, ref64, t32 = _loss_truth(n, curve, per_row, l2)
    d = _dev_case(case, dev)
    loss, g_rgb, g_shift = ops.pl_image_loss(d["sg_rgb"], d["indir_rgb"], d["gt"], d["net_mask"], d["obj_mask"], d["shift"], curve, l2)
    got = {"loss": loss.cpu(), "g_rgb": g_rgb.cpu()}
    if g_shift is not None:
        got["g_shift"] = g_shift.cpu()
    assert set(got) == set(ref64)
    assert_parity(f"image_loss/c{curve}_{'L2' if l2 else 'L1'}_{'row' if per_row else 'one'}/n{n}", got, t32, ref64)
    outside = ~(case["net_mask"] & case["obj_mask"])
    assert float(got["g_rgb"][outside].abs().max() if bool(outside.any()) else 0.0) == 0.0          # exact zeros outside the mask
    if per_row and g_shift is not None and bool(outside.any()):
        assert float(got["g_shift"][outside].abs().max()) == 0.0
    # the value alone (no gradient asked for): the same bits
    alone, no_rgb, no_shift = ops.pl_image_loss(d["sg_rgb"], d["indir_rgb"], d["gt"], d["net_mask"], d["obj_mask"], d["shift"], curve, l2,
                                                want_rgb=False, want_shift=False)
    assert no_rgb is None and no_shift is None and torch.equal(alone, loss)


def test_photometric_loss_autograd(dev):
    """training.photometric_loss: gradients to sg_rgb, indir_rgb (the same array) and adapt_illum of a marked tone, scaled by the upstream
    scalar; an unmarked tone is a constant curve; tone=None is x / (x + 1)."""
    from robir_amd import nets, training
    case, ref64, t32 = _loss_truth(257, 0, False, False)
    d = _dev_case(case, dev)
    tone = nets.ACESToneMapping(hdr_mode=0).to(dev)
    a0 = (float(case["shift"]) - 0.5) / 10
    with torch.no_grad():
        tone.adapt_illum.fill_(a0)
    sh32 = plo.as_input(torch.tensor(a0)).reshape(1)

    def oracle(dtype):
        with torch.enable_grad():
            a = torch.tensor(a0, dtype=torch.float32).to(dtype).requires_grad_(True)
            sg, ind = (case[k].to(dtype).clone().requires_grad_(True) for k in ("sg_rgb", "indir_rgb"))
            loss = 3.0 * plo.image_loss(sg, ind, case["gt"].to(dtype), case["net_mask"], case["obj_mask"], plo.as_input(a).reshape(1), 0)
            g = torch.autograd.grad(loss, [sg, ind, a])
        return {"sg_rgb": g[0], "indir_rgb": g[1], "adapt_illum": g[2]}
    with torch.enable_grad():
        sg, ind = d["sg_rgb"].clone().requires_grad_(True), d["indir_rgb"].clone().requires_grad_(True)
        loss = training.photometric_loss(sg, ind, d["gt"], d["net_mask"], d["obj_mask"], tone=tone)
        assert loss.requires_grad and loss.dim() == 0
        (3.0 * loss).backward()
        assert tone.adapt_illum.grad is None                                   # unmarked: a constant curve
        g_unmarked = sg.grad.clone()
        training.enable_tonemap_training(tone)
        sg.grad = ind.grad = None
        loss2 = training.photometric_loss(sg, ind, d["gt"], d["net_mask"], d["obj_mask"], tone=tone)
        (3.0 * loss2).backward()
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(sg.grad, g_unmarked) and torch.equal(sg.grad, ind.grad)
    assert abs(float(sh32) - float(case["shift"])) < 1e-6
    assert_parity("photometric_loss/marked", {"sg_rgb": sg.grad.cpu(), "indir_rgb": ind.grad.cpu(), "adapt_illum": tone.adapt_illum.grad.cpu()},
                  oracle(torch.float32), oracle(torch.float64))
    with torch.enable_grad():
        sg2 = d["sg_rgb"].clone().requires_grad_(True)
        fb = training.photometric_loss(sg2, None, d["gt"], d["net_mask"], d["obj_mask"], loss_type="L2")
        w = torch.ones((), device=dev).requires_grad_(True)
        (g_fb,) = torch.autograd.grad(fb * w, sg2, create_graph=True)
        with pytest.raises(RuntimeError, match="once_differentiable|differentiated twice"):
            g_fb.sum().backward()
    c2 = dict(case, indir_rgb=None, shift=None)
    r_loss, r_sg, _, _ = plo.loss_grads(c2, plo.RATIONAL, True, torch.float64)
    t_loss, t_sg, _, _ = plo.loss_grads(c2, plo.RATIONAL, True, torch.float32)
    assert_parity("photometric_loss/fallback_L2_no_indir", {"loss": fb.detach().cpu(), "sg_rgb": g_fb.detach().cpu()}, {"loss": t_loss, "sg_rgb": t_sg},
                  {"loss": r_loss, "sg_rgb": r_sg})


# ------------------------------------------------------------------------------------------------ 4. edges
def test_shift_outside_the_clamp(dev):
    """Shift 0.0 and 1.5: the shift's gradient is exactly 0 and gx comes from the clamped value (1e-4 resp. 1)."""
    from robir_amd import ops
    x, _, gy = plo.tonemap_case(257, 0, False, True)
    x, gy = x.to(dev), gy.to(dev)
    for raw, clamped in ((0.0, 1e-4), (1.5, 1.0)):
        for curve in (0, 1, 2):
            t = torch.full((257,), raw)
            t[-1] = 0.5                                                      # one row inside: its gradient is not zero
            for shift in (t, torch.tensor([raw])):
                gx, gs = ops.pl_tonemap_backward(x, shift.to(dev), curve, 0, gy)
                ref = plo.tonemap_grads(x.cpu(), torch.where(shift == raw, torch.tensor(clamped), shift), gy.cpu(), curve, False, torch.float64)[1]
                t32 = plo.tonemap_grads(x.cpu(), shift, gy.cpu(), curve, False, torch.float32)[1]
                assert_parity(f"edges/shift_{raw}/c{curve}_{shift.numel()}", {"gx": gx.cpu()}, {"gx": t32}, {"gx": ref})
                if shift.numel() == 1:
                    assert float(gs) == 0.0
                else:
                    assert float(gs[:-1].abs().max()) == 0.0 and float(gs[-1].abs()) > 0
            case = plo.loss_case(257, curve, False, False)
            d = _dev_case(dict(case, shift=torch.tensor([raw])), dev)
            _, _, g_shift = ops.pl_image_loss(d["sg_rgb"], d["indir_rgb"], d["gt"], d["net_mask"], d["obj_mask"], d["shift"], curve)
            assert float(g_shift) == 0.0


def test_l1_at_zero_distance_empty_and_full_masks_no_indir_and_n0(dev):
    from robir_amd import ops, training
    n = 300
    g = torch.Generator().manual_seed(5)
    x = (4 * torch.rand(n, 3, generator=g)).to(dev)
    ones, zeros = torch.ones(n, dtype=torch.bool, device=dev), torch.zeros(n, dtype=torch.bool, device=dev)
    one = torch.tensor([0.7], device=dev)
    # pred == gt under L1 (the identity curve; x / (x + 1) at x = 1; aces(0) = 0): gradient exactly 0, loss exactly 0
    for sg, gt, shift, curve in ((x, x, None, 3), (torch.ones_like(x), torch.full_like(x, 0.5), None, plo.RATIONAL), (torch.zeros_like(x), torch.zeros_like(x), one, 0)):
        loss, g_rgb, g_shift = ops.pl_image_loss(sg, None, gt, ones, ones, shift, curve, False)
        assert float(loss) == 0.0 and float(g_rgb.abs().max()) == 0.0 and (g_shift is None or float(g_shift) == 0.0)
    # empty mask: loss 0, zero gradients, no error -- through the kernel and through autograd
    gt = torch.rand(n, 3, generator=g).to(dev)
    for m1, m2 in ((zeros, ones), (ones, zeros)):
        loss, g_rgb, g_shift = ops.pl_image_loss(x, x, gt, m1, m2, one, 0, False)
        assert float(loss) == 0.0 and float(g_rgb.abs().max()) == 0.0 and float(g_shift) == 0.0
    with torch.enable_grad():
        xr = x.clone().requires_grad_(True)
        training.photometric_loss(xr, None, gt, zeros, ones).backward()
    assert float(xr.grad.abs().max()) == 0.0
    # all-true mask and indir_rgb=None against the oracle
    case = dict(plo.loss_case(n, 0, True, False, indir=False), net_mask=torch.ones(n, dtype=torch.bool), obj_mask=torch.ones(n, dtype=torch.bool))
    d = _dev_case(case, dev)
    loss, g_rgb, g_shift = ops.pl_image_loss(d["sg_rgb"], None, d["gt"], d["net_mask"], d["obj_mask"], d["shift"], 0, False)
    r = plo.loss_grads(case, 0, False, torch.float64)
    t = plo.loss_grads(case, 0, False, torch.float32)
    assert_parity("edges/full_mask_no_indir", {"loss": loss.cpu(), "g_rgb": g_rgb.cpu(), "g_shift": g_shift.cpu()},
                  {"loss": t[0], "g_rgb": t[1], "g_shift": t[3]}, {"loss": r[0], "g_rgb": r[1], "g_shift": r[3]})
    # N = 0
    e3, eb = torch.zeros(0, 3, device=dev), torch.zeros(0, dtype=torch.bool, device=dev)
    loss, g_rgb, g_shift = ops.pl_image_loss(e3, e3, e3, eb, eb, one, 0, False)
    assert float(loss) == 0.0 and tuple(g_rgb.shape) == (0, 3) and float(g_shift) == 0.0
    gx, gs = ops.pl_tonemap_backward(e3, one, 0, 0, e3)
    assert tuple(gx.shape) == (0, 3) and float(gs) == 0.0
    assert tuple(ops.pl_tonemap(e3, one, 0).shape) == (0, 3)
    with torch.enable_grad():
        er = e3.clone().requires_grad_(True)
        l0 = training.photometric_loss(er, None, e3, eb, eb)
        l0.backward()
    assert float(l0) == 0.0 and tuple(er.grad.shape) == (0, 3)


def test_determinism(dev):
    """Two runs of n = 70 001 with a scalar shift are bit-equal in the loss and in every gradient."""
    from robir_amd import ops
    case, _, _ = _loss_truth(70001, 0, False, False)
    d = _dev_case(case, dev)
    runs = [ops.pl_image_loss(d["sg_rgb"], d["indir_rgb"], d["gt"], d["net_mask"], d["obj_mask"], d["shift"], 0, False) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    x, t, gy, _, _ = _tm_truth(70001, 0, False, False)
    a = ops.pl_tonemap_backward(x.to(dev), t.to(dev), 0, 0, gy.to(dev))
    b = ops.pl_tonemap_backward(x.to(dev), t.to(dev), 0, 0, gy.to(dev))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ 5. default behaviour
def test_default_behaviour_is_unchanged(dev):
    """Unmarked (never marked, and marked then unmarked), under no_grad, and marked with nothing that requires grad: today's bits and
    requires_grad False."""
    from robir_amd import nets, ops, training
    tone = nets.ACESToneMapping(hdr_mode=0).to(dev)
    x = plo.tonemap_case(257, 0, False, False)[0].to(dev)
    half = torch.tensor([0.5], device=dev)
    want = ops.tonemap(x, half, 0)
    with torch.enable_grad():
        xr = x.clone().requires_grad_(True)
        y = tone.hdr2ldr(xr)
        assert not y.requires_grad and torch.equal(y, want)
        training.enable_tonemap_training(tone)
        y = tone.hdr2ldr(xr)
        assert y.requires_grad and y.grad_fn is not None and torch.equal(y.detach(), want)
        y.sum().backward()
        assert tone.adapt_illum.grad is not None and xr.grad is not None
        with torch.no_grad():
            assert not tone.hdr2ldr(xr).requires_grad
        assert not tone.hdr2ldr(x.clone().requires_grad_(False), 0.3).requires_grad        # nothing requires grad: the forward-only path
        training.enable_tonemap_training(tone, on=False)
        y = tone.hdr2ldr(xr)
        assert not y.requires_grad and torch.equal(y, want)
        assert not tone.ldr2hdr(xr * 0.1, half).requires_grad


# ------------------------------------------------------------------------------------------------ 6. the chain (fails without the feature)
@pytest.fixture(scope="module")
def model(dev):
    from robir_amd import renderer
    m = renderer.build_synthetic_model(dev, seed=0, variance=0.3)
    m.deferred_chunks = 0
    return m


def _stage3(dev, model, adapt=None):
    """The 1024-pixel chunk of the 64 x 64 synthetic view as in test_material_train_gpu's stage-3 test: the constants of one step."""
    from robir_amd import synth
    uv, pose, K = synth.synth_camera(64, 64)
    sl = slice(1024, 2048)
    inp = {"uv": torch.from_numpy(uv[sl]).to(dev)[None], "pose": torch.from_numpy(pose).to(dev)[None], "intrinsics": torch.from_numpy(K).to(dev)[None],
           "object_mask": torch.ones(1, 1024, dtype=torch.bool, device=dev), "hdr_shift": torch.full((1024, 1), 0.5, device=dev)}
    model.eval()
    first = model(inp, trainstage="Material", train_spec=True)
    hit = first["network_object_mask"].reshape(-1)
    n = int(hit.sum())
    assert 100 <= n
    points, view_dirs = first["points"][hit].contiguous(), (-first["ray_dirs"][hit]).contiguous()
    dr = {k: torch.from_numpy(v).to(dev) for k, v in synth.pbr_draws(7, n, chunk_id=1).items()}
    indir_sgs, indir_int = model.indirect_illum_network(points, torch.full((n, 1), 0.5, device=dev), noise=dr["illum_randn"])
    g = torch.Generator().manual_seed(9)
    gt = torch.rand(1, 1024, 3, generator=g).to(dev)
    obj = (torch.rand(1024, generator=g) < 0.9).to(dev)
    return dict(first=first, hit=hit, n=n, points=points, view=view_dirs / (torch.norm(view_dirs, dim=-1, keepdim=True) + 1e-6), dr=dr,
                indir_sgs=indir_sgs, indir_int=indir_int, gt=gt, obj=obj)


def _stage3_forward(model, S):
    """One differentiable stage-3 forward (grad mode is the caller's) -> the model-output dict InvLoss reads, full [1024, .] rows."""
    from robir_amd import sg_render
    mat_net, dr, hit = model.envmap_material_network, S["dr"], S["hit"]
    mat = mat_net(S["points"], train_spec=True, noise={"spec": dr["spec_randn"], "normal": dr["normal_randn"]})
    nrm = mat["sg_normal_map"].detach()
    out = sg_render.render_with_all_sg(points=S["points"].detach(), normal=nrm, viewdirs=S["view"], lgtSGs=mat["sg_lgtSGs"],
                                       indir_integral=S["indir_int"] * 2 * np.pi, specular_reflectance=mat["sg_specular_reflectance"].abs(),
                                       roughness=mat["sg_roughness"], diffuse_albedo=mat["sg_diffuse_albedo"], indir_lgtSGs=S["indir_sgs"],
                                       VisModel=model.visibility_network, fun_spec=False, lin_diff=False, testing=False, metallic=None, draws=dr)

    def full(v):          # the renderer's scatter of the hit rows into the chunk's rows
        buf = torch.zeros(1024, v.shape[-1], device=v.device)
        return buf.index_put((hit.nonzero()[:, 0],), v)
    return {"sg_rgb": full(out["sg_rgb"]), "indir_rgb": full(out["indir_rgb"]), "network_object_mask": hit, "object_mask": S["obj"],
            "points": S["first"]["points"], "diffuse_albedo": mat["sg_diffuse_albedo"], "roughness": mat["sg_roughness"],
            "random_xi_diffuse_albedo": mat["random_xi_diffuse_albedo"], "random_xi_roughness": mat["random_xi_roughness"],
            "surface_mask": hit, "normal_map": full(nrm), "normals": S["first"]["normals"].detach()}


def test_chain_from_the_image_to_every_stage3_parameter(dev, model, synth_weights):
    """InvLoss(...).forward(out, {"rgb": gt}, hdr_fn=model.gamma.hdr_shift.hdr2ldr)["loss"].backward() reaches every spec-auto-encoder
    tensor, lgtSGs, specular_reflectance and adapt_illum.  Those gradients equal the ones obtained by feeding the float64 oracle's
    d loss / d sg_rgb, d loss / d indir_rgb into torch.autograd.backward of the same forward's outputs; adapt_illum.grad is compared with the
    oracle directly."""
    from robir_amd import loss as rloss, training
    S = _stage3(dev, model)
    mat_net, tone = model.envmap_material_network, model.gamma.hdr_shift
    crit = rloss.InvLoss(idr_rgb_weight=0.0, eikonal_weight=0.0, mask_weight=0.0, alpha=50.0, sg_rgb_weight=1.0, kl_weight=0.01,
                         latent_smooth_weight=0.1)
    a0 = float(tone.adapt_illum.detach())
    names = [k for k, _ in mat_net.named_parameters() if k.startswith("spec_brdf_encoder_layer.") or k in ("lgtSGs", "specular_reflectance")]
    params = dict(mat_net.named_parameters())
    try:
        mat_net.train()
        training.enable_material_training(model)
        assert training.enable_tonemap_training(model) is tone
        with torch.no_grad():
            tone.adapt_illum.fill_(0.013)                                       # as_input() = 0.63: inside the clamp
        with torch.enable_grad():
            out = _stage3_forward(model, S)
            res = crit.forward(out, {"rgb": S["gt"]}, mat_model=mat_net, train_spec=True, hdr_fn=tone.hdr2ldr)
            assert set(res) == {"sg_rgb_loss", "kl_loss", "latent_smooth_loss", "normal_loss", "loss"}
            assert res["loss"].requires_grad and res["kl_loss"].requires_grad and res["latent_smooth_loss"].requires_grad
            res["loss"].backward(retain_graph=True)
            kernel = {k: params[k].grad.detach().cpu().clone() for k in names}
            kernel["adapt_illum"] = tone.adapt_illum.grad.detach().cpu().clone()
            for k, g in kernel.items():
                assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
            # the oracle's image gradients pushed through the SAME forward's graph
            case = dict(sg_rgb=out["sg_rgb"].detach().cpu(), indir_rgb=out["indir_rgb"].detach().cpu(), gt=S["gt"].reshape(-1, 3).cpu(),
                        net_mask=S["hit"].cpu(), obj_mask=S["obj"].cpu(), shift=None)
            chained = {}
            for dtype in (torch.float64, torch.float32):
                with torch.enable_grad():
                    a = torch.tensor(0.013, dtype=torch.float32).to(dtype).requires_grad_(True)
                    sg, ind = (case[k].to(dtype).clone().requires_grad_(True) for k in ("sg_rgb", "indir_rgb"))
                    l = plo.image_loss(sg, ind, case["gt"].to(dtype), case["net_mask"], case["obj_mask"], plo.as_input(a).reshape(1), 0)
                    g_sg, g_ind, g_a = torch.autograd.grad(l, [sg, ind, a])
                mat_net.zero_grad(set_to_none=True)
                torch.autograd.backward([out["sg_rgb"], out["indir_rgb"]], [g_sg.float().to(dev), g_ind.float().to(dev)], retain_graph=True)
                chained[dtype] = {k: params[k].grad.detach().cpu().clone() for k in names}
                chained[dtype]["adapt_illum"] = g_a.reshape(())
                chained[dtype]["loss"] = l.detach()
        kernel["loss"] = res["sg_rgb_loss"].detach().cpu()
        record_metric("photoloss/chain/loss", hip=float(kernel["loss"]), oracle64=float(chained[torch.float64]["loss"]))
        assert_parity("chain", kernel, chained[torch.float32], chained[torch.float64])
    finally:
        training.enable_material_training(model, on=False)
        training.enable_tonemap_training(model, on=False)
        mat_net.zero_grad(set_to_none=True)
        tone.zero_grad(set_to_none=True)
        with torch.no_grad():
            tone.adapt_illum.fill_(a0)
        model.eval()


def test_other_hdr_fn_and_the_fallback(dev, model):
    """InvLoss.forward's three branches on one model-output dict of the synthetic chunk: hdr_fn=None is the reference's x / (x + 1); a
    callable that is not an ACESToneMapping's hdr2ldr is applied as given and followed by the fused masked distance; the bound hdr2ldr
    takes the fused path with the module's own shift.  Values and d loss / d sg_rgb against the oracle."""
    from robir_amd import loss as rloss
    S = _stage3(dev, model)
    mat_net, tone = model.envmap_material_network, model.gamma.hdr_shift
    base = _stage3_forward(model, S)                                            # no_grad (conftest): constants
    sg0, ind0 = base["sg_rgb"].cpu(), base["indir_rgb"].cpu()
    gt, hit, obj = S["gt"].reshape(-1, 3).cpu(), S["hit"].cpu(), S["obj"].cpu()
    shift = tone.as_input().reshape(1).cpu()
    branches = {"none": (None, lambda x, dt: plo.curve_fn(x, None, plo.RATIONAL)),
                "callable": (lambda v: v * 0.25 + 0.125, lambda x, dt: x * 0.25 + 0.125),
                "aces": (tone.hdr2ldr, lambda x, dt: plo.tonemap(x, shift.to(dt), 0))}
    for l2 in (False, True):
        crit = rloss.InvLoss(0.0, 0.0, 0.0, 50.0, 2.0, 0.01, 0.1, loss_type="L2" if l2 else "L1")
        for name, (hdr_fn, curve) in branches.items():
            with torch.enable_grad():
                sg = base["sg_rgb"].clone().requires_grad_(True)
                res = crit.forward(dict(base, sg_rgb=sg), {"rgb": S["gt"]}, mat_model=mat_net, train_spec=True, hdr_fn=hdr_fn)
                (g_sg,) = torch.autograd.grad(res["loss"], sg)
            assert float(res["loss"]) == 2.0 * float(res["sg_rgb_loss"])
            want = {}
            for dt in (torch.float64, torch.float32):
                with torch.enable_grad():
                    x = sg0.to(dt).clone().requires_grad_(True)
                    d = curve(x + ind0.to(dt), dt)[hit & obj] - gt.to(dt)[hit & obj]
                    l = ((d * d).sum() if l2 else d.abs().sum()) / 1024.0
                    (gx,) = torch.autograd.grad(2.0 * l, x)
                want[dt] = {"sg_rgb_loss": l.detach(), "d_sg_rgb": gx}
            assert_parity(f"invloss_forward/{name}_{'L2' if l2 else 'L1'}", {"sg_rgb_loss": res["sg_rgb_loss"].detach().cpu(), "d_sg_rgb": g_sg.cpu()},
                          want[torch.float32], want[torch.float64])


def test_kl_illum_and_query_values(dev, model):
    """What no other test reads: InvLoss.get_kl_loss (both auto-encoders) against training.kl_sparsity on the same latent and against the
    formula in float64; loss.query_indir_illum and IllumLoss.forward (L1 and L2) against model/loss.py:128-179 written out in float64.
    1e-5: sums of at most a few thousand fp32 terms."""
    from robir_amd import loss as rloss, ops, training
    g = torch.Generator().manual_seed(21)
    mat_net = model.envmap_material_network
    crit = rloss.InvLoss(0.0, 0.0, 0.0, 50.0, 1.0, 0.01, 0.1)
    pts = (0.5 * torch.randn(200, 3, generator=g)).to(dev)
    for train_spec, layer in ((True, mat_net.spec_brdf_encoder_layer), (False, mat_net.brdf_encoder_layer)):
        raw = layer.encode(ops.feat_pe10(pts)[:, :63])
        got = crit.get_kl_loss(mat_net, pts, train_spec)
        assert torch.equal(got, training.kl_sparsity(raw, 0.05))
        rho_hat = torch.sigmoid(raw.double().cpu()).mean(0)
        want = (0.05 * torch.log(0.05 / (rho_hat + 1e-4)) + 0.95 * torch.log(0.95 / (1 - rho_hat + 1e-4))).mean()
        assert rel_err(got.cpu(), want) <= 1e-5, train_spec
    N, S, L = 64, 16, 24
    hit = torch.rand(N, generator=g) < 0.7
    n = int(hit.sum())
    sgs = torch.randn(N, L, 7, generator=g)
    sgs[..., 3] = sgs[..., 3].abs() * 5
    sgs[..., 4:] = sgs[..., 4:].abs()
    dirs = torch.nn.functional.normalize(torch.randn(n, S, 3, generator=g), dim=-1)
    indir = torch.zeros(N, S, dtype=torch.bool)
    indir[hit] = torch.rand(n, S, generator=g) < 0.5
    tr = {"indir_mask": indir, "trace_radiance": torch.rand(N, S, 3, generator=g), "sample_dirs": dirs, "gt_integral": torch.rand(N, 3, generator=g),
          "gt_vis": torch.rand(N, S, 1, generator=g) < 0.5, "pred_vis": torch.randn(N, S, 2, generator=g)}
    mo = {"network_object_mask": hit, "indirect_sgs": sgs, "indir_integral": torch.rand(N, 3, generator=g)}
    D = lambda d: {k: v.to(dev) for k, v in d.items()}

    def query64(lgt, d):                                                        # sum_j mu_j exp(lambda_j (d . l_j / |l_j| - 1))
        lgt, d = lgt.double(), d.double()
        axis = lgt[..., :3] / lgt[..., :3].norm(dim=-1, keepdim=True)
        cos = torch.einsum("nsk,nlk->nsl", d, axis)
        return torch.einsum("nsl,nlc->nsc", torch.exp(lgt[:, None, :, 3] * (cos - 1)), lgt[..., 4:])
    pred64 = query64(sgs[hit], dirs)
    assert rel_err(rloss.query_indir_illum(sgs[hit].to(dev), dirs.to(dev)).cpu(), pred64) <= 1e-5
    for loss_type in ("L1", "L2"):
        dist = (lambda a, b: (a - b).abs().mean()) if loss_type == "L1" else (lambda a, b: ((a - b) ** 2).mean())
        rad, vis = rloss.IllumLoss(loss_type).forward(D(mo), D(tr), 0.03)
        want_rad = dist(pred64[indir[hit]], tr["trace_radiance"].double()[indir] + 0.03) + dist(mo["indir_integral"].double()[hit], tr["gt_integral"].double()[hit])
        logits = tr["pred_vis"].double()[hit].reshape(-1, 2)
        cls = (~tr["gt_vis"][hit]).reshape(-1).long()
        want_vis = (torch.logsumexp(logits, 1) - logits.gather(1, cls[:, None])[:, 0]).mean()
        assert rel_err(rad.cpu(), want_rad) <= 1e-5 and rel_err(vis.cpu(), want_vis) <= 1e-5, loss_type


# ------------------------------------------------------------------------------------------------ 7. a short fit
def test_short_fit_lowers_the_loss_and_the_cached_shift_follows(dev, model):
    """Five Adam steps on adapt_illum and lgtSGs from a perturbed shift lower the loss monotonically; after a step the forward-only
    hdr2ldr (the cached shift) sees the new as_input()."""
    from robir_amd import loss as rloss, ops, training
    S = _stage3(dev, model)
    mat_net, tone = model.envmap_material_network, model.gamma.hdr_shift
    crit = rloss.InvLoss(0.0, 0.0, 0.0, 50.0, 1.0, 0.01, 0.1)
    a0, l0 = float(tone.adapt_illum.detach()), mat_net.lgtSGs.detach().clone()
    x = plo.tonemap_case(86, 0, False, False)[0].to(dev)
    try:
        mat_net.train()
        training.enable_material_training(model)
        training.enable_tonemap_training(model)
        first = _stage3_forward(model, S)                                       # no_grad (conftest): the forward-only path
        target = tone.hdr2ldr(first["sg_rgb"] + first["indir_rgb"]).reshape(1, 1024, 3)
        with torch.no_grad():
            tone.adapt_illum.fill_(0.03)                                        # as_input() 0.5 -> 0.8
        opt = torch.optim.Adam([tone.adapt_illum, mat_net.lgtSGs], lr=1e-3)
        losses = []
        for step in range(6):
            before = tone.hdr2ldr(x)                                            # no_grad (conftest): the cached, forward-only path
            assert torch.equal(before, ops.tonemap(x, tone.as_input().reshape(1), 0))
            with torch.enable_grad():
                opt.zero_grad()
                out = _stage3_forward(model, S)
                loss = crit.forward(out, {"rgb": target}, mat_model=mat_net, train_spec=True, hdr_fn=tone.hdr2ldr)["loss"]
                loss.backward()
            losses.append(float(loss.detach()))
            if step < 5:
                opt.step()
        record_metric("photoloss/fit", **{f"hip_{i}": v for i, v in enumerate(losses)})
        print("photoloss fit", " ".join(f"{v:.5e}" for v in losses))
        assert all(b < a for a, b in zip(losses, losses[1:])), losses
    finally:
        training.enable_material_training(model, on=False)
        training.enable_tonemap_training(model, on=False)
        mat_net.zero_grad(set_to_none=True)
        tone.zero_grad(set_to_none=True)
        with torch.no_grad():
            tone.adapt_illum.fill_(a0)
            mat_net.lgtSGs.copy_(l0)
        model.eval()
