"""The light-SG fit on the device (librobir_hip_lightfit.so, robir_amd/lightfit.py, robir_amd/fit_light.py) against the float64
PyTorch-CPU oracle tests/lightfit_oracle.py.

The parity rule is DESIGN 4.3's: e_kernel <= max(2 e_torch, 1e-5), e = conftest.rel_err against the float64 evaluation, e_torch = the
distance of the fp32 PyTorch-CPU evaluation of the same thing from the float64 one, measured here.  Every compared pair is recorded under
lightfit/*."""
import ctypes
import functools
import os
import shutil

import numpy as np
import pytest
import torch

import lightfit_oracle as lfo
from conftest import GOLD, record_metric, rel_err

pytestmark = pytest.mark.gpu
FLOOR = 1e-5
c_long, c_int, c_double = ctypes.c_long, ctypes.c_int, ctypes.c_double
EXR_CROP = os.path.join(GOLD, "envmap6_rows0_31.exr")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def parity(name, got, ref64, ref32):
    e, e_torch = rel_err(got, ref64), rel_err(ref32, ref64)
    record_metric("lightfit/" + name, e=e, e_torch=e_torch, bound=max(2 * e_torch, FLOOR))
    print(f"lightfit/{name}: e {e:.2e}  e_torch {e_torch:.2e}")
    assert e <= max(2 * e_torch, FLOOR), (name, e, e_torch)


@functools.lru_cache(maxsize=None)
def case(name):
    return lfo.make_case(name)


@functools.lru_cache(maxsize=None)
def oracle_fit(name, steps, dtype):
    c = case(name)
    return lfo.fit(c["lgt"], c["dirs"], c["target"], steps, dtype)


def fit_steps(dev, c, steps, calls=1):
    """rb_lf_fit_steps on a case from zero moments: `steps` steps in `calls` equal calls -> parameters, moments (CPU fp32), losses (float64)."""
    from robir_amd import _lib
    from robir_amd._lib import ptr
    lgt, dirs, target = (c[k].to(dev).clone().contiguous() for k in ("lgt", "dirs", "target"))
    M, n = lgt.shape[0], dirs.shape[0]
    m, v = torch.zeros_like(lgt), torch.zeros_like(lgt)
    need = _lib.lightfit().rb_lf_scratch_bytes(c_long(n), c_int(M))
    scratch = torch.empty(need // 8, dtype=torch.float64, device=dev)
    hist = torch.full((steps,), float("nan"), dtype=torch.float64, device=dev)
    per = steps // calls
    for i in range(calls):
        _lib.call_lightfit("rb_lf_fit_steps", ptr(lgt), ptr(m), ptr(v), c_int(M), ptr(dirs), ptr(target), c_long(n), c_long(i * per), c_long(per),
                           c_double(1e-2), c_double(0.9), c_double(0.999), c_double(1e-8), ctypes.c_void_p(hist.data_ptr() + 8 * i * per),
                           ptr(scratch), c_long(need), _lib.stream_ptr())
    torch.cuda.synchronize()
    return lgt.cpu(), m.cpu(), v.cpu(), hist.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ 1. backward parity
@pytest.mark.parametrize("name", list(lfo.CASES))
def test_backward_parity(dev, name):
    """rb_lf_envmap_sg_bwd with a random upstream against float64 autograd; twice, bit-identical."""
    from robir_amd import lightfit
    c = case(name)
    D = lambda k: c[k].to(dev)
    got = lightfit.envmap_sg_backward(D("lgt"), D("dirs"), D("g_rgb")).cpu()
    again = lightfit.envmap_sg_backward(D("lgt"), D("dirs"), D("g_rgb")).cpu()
    assert torch.equal(got, again)
    g64 = lfo.backward(c["lgt"], c["dirs"], c["g_rgb"])
    g32 = lfo.backward(c["lgt"], c["dirs"], c["g_rgb"], torch.float32)
    parity(f"{name}/backward", got, g64, g32)
    if name == "signs":
        assert float(got[2, 5]) == 0.0 and float(g64[2, 5]) == 0.0          # mu_raw exactly 0: sign 0, as torch.abs


@pytest.mark.parametrize("upper_hemi", [False, True])
@pytest.mark.parametrize("name", ["12x20x130", "16x32x24", "signs", "norms"])
def test_backward_through_compute_envmap(dev, name, upper_hemi):
    """lightfit.compute_envmap(...).backward(): the forward is the existing kernel's, bit for bit; the gradient is float64 autograd's."""
    from robir_amd import lightfit, sg_render
    c = case(name)
    H, W = c["H"], c["W"]
    dirs = lfo.envmap_dirs(H, W, upper_hemi)
    G = c["g_rgb"].reshape(H, W, 3)
    with torch.enable_grad():
        lgt = c["lgt"].to(dev).clone().requires_grad_()
        out = lightfit.compute_envmap(lgt, H, W, upper_hemi)
        assert out.requires_grad and tuple(out.shape) == (H, W, 3)
        (out * G.to(dev)).sum().backward()
    plain = sg_render.compute_envmap(c["lgt"].to(dev), H, W, upper_hemi)
    assert torch.equal(out.detach(), plain)
    assert torch.equal(lightfit.compute_envmap(c["lgt"].to(dev), H, W, upper_hemi), plain)          # grad mode off / nothing requires grad
    with torch.enable_grad():
        assert not lightfit.compute_envmap(c["lgt"].to(dev), H, W, upper_hemi).requires_grad
    tag = f"{name}/compute_envmap_backward" + ("_upper" if upper_hemi else "")
    parity(tag, lgt.grad.cpu(), lfo.backward(c["lgt"], dirs, c["g_rgb"]), lfo.backward(c["lgt"], dirs, c["g_rgb"], torch.float32))


# ------------------------------------------------------------------------------------------------------------ 2. one step
@pytest.mark.parametrize("name", list(lfo.CASES))
def test_one_step(dev, name):
    c = case(name)
    p, m, v, h = fit_steps(dev, c, 1)
    p64, m64, v64, h64 = lfo.fit(c["lgt"], c["dirs"], c["target"], 1)
    p32, m32, v32, h32 = lfo.fit(c["lgt"], c["dirs"], c["target"], 1, torch.float32)
    parity(f"{name}/step1/loss", h, h64, h32)
    parity(f"{name}/step1/parameters", p, p64, p32)
    parity(f"{name}/step1/exp_avg", m, m64, m32)
    parity(f"{name}/step1/exp_avg_sq", v, v64, v32)


# ------------------------------------------------------------------------------------------------------------ 3. trajectory, 5. determinism
@pytest.mark.parametrize("name", lfo.TRAJECTORY_CASES)
def test_trajectory(dev, name):
    """50 steps against the float64 loop from the same init: the parameters and every entry of loss_hist; 50 steps in one call equal 5 calls
    of 10 with first_step advanced, bit for bit; two runs give identical bytes."""
    c = case(name)
    p, m, v, h = fit_steps(dev, c, 50)
    p64, m64, v64, h64 = oracle_fit(name, 50, torch.float64)
    p32, m32, v32, h32 = oracle_fit(name, 50, torch.float32)
    parity(f"{name}/steps50/parameters", p, p64, p32)
    parity(f"{name}/steps50/loss_hist", h, h64, h32)
    parity(f"{name}/steps50/exp_avg", m, m64, m32)
    parity(f"{name}/steps50/exp_avg_sq", v, v64, v32)
    for what, other in (("5 calls of 10", fit_steps(dev, c, 50, calls=5)), ("a second run", fit_steps(dev, c, 50))):
        assert torch.equal(other[0], p) and torch.equal(other[1], m) and torch.equal(other[2], v), what
        assert other[3].tobytes() == h.tobytes(), what


# ------------------------------------------------------------------------------------------------------------ 4. descent, independent forward
def test_descent_and_the_independent_forward(dev):
    """fit_envmap at 32 x 64, M = 32 on a 128-lobe target, 300 steps: the last loss is below 0.1 x the first (a condition: the float64 loop
    reaches 0.042 x, the first loss is 0.186), and the MSE of the EXISTING forward kernel (sg_render.compute_envmap) on the fitted lobes
    equals the loss the fused step reports next."""
    from robir_amd import lightfit, sg_render
    c = lfo.make_case("descent", 32, 64, 32, 128)
    env = c["target"].reshape(32, 64, 3)
    seen, state = [], {}
    lgt, hist = lightfit.fit_envmap(env, num_sg=32, iters=300, size=(32, 64), seed=5, block=100, callback=lambda s, l, p: seen.append((s, l)),
                                    state=state)
    assert torch.equal(lightfit.init_light_sgs(32, 5), c["lgt"])
    assert hist.shape == (300,) and hist.dtype == np.float64 and np.isfinite(hist).all()
    assert [s for s, _ in seen] == [100, 200, 300] and [l for _, l in seen] == [hist[99], hist[199], hist[299]] and state["step"] == 300
    record_metric("lightfit/descent", first=hist[0], last=hist[-1], ratio=hist[-1] / hist[0])
    print(f"lightfit/descent: loss {hist[0]:.4g} -> {hist[-1]:.4g} ({hist[-1] / hist[0]:.3f} x)")
    assert hist[-1] < 0.1 * hist[0]
    fitted = lgt.clone()
    _, nxt = lightfit.fit_envmap(env, num_sg=32, iters=1, size=(32, 64), init=fitted, state=dict(state))
    assert torch.equal(lgt, fitted)                                                     # fit_envmap works on a copy of init
    mse = lambda img, dt: float(((img.cpu().to(dt) - env.to(dt)) ** 2).mean())
    fwd = sg_render.compute_envmap(fitted, 32, 64)
    loss64, _ = lfo.loss_and_grad(fitted.cpu(), c["dirs"], c["target"])
    loss32, _ = lfo.loss_and_grad(fitted.cpu(), c["dirs"], c["target"], torch.float32)
    parity("descent/next_loss", nxt[0], loss64, loss32)
    parity("descent/forward_kernel_mse", mse(fwd, torch.float64), loss64, loss32)
    # the two figures against each other, under the same rule
    e, e_torch = rel_err(mse(fwd, torch.float64), nxt[0]), rel_err(loss32, loss64)
    record_metric("lightfit/descent/forward_kernel_mse_vs_next_loss", e=e, e_torch=e_torch)
    assert e <= max(2 * e_torch, FLOOR), (e, e_torch)


def test_non_finite_loss_is_reported(dev):
    from robir_amd import lightfit
    c = case("16x32x8")
    env = c["target"].reshape(16, 32, 3).clone()
    env[3, 4, 1] = float("inf")
    calls = []
    with pytest.raises(FloatingPointError, match="step 0") as e:
        lightfit.fit_envmap(env, num_sg=8, iters=4, size=(16, 32), seed=5, block=2, callback=lambda *a: calls.append(a))
    assert not calls and e.value.step == 0 and torch.equal(e.value.lgtSGs.cpu(), c["lgt"])


# ------------------------------------------------------------------------------------------------------------ 6. area resize
@functools.lru_cache(maxsize=None)
def exr_crop():
    from robir_amd.exr import read_exr
    img = np.ascontiguousarray(read_exr(EXR_CROP)[:, :, :3], dtype=np.float32)
    assert img.shape[0] >= 16 and img.shape[1] >= 32
    return img


@pytest.mark.parametrize("src,dst", [((16, 32), (8, 16)), ((15, 31), (4, 7)), ((16, 32), (16, 32)), ((16, 32), (1, 1)), ((15, 31), (15, 7))])
def test_area_resize(dev, src, dst):
    from robir_amd import lightfit
    img = exr_crop()[:src[0], :src[1]]
    got = lightfit.area_resize(img, *dst)
    assert got.dtype == torch.float32 and tuple(got.shape) == (*dst, 3) and got.is_cuda
    ref64 = lfo.area_resize(img, *dst)
    ref32 = np.einsum("yj,jqc,xq->yxc", lfo._overlap(src[0], dst[0]).astype(np.float32), img, lfo._overlap(src[1], dst[1]).astype(np.float32))
    parity(f"area_resize/{src[0]}x{src[1]}_to_{dst[0]}x{dst[1]}", got.cpu().numpy(), ref64, ref32)
    if src == dst:
        assert np.array_equal(got.cpu().numpy(), img)                                   # the identity, bit for bit
    if src == (16, 32) and dst == (8, 16):
        assert rel_err(ref64, img.astype(np.float64).reshape(8, 2, 16, 2, 3).mean((1, 3))) <= 1e-14          # the reshape-mean
    assert torch.equal(lightfit.area_resize(torch.from_numpy(img), *dst), got)          # a torch tensor or a numpy array


def test_area_resize_keeps_a_constant_and_refuses_to_enlarge(dev):
    from robir_amd import _lib, lightfit
    const = np.full((15, 31, 3), np.float32(0.7))
    got = lightfit.area_resize(const, 4, 7).cpu().numpy().astype(np.float64)
    assert np.abs(got - np.float64(np.float32(0.7))).max() <= np.spacing(np.float32(0.7))          # one fp32 rounding
    with pytest.raises(_lib.RobirHipError, match="up-sampling refused"):
        lightfit.area_resize(const, 16, 31)


# ------------------------------------------------------------------------------------------------------------ 7. command line
def test_cli(dev, tmp_path, capsys):
    from robir_amd import fit_light, lightfit
    c = case("16x32x8")
    env = c["target"].reshape(16, 32, 3).numpy()
    path = str(tmp_path / "mymap.npy")
    np.save(path, env)
    res = fit_light.main(["--envmap", path, "--iters", "20", "--size", "16", "32", "--num_sg", "8", "--block", "10"])
    sg_file = str(tmp_path / "mymap" / "sg_8.npy")
    assert res["sg_file"] == sg_file and res["step"] == 20
    sg = np.load(sg_file)
    assert sg.dtype == np.float32 and sg.shape == (8, 7)
    ref, hist = lightfit.fit_envmap(env, num_sg=8, iters=20, size=(16, 32), seed=0, block=10)
    assert np.array_equal(sg, ref.cpu().numpy()) and np.array_equal(res["loss"], hist)
    out = capsys.readouterr().out
    assert "step: 10, loss:" in out and "step: 20, loss:" in out
    # --resume continues from the files: the step count goes on from 20, and 20 + 10 steps are 30 steps
    res2 = fit_light.main(["--envmap", path, "--iters", "10", "--size", "16", "32", "--num_sg", "8", "--resume"])
    assert res2["step"] == 30 and "at step 20" in capsys.readouterr().out
    ref30, hist30 = lightfit.fit_envmap(env, num_sg=8, iters=30, size=(16, 32), seed=0, block=30)
    assert np.array_equal(np.load(sg_file), ref30.cpu().numpy()) and np.array_equal(res2["loss"], hist30[20:])
    # from sg_8.npy alone (what the reference's fits are): fresh moments, step 0
    os.remove(str(tmp_path / "mymap" / "fit_8.npz"))
    res3 = fit_light.main(["--envmap", path, "--iters", "5", "--size", "16", "32", "--num_sg", "8", "--resume"])
    assert res3["step"] == 5 and "fresh moments" in capsys.readouterr().out
    # what render --light / load_light read
    assert np.load(sg_file).shape == (8, 7)


def test_cli_on_an_exr(dev, tmp_path):
    from robir_amd import fit_light
    path = str(tmp_path / "crop.exr")
    shutil.copyfile(EXR_CROP, path)
    res = fit_light.main(["--envmap", path, "--iters", "60", "--size", "8", "64", "--num_sg", "8", "--block", "30", "--seed", "1"])
    loss = res["loss"]
    assert loss.shape == (60,) and np.isfinite(loss).all() and loss[-1] < loss[0]
    record_metric("lightfit/cli_exr", first=loss[0], last=loss[-1])
    sg = np.load(str(tmp_path / "crop" / "sg_8.npy"))
    assert sg.dtype == np.float32 and sg.shape == (8, 7) and np.isfinite(sg).all()
