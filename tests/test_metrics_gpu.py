"""Image metrics on the GPU: rb_mt_pair_stats / rb_mt_angular_stats / rb_mt_ssim (librobir_hip_metrics.so), robir_amd/metrics.py and
robir_amd/evaluate.py against the float64 numpy oracle of tests/metrics_oracle.py, fed the same fp32 inputs.

Bounds:
  * every SSIM map entry: absolute 1e-5 -- the floor of the project's rule e_kernel <= max(2 e_torch, 1e-5) WITHOUT its 2 e_torch branch:
    here e_torch, the error of the fp32 PyTorch restatement, is the defect being avoided (asserted to exceed 1e-4 on the flat-bright pair);
  * every per-view sum and mean: relative 1e-9 -- an fp64 sum of at most 70 001 terms in another order (eps 1.1e-16 times the term count
    bounds it by 7.8e-12 of the sum of magnitudes) plus the device's pow / acos against numpy's (a few ulp per term);
  * counts, zeros at windows that are not counted, SSIM(x, x) == 1, determinism: exact.
Every (case, e_kernel, e_torch) is recorded (conftest.record_metric, names metrics/...; profiles/metrics_test_metrics.jsonl keeps the MI355X
run).  Shapes: with the SSIM tile T = 16 and R = 256 rows per workgroup, the smallest at which a kernel takes another path."""
import json

import numpy as np
import pytest
import torch

import metrics_oracle as mo
from conftest import record_metric

pytestmark = pytest.mark.gpu
T, R = mo.TILE, mo.ROWS
TOL_MAP, TOL_SUM = 1e-5, 1e-9
SSIM_SHAPES = [(11, 11), (11, 12), (T + 10, T + 10), (T + 11, T + 10 + 3), (45, 53)]
ROWS = [1, R - 1, R, R + 1, 70001]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _record(tag, e_kernel, e_torch, bound):
    record_metric(f"metrics/{tag}", e_kernel=e_kernel, e_torch=e_torch, bound=bound)
    print(f"{tag:56s} e_kernel {e_kernel:.2e}  e_torch {e_torch:.2e}  (bound {bound:.0e})")


_REF = {}


def _ssim_truth(kind, V, H, W, C, masked=True, t=mo.NONE):
    """The case and the oracle's (count, sum, map), computed once and shared; never modified."""
    key = (kind, V, H, W, C, masked, t)
    if key not in _REF:
        p, g = mo.images(kind, V, H, W, C)
        m = mo.masks(V, H, W) if masked else None
        _REF[key] = (p, g, m) + mo.ssim(p, g, m, t)
    return _REF[key]


def _check_ssim(tag, dev, p, g, m, n_ref, s_ref, map_ref, t=mo.NONE, scale=None, e_torch=-1.0):
    from robir_amd import metrics
    V, H, W, C = p.shape
    mean, out = metrics.ssim(_t(p, dev), _t(g, dev), None if m is None else _t(m, dev), t, scale, return_map=True)
    n, s, _ = metrics.ssim_stats(_t(p, dev), _t(g, dev), None if m is None else _t(m, dev), t, scale)
    out, n, s, mean = out.cpu().numpy(), n.cpu().numpy(), s.cpu().numpy(), mean.cpu().numpy()
    assert out.shape == (V, H - 10, W - 10, C) and out.dtype == np.float32 and mean.dtype == np.float64
    e_map = float(np.abs(out.astype(np.float64) - map_ref).max())
    _record(f"ssim/{tag}/map", e_map, e_torch, TOL_MAP)
    assert e_map <= TOL_MAP, (tag, e_map)
    assert np.array_equal(n, n_ref), (tag, n, n_ref)
    e_sum = mo.rel(s, s_ref)
    counted = n_ref > 0
    e_mean = mo.rel(mean[counted], s_ref[counted] / (n_ref[counted] * C))
    _record(f"ssim/{tag}/sum", e_sum, -1.0, TOL_SUM)
    _record(f"ssim/{tag}/mean", e_mean, -1.0, TOL_SUM)
    assert e_sum <= TOL_SUM and e_mean <= TOL_SUM, (tag, e_sum, e_mean)
    assert bool(np.isnan(mean[~counted]).all())                         # no counted window: 0 / 0
    if m is not None:
        off = ~np.asarray(m)[:, 5:H - 5, 5:W - 5]
        assert not out[off].any() and not np.signbit(out[off]).any(), tag          # exact (positive) zeros where no window is counted
    return out


# ------------------------------------------------------------------------------------------------ SSIM
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", SSIM_SHAPES)
def test_ssim_noise_against_the_oracle(dev, H, W, C, V):
    """Uniform noise with a different mask per view: view 1 is empty and view 2 has a single centre (V = 3)."""
    p, g, m, n, s, ref = _ssim_truth("noise", V, H, W, C)
    e32 = float(np.abs(np.stack([mo.ssim_f32_torch(p[v], g[v]) for v in range(V)]) * m[:, 5:H - 5, 5:W - 5, None] - ref).max())
    _check_ssim(f"noise_{H}x{W}x{C}_V{V}", dev, p, g, m, n, s, ref, e_torch=e32)
    if V == 3:
        assert n[1] == 0 and n[2] == 1


@pytest.mark.parametrize("kind", ["smooth", "flat"])
@pytest.mark.parametrize("H,W", [(T + 11, T + 10 + 3), (45, 53)])
def test_ssim_smooth_and_flat_bright(dev, kind, H, W):
    """The smooth sine pair and the flat-bright pair (mean 0.9, noise 1e-3): the fp32 PyTorch restatement of the latter is more than 1e-4
    off on the same input, the kernel holds 1e-5 on every entry."""
    p, g, _, n, s, ref = _ssim_truth(kind, 3, H, W, 3, masked=False)
    e32 = float(np.abs(np.stack([mo.ssim_f32_torch(p[v], g[v]) for v in range(3)]) - ref).max())
    _check_ssim(f"{kind}_{H}x{W}x3_V3", dev, p, g, None, n, s, ref, e_torch=e32)
    if kind == "flat":
        assert e32 > 1e-4, e32
    p, g, m, n, s, ref = _ssim_truth(kind, 3, H, W, 3)
    _check_ssim(f"{kind}_{H}x{W}x3_V3_masked", dev, p, g, m, n, s, ref)


def test_ssim_of_an_image_with_itself_is_exactly_one(dev):
    from robir_amd import metrics
    p, _ = mo.images("noise", 2, 45, 53, 3)
    x = _t(1.5 * p - 0.2, dev)
    for t in mo.TRANSFERS:
        mean, out = metrics.ssim(x, x.clone(), None, t, return_map=True)
        assert bool((out == 1.0).all()) and bool((mean == 1.0).all()), t
    one = metrics.ssim(x[0], x[0])                                       # [H,W,C]: one view
    assert tuple(one.shape) == (1,) and float(one) == 1.0


def test_ssim_every_transfer_and_scale(dev):
    """All four transfers on the partial-tile shape with values on both sides of [0, 1]; a per-channel scale against the oracle, and -- with
    powers of two, where the fp32 product is exact -- bit-equal to pre-multiplying the prediction."""
    from robir_amd import metrics
    H, W = T + 11, T + 10 + 3
    p, g = mo.images("noise", 1, H, W, 3)
    p, g = (1.5 * p - 0.2).astype(np.float32), (1.5 * g - 0.2).astype(np.float32)
    m = mo.masks(1, H, W)
    for t in mo.TRANSFERS:
        for scale in (None, np.array([0.7, 1.3, 1.1], np.float32)):
            n, s, ref = mo.ssim(p, g, m, t, scale)
            _check_ssim(f"transfer{t}_{'scaled' if scale is not None else 'plain'}", dev, p, g, m, n, s, ref, t, None if scale is None else _t(scale, dev))
    pow2 = np.array([0.5, 2.0, 0.25], np.float32)
    a = metrics.ssim(_t(p, dev), _t(g, dev), _t(m, dev), mo.GAMMA22, scale=pow2.tolist(), return_map=True)
    b = metrics.ssim(_t(p * pow2, dev), _t(g, dev), _t(m, dev), mo.GAMMA22, return_map=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ps = metrics.pair_stats(_t(p, dev), _t(g, dev), _t(m, dev), mo.GAMMA22, scale=pow2.tolist())
    qs = metrics.pair_stats(_t(p * pow2, dev), _t(g, dev), _t(m, dev), mo.GAMMA22)
    assert torch.equal(ps[0], qs[0]) and torch.equal(ps[1], qs[1])


def test_ssim_refuses_small_images(dev):
    from robir_amd import _lib, metrics
    x = torch.zeros(10, 20, 3, device=dev)
    with pytest.raises(_lib.RobirHipError, match="11 x 11"):
        metrics.ssim(x, x)


# ------------------------------------------------------------------------------------------------ pair sums
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("C,t", [(1, mo.NONE), (3, mo.GAMMA22), (4, mo.CLIP)])
@pytest.mark.parametrize("P", ROWS)
def test_pair_stats_against_the_oracle(dev, P, C, t, V):
    """Count and the five sums per channel, and mse / mae / psnr derived from them; the last view's mask is empty when V = 3."""
    from robir_amd import metrics
    p, g, m = mo.rows(V, P, C)
    n_ref, s_ref = mo.pair_stats(p, g, m, t)
    n, s = metrics.pair_stats(_t(p, dev), _t(g, dev), _t(m, dev), t, views=True)
    assert n.dtype == torch.float64 and tuple(s.shape) == (V, C, 5)
    assert np.array_equal(n.cpu().numpy(), n_ref)
    e = mo.rel(s.cpu().numpy(), s_ref)
    e32 = -1.0
    if t == mo.NONE:
        w = torch.from_numpy(m)[..., None].float()
        tp, tg = torch.from_numpy(p), torch.from_numpy(g)
        t32 = torch.stack([(w * (tp - tg) ** 2).sum(1), (w * (tp - tg).abs()).sum(1), (w * tp * tg).sum(1), (w * tp * tp).sum(1), (w * tg * tg).sum(1)], -1)
        e32 = mo.rel(t32.numpy(), s_ref)
    _record(f"pair/P{P}_C{C}_V{V}_t{t}", e, e32, TOL_SUM)
    assert e <= TOL_SUM, e
    args = (_t(p, dev), _t(g, dev), _t(m, dev), t)
    got = {"mse": metrics.mse(*args, views=True), "mae": metrics.mae(*args, views=True), "psnr": metrics.psnr(*args, views=True)}
    ok = n_ref > 0
    want = {"mse": s_ref[:, :, 0].sum(1)[ok] / (C * n_ref[ok]), "mae": s_ref[:, :, 1].sum(1)[ok] / (C * n_ref[ok])}
    want["psnr"] = -10.0 * np.log10(want["mse"])
    for k, v in got.items():
        v = v.cpu().numpy()
        assert v.dtype == np.float64 and v.shape == (V,)
        assert mo.rel(v[ok], want[k]) <= TOL_SUM, k
        assert bool(np.isnan(v[~ok]).all())
    if V == 3:
        assert n_ref[-1] == 0 and not s.cpu().numpy()[-1].any()          # an empty mask gives zeros


def test_pair_stats_every_transfer_no_mask_and_one_image(dev):
    from robir_amd import metrics
    p, g, _ = mo.rows(1, R + 1, 3)
    for t in mo.TRANSFERS:
        n_ref, s_ref = mo.pair_stats(p, g, None, t)
        n, s = metrics.pair_stats(_t(p[0], dev), _t(g[0], dev), None, t)                 # [P,C]: one view
        e = mo.rel(s.cpu().numpy(), s_ref)
        _record(f"pair/all_pixels_t{t}", e, -1.0, TOL_SUM)
        assert float(n) == R + 1 and e <= TOL_SUM
    img = _t(p.reshape(1, R + 1, 3)[:, :256].reshape(16, 16, 3), dev)                        # [H,W,C] is ONE view of 256 pixels, not 16 views
    assert tuple(metrics.mse(img, img).shape) == (1,)
    assert tuple(metrics.mse(img, img, views=True).shape) == (16,)


def test_psnr_of_identical_images_is_inf(dev):
    from robir_amd import metrics
    p, _, m = mo.rows(3, R + 1, 3)
    x = _t(p, dev)
    v = metrics.psnr(x, x.clone(), _t(m, dev), mo.GAMMA22, views=True).cpu().numpy()
    assert np.isposinf(v[0]) and np.isposinf(v[1]) and np.isnan(v[2])    # the third mask is empty: 0 / 0, not an error
    assert float(metrics.mse(x, x.clone(), views=True).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ angular error
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("P", ROWS)
def test_angular_stats_against_the_oracle(dev, P, V):
    """Rows where either vector is shorter than 1e-6 (zeros, and 1e-7 long) are in neither the count nor the sum."""
    from robir_amd import metrics
    a, b, m = mo.normals(V, P)
    n_ref, s_ref = mo.angular_stats(a, b, m)
    n, s = metrics.angular_stats(_t(a, dev), _t(b, dev), _t(m, dev), views=True)
    assert np.array_equal(n.cpu().numpy(), n_ref)
    short = (np.linalg.norm(a.astype(np.float64), axis=-1) < 1e-6) | (np.linalg.norm(b.astype(np.float64), axis=-1) < 1e-6)
    assert np.array_equal(n_ref, (m & ~short).sum(1)) and (P < 12 or short.any())
    e = mo.rel(s.cpu().numpy(), s_ref)
    ang32 = torch.acos((torch.nn.functional.normalize(torch.from_numpy(a), dim=-1) * torch.nn.functional.normalize(torch.from_numpy(b), dim=-1)).sum(-1).clamp(-1, 1))
    e32 = mo.rel((ang32 * torch.from_numpy(m & ~short)).sum(1).numpy(), s_ref)
    _record(f"angular/P{P}_V{V}", e, e32, TOL_SUM)
    assert e <= TOL_SUM, e
    deg = metrics.normal_error_deg(_t(a, dev), _t(b, dev), _t(m, dev), views=True).cpu().numpy()
    ok = n_ref > 0
    assert mo.rel(deg[ok], np.degrees(s_ref[ok] / n_ref[ok])) <= TOL_SUM


def test_normal_error_of_a_field_rotated_by_a_known_angle(dev):
    """Fields whose rotated copy is EXACT in fp32 (components are multiples of 1/8 below 8, so sums and differences round nowhere): b = the
    in-plane a turned by 45 degrees and scaled by sqrt 2, and b = a x e_x, 90 degrees from a.  The angle comes back to 1e-6 degrees."""
    from robir_amd import metrics
    rng = np.random.default_rng(4)
    P = 70001
    x, y = rng.integers(-32, 33, P).astype(np.float32) / 8, rng.integers(1, 33, P).astype(np.float32) / 8
    z = rng.integers(-32, 33, P).astype(np.float32) / 8
    flat = np.stack([x, y, np.zeros_like(x)], -1)
    turned = np.stack([x - y, x + y, np.zeros_like(x)], -1)
    full = np.stack([x, y, z], -1)
    crossed = np.stack([np.zeros_like(x), z, -y], -1)                   # (x, y, z) x (1, 0, 0)
    for a, b, want in ((flat, turned, 45.0), (full, crossed, 90.0)):      # not 0 / 180: acos is ill-conditioned there (1 ulp of the cosine = 8.5e-7 degrees)
        got = float(metrics.normal_error_deg(_t(a, dev), _t(b, dev)))
        _record(f"angular/rotated_{want:g}", abs(got - want), -1.0, 1e-6)
        assert abs(got - want) <= 1e-6, (want, got)


# ------------------------------------------------------------------------------------------------ determinism
def test_two_runs_are_bit_equal(dev):
    from robir_amd import metrics
    p, g, m = mo.rows(3, 70001, 3)
    a, b, am = mo.normals(3, 70001)
    ip, ig, im, _, _, _ = _ssim_truth("noise", 3, 45, 53, 3)
    runs = []
    for _ in range(2):
        out = list(metrics.pair_stats(_t(p, dev), _t(g, dev), _t(m, dev), mo.GAMMA22, views=True))
        out += list(metrics.angular_stats(_t(a, dev), _t(b, dev), _t(am, dev), views=True))
        out += list(metrics.ssim_stats(_t(ip, dev), _t(ig, dev), _t(im, dev), mo.GAMMA22, want_map=True))
        runs.append(out)
    assert len(runs[0]) == 7
    for x, y in zip(*runs):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ albedo ratio and the chain
def test_albedo_ratio_modes_and_degenerate_channels(dev):
    from robir_amd import metrics
    rng = np.random.default_rng(8)
    p = (rng.random((2, 24, 20, 3), dtype=np.float32) + 0.05).astype(np.float32)
    g = (p * np.array([0.5, 2.0, 1.5], np.float32) + 0.01 * rng.standard_normal(p.shape)).astype(np.float32)
    m = rng.random((2, 24, 20)) < 0.7
    for mode, ref in (("lsq", mo.ratio_lsq(p, g, m)), ("median", mo.ratio_median(p, g, m))):
        r = metrics.albedo_ratio(_t(p, dev), _t(g, dev), _t(m, dev), mode)
        assert r.dtype == torch.float32 and r.is_cuda and tuple(r.shape) == (3,)
        e = float(np.abs(r.cpu().numpy() - ref.astype(np.float32)).max())
        _record(f"albedo_ratio/{mode}", e, -1.0, 0.0)
        assert e == 0.0, (mode, e)                                      # fp64 sums rounded to fp32 once; the lower median of fp32 quotients
    p[..., 1] = 0.0
    for mode in ("lsq", "median"):
        assert float(metrics.albedo_ratio(_t(p, dev), _t(g, dev), _t(m, dev), mode)[1]) == 1.0
    with pytest.raises(ValueError, match="mode"):
        metrics.albedo_ratio(_t(p, dev), _t(g, dev), None, "mean")


@pytest.fixture(scope="module")
def model(dev):
    from robir_amd import renderer
    m = renderer.build_synthetic_model(dev, seed=0, variance=0.3)
    m.deferred_chunks = 0
    return m


def test_chain_albedo_ratio_into_the_renderer(dev, model):
    """The 1024-pixel chunk of the 64 x 64 synthetic view (smoke()'s inputs, built here): with gt_albedo = diffuse_albedo (0.5, 2.0, 1.5) on
    the hit rows, albedo_ratio returns those factors to 1e-6 in both modes; fed back as input['albedo_ratio'] the render's diffuse_albedo
    is within 1e-5 of gt_albedo and the aligned albedo PSNR is above the unaligned one."""
    from robir_amd import metrics, synth
    uv, pose, K = synth.synth_camera(64, 64)
    sl = slice(1024, 2048)
    inp = {"uv": torch.from_numpy(uv[sl]).to(dev)[None], "pose": torch.from_numpy(pose).to(dev)[None], "intrinsics": torch.from_numpy(K).to(dev)[None],
           "object_mask": torch.ones(1, 1024, dtype=torch.bool, device=dev), "hdr_shift": torch.full((1024, 1), 0.5, device=dev)}
    model.eval()
    first = model(inp, trainstage="Material", train_spec=True)
    hit = first["network_object_mask"].reshape(-1)
    n = int(hit.sum())
    assert 100 <= n < 1024
    dr = {k: torch.from_numpy(v).to(dev) for k, v in synth.pbr_draws(0, n, chunk_id=1).items()}
    base = model(inp, trainstage="Material", train_spec=True, draws=dr)
    albedo = base["diffuse_albedo"].reshape(1024, 3)
    factors = torch.tensor([0.5, 2.0, 1.5], device=dev)
    gt_albedo = torch.where(hit[:, None], albedo * factors, torch.zeros_like(albedo))
    ratios = {mode: metrics.albedo_ratio(albedo, gt_albedo, hit, mode) for mode in ("lsq", "median")}
    for mode, r in ratios.items():
        e = float((r - factors).abs().max())
        _record(f"chain/ratio_{mode}", e, -1.0, 1e-6)
        assert e <= 1e-6, (mode, r)
    aligned = model(dict(inp, albedo_ratio=ratios["lsq"]), trainstage="Material", train_spec=True, draws=dr)
    assert torch.equal(aligned["network_object_mask"].reshape(-1), hit)
    got = aligned["diffuse_albedo"].reshape(1024, 3)
    e = float((got - gt_albedo)[hit].abs().max())
    _record("chain/aligned_albedo", e, -1.0, 1e-5)
    assert e <= 1e-5, e
    assert not torch.equal(aligned["sg_rgb"], base["sg_rgb"])            # the aligned albedo is shaded, not only returned
    before = float(metrics.psnr(albedo, gt_albedo, hit, mo.GAMMA22))
    after = float(metrics.psnr(got, gt_albedo, hit, mo.GAMMA22))
    by_scale = float(metrics.psnr(albedo, gt_albedo, hit, mo.GAMMA22, scale=ratios["lsq"]))
    record_metric("metrics/chain/albedo_psnr", unaligned=before, aligned=min(after, 999.0), scaled=by_scale)      # inf is not JSON: capped
    assert after > before and by_scale > before
    again = model(inp, trainstage="Material", train_spec=True, draws=dr)  # albedo_ratio=None: nothing changed
    assert torch.equal(again["diffuse_albedo"], base["diffuse_albedo"]) and torch.equal(again["sg_rgb"], base["sg_rgb"])


# ------------------------------------------------------------------------------------------------ evaluate_views and the CLI
def _view(seed, H=24, W=20):
    rng = np.random.default_rng(seed)
    hit = rng.random((H, W, 1)) < 0.8
    nrm = rng.standard_normal((H, W, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    return {"sg_rgb": rng.random((H, W, 3), dtype=np.float32), "indir_rgb": 0.1 * rng.random((H, W, 3), dtype=np.float32),
            "diffuse_albedo": rng.random((H, W, 3), dtype=np.float32), "roughness": rng.random((H, W, 1), dtype=np.float32),
            "normals": (nrm * hit).astype(np.float32), "network_object_mask": hit}


def test_cli_equals_the_python_calls(dev, tmp_path, capsys):
    """Two .npz views and an .npz ground truth written here: the JSON's numbers are those of the Python calls, and a prediction scored
    against itself reports SSIM 1, infinite PSNR and a ratio of (1, 1, 1)."""
    from robir_amd import evaluate, metrics
    H, W = 24, 20
    views = [_view(0, H, W), _view(1, H, W)]
    paths = []
    for i, v in enumerate(views):
        paths.append(str(tmp_path / f"view{i}.npz"))
        np.savez_compressed(paths[-1], **v)
    rng = np.random.default_rng(5)
    gt = {"rgb": rng.random((2, H, W, 3), dtype=np.float32), "albedo": (0.5 * np.stack([v["diffuse_albedo"] for v in views]) + 0.02 * rng.random((2, H, W, 3))).astype(np.float32),
          "roughness": rng.random((2, H, W, 1), dtype=np.float32), "normal": np.stack([_view(7 + i, H, W)["normals"] for i in range(2)]),
          "mask": rng.random((2, H, W)) < 0.7}
    np.savez(str(tmp_path / "gt.npz"), **gt)
    out = str(tmp_path / "m.json")
    evaluate.main(["--pred", *paths, "--gt", str(tmp_path / "gt.npz"), "--out", out, "--transfer", "gamma22_q8", "--ssim-maps", str(tmp_path / "maps")])
    doc = json.load(open(out))
    assert "psnr" in capsys.readouterr().out
    st = lambda k: _t(np.stack([v[k] for v in views]), dev)
    m = _t(gt["mask"], dev)
    rgb = st("sg_rgb") + st("indir_rgb")
    ratio = metrics.albedo_ratio(st("diffuse_albedo"), _t(gt["albedo"], dev), m)
    want = {"psnr": metrics.psnr(rgb, _t(gt["rgb"], dev), m, "gamma22_q8"), "ssim": metrics.ssim(rgb, _t(gt["rgb"], dev), m, "gamma22_q8"),
            "albedo_psnr": metrics.psnr(st("diffuse_albedo"), _t(gt["albedo"], dev), m, "gamma22_q8", scale=ratio),
            "albedo_ssim": metrics.ssim(st("diffuse_albedo"), _t(gt["albedo"], dev), m, "gamma22_q8", scale=ratio),
            "roughness_mse": metrics.mse(st("roughness"), _t(gt["roughness"], dev), m),
            "normal_mae_deg": metrics.normal_error_deg(st("normals"), _t(gt["normal"], dev), m)}
    assert doc["transfer"] == "gamma22_q8" and doc["pred"] == paths and len(doc["views"]) == 2
    assert doc["albedo_ratio"] == [float(x) for x in ratio.cpu()]
    for k, v in want.items():
        assert [d[k] for d in doc["views"]] == [float(x) for x in v.cpu()], k
        assert doc["mean"][k] == float(v.cpu().mean()), k
    assert abs(doc["albedo_ratio"][0] - 0.5) < 0.05
    from PIL import Image
    for name in ("ssim_0.png", "ssim_1.png", "albedo_ssim_0.png", "albedo_ssim_1.png"):
        assert Image.open(str(tmp_path / "maps" / name)).size == (W - 10, H - 10)
    # a prediction against itself
    res, doc = evaluate.evaluate_files(paths[:1], paths[0])
    d = doc["views"][0]
    assert d["ssim"] == 1.0 and d["psnr"] == "inf" and d["albedo_ssim"] == 1.0 and d["albedo_psnr"] == "inf" and d["roughness_mse"] == 0.0
    assert doc["albedo_ratio"] == [1.0, 1.0, 1.0] and d["normal_mae_deg"] <= 1e-5
    # evaluate_views on what render_view returns: flat device tensors, the image size taken from the ground truth
    flat = {k: _t(v.reshape(H * W, -1), dev) for k, v in views[0].items()}
    r2 = metrics.evaluate_views(flat, {k: v[0] for k, v in gt.items()})
    r1 = metrics.evaluate_views({k: v for k, v in views[0].items()}, {k: v[0] for k, v in gt.items()})
    assert r1 == r2 and sorted(r1["mean"]) == sorted(evaluate.KEYS)
    only = metrics.evaluate_views(views[0], {"roughness": gt["roughness"][0]})
    assert sorted(only["mean"]) == ["roughness_mse"] and "albedo_ratio" not in only
