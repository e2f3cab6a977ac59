"""The atlas fit on the device (robir_amd/csrc/texfit/texfit.hip, robir_amd/texfit.py) against the numpy restatement of its rules
(tests/texfit_restatement.py): every kernel bit for bit, the fetch against the mesh view's own G-buffer fetch; then the loop closed on a
known answer against a float64 restatement of the same loop, and end to end on the baked synthetic scene and through the command line."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshrender_restatement as mr  # noqa: E402
import meshrender_scene as ms  # noqa: E402
import texbake_restatement as tr  # noqa: E402
import texfit_restatement as tf  # noqa: E402
from conftest import GOLD, record_metric  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def uvs(R):
    return tf.tap_uvs(R)


# ----------------------------------------------------------------------------------------- kernels against the restatement
@pytest.mark.parametrize("filt", (0, 1))
@pytest.mark.parametrize("R", (1, 8, 64))
def test_taps_and_fetch_equal_restatement(R, filt):
    """The G-buffer case's uvs, texel centres, u or v = 0 and 1, uv outside [0, 1], NaN and infinite uv; n = 1, 63, 64, 65, 257 and all."""
    from robir_amd import ops
    uv = uvs(R)
    planes = np.random.default_rng(R).uniform(0.05, 1.0, (R, R, 8)).astype(np.float32)
    assert len(uv) > 257 and np.isnan(uv).any()
    for n in (1, 63, 64, 65, 257, len(uv)):
        texel, weight = ops.tf_taps(dev(uv[:n]), R, filt)
        want_t, want_w = tf.taps(uv[:n], R, filt)
        assert texel.dtype == torch.int32 and tuple(texel.shape) == (n, 4) and np.array_equal(texel.cpu().numpy(), want_t), n
        assert same_bits(weight, want_w), n
        for C in (4, 8):
            assert same_bits(ops.tf_fetch(dev(planes), texel, weight, C), tf.fetch(planes, want_t, want_w, C)), (n, C)
    if R >= 8 and filt == 1:          # a texel centre: weights exactly 1, 0, 0, 0 and the texel's own bits
        centre = np.array([[(3 + 0.5) / R, 1.0 - (5 + 0.5) / R]], dtype=np.float32)
        texel, weight = ops.tf_taps(dev(centre), R, 1)
        assert weight.cpu().tolist() == [[1.0, 0.0, 0.0, 0.0]] and int(texel[0, 0]) == 5 * R + 3
        assert same_bits(ops.tf_fetch(dev(planes), texel, weight, 8), planes[5:6, 3])


@pytest.mark.parametrize("size", ((13, 21), (64, 64)))
def test_fetch_equals_the_gbuffers_tex(size):
    """The list form of an 80-face icosphere view, R = 64, Cs = 8, C = 4: the fetch formed from the taps has the bits of rb_rs_gbuffer's tex
    for the same uv -- forward and backward use one linearisation."""
    from robir_amd import meshrender, ops, synth
    H, W = size
    R = 64
    v, f = mr.icosphere(1)
    uv = tr.atlas_uv(80, R)
    planes = np.random.default_rng(3).uniform(0.05, 1.0, (R, R, 8)).astype(np.float32)
    _, _, K = synth.synth_camera(H, W)
    pose = mr.rotated_pose()
    fid, bary, _ = meshrender.rasterize(dev(v), dev(f), dev(pose), dev(K), H, W)
    idx = (fid.reshape(-1) >= 0).nonzero()[:, 0].contiguous()
    assert idx.numel() > (40 if H == 13 else 900)
    for filt in (0, 1):
        g = meshrender.gbuffer(fid, bary, dev(v), dev(f), dev(uv), dev(pose[:3, 3].copy()), dev(planes), filt, index=idx)
        texel, weight = ops.tf_taps(g["uv"], R, filt)
        tex = ops.tf_fetch(dev(planes), texel, weight, 4)
        assert tuple(tex.shape) == (idx.numel(), 4) and same_bits(tex, g["tex"][:, :4]), filt
        assert same_bits(ops.tf_fetch(dev(planes), texel, weight), g["tex"]), filt


@pytest.mark.parametrize("C", (1, 4, 16))
def test_scatter_equals_restatement(C):
    """Segments of 1, 63, 64, 65 and 300 pairs, the first and the last segment, rows out of range inside a segment, invalid pairs at the
    tail; n = 131.  Two runs give the same bytes."""
    from robir_amd import ops
    pr, pw, ss, g = tf.scatter_case(C)
    want = tf.scatter(pr, pw, ss, g)
    runs = [ops.tf_scatter(dev(pr), dev(pw), dev(ss), dev(g)) for _ in range(2)]
    assert tuple(runs[0].shape) == (len(tf.SEGMENTS), C) and same_bits(runs[0], want)
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    assert np.abs(want[[0, 4, -1]]).min() > 0


def _coarse_view(C):
    """The uv rows of a 64 x 64 view of the icosphere against a coarse R = 8 atlas: long segments from a real pair list."""
    from robir_amd import synth
    v, f = mr.icosphere(1)
    _, _, K = synth.synth_camera(64, 64)
    pose = mr.rotated_pose()
    fid, bary, _ = mr.raster(mr.project(v, mr.pose_inverse(pose), K), f, 64, 64)
    idx = np.nonzero(fid.reshape(-1) >= 0)[0]
    uv = mr.gbuffer(fid, bary, f, v, tr.atlas_uv(80, 64), pose[:3, 3], index=idx)["uv"]
    return uv, np.random.default_rng(C).normal(size=(len(uv), C)).astype(np.float32)


def test_scatter_of_a_coarse_atlas_under_a_fine_view():
    from robir_amd import ops, texfit
    uv, g = _coarse_view(4)
    R = 8
    texel, weight = ops.tf_taps(dev(uv), R, 1)
    pr, pw, st, ss = texfit.sort_pairs(texel, weight, R)
    want = tf.sort_pairs(*tf.taps(uv, R, 1), R)
    for got, ref in zip((pr, pw, st, ss), want):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), np.ascontiguousarray(ref).view(np.uint32))
    assert len(uv) % 64 and np.diff(want[3]).max() >= 300 and len(want[2]) <= 64
    assert same_bits(ops.tf_scatter(pr, pw, ss, dev(g)), tf.scatter(*want[:2], want[3], g))


@pytest.mark.parametrize("case", tf.ADAM_CASES, ids=lambda c: "Cs%d-C%d-T%d-t%d" % c)
def test_adam_equals_restatement(case):
    """Both clamps active, the channel offset of Cs = 8 / C = 4, T = 1, t = 1 and t = 1000, texel indices out of range: planes and both
    moments bit for bit; every operation is an IEEE basic operation in fp64."""
    from robir_amd import ops
    c = tf.adam_case(*case)
    planes, m, v = dev(c["planes"]), dev(c["m"]), dev(c["v"])
    ops.tf_adam(planes, m, v, dev(c["seg_texel"]), dev(c["grad"]), c["lr"], c["lo"], c["hi"], c["beta1"], c["beta2"], c["eps"], c["t"])
    want = [c[k].copy() for k in ("planes", "m", "v")]
    tf.adam(*want, c["seg_texel"], c["grad"], c["lr"], c["lo"], c["hi"], c["beta1"], c["beta2"], c["eps"], c["t"])
    assert same_bits(planes, want[0]) and same_bits(m, want[1]) and same_bits(v, want[2])
    assert not same_bits(planes, c["planes"])


def test_fetch_autograd_places_the_scatter_by_texel():
    from robir_amd import ops, texfit
    R = 8
    uv, g = _coarse_view(4)
    uv = np.concatenate([uv, uvs(R)[:70]])
    g = np.concatenate([g, np.ones((70, 4), dtype=np.float32)])
    planes = dev(np.random.default_rng(1).uniform(0.05, 1.0, (R, R, 4)).astype(np.float32)).requires_grad_(True)
    with torch.enable_grad():
        out = texfit.fetch(planes, dev(uv))
        out.backward(dev(g))
    t, w = tf.taps(uv, R, 1)
    assert same_bits(out, tf.fetch(planes.detach().cpu().numpy(), t, w))
    pr, pw, st, ss = tf.sort_pairs(t, w, R)
    assert same_bits(planes.grad, tf.dense(st, tf.scatter(pr, pw, ss, g), R))
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match="uv"):
            texfit.fetch(planes, dev(uv).requires_grad_(True))


# ----------------------------------------------------------------------------------------- the loop, closed on a known answer
def test_loop_recovers_a_known_atlas():
    """An 80-face icosphere, the per-face atlas at R = 64, four rotated cameras at 32 x 32 (cull = 1), a 16-lobe light, direct shading,
    tone = None, L2; the targets are rendered from a smooth truth atlas, the start is the truth plus uniform +-0.2 noise; lr = 0.02, 50 steps.

    The same loop in float64 torch on the CPU (texfit_restatement.fit_loop64: sg_backward_oracle.shade, the restatement's taps, lazy Adam)
    gives, on these inputs: 1927 hit rows, 2029 of 4096 texels touched, loss 1.31e-3 -> 3.05e-6, mean absolute albedo error over the touched
    texels 0.0995 -> 0.0440, roughness 0.0985 -> 0.0993 (at f0 = 0.02 the views barely constrain roughness: no condition on it).
    Conditions on the device: the loss falls, the albedo error over the touched texels falls, untouched texels keep their bits.  The
    device's loss history is compared step by step with the float64 loop's; the largest relative deviation is recorded and capped at twice
    the value measured on an MI355X (tests/golden/texfit_caps.json)."""
    from robir_amd import meshrender, texfit
    L, scene = tf.LOOP, tf.loop_scene()
    R, H, W = L["R"], L["H"], L["W"]
    lgt = dev(scene["light"])
    asset = lambda planes: meshrender.MeshAsset(dev(scene["v"]), dev(scene["f"]), dev(scene["uv"]), dev(planes), False, dev(scene["vn"]))
    K = torch.from_numpy(scene["K"])
    images = []
    for pose in scene["poses"]:
        view = meshrender.render_mesh(asset(scene["truth"]), torch.from_numpy(pose), K, H, W, light=lgt, vis="none", cull=L["cull"])
        x = view["sg_rgb"]
        images.append(torch.where(view["network_object_mask"][:, None], x / (x + 1.0), torch.zeros_like(x)).reshape(H, W, 3))
    views = {"images": torch.stack(images), "poses": torch.from_numpy(scene["poses"]), "intrinsics": K[None].repeat(L["views"], 1, 1)}
    fit = texfit.AtlasFit(asset(scene["start"]), views, light=lgt, vis="none", tone=None, loss_type="L2", lr=L["lr"], betas=L["betas"],
                          eps=L["eps"], lo=L["lo"], hi=L["hi"], cull=L["cull"])
    hist = fit.run(L["steps"])
    b = fit.view_batch(range(L["views"]))
    assert len(hist) == L["steps"] and 1800 < b.n < 2100 and abs(b.n - sum(len(r["idx"]) for r in scene["rows"])) <= 8
    got = fit.result().planes.cpu().numpy()
    touched = np.zeros(R * R, dtype=bool)
    touched[b.seg_texel.cpu().numpy()] = True
    touched = touched.reshape(R, R)
    err = lambda p, ch: float(np.abs(p[..., ch] - scene["truth"][..., ch])[touched].mean())
    before, after = err(scene["start"], slice(0, 3)), err(got, slice(0, 3))
    rows = {"normal": b.normal.cpu().numpy(), "view_dir": b.view_dir.cpu().numpy(), "uv": b.uv.cpu().numpy()}
    hist64, planes64, touched64 = tf.fit_loop64(scene, b.target.cpu().numpy(), rows)
    rel = [abs(a - r) / r for a, r in zip(hist, hist64)]
    dev_rel, worst = max(rel), int(np.argmax(rel))
    print("rows", b.n, "touched", int(touched.sum()), "loss", hist[0], "->", hist[-1], "float64", hist64[0], "->", hist64[-1],
          "albedo error", before, "->", after, "roughness error", err(scene["start"], 3), "->", err(got, 3),
          "largest relative deviation of the loss history", dev_rel, "at step", worst, "planes vs float64", float(np.abs(got - planes64).max()))
    record_metric("texfit_loop", rows=b.n, touched=int(touched.sum()), loss_first=hist[0], loss_last=hist[-1], loss64_last=hist64[-1],
                  albedo_before=before, albedo_after=after, loss_history_rel_dev=dev_rel, worst_step=worst, loss_history=hist,
                  loss_history64=hist64, planes_abs_dev=float(np.abs(got - planes64).max()))
    assert hist[-1] < hist[0] and hist[-1] < 0.05 * hist[0]
    assert after < before
    assert np.array_equal(touched, touched64) and abs(fit.touched_fraction() - touched.mean()) < 1e-7
    assert np.array_equal(got[~touched].view(np.uint32), scene["start"][~touched].view(np.uint32))
    assert np.array_equal(got[..., 4:].view(np.uint32), scene["start"][..., 4:].view(np.uint32))
    assert (got[..., :3] >= 0).all() and (got[..., :4] <= 1).all() and (got[..., 3] >= np.float32(0.02)).all()
    caps = json.load(open(os.path.join(GOLD, "texfit_caps.json")))["caps"]
    assert dev_rel <= 2.0 * caps["loss_history_rel_dev"], (dev_rel, caps)


# ----------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def scene():
    return ms.build(DEV)


@pytest.fixture(scope="module")
def asset_dir(scene, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("texfit") / "asset")
    scene["ts"].export(out)
    return out


def test_fit_of_the_baked_scene_against_its_neural_view(scene, asset_dir, tmp_path):
    """The bake of the synthetic scene fitted for 20 steps of direct shading to the neural view it was baked from: the loss falls; the saved
    asset loads through meshrender.load_asset, and render_mesh of it equals the fit's own forward of its final planes bit for bit."""
    from robir_amd import meshrender, texfit
    model, neural = scene["model"], scene["neural"]
    tone = model.gamma.hdr_shift
    target = tone.hdr2ldr(neural["sg_rgb"] + neural["indir_rgb"], tone.as_input().detach()).reshape(1, ms.H, ms.W, 3).float()
    views = {"images": target, "masks": neural["network_object_mask"].reshape(1, ms.H, ms.W).float(),
             "poses": torch.from_numpy(scene["pose"])[None], "intrinsics": torch.from_numpy(scene["K"])[None]}
    fit = texfit.AtlasFit(asset_dir, views, model=model, vis="none", tone=tone, loss_type="L1", lr=0.01)
    hist = fit.run(20)
    print("loss", hist[0], "->", hist[-1], "touched fraction", fit.touched_fraction())
    record_metric("texfit_scene", loss_first=hist[0], loss_last=hist[-1], touched=fit.touched_fraction())
    assert len(hist) == 20 and hist[-1] < hist[0]
    out = fit.save(str(tmp_path / "fitted"), extra={"note": "test"})
    for name in ("mesh.obj", "mesh.mtl", "maps.npz", "albedo.png", "roughness.png", "metallic.png", "normal.png", "fit.json"):
        assert os.path.getsize(os.path.join(out, name)) > 0, name
    with np.load(os.path.join(asset_dir, "maps.npz")) as a, np.load(os.path.join(out, "maps.npz")) as b:
        assert set(a.files) == set(b.files)
        for k in a.files:
            assert a[k].shape == b[k].shape and (k in ("albedo", "roughness")) != np.array_equal(a[k], b[k]), k
    doc = json.load(open(os.path.join(out, "fit.json")))
    assert doc["loss_hist"] == hist and 0 < doc["touched_fraction"] < 0.2 and doc["settings"]["steps"] == 20
    loaded = meshrender.load_asset(out, DEV)
    assert torch.equal(loaded.planes.view(torch.int32), fit.result().planes.view(torch.int32))
    view = meshrender.render_mesh(out, torch.from_numpy(scene["pose"]), torch.from_numpy(scene["K"]), ms.H, ms.W, model=model, vis="none")
    mine = fit.forward()
    idx = mine["batch"].pixels[0]
    assert torch.equal(idx, view["network_object_mask"].nonzero()[:, 0]) and idx.numel() > 500
    for k in ("sg_rgb", "diffuse_albedo"):
        assert same_bits(view[k][idx], mine[k]), k
    assert same_bits(view["roughness"][idx][:, :1], mine["roughness"])


def test_visibility_and_indirect_term_are_constants_of_the_batch(scene, asset_dir):
    """vis='network': the sampled light visibility, the sampled specular visibility and the indirect term are formed once per batch and
    reused by every step; the loss of the fit against the neural view falls."""
    from robir_amd import texfit
    model, neural = scene["model"], scene["neural"]
    tone = model.gamma.hdr_shift
    target = tone.hdr2ldr(neural["sg_rgb"] + neural["indir_rgb"], tone.as_input().detach()).reshape(1, ms.H, ms.W, 3).float()
    views = {"images": target, "masks": neural["network_object_mask"].reshape(1, ms.H, ms.W).float(),
             "poses": torch.from_numpy(scene["pose"])[None], "intrinsics": torch.from_numpy(scene["K"])[None]}
    fit = texfit.AtlasFit(asset_dir, views, model=model, vis="network", tone=tone, loss_type="L1", lr=0.01)
    fit.step()
    b = fit.view_batch([0])
    held = (b.light_vis, b.bvis, b.indir)
    assert tuple(b.light_vis.shape) == (b.n, fit.lgt.shape[0]) and tuple(b.bvis.shape) == (b.n,) and tuple(b.indir.shape) == (b.n, 3)
    assert 0 <= float(b.light_vis.min()) and float(b.light_vis.max()) <= 1 + 1e-6 and float(b.indir.abs().max()) > 0
    copies = [t.clone() for t in held]
    hist = fit.run(9)
    assert all(x is y for x, y in zip(held, (b.light_vis, b.bvis, b.indir))) and all(torch.equal(x, y) for x, y in zip(held, copies))
    print("vis='network' loss", hist[0], "->", hist[-1])
    assert len(hist) == 10 and hist[-1] < hist[0] and np.isfinite(fit.psnr())
    with pytest.raises(ValueError, match="needs the model"):
        texfit.AtlasFit(asset_dir, views, light=fit.lgt, vis="octree")


def test_command_line_writes_the_file_set(asset_dir, tmp_path):
    from robir_amd import texfit
    out = str(tmp_path / "fitted")
    texfit.main(["--asset", asset_dir, "--synthetic", "--n-views", "2", "--size", "64", "--steps", "5", "--out", out])
    for name in ("mesh.obj", "mesh.mtl", "maps.npz", "albedo.png", "roughness.png", "fit.json"):
        assert os.path.getsize(os.path.join(out, name)) > 0, name
    doc = json.load(open(os.path.join(out, "fit.json")))
    assert len(doc["loss_hist"]) == 5 and doc["settings"]["views"] == 2 and np.isfinite([doc["psnr_before"], doc["psnr_after"]]).all()
    print("PSNR of the mesh view against the neural targets:", doc["psnr_before"], "->", doc["psnr_after"])
