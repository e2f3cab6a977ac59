"""The photometric-loss library and its Python surface without a GPU: librobir_hip_photoloss.so against its header, its argument checks, the
host build of photoloss_math.h against tests/photoloss_oracle.py, that oracle against the reference's own tone-mapping output
(tests/golden/tonemap.npz), robir_amd/loss.py's signatures against the reference's, and the opt-in guards."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import pytest
import torch

import photoloss_oracle as plo
from conftest import ROOT, load_golden, rel_err

c_long, c_int = ctypes.c_long, ctypes.c_int
NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(4096)                    # never read: every call below is refused, or has nothing to do, before a launch
OTHER_HEADERS = ("robir_hip.h", "robir_hip_legacy.h", "robir_hip_train.h", "robir_hip_vistrain.h", "robir_hip_illumtrain.h",
                 "robir_hip_cesrtrain.h", "robir_hip_lightfit.h", "robir_hip_texbake.h", "robir_hip_observe.h")
REFERENCE_LOSS = os.path.join(os.environ.get("ROBIR_REFERENCE", "/root/reference"), "model", "loss.py")      # oracle/ref_shim.py's convention


def _header_symbols(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return sorted(set(re.findall(r"^(?:int|long|const char\*) (rb_[a-z0-9_]+)\s*\(", hdr, re.M)))


def _pl_lib():
    from robir_amd import _lib
    if not os.path.exists(_lib.PHOTOLOSS_PATH):
        _lib.build(legacy=False)
    return _lib.photoloss()


def test_photoloss_library_exports_its_header():
    """librobir_hip_photoloss.so loads without a GPU and exports exactly what include/robir_hip_photoloss.h declares, every name rb_pl_*; no
    rb_ name is shared with the other nine headers, and none of them names this one."""
    from robir_amd import _lib
    L = _pl_lib()
    assert L.rb_pl_abi_version() == _lib.PHOTOLOSS_ABI_VERSION == 1
    syms = _header_symbols("robir_hip_photoloss.h")
    assert syms == ["rb_pl_abi_version", "rb_pl_groups", "rb_pl_image_loss", "rb_pl_last_error", "rb_pl_scratch_bytes", "rb_pl_tonemap",
                    "rb_pl_tonemap_bwd"]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.PHOTOLOSS_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[-1] for l in out.splitlines() if " T rb_" in l) == syms
    others = set()
    for h in OTHER_HEADERS:
        text = open(os.path.join(ROOT, "include", h)).read()
        others |= set(_header_symbols(h))
        assert "rb_pl_" not in text and "photoloss" not in text
    assert not set(syms) & others
    assert "#define RB_PL_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "robir_hip_photoloss.h")).read()


def test_missing_photoloss_library_has_its_own_message(monkeypatch, tmp_path):
    from robir_amd import _lib
    monkeypatch.setattr(_lib, "_photoloss", None)
    monkeypatch.setattr(_lib, "PHOTOLOSS_PATH", str(tmp_path / "nope_photoloss.so"))
    with pytest.raises(_lib.RobirHipError, match="PHOTOMETRIC-LOSS library") as e:
        _lib.call_photoloss("rb_pl_image_loss")
    msg = str(e.value)
    assert "make -C robir_amd/csrc photoloss" in msg and "librobir_hip_photoloss.so" in msg and "LEGACY" not in msg


def test_photoloss_size_queries():
    L = _pl_lib()
    L.rb_pl_groups.restype = L.rb_pl_scratch_bytes.restype = ctypes.c_long
    for n, g in ((-1, -1), (0, 0), (1, 1), (256, 1), (257, 2), (70001, 274), (256 * 1024, 1024), (256 * 1024 + 1, 1024), (1 << 30, 1024)):
        assert L.rb_pl_groups(c_long(n)) == g, n
        assert L.rb_pl_scratch_bytes(c_long(n)) == (16 * g if g >= 0 else -1), n


def test_photoloss_argument_errors_before_any_launch():
    L = _pl_lib()
    err = L.rb_pl_last_error

    def fwd(x=FAKE, n=8, shift=FAKE, stride=1, curve=0, inverse=0, y=FAKE):
        return L.rb_pl_tonemap(x, c_long(n), shift, c_int(stride), c_int(curve), c_int(inverse), y, NULL)
    assert fwd(n=-1) != 0 and b"negative" in err()
    assert fwd(n=1 << 31) != 0 and b"2^31" in err()
    assert fwd(curve=5) != 0 and b"curve = 5" in err()
    assert fwd(curve=-1) != 0 and b"curve = -1" in err()
    assert fwd(inverse=2) != 0 and b"x^2.2" in err()
    assert fwd(inverse=3) != 0 and b"inverse = 3" in err()
    assert fwd(curve=4, inverse=1) != 0 and b"no inverse" in err()
    assert fwd(stride=2) != 0 and b"shift_stride = 2" in err()
    assert fwd(shift=NULL) != 0 and b"null pointer: shift" in err()
    assert fwd(x=NULL) != 0 and b"null pointer" in err()
    assert fwd(y=NULL) != 0 and b"null pointer" in err()
    assert fwd(n=0, x=NULL, y=NULL) == 0
    assert fwd(n=0, x=NULL, y=NULL, shift=NULL, curve=3) == 0          # the identity and x / (x + 1) read no shift

    def bwd(x=FAKE, n=8, shift=FAKE, stride=1, curve=0, inverse=0, gy=FAKE, gx=FAKE, gshift=FAKE, scratch=FAKE, nbytes=16):
        return L.rb_pl_tonemap_bwd(x, c_long(n), shift, c_int(stride), c_int(curve), c_int(inverse), gy, gx, gshift, scratch, c_long(nbytes), NULL)
    assert bwd(n=-3) != 0 and b"negative" in err()
    assert bwd(curve=7) != 0 and b"curve = 7" in err()
    assert bwd(inverse=2) != 0 and b"no backward" in err()
    assert bwd(stride=3) != 0 and b"shift_stride = 3" in err()
    assert bwd(stride=-1) != 0 and b"shift_stride = -1" in err()
    assert bwd(shift=NULL) != 0 and b"null pointer: shift" in err()
    assert bwd(gy=NULL) != 0 and b"null pointer" in err()
    assert bwd(stride=0, scratch=NULL) != 0 and b"scratch" in err()
    assert bwd(stride=0, scratch=ctypes.c_void_p(4100)) != 0 and b"aligned" in err()
    assert bwd(stride=0, n=257, nbytes=16) != 0 and b"scratch_bytes = 16" in err()
    assert bwd(n=0, x=NULL, gy=NULL, gx=NULL, gshift=NULL) == 0
    assert bwd(gx=NULL, gshift=NULL) == 0                              # nothing asked for: nothing launched

    def loss(sg=FAKE, indir=NULL, gt=FAKE, m1=FAKE, m2=FAKE, N=8, shift=FAKE, stride=0, curve=0, l2=0, out=FAKE, scratch=FAKE, nbytes=16):
        return L.rb_pl_image_loss(sg, indir, gt, m1, m2, c_long(N), shift, c_int(stride), c_int(curve), c_int(l2), out, NULL, NULL, scratch,
                                  c_long(nbytes), NULL)
    assert loss(N=-1) != 0 and b"negative" in err()
    assert loss(N=1 << 31) != 0 and b"2^31" in err()
    assert loss(curve=9) != 0 and b"curve = 9" in err()
    assert loss(stride=2) != 0 and b"shift_stride = 2" in err()
    assert loss(l2=2) != 0 and b"l2 = 2" in err()
    assert loss(shift=NULL) != 0 and b"null pointer: shift" in err()
    assert loss(sg=NULL) != 0 and b"null pointer" in err()
    assert loss(gt=NULL) != 0 and b"null pointer" in err()
    assert loss(m1=NULL) != 0 and b"null pointer" in err()
    assert loss(m2=NULL) != 0 and b"null pointer" in err()
    assert loss(out=NULL) != 0 and b"null pointer: loss" in err()
    assert loss(scratch=NULL) != 0 and b"scratch" in err()
    assert loss(N=600, nbytes=32) != 0 and b"scratch_bytes = 32" in err()
    assert loss(N=0, sg=NULL, gt=NULL, m1=NULL, m2=NULL, out=NULL, scratch=NULL, shift=NULL, curve=4) == 0


def _host_tool():
    spec = importlib.util.spec_from_file_location("check_photoloss_host", os.path.join(ROOT, "tools", "check_photoloss_host.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_host_build_of_the_math_equals_the_oracle(tmp_path):
    """tools/check_photoloss_host.py: photoloss_math.h compiled with the host C++ compiler as a stand-alone program
    (tools/photoloss_host.cpp supplies main and the loops).  The fp32 forward holds max(2 e_torch, 1e-5) against the float64 oracle; the
    fp64 value, both partial derivatives and the loss rows hold 1e-10 against float64 autograd; d/dt is exactly 0 outside the clamp and the
    rows outside the mask are exact zeros."""
    tool = _host_tool()
    assert tool.compiler() is not None, "no host C++ compiler, not even the clang++ beside hipcc"
    rows = tool.check(tool.build(out_dir=str(tmp_path)))
    assert len(rows) == 153
    assert [(what, fig, bound) for what, fig, bound, ok in rows if not ok] == []


def test_oracle_fp32_forward_equals_the_reference_goldens():
    """tests/golden/tonemap.npz is the reference's ACESToneMapping output for every hdr_mode (what test_oracle_golden.py pins robir_oracle
    on): this file's oracle, run in float32, gives the same values."""
    g = load_golden("tonemap")
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    for tag in ("rows", "scalar"):
        sh = torch.from_numpy(g["shift_" + tag]).reshape(-1)
        for curve, key in ((0, ""), (1, "m1_"), (2, "m2_"), (3, "m9_")):
            yy = y if curve == 0 else y * 0.7
            assert rel_err(plo.tonemap(x.reshape(-1, 3), sh, curve).reshape(x.shape), g["ldr_" + key + tag]) <= 1e-6, (tag, curve)
            assert rel_err(plo.tonemap(yy.reshape(-1, 3), sh, curve, inverse=True).reshape(y.shape), g["hdr_" + key + tag]) <= 1e-6, (tag, curve)


def test_generated_cases_stay_inside_the_curves_domains():
    """The bounds the GPU tests rely on, checked on the float64 oracle: finite everywhere, aces_inv's argument <= 0.95, and every L1 case
    keeps |pred - gt| >= 1e-3 on every entry."""
    for n in (1, 85, 257):
        for curve in plo.CURVES:
            for inverse in (False, True):
                for per_row in (False, True):
                    x, t, gy = plo.tonemap_case(n, curve, inverse, per_row)
                    y, gx, gs = plo.tonemap_grads(x, t, gy, curve, inverse, torch.float64)
                    assert bool(torch.isfinite(y).all() and torch.isfinite(gx).all() and torch.isfinite(gs).all())
                    assert float(t.min()) >= 0.05 and float(t.max()) <= 1.0
        for curve in plo.CURVES + (plo.RATIONAL,):
            case = plo.loss_case(n, curve, True, False)
            x = case["sg_rgb"].double() + case["indir_rgb"].double()
            assert 0.0 <= float(x.min()) and float(x.max()) <= 8.0
            pred = plo.tonemap(x, case["shift"].double(), curve) if case["shift"] is not None else plo.curve_fn(x, None, curve)
            assert float((pred - case["gt"].double()).abs().min()) >= 1e-3


def test_oracle_clamp_rule_and_white_loss():
    """torch's clamp passes the gradient on the closed interval: shift 1.0 has one, 0.0 and 1.5 have none; white_loss restates
    train_pbr.py:313-316."""
    x = torch.rand(3, 3, dtype=torch.float64) + 0.1
    _, _, gs = plo.tonemap_grads(x, torch.tensor([0.0, 1.5, 1.0]), torch.ones(3, 3), 0, False, torch.float64)
    assert float(gs[0]) == 0.0 and float(gs[1]) == 0.0 and float(gs[2]) != 0.0
    from robir_amd import training
    lgt = torch.randn(16, 7, generator=torch.Generator().manual_seed(0))
    mu = lgt[:, -3:].abs()
    want = (mu / (mu.norm(dim=-1, keepdim=True) + 1e-4)).var(-1).mean() * 0.01
    assert torch.equal(training.white_loss(lgt), want)
    assert float(training.white_loss(torch.ones(4, 7))) == 0.0


@pytest.mark.skipif(not os.path.exists(REFERENCE_LOSS), reason="no reference checkout on this machine")
def test_loss_module_signatures_equal_the_reference():
    """Names, parameter order and defaults of InvLoss, IllumLoss and query_indir_illum, read from the reference's source text (its imports
    are not importable here)."""
    import ast
    from robir_amd import loss as mine
    tree = ast.parse(open(REFERENCE_LOSS).read())

    def sig(fn):
        a = fn.args
        names = [x.arg for x in a.args]
        defaults = [None] * (len(names) - len(a.defaults)) + [ast.literal_eval(d) for d in a.defaults]
        return list(zip(names, defaults))

    def my_sig(fn):
        ps = inspect.signature(fn).parameters.values()
        return [(p.name, None if p.default is inspect.Parameter.empty else p.default) for p in ps]

    seen = 0
    for node in tree.body:
        if isinstance(node, ast.FunctionDef):
            assert my_sig(getattr(mine, node.name)) == sig(node), node.name
            seen += 1
        elif isinstance(node, ast.ClassDef):
            cls = getattr(mine, node.name)
            assert issubclass(cls, torch.nn.Module)
            for item in node.body:
                if isinstance(item, ast.FunctionDef):
                    assert my_sig(getattr(cls, item.name)) == sig(item), (node.name, item.name)
                    seen += 1
    assert seen == 12          # InvLoss: __init__, six get_*, kl_divergence and forward; IllumLoss: two; one function


def test_opt_in_guards():
    """enable_tonemap_training accepts the tone mapper, a GammaCorrect and a model holding .gamma, returns the tone mapper and refuses
    anything else; the mark is off by default; unknown loss types and rb_tonemap's op 2 are refused."""
    from robir_amd import loss, nets, tonemap_autograd, training
    gamma = nets.GammaCorrect()
    tone = gamma.hdr_shift
    holder = torch.nn.Module()
    holder.gamma = gamma
    assert not training.tonemap_training_enabled(tone)
    for obj in (tone, gamma, holder):
        assert training.enable_tonemap_training(obj) is tone and training.tonemap_training_enabled(obj)
        assert training.enable_tonemap_training(obj, on=False) is tone and not training.tonemap_training_enabled(tone)
    with pytest.raises(TypeError, match="enable_tonemap_training"):
        training.enable_tonemap_training(torch.nn.Linear(2, 2))
    z = torch.zeros(2, 3)
    m = torch.ones(2, dtype=torch.bool)
    with pytest.raises(ValueError, match="loss_type"):
        training.photometric_loss(z, z, z, m, m, loss_type="L3")
    with pytest.raises(TypeError, match="photometric_loss"):
        training.photometric_loss(z, z, z, m, m, tone=torch.nn.Linear(2, 2))
    with pytest.raises(NotImplementedError, match="no backward"):
        tonemap_autograd.tonemap(z, torch.ones(1), 0, 2)
    with pytest.raises(Exception, match="Unknown loss_type"):
        loss.InvLoss(0, 0, 0, 50.0, 1.0, 0.01, 0.1, loss_type="huber")
    with pytest.raises(Exception, match="Unknown loss_type"):
        loss.IllumLoss(loss_type="huber")
    assert loss._tone_of(tone.hdr2ldr) is tone and loss._tone_of(tone.ldr2hdr) is None and loss._tone_of(lambda x: x) is None


def test_geometry_terms_against_float64_restatements():
    """InvLoss.get_eikonal_loss / get_mask_loss / get_normal_loss (training.eikonal_loss / mask_loss / normal_loss) in float32 against the
    formulas of model/loss.py:44-59,69-73 written out in float64 here; 1e-6: a mean or a sum of a few hundred fp32 terms of one sign."""
    from robir_amd import loss
    g = torch.Generator().manual_seed(3)
    crit = loss.InvLoss(1.0, 0.1, 100.0, 50.0, 1.0, 0.01, 0.1)
    assert (crit.idr_rgb_weight, crit.eikonal_weight, crit.mask_weight, crit.alpha, crit.sg_rgb_weight, crit.kl_weight,
            crit.latent_smooth_weight, crit.brdf_multires, crit.loss_type) == (1.0, 0.1, 100.0, 50.0, 1.0, 0.01, 0.1, 10, "L1")
    assert isinstance(crit.img_loss, torch.nn.L1Loss) and isinstance(loss.InvLoss(0, 0, 0, 1.0, 1, 1, 1, loss_type="L2").img_loss, torch.nn.MSELoss)
    n = 300
    grad = torch.randn(n, 3, generator=g)
    want = ((grad.double() ** 2).sum(1).sqrt() - 1).pow(2).sum() / n
    assert rel_err(crit.get_eikonal_loss(grad), want) <= 1e-6
    assert float(crit.get_eikonal_loss(torch.zeros(0, 3))) == 0.0
    sdf = 0.05 * torch.randn(n, 1, generator=g)
    hit, inside = torch.rand(n, generator=g) < 0.6, torch.rand(n, generator=g) < 0.7
    rows = ~(hit & inside)
    z = -50.0 * sdf.double()[rows, 0]
    y = inside[rows].double()
    bce = (torch.clamp(z, min=0) - z * y + torch.log1p(torch.exp(-z.abs()))).sum()          # -y log s(z) - (1 - y) log(1 - s(z))
    assert rel_err(crit.get_mask_loss(sdf, hit, inside), bce / 50.0 / n) <= 1e-6
    every = torch.ones(n, dtype=torch.bool)
    assert float(crit.get_mask_loss(sdf, every, every)) == 0.0
    nm, nr = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
    want = (nm.double()[hit] - nr.double()[hit]).pow(2).sum() / (3 * int(hit.sum()))
    assert rel_err(crit.get_normal_loss({"surface_mask": hit, "normal_map": nm, "normals": nr}), want) <= 1e-6
    lat = torch.randn(n, 32, generator=g)
    rho_hat = torch.sigmoid(lat.double()).mean(0)
    want = (0.05 * torch.log(0.05 / (rho_hat + 1e-4)) + 0.95 * torch.log(0.95 / (1 - rho_hat + 1e-4))).mean()
    assert rel_err(crit.kl_divergence(0.05, lat), want) <= 1e-5
    a, b = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
    ra, rb = torch.rand(n, 1, generator=g), torch.rand(n, 1, generator=g)
    want = (a.double() - b.double()).abs().mean() + 0.2 * (ra.double() - rb.double()).abs().mean()
    out = {"diffuse_albedo": a, "roughness": ra, "random_xi_diffuse_albedo": b, "random_xi_roughness": rb}
    assert rel_err(crit.get_latent_smooth_loss(out), want) <= 1e-6
