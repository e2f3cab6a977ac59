"""The training library and the opt-in for material training, as far as they go without a GPU: loading, the export list, argument errors
before any launch, the guard's behaviour with and without the mark, the refusals, and the two loss helpers against a float64 restatement of
model/loss.py."""
import ctypes
import os
import re
import subprocess
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return sorted(set(re.findall(r"^(?:int|long|const char\*) (rb_[a-z0-9_]+)\s*\(", hdr, re.M)))


def _train_lib():
    from robir_amd import _lib
    if not os.path.exists(_lib.TRAIN_PATH):
        _lib.build(legacy=False)
    return _lib.train()


def test_train_library_exports_its_header():
    """librobir_hip_train.so loads without a GPU and exports exactly what include/robir_hip_train.h declares; no rb_ name is shared with the
    other two headers, whose libraries keep their export lists."""
    from robir_amd import _lib
    L = _train_lib()
    assert L.rb_train_abi_version() == _lib.TRAIN_ABI_VERSION == 1
    syms = _header_symbols("robir_hip_train.h")
    assert len(syms) == 4 and all(s.startswith("rb_train_") for s in syms)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.TRAIN_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[-1] for l in out.splitlines() if " T rb_" in l) == syms
    assert not set(syms) & (set(_header_symbols("robir_hip.h")) | set(_header_symbols("robir_hip_legacy.h")))
    assert len(_header_symbols("robir_hip.h")) <= 100
    # scratch: a function of min(n, slab_rows), not of n
    q = L.rb_train_ae_bwd_scratch_bytes
    a, b, c = q(ctypes.c_long(1 << 20), ctypes.c_long(4096), 63, 5), q(ctypes.c_long(4096), ctypes.c_long(16384), 63, 5), q(ctypes.c_long(64), ctypes.c_long(4096), 63, 5)
    assert a == b and 0 < c < a and a % 8 == 0


def test_train_library_argument_errors_before_any_launch():
    L = _train_lib()
    null = ctypes.c_void_p(0)
    arr = (ctypes.c_void_p * 16)()

    def call(X=null, n=8, params=arr, grads=arr, slab=64, scratch=null, in_dim=63, out_dim=5, lat=0):
        return L.rb_train_ae_bwd(X, ctypes.c_long(n), in_dim, null, ctypes.c_double(0.01), null, lat, 1, out_dim, params, null, null, null, grads,
                                 ctypes.c_long(slab), scratch, ctypes.c_long(0), None, null)
    assert call() != 0 and b"null pointer" in L.rb_train_last_error()
    assert call(params=None) != 0 and b"null pointer" in L.rb_train_last_error()
    assert call(n=0) == 0                                       # nothing to do: no launch, no error
    assert call(slab=0) != 0 and b"slab_rows" in L.rb_train_last_error()
    assert call(out_dim=17) != 0 and b"out_dim" in L.rb_train_last_error()
    assert call(in_dim=65) != 0 and b"in_dim" in L.rb_train_last_error()
    assert call(lat=2) != 0 and b"latent_act" in L.rb_train_last_error()
    assert L.rb_train_ae_bwd_scratch_bytes(ctypes.c_long(8), ctypes.c_long(0), 63, 5) == -1


def test_missing_train_library_has_its_own_message(monkeypatch, tmp_path):
    from robir_amd import _lib
    monkeypatch.setattr(_lib, "_train", None)
    monkeypatch.setattr(_lib, "TRAIN_PATH", str(tmp_path / "nope_train.so"))
    with pytest.raises(_lib.RobirHipError, match="TRAINING library") as e:
        _lib.call_train("rb_train_ae_bwd")
    assert "LEGACY" not in str(e.value)


def test_guard_with_and_without_the_mark():
    """The mark lets the material network and its spec auto-encoder through forward_only_guard; unmarked sub-networks and every other
    network still raise; unmarking restores today's behaviour."""
    from robir_amd import nets, renderer, training
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = renderer.IDRNetwork(renderer.hotdog_conf())
    mat = m.envmap_material_network
    x = torch.zeros(4, 3)
    with torch.enable_grad():
        m.train()
        with pytest.raises(nets.ForwardOnlyError):
            nets.forward_only_guard(mat)
        assert training.enable_material_training(m) is mat and training.material_training_enabled(m)
        nets.forward_only_guard(mat)
        nets.forward_only_guard(mat.spec_brdf_encoder_layer)
        for sub in (mat.normal_decoder_layer, mat.brdf_encoder_layer, m.visibility_network, m.indirect_illum_network, m.implicit_network, m):
            with pytest.raises(nets.ForwardOnlyError):
                nets.forward_only_guard(sub)
        with pytest.raises(nets.ForwardOnlyError):
            mat.normal_decoder_layer.run_pass(torch.zeros(4, 64))
        with pytest.raises(nets.ForwardOnlyError):
            mat.brdf_encoder_layer(torch.zeros(4, 63))
        with pytest.raises(nets.ForwardOnlyError):
            m.visibility_network(x, x)
        # a point that requires grad is refused before any kernel
        with pytest.raises(NotImplementedError, match="points"):
            mat(x.clone().requires_grad_(), train_spec=True)
        training.enable_material_training(m, on=False)
        assert not training.material_training_enabled(m)
        with pytest.raises(nets.ForwardOnlyError):
            mat(x, train_spec=True)
        with pytest.raises(nets.ForwardOnlyError):
            mat.spec_brdf_encoder_layer.encode(torch.zeros(4, 63))


def test_marking_an_input_perturbed_autoencoder_is_refused():
    from robir_amd import nets, training
    mat = nets.EnvmapMaterialNetwork(multires=10, num_lgt_sgs=128)
    illum = nets.IndirctIllumNetwork(multires=10, dims=[512] * 4, num_lgt_sgs=24)
    for ae in (mat.normal_decoder_layer, illum.integral_layer):
        with pytest.raises(NotImplementedError, match="not built") as e:
            training.enable_material_training(ae)
        assert "OUT OF SCOPE" not in str(e.value) and not getattr(ae, "_material_training", False)
    with pytest.raises(TypeError):
        training.enable_material_training(illum)
    assert training.enable_material_training(mat.spec_brdf_encoder_layer) is mat.spec_brdf_encoder_layer


def test_loss_helpers_equal_the_reference_formulas():
    """kl_sparsity / latent_smooth against a float64 restatement of model/loss.py:61-79 written out here."""
    from robir_amd import training
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(37, 32, generator=g, dtype=torch.float64) * 2
    rho = 0.05
    rho_hat = torch.sigmoid(lat).mean(0)
    want = sum(rho * torch.log(rho / (r + 1e-4)) + (1 - rho) * torch.log((1 - rho) / (1 - r + 1e-4)) for r in rho_hat) / 32
    assert abs(float(training.kl_sparsity(lat)) - float(want)) <= 1e-14
    assert abs(float(training.kl_sparsity(lat.float())) - float(want)) <= 1e-6
    out = {"diffuse_albedo": torch.rand(37, 3, generator=g, dtype=torch.float64), "roughness": torch.rand(37, 1, generator=g, dtype=torch.float64),
           "random_xi_diffuse_albedo": torch.rand(37, 3, generator=g, dtype=torch.float64),
           "random_xi_roughness": torch.rand(37, 1, generator=g, dtype=torch.float64)}
    want = torch.nn.L1Loss()(out["diffuse_albedo"], out["random_xi_diffuse_albedo"]) \
        + torch.nn.L1Loss()(out["roughness"][..., 0], out["random_xi_roughness"][..., 0]) * 0.2
    assert abs(float(training.latent_smooth(out)) - float(want)) <= 1e-15
    net_keys = {"sg_diffuse_albedo": out["diffuse_albedo"], "sg_roughness": out["roughness"],
                "random_xi_diffuse_albedo": out["random_xi_diffuse_albedo"], "random_xi_roughness": out["random_xi_roughness"]}
    assert float(training.latent_smooth(net_keys)) == float(training.latent_smooth(out))
    with torch.enable_grad():
        x = lat.clone().requires_grad_()
        training.kl_sparsity(x).backward()
    assert x.grad is not None and float(x.grad.abs().max()) > 0
