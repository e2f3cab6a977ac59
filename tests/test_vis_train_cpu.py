"""The visibility-training library and the opt-in for visibility training, as far as they go without a GPU: loading, the export list,
argument errors before any launch, the scratch query, the guard's behaviour with and without the mark, and visibility_loss against a float64
restatement of model/loss.py:173-177."""
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


def _vt_lib():
    from robir_amd import _lib
    if not os.path.exists(_lib.VISTRAIN_PATH):
        _lib.build(legacy=False)
    return _lib.vistrain()


def test_vistrain_library_exports_its_header():
    """librobir_hip_vistrain.so loads without a GPU and exports exactly what include/robir_hip_vistrain.h declares, every name rb_vt_*; no
    rb_ name is shared with the other three headers."""
    from robir_amd import _lib
    L = _vt_lib()
    assert L.rb_vt_abi_version() == _lib.VISTRAIN_ABI_VERSION == 1
    syms = _header_symbols("robir_hip_vistrain.h")
    assert syms == ["rb_vt_abi_version", "rb_vt_last_error", "rb_vt_vis_bwd", "rb_vt_vis_bwd_scratch_bytes"]
    assert all(s.startswith("rb_vt_") for s in syms)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.VISTRAIN_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[-1] for l in out.splitlines() if " T rb_" in l) == syms
    others = set(_header_symbols("robir_hip.h")) | set(_header_symbols("robir_hip_legacy.h")) | set(_header_symbols("robir_hip_train.h"))
    assert not set(syms) & others


def test_scratch_query_depends_on_the_slab_not_on_the_batch():
    L = _vt_lib()
    q = lambda M, slab, part: L.rb_vt_vis_bwd_scratch_bytes(ctypes.c_long(M), ctypes.c_long(slab), ctypes.c_long(part))
    a, b, c = q(1 << 20, 4096, 512), q(4096, 16384, 512), q(64, 4096, 512)
    assert a == b and 0 < c < a and a % 8 == 0
    assert q(1 << 20, 4096, 4096) < a < q(1 << 20, 4096, 256)          # more partitions, more partials
    # the header's figures: 13312 B per slab row and one 256 x 257 fp64 partial per partition
    assert q(8192, 8192, 512) - q(4096, 4096, 512) == 4096 * 13312 + 8 * 256 * 257 * 8
    assert q(8, 0, 1) == -1 and b"slab_rows" in L.rb_vt_last_error()
    assert q(8, 64, 65) == -1 and b"part_rows" in L.rb_vt_last_error()
    assert q(8, (1 << 20) + 1, 1) == -1


def test_vistrain_library_argument_errors_before_any_launch():
    """Every call here is refused (or has nothing to do) before a launch: the non-null pointers are never dereferenced."""
    L = _vt_lib()
    null = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(4096)                    # 8-byte aligned, never read
    nulls = (ctypes.c_void_p * 10)()
    full = (ctypes.c_void_p * 10)(*[4096] * 10)
    err = L.rb_vt_last_error

    def call(p=fake, d=fake, M=8, rep=1, params=full, g=fake, grads=full, slab=64, part=16, scratch=fake, nbytes=1 << 40):
        return L.rb_vt_vis_bwd(p, d, ctypes.c_long(M), rep, params, g, grads, ctypes.c_long(slab), ctypes.c_long(part), scratch,
                               ctypes.c_long(nbytes), None, null)
    assert call(params=None) != 0 and b"null pointer" in err()
    assert call(grads=None) != 0 and b"null pointer" in err()
    assert call(p=null) != 0 and b"null pointer" in err()
    assert call(params=nulls) != 0 and b"params[0]" in err()
    assert call(M=9, rep=2) != 0 and b"multiple of rep" in err()
    assert call(rep=0) != 0 and b"rep" in err()
    assert call(part=65) != 0 and b"part_rows" in err()
    assert call(slab=0) != 0 and b"slab_rows" in err()
    need = L.rb_vt_vis_bwd_scratch_bytes(ctypes.c_long(8), ctypes.c_long(64), ctypes.c_long(16))
    assert call(nbytes=need - 8) != 0 and b"scratch too small" in err()
    assert call(scratch=ctypes.c_void_p(4100)) != 0 and b"aligned" in err()
    assert call(scratch=null) != 0 and b"null pointer" in err()
    # nothing to do: no launch, no error -- M = 0 (whatever the other pointers), or no gradient wanted
    stats = (ctypes.c_int * 3)(7, 7, 7)
    assert L.rb_vt_vis_bwd(null, null, ctypes.c_long(0), 1, nulls, null, nulls, ctypes.c_long(64), ctypes.c_long(16), null, ctypes.c_long(0),
                           stats, null) == 0
    assert list(stats) == [0, 5, 0]
    assert call(grads=nulls, scratch=null, nbytes=0) == 0


def test_missing_vistrain_library_has_its_own_message(monkeypatch, tmp_path):
    from robir_amd import _lib
    monkeypatch.setattr(_lib, "_vistrain", None)
    monkeypatch.setattr(_lib, "VISTRAIN_PATH", str(tmp_path / "nope_vistrain.so"))
    with pytest.raises(_lib.RobirHipError, match="VISIBILITY-TRAINING library") as e:
        _lib.call_vistrain("rb_vt_vis_bwd")
    assert "make -C robir_amd/csrc vistrain" in str(e.value) and "librobir_hip_vistrain.so" in str(e.value)
    assert "LEGACY" not in str(e.value) and "librobir_hip_train.so" not in str(e.value)


def test_guard_with_and_without_the_mark():
    """The mark lets the visibility network through forward_only_guard; an unmarked VisNetwork and every other network still raise;
    unmarking restores today's behaviour."""
    from robir_amd import nets, renderer, training
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = renderer.IDRNetwork(renderer.hotdog_conf())
    vis = m.visibility_network
    other = nets.VisNetwork(points_multires=10, dirs_multires=10, dims=[256] * 4)
    x = torch.zeros(4, 3)
    with torch.enable_grad():
        m.train()
        other.train()
        with pytest.raises(nets.ForwardOnlyError):
            nets.forward_only_guard(vis)
        assert not training.visibility_training_enabled(m)
        assert training.enable_visibility_training(m) is vis
        assert training.visibility_training_enabled(m) and training.visibility_training_enabled(vis)
        assert not training.visibility_training_enabled(other) and not training.material_training_enabled(m)
        nets.forward_only_guard(vis)
        assert vis._trainable()
        for sub in (other, m.envmap_material_network, m.envmap_material_network.spec_brdf_encoder_layer, m.indirect_illum_network,
                    m.implicit_network, m):
            with pytest.raises(nets.ForwardOnlyError):
                nets.forward_only_guard(sub)
        with pytest.raises(nets.ForwardOnlyError):
            other(x, x)
        # inputs that require grad are refused before any kernel, and so is the feature-row form
        with pytest.raises(NotImplementedError, match="points"):
            vis(x.clone().requires_grad_(), x)
        with pytest.raises(NotImplementedError, match="dirs"):
            vis.logits_from_points(x, x.clone().requires_grad_())
        with pytest.raises(NotImplementedError, match="logits_from_points"):
            vis.logits_from_features(torch.zeros(4, 128))
        # frozen parameters, or grad mode off: not trainable, today's path
        for p in vis.parameters():
            p.requires_grad_(False)
        assert not vis._trainable()
        for p in vis.parameters():
            p.requires_grad_(True)
        with torch.no_grad():
            assert not vis._trainable()
        assert training.enable_visibility_training(vis, on=False) is vis
        assert not training.visibility_training_enabled(m)
        with pytest.raises(nets.ForwardOnlyError):
            vis(x, x)
        with pytest.raises(nets.ForwardOnlyError):
            vis.logits_from_features(torch.zeros(4, 128))


def test_enable_visibility_training_refuses_other_types():
    from robir_amd import nets, training
    for wrong in (nets.EnvmapMaterialNetwork(multires=10, num_lgt_sgs=128), torch.nn.Linear(3, 3), object()):
        with pytest.raises(TypeError, match="VisNetwork"):
            training.enable_visibility_training(wrong)
        assert not training.visibility_training_enabled(wrong)


def test_visibility_loss_equals_the_reference_formula():
    """visibility_loss against a float64 restatement of model/loss.py:173-177 written out here: the class index is the negated traced label,
    the loss the mean over the masked rows of -log softmax(logits)[class]."""
    from robir_amd import training
    g = torch.Generator().manual_seed(0)
    N, S = 23, 8
    pred = torch.randn(N, S, 2, generator=g, dtype=torch.float64) * 3
    gt = torch.rand(N, S, 1, generator=g) < 0.4
    mask = torch.rand(N, generator=g) < 0.7
    assert 0 < int(mask.sum()) < N
    total, rows = 0.0, 0
    for i in range(N):
        if not bool(mask[i]):
            continue
        for s in range(S):
            cls = 0 if bool(gt[i, s, 0]) else 1
            z = pred[i, s]
            total += float(torch.log(torch.exp(z[0]) + torch.exp(z[1])) - z[cls])
            rows += 1
    want = total / rows
    assert abs(float(training.visibility_loss(pred, gt, mask)) - want) <= 1e-13
    assert abs(float(training.visibility_loss(pred.float(), gt, mask)) - want) <= 1e-6
    with torch.enable_grad():
        x = pred.clone().requires_grad_()
        training.visibility_loss(x, gt, mask).backward()
    assert float(x.grad[mask].abs().min()) > 0 and float(x.grad[~mask].abs().max()) == 0
