"""The illumination-training library and the opt-in for indirect-illumination training, as far as they go without a GPU: loading, the export
list, argument errors before any launch, the scratch query, the guard's behaviour with and without the mark, and radiance_loss against a
float64 loop-written restatement of model/loss.py:156-171."""
import ctypes
import os
import re
import subprocess
import warnings

import pytest
import torch

import illum_train_oracle as ito

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c_long = ctypes.c_long


def _header_symbols(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return sorted(set(re.findall(r"^(?:int|long|const char\*) (rb_[a-z0-9_]+)\s*\(", hdr, re.M)))


def _it_lib():
    from robir_amd import _lib
    if not os.path.exists(_lib.ILLUMTRAIN_PATH):
        _lib.build(legacy=False)
    return _lib.illumtrain()


def test_illumtrain_library_exports_its_header():
    """librobir_hip_illumtrain.so loads without a GPU and exports exactly what include/robir_hip_illumtrain.h declares, every name rb_it_*;
    no rb_ name is shared with the other four headers."""
    from robir_amd import _lib
    L = _it_lib()
    assert L.rb_it_abi_version() == _lib.ILLUMTRAIN_ABI_VERSION == 1
    syms = _header_symbols("robir_hip_illumtrain.h")
    assert syms == ["rb_it_abi_version", "rb_it_last_error", "rb_it_lobe_bwd", "rb_it_lobe_bwd_scratch_bytes", "rb_it_sg_query",
                    "rb_it_sg_query_bwd"]
    assert all(s.startswith("rb_it_") for s in syms)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.ILLUMTRAIN_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[-1] for l in out.splitlines() if " T rb_" in l) == syms
    others = set()
    for h in ("robir_hip.h", "robir_hip_legacy.h", "robir_hip_train.h", "robir_hip_vistrain.h"):
        others |= set(_header_symbols(h))
    assert not set(syms) & others


def test_scratch_query_depends_on_the_slab_not_on_the_batch():
    L = _it_lib()
    q = lambda n, slab, part: L.rb_it_lobe_bwd_scratch_bytes(c_long(n), c_long(slab), c_long(part))
    a, b, c = q(1 << 20, 4096, 512), q(4096, 16384, 512), q(64, 4096, 512)
    assert a == b and 0 < c < a and a % 8 == 0
    assert q(1 << 20, 4096, 4096) < a < q(1 << 20, 4096, 256)          # more partitions, more partials
    # the header's figures: 26240 B per slab row = (64 + 4 x 512 + 144 + 2 x 512) doubles, one 512 x 513 fp64 partial per partition ...
    assert 26240 == 8 * (64 + 4 * 512 + 144 + 2 * 512) and 2101248 == 8 * 512 * 513
    assert q(8192, 8192, 512) - q(4096, 4096, 512) == 4096 * 26240 + 8 * 2101248
    # ... and 7160960 B of accumulators (512 x 65 + 3 x 512 x 513 + 144 x 513 doubles): the Python defaults' 148 MB
    assert q(8, 8, 8) == 8 * 26240 + 2101248 + 7160960 == q(8, 64, 8)
    assert q(4096, 4096, 256) == 4096 * 26240 + 16 * 2101248 + 7160960
    assert q(8, 0, 1) == -1 and b"slab_rows" in L.rb_it_last_error()
    assert q(8, 64, 65) == -1 and b"part_rows" in L.rb_it_last_error()
    assert q(8, (1 << 20) + 1, 1) == -1


def test_illumtrain_library_argument_errors_before_any_launch():
    """Every call here is refused (or has nothing to do) before a launch: the non-null pointers are never dereferenced."""
    L = _it_lib()
    null = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(4096)                    # 8-byte aligned, never read
    nulls = (ctypes.c_void_p * 10)()
    full = (ctypes.c_void_p * 10)(*[4096] * 10)
    err = L.rb_it_last_error

    def call(points=fake, hdr=fake, n=8, params=full, g=fake, grads=full, slab=64, part=16, scratch=fake, nbytes=1 << 40):
        return L.rb_it_lobe_bwd(points, hdr, c_long(n), params, g, grads, c_long(slab), c_long(part), scratch, c_long(nbytes), None, null)
    assert call(params=None) != 0 and b"null pointer" in err()
    assert call(grads=None) != 0 and b"null pointer" in err()
    assert call(points=null) != 0 and b"null pointer" in err()
    assert call(params=nulls) != 0 and b"params[0]" in err()
    assert call(part=65) != 0 and b"part_rows" in err()
    assert call(slab=0) != 0 and b"slab_rows" in err()
    assert call(slab=(1 << 20) + 1) != 0 and b"slab_rows" in err()
    need = L.rb_it_lobe_bwd_scratch_bytes(c_long(8), c_long(64), c_long(16))
    assert call(nbytes=need - 8) != 0 and b"scratch too small" in err()
    assert call(scratch=ctypes.c_void_p(4100)) != 0 and b"aligned" in err()
    assert call(scratch=null) != 0 and b"null pointer" in err()
    # nothing to do: no launch, no error -- n = 0 (whatever the other pointers), or no gradient wanted
    stats = (ctypes.c_int * 3)(7, 7, 7)
    assert L.rb_it_lobe_bwd(null, null, c_long(0), nulls, null, nulls, c_long(64), c_long(16), null, c_long(0), stats, null) == 0
    assert list(stats) == [0, 5, 0]
    stats = (ctypes.c_int * 3)(7, 7, 7)
    assert L.rb_it_lobe_bwd(fake, fake, c_long(8), full, fake, nulls, c_long(64), c_long(16), null, c_long(0), stats, null) == 0
    assert list(stats) == [0, 5, 0]
    # the query: the lobe count and null pointers
    for lobes in (0, 33):
        assert L.rb_it_sg_query(fake, fake, c_long(4), lobes, c_long(8), fake, null) != 0 and b"L = " in err()
        assert L.rb_it_sg_query_bwd(fake, fake, fake, c_long(4), lobes, c_long(8), fake, null) != 0 and b"L = " in err()
    assert L.rb_it_sg_query(null, fake, c_long(4), 24, c_long(8), fake, null) != 0 and b"null pointer" in err()
    assert L.rb_it_sg_query_bwd(fake, fake, null, c_long(4), 24, c_long(8), fake, null) != 0 and b"null pointer" in err()
    assert L.rb_it_sg_query(null, null, c_long(0), 24, c_long(8), null, null) == 0
    assert L.rb_it_sg_query_bwd(null, null, null, c_long(0), 24, c_long(8), null, null) == 0


def test_missing_illumtrain_library_has_its_own_message(monkeypatch, tmp_path):
    from robir_amd import _lib
    monkeypatch.setattr(_lib, "_illumtrain", None)
    monkeypatch.setattr(_lib, "ILLUMTRAIN_PATH", str(tmp_path / "nope_illumtrain.so"))
    with pytest.raises(_lib.RobirHipError, match="ILLUMINATION-TRAINING library") as e:
        _lib.call_illumtrain("rb_it_lobe_bwd")
    msg = str(e.value)
    assert "make -C robir_amd/csrc illumtrain" in msg and "librobir_hip_illumtrain.so" in msg
    assert "LEGACY" not in msg and "librobir_hip_train.so" not in msg and "librobir_hip_vistrain.so" not in msg
    assert "librobir_hip.so" not in msg and "librobir_hip_legacy.so" not in msg


def test_guard_with_and_without_the_mark():
    """The mark lets the indirect-illumination network through forward_only_guard; an unmarked IndirctIllumNetwork and every other network
    still raise; unmarking restores today's behaviour."""
    from robir_amd import nets, renderer, training
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = renderer.IDRNetwork(renderer.hotdog_conf())
    ill = m.indirect_illum_network
    other = nets.IndirctIllumNetwork(multires=10, dims=[512] * 4, num_lgt_sgs=24)
    x, h = torch.zeros(4, 3), torch.zeros(4, 1)
    with torch.enable_grad():
        m.train()
        other.train()
        with pytest.raises(nets.ForwardOnlyError):
            nets.forward_only_guard(ill)
        assert not training.illumination_training_enabled(m)
        assert training.enable_illumination_training(m) is ill
        assert training.illumination_training_enabled(m) and training.illumination_training_enabled(ill)
        assert not training.illumination_training_enabled(other)
        assert not training.material_training_enabled(m) and not training.visibility_training_enabled(m)
        nets.forward_only_guard(ill)
        assert ill._trainable()
        for sub in (other, ill.integral_layer, m.visibility_network, m.envmap_material_network,
                    m.envmap_material_network.spec_brdf_encoder_layer, m.implicit_network, m):
            with pytest.raises(nets.ForwardOnlyError):
                nets.forward_only_guard(sub)
        with pytest.raises(nets.ForwardOnlyError):
            other(x, h)
        # inputs that require grad are refused before any kernel
        with pytest.raises(NotImplementedError, match="points"):
            ill(x.clone().requires_grad_(), h)
        with pytest.raises(NotImplementedError, match="hdr_shift"):
            ill(x, h.clone().requires_grad_())
        with pytest.raises(NotImplementedError, match="noise"):
            ill(x, h, noise=torch.zeros(4, 64, requires_grad=True))
        with pytest.raises(NotImplementedError, match="sample_dirs"):
            training.query_indir_illum(torch.zeros(4, 24, 7), torch.zeros(4, 2, 3, requires_grad=True))
        # the stand-alone integral layer keeps its refusals
        with pytest.raises(NotImplementedError, match="not built"):
            training.enable_material_training(ill.integral_layer)
        # frozen parameters, or grad mode off: not trainable, today's path
        for p in ill.parameters():
            p.requires_grad_(False)
        assert not ill._trainable()
        for p in ill.parameters():
            p.requires_grad_(True)
        with torch.no_grad():
            assert not ill._trainable()
        assert training.enable_illumination_training(ill, on=False) is ill
        assert not training.illumination_training_enabled(m) and not ill._trainable()
        with pytest.raises(nets.ForwardOnlyError):
            ill(x, h)


def test_enable_illumination_training_refuses_other_types():
    from robir_amd import nets, training
    for wrong in (nets.VisNetwork(points_multires=10, dirs_multires=10, dims=[256] * 4), nets.SparseAE(64, 3, out_act=None, smooth_on_latent=False),
                  torch.nn.Linear(3, 3), object()):
        with pytest.raises(TypeError, match="IndirctIllumNetwork"):
            training.enable_illumination_training(wrong)
        assert not training.illumination_training_enabled(wrong)


@pytest.mark.parametrize("loss_type", ["L1", "L2"])
def test_radiance_loss_equals_the_reference_formula(loss_type):
    """radiance_loss against a float64 restatement of model/loss.py:156-171 written out as loops here, the query injected in plain torch
    (the oracle's restatement of query_indir_illum); the masks leave some points and some samples out."""
    from robir_amd import training
    g = torch.Generator().manual_seed(3)
    N, S, L, t = 19, 6, 24, 0.25
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sgs = torch.cat([rnd(N, L, 3) * 1.7, rnd(N, L, 1).abs() * 5 + 0.1, rnd(N, L, 3).abs()], -1)
    points_mask = torch.rand(N, generator=g) < 0.7
    n = int(points_mask.sum())
    assert 0 < n < N
    indir_mask = (torch.rand(N, S, generator=g) < 0.6) & points_mask[:, None]
    assert 0 < int(indir_mask.sum()) < n * S
    dirs = torch.nn.functional.normalize(rnd(n, S, 3), dim=-1)
    model_out = {"network_object_mask": points_mask, "indirect_sgs": sgs, "indir_integral": rnd(N, 3).abs()}
    trace = {"indir_mask": indir_mask, "trace_radiance": rnd(N, S, 3).abs(), "sample_dirs": dirs, "gt_integral": rnd(N, 3).abs()}

    dist = (lambda a, b: abs(a - b)) if loss_type == "L1" else (lambda a, b: (a - b) ** 2)
    rad_sum = rad_cnt = int_sum = int_cnt = 0
    row = 0
    for i in range(N):
        if not bool(points_mask[i]):
            continue
        for s in range(S):
            if bool(indir_mask[i, s]):
                for c in range(3):
                    pred = 0.0
                    for j in range(L):
                        axis = sgs[i, j, :3] / float(torch.sqrt((sgs[i, j, :3] ** 2).sum()))
                        pred += float(sgs[i, j, 4 + c]) * float(torch.exp(sgs[i, j, 3] * (float((dirs[row, s] * axis).sum()) - 1.0)))
                    rad_sum += dist(float(trace["trace_radiance"][i, s, c]) + t, pred)
                    rad_cnt += 1
        for c in range(3):
            int_sum += dist(float(trace["gt_integral"][i, c]), float(model_out["indir_integral"][i, c]))
            int_cnt += 1
        row += 1
    want = rad_sum / rad_cnt + int_sum / int_cnt
    got = training.radiance_loss(model_out, trace, anneal_t=t, loss_type=loss_type, query=ito.query)
    assert abs(float(got) - want) <= 1e-12 * max(1.0, want)
    f32 = lambda d: {k: (v.float() if v.is_floating_point() else v) for k, v in d.items()}
    assert abs(float(training.radiance_loss(f32(model_out), f32(trace), t, loss_type, query=ito.query)) - want) <= 1e-5 * max(1.0, want)
    with pytest.raises(ValueError):
        training.radiance_loss(model_out, trace, loss_type="huber", query=ito.query)
    with torch.enable_grad():
        x = sgs.clone().requires_grad_()
        training.radiance_loss(dict(model_out, indirect_sgs=x), trace, t, loss_type, query=ito.query).backward()
    assert float(x.grad[points_mask].abs().max()) > 0 and float(x.grad[~points_mask].abs().max()) == 0
