"""The CESR-training library and the opt-in for shadow_net / normal_net training, as far as they go without a GPU: loading, the export list,
argument errors before any launch, the scratch query against the header's formula, the guard with and without the mark, and the float64 oracle
(tests/cesr_train_oracle.py) against the reference fixture tests/golden/cesr_grad.npz / cesr_grad_normal.npz (tools/gen_cesr_grad_golden.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cesr_train_oracle as cto
from conftest import load_golden, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c_long, c_int = ctypes.c_long, ctypes.c_int


def _header_symbols(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return sorted(set(re.findall(r"^(?:int|long|const char\*) (rb_[a-z0-9_]+)\s*\(", hdr, re.M)))


def _ct_lib():
    from robir_amd import _lib
    if not os.path.exists(_lib.CESRTRAIN_PATH):
        _lib.build(legacy=False)
    return _lib.cesrtrain()


def test_cesrtrain_library_exports_its_header():
    """librobir_hip_cesrtrain.so loads without a GPU and exports exactly what include/robir_hip_cesrtrain.h declares, every name rb_ct_*; no
    rb_ name is shared with the other five headers, and none of them names this one."""
    from robir_amd import _lib
    L = _ct_lib()
    assert L.rb_ct_abi_version() == _lib.CESRTRAIN_ABI_VERSION == 1
    syms = _header_symbols("robir_hip_cesrtrain.h")
    assert syms == ["rb_ct_abi_version", "rb_ct_cesr_bwd", "rb_ct_cesr_bwd_scratch_bytes", "rb_ct_last_error"]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.CESRTRAIN_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[-1] for l in out.splitlines() if " T rb_" in l) == syms
    others = set()
    for h in ("robir_hip.h", "robir_hip_legacy.h", "robir_hip_train.h", "robir_hip_vistrain.h", "robir_hip_illumtrain.h"):
        others |= set(_header_symbols(h))
        assert "rb_ct_" not in open(os.path.join(ROOT, "include", h)).read() and "cesrtrain" not in open(os.path.join(ROOT, "include", h)).read()
    assert not set(syms) & others


def test_scratch_query_matches_the_header():
    L = _ct_lib()
    q = lambda M, slab, part: L.rb_ct_cesr_bwd_scratch_bytes(c_long(M), c_long(slab), c_long(part))
    # the header's figures: 42560 B per slab row = (192 + 8 x 512 + 8 + 2 x 512) doubles, one 512 x 513 fp64 partial per partition, and
    # 30986304 B fixed = folded weights (512 x 192 + 7 x 512 x 512 + 3 x 512) + accumulators (512 x 192 + 7 x 512 x 513 + 3 x 513 -> 1544)
    row, part, fixed = 42560, 2101248, 30986304
    assert row == 8 * (192 + 8 * 512 + 8 + 2 * 512) and part == 8 * 512 * 513
    assert fixed == 8 * (512 * 192 + 7 * 512 * 512 + 3 * 512 + 512 * 192 + 7 * 512 * 513 + 1544)
    for M, slab, pr in ((8, 8, 8), (8, 64, 8), (200, 64, 48), (120320, 16384, 1024), (1 << 20, 4096, 512), (5, 1 << 20, 1)):
        S = min(M, slab)
        assert q(M, slab, pr) == S * row + -(-S // pr) * part + fixed, (M, slab, pr)
    assert q(1 << 20, 4096, 512) == q(4096, 16384, 512) and q(64, 4096, 512) < q(4096, 4096, 512)          # the slab, not the batch
    hdr = open(os.path.join(ROOT, "include", "robir_hip_cesrtrain.h")).read()
    assert all(str(v) + " B" in hdr for v in (row, part, fixed))
    assert q(8, 0, 1) == -1 and b"slab_rows" in L.rb_ct_last_error()
    assert q(8, 64, 65) == -1 and b"part_rows" in L.rb_ct_last_error()
    assert q(8, (1 << 20) + 1, 1) == -1


def test_cesrtrain_library_argument_errors_before_any_launch():
    """Every call here is refused (or has nothing to do) before a launch: the non-null pointers are never dereferenced."""
    L = _ct_lib()
    null = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(4096)                    # 8-byte aligned, never read
    nulls = (ctypes.c_void_p * 27)()
    full = (ctypes.c_void_p * 27)(*[4096] * 27)
    err = L.rb_ct_last_error

    def call(points=fake, rows=null, ld=0, M=256, kind=1, n_label=128, head=1, params=full, g=fake, grads=full, slab=64, part=16, scratch=fake,
             nbytes=1 << 40, stats=None):
        return L.rb_ct_cesr_bwd(points, rows, c_long(ld), c_long(M), c_int(kind), c_int(n_label), c_int(head), params, g, grads, c_long(slab),
                                c_long(part), scratch, c_long(nbytes), stats, null)
    assert call(params=None) != 0 and b"null pointer" in err()
    assert call(grads=None) != 0 and b"null pointer" in err()
    assert call(params=nulls) != 0 and b"params[0]" in err()
    assert call(M=255) != 0 and b"multiple of n_label" in err()
    assert call(n_label=0) != 0 and b"n_label" in err()
    assert call(n_label=129, M=258) != 0 and b"n_label" in err()
    assert call(part=65) != 0 and b"part_rows" in err()
    assert call(slab=0) != 0 and b"slab_rows" in err()
    assert call(slab=(1 << 20) + 1) != 0 and b"slab_rows" in err()
    need = L.rb_ct_cesr_bwd_scratch_bytes(c_long(256), c_long(64), c_long(16))
    assert call(nbytes=need - 8) != 0 and b"scratch too small" in err()
    assert call(scratch=ctypes.c_void_p(4100)) != 0 and b"aligned" in err()
    assert call(scratch=null) != 0 and b"null pointer" in err()
    for head, kind in ((3, 1), (-1, 0), (1, 0), (2, 1)):          # a bad head code; a head of the other network
        assert call(head=head, kind=kind, n_label=1) != 0 and b"head" in err()
    assert call(kind=2) != 0 and b"kind" in err()
    assert call(points=null) != 0 and b"exactly one" in err()          # neither form
    assert call(rows=fake, ld=192) != 0 and b"exactly one" in err()    # both
    assert call(points=null, rows=fake, ld=190) != 0 and b"ld" in err()
    assert call(kind=0, head=2, n_label=2) != 0 and b"one row per point" in err()
    assert call(g=null) != 0 and b"g_out" in err()
    # nothing to do: no launch, no error -- M = 0 (whatever the other pointers), or no gradient wanted
    stats = (ctypes.c_int * 3)(7, 7, 7)
    assert call(points=null, M=0, g=null, params=nulls, grads=nulls, scratch=null, nbytes=0, stats=stats) == 0 and list(stats) == [0, 9, 0]
    stats = (ctypes.c_int * 3)(7, 7, 7)
    assert call(grads=nulls, scratch=null, nbytes=0, stats=stats) == 0 and list(stats) == [0, 9, 0]


def test_missing_cesrtrain_library_has_its_own_message(monkeypatch, tmp_path):
    from robir_amd import _lib
    monkeypatch.setattr(_lib, "_cesrtrain", None)
    monkeypatch.setattr(_lib, "CESRTRAIN_PATH", str(tmp_path / "nope_cesrtrain.so"))
    with pytest.raises(_lib.RobirHipError, match="CESR-TRAINING library") as e:
        _lib.call_cesrtrain("rb_ct_cesr_bwd")
    msg = str(e.value)
    assert "make -C robir_amd/csrc cesrtrain" in msg and "librobir_hip_cesrtrain.so" in msg and "LEGACY" not in msg


def _net(kind):
    from robir_amd import nets
    return nets.SDFNetwork(191, 2, 512, 8, (4,), 0) if kind == "shadow" else nets.SDFNetwork(63, 3, 512, 8, (4,), 0)


def test_guard_and_mark_round_trip():
    """enable_cesr_training marks shadow_net / normal_net, refuses the NeuS shape and other types; the mark lets the network through
    forward_only_guard, unmarking restores today's behaviour; rows that require grad are refused before any kernel."""
    from robir_amd import cesr_autograd, nets, ops, training
    neus = nets.SDFNetwork(3, 257, 256, 8)
    with pytest.raises(NotImplementedError, match="not built"):
        training.enable_cesr_training(neus)
    assert not training.cesr_training_enabled(neus)
    for wrong in (torch.nn.Linear(3, 3), object(), nets.VisNetwork(points_multires=10, dirs_multires=10, dims=[256] * 4)):
        with pytest.raises(TypeError, match="SDFNetwork"):
            training.enable_cesr_training(wrong)
        assert not training.cesr_training_enabled(wrong)
    for kind in ("shadow", "normal"):
        net, other = _net(kind).train(), _net(kind).train()
        assert [tuple(p.shape) for p in cesr_autograd.cesr_params(net)][:3] == [(512, 1), (512, cto.DIMS[kind][0]), (512,)]
        assert len(cesr_autograd.cesr_params(net)) == len(ops.CESR_PARAM_NAMES) == 27 and ops.CESR_PARAM_NAMES == cto.NAMES
        assert set(ops.CESR_PARAM_NAMES) == set(dict(net.named_parameters()))
        with torch.enable_grad():
            with pytest.raises(nets.ForwardOnlyError):
                nets.forward_only_guard(net)
            assert training.enable_cesr_training(net) is net
            assert training.cesr_training_enabled(net) and not training.cesr_training_enabled(other)
            nets.forward_only_guard(net)
            assert net._trainable()
            with pytest.raises(nets.ForwardOnlyError):
                nets.forward_only_guard(other)
            with pytest.raises(NotImplementedError, match="rows"):
                net(torch.zeros(4, cto.DIMS[kind][0], requires_grad=True))
            for p in net.parameters():
                p.requires_grad_(False)
            assert not net._trainable()
            for p in net.parameters():
                p.requires_grad_(True)
            with torch.no_grad():
                assert not net._trainable()
            assert training.enable_cesr_training(net, on=False) is net
            assert not training.cesr_training_enabled(net) and not net._trainable()
            with pytest.raises(nets.ForwardOnlyError):
                net(torch.zeros(4, cto.DIMS[kind][0]))


def test_hook_with_a_trainable_net_is_not_recorded():
    from robir_amd import deferred, training

    class Hook:
        def __init__(self, s, n):
            self.shadow_net, self.normal_net = s, n
    s, n = _net("shadow").train(), _net("normal").train()
    with torch.enable_grad():
        assert not deferred.hook_trains(Hook(s, n)) and not deferred.hook_trains(lambda *a, **k: None)
        training.enable_cesr_training(n)
        assert deferred.hook_trains(Hook(s, n))
        with torch.no_grad():
            assert not deferred.hook_trains(Hook(s, n))


@pytest.mark.parametrize("kind", ["shadow", "normal"])
def test_oracle_matches_the_reference_fixture(kind):
    """float64 autograd of the oracle (softplus_net512) against float64 autograd of the reference's own SDFNetwork on the fixture's dense
    rows: 1e-10 relative, a float64-against-float64 check, on every stored piece of all 27 gradients and on the output."""
    from robir_amd import synth
    gold = load_golden("cesr_grad" if kind == "shadow" else "cesr_grad_normal")
    params = cto.cesr_params({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_cesr_nets(0)[kind + "_net"].items()})
    rows, g = torch.from_numpy(gold[kind + ".rows"]), torch.from_numpy(gold[kind + ".g_out"])
    n_label = int(gold[kind + ".n_label"])
    # the stored dense rows are the points form's rows: the one-hot block sits where the row index puts it
    assert torch.equal(rows, cto.rows_of_points(torch.from_numpy(gold[kind + ".points"]), n_label, kind, torch.float32))
    assert rows.shape[0] == (8 if kind == "normal" else 2 * 4)
    out = cto.forward({k: v.double() for k, v in params.items()}, rows, kind)
    assert rel_err(out, gold[kind + ".out"]) <= 1e-10
    og = cto.grads(params, rows, kind, g, torch.float64)
    worst = 0.0
    for k in cto.NAMES:
        gk = og[k].double()
        parts = {"full": gk} if not k.endswith("weight_v") else {"rows8": gk[:8], "cols8": gk[:, :8], "sum": gk.sum(), "fro": gk.norm()}
        for part, v in parts.items():
            e = rel_err(v, gold[f"{kind}.grad.{k}.{part}"])
            worst = max(worst, e)
            assert e <= 1e-10, (k, part, e)
    print(f"{kind}: oracle64 vs reference64, worst piece {worst:.2e}")
