"""The two-tile light-visibility kernel (csrc/vis_diffuse_x6t.hip) around the end of a point's direction list and over long runs of
its weight ring: last rounds with one live tile per wave (at most 64 samples) next to two-tile ones, the per-point form against the
stream form (bit for bit) and against the fp32 kernel (2e-6, the bound of tests/test_edge_cases_gpu.py for this pair).

ops.dvis_fused is driven directly: directions are a fan in the xz-plane from +z towards +x, d_j = (sin j*delta, 0, cos j*delta), and a
point's normal is tilted to (sin b, 0, cos b) with b = -pi/2 + (k - 1/2)*delta, so that n.d_j = cos(j*delta - b) > 0 exactly for j < k:
the point has S = k front-facing directions, the nearest cosine half a step (>= 1e-4) away from the cull's 1e-6."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

TAIL_S = (0, 1, 16, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257)
FORMS = ("f16x6-pt", "f16x6-stream", "fp32")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def split(dev):
    from robir_amd import renderer
    return renderer.build_synthetic_model(dev, build_octrees=False).visibility_network.packed_split()


def _fan(LS, span):
    a = torch.arange(LS, dtype=torch.float64) * (span / LS)
    return torch.stack([a.sin(), torch.zeros_like(a), a.cos()], -1).float(), span / LS


def _normals(counts, delta):
    b = torch.tensor([-math.pi / 2 + (k - 0.5) * delta for k in counts], dtype=torch.float64)
    return torch.stack([b.sin(), torch.zeros_like(b), b.cos()], -1).float()


def _inputs(dev, split, L, nsamp, counts, span=math.pi / 2, seed=0):
    """-> dict of device tensors for ops.dvis_fused and the realised S per point (counted on the CPU with the kernel's fp32 test)."""
    from robir_amd import ops
    LS = L * nsamp
    g = torch.Generator().manual_seed(seed)
    dirs, delta = _fan(LS, span)
    nrm = _normals(counts, delta)
    S = ((nrm[:, None, :] * dirs[None]).sum(-1) > 1e-6).sum(-1).tolist()
    pts = (torch.rand(len(counts), 3, generator=g) - 0.5) * 0.6
    wdir = torch.rand(LS, generator=g) + 0.25
    d = dirs.to(dev).contiguous()
    return dict(nrm=nrm.to(dev).contiguous(), A=ops.linear_64_256(ops.feat_pe10(pts.to(dev)), split["point"]),
                Bd=ops.linear_64_256(ops.feat_pe10(d), split["dir"]), dirs=d, wdir=wdir.to(dev).contiguous(),
                wsum=wdir.reshape(L, nsamp).sum(-1).to(dev).contiguous(), L=L, nsamp=nsamp), S


def _run(x, split, form, argmax, sel=None):
    from robir_amd import ops
    nrm, A = (x["nrm"], x["A"]) if sel is None else (x["nrm"][sel].contiguous(), x["A"][sel].contiguous())
    out = ops.dvis_fused(nrm, None, A, x["Bd"], x["dirs"], x["wdir"], x["wsum"], split, x["L"], x["nsamp"], argmax, None, precision=form)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.fixture(scope="module")
def tail_case(dev, split):
    x, S = _inputs(dev, split, 16, 32, TAIL_S)
    res = {(f, am): _run(x, split, f, am) for f in FORMS for am in (False, True)}
    return x, S, res


def test_tail_sizes(tail_case):
    """Points with S on both sides of every tile and round boundary: last rounds with one live tile (S mod 128 in 1..64), with two, and
    none at all; both argmax_vis values."""
    x, S, res = tail_case
    assert tuple(S) == TAIL_S                                          # the realised counts cover the set
    for am in (False, True):
        pt, st, ref = res["f16x6-pt", am], res["f16x6-stream", am], res["fp32", am]
        print("argmax_vis", am, "max |pt - fp32| %.3g" % float((pt - ref).abs().max()))
        assert pt.shape == (len(TAIL_S), 16) and bool(torch.isfinite(pt).all())
        assert float(pt[0].abs().max()) == 0.0                        # S = 0: nothing evaluated, zeros
        assert torch.equal(pt, st)                                     # two forms of one kernel body
        assert float((pt - ref).abs().max()) <= 2e-6
    assert float(res["f16x6-pt", False][1:].abs().max()) > 0.0         # (the comparison is not one of zeros)


def test_mixed_launch(tail_case, split):
    """One-tile and two-tile last rounds in one launch, in any order: a point's values are those of a launch of its own."""
    x, S, res = tail_case
    perm = torch.randperm(len(TAIL_S), generator=torch.Generator().manual_seed(5)).to(x["nrm"].device)
    for am in (False, True):
        whole = res["f16x6-pt", am]
        assert torch.equal(_run(x, split, "f16x6-pt", am, perm), whole[perm.cpu()])
        for i in range(len(TAIL_S)):
            alone = _run(x, split, "f16x6-pt", am, torch.tensor([i], device=x["nrm"].device))
            assert torch.equal(alone[0], whole[i]), (am, S[i])


def test_ring_soak(dev, split):
    """Long runs of the weight ring.  Per-point form: 8 points with all 4096 directions front-facing, 32 rounds = 1536 chunks per
    workgroup (the most the form allows: L*nsamp <= 4096).  Stream form on the same input with 4 persistent workgroups: 2048 tiles =
    256 rounds, 64 rounds = 3072 chunks per workgroup.  Each launch twice: identical run to run and between the forms."""
    from robir_amd import ops
    x, S = _inputs(dev, split, 128, 32, [4096] * 8, span=math.pi / 3, seed=1)
    assert S == [4096] * 8
    old = ops.DVIS_STREAM_WORKGROUPS
    try:
        ops.DVIS_STREAM_WORKGROUPS = 4
        for am in (False, True):
            pt = [_run(x, split, "f16x6-pt", am) for _ in range(2)]
            st = [_run(x, split, "f16x6-stream", am) for _ in range(2)]
            assert torch.equal(pt[0], pt[1]) and torch.equal(st[0], st[1])
            assert torch.equal(pt[0], st[0])
            assert bool(torch.isfinite(pt[0]).all())
            assert float((pt[0] - _run(x, split, "fp32", am)).abs().max()) <= 2e-6
    finally:
        ops.DVIS_STREAM_WORKGROUPS = old


@pytest.mark.parametrize("L,nsamp", [(3, 8), (6, 16)])
def test_small_direction_lists(dev, split, L, nsamp):
    """L*nsamp = 24: the only round has one live tile; 96: two.  (24 is no multiple of 16: the tile-list form does not take it.)"""
    LS = L * nsamp
    x, S = _inputs(dev, split, L, nsamp, [LS, LS, 0, LS // 2], span=math.pi / 4, seed=2)
    assert S == [LS, LS, 0, LS // 2]
    for am in (False, True):
        pt, ref = _run(x, split, "f16x6-pt", am), _run(x, split, "fp32", am)
        assert pt.shape == (4, L) and float(pt[2].abs().max()) == 0.0
        assert float((pt - ref).abs().max()) <= 2e-6
        if LS % 16 == 0:
            assert torch.equal(pt, _run(x, split, "f16x6-stream", am))
