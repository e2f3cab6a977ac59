"""The per-point form of the two-tile light-visibility kernel (csrc/vis_diffuse_x6t.hip) as a PERSISTENT grid: a workgroup takes point
after point from a queue and keeps its weight ring running across them.  What can go wrong is at the boundary between two points
of one workgroup -- the ring position a point inherits (after a one-tile last round, a two-tile one, or no round at all), the
per-point tables in the LDS, the queue -- so every case runs with few workgroups (ops.DVIS_PT_WORKGROUPS), where each of them
crosses many boundaries, next to the default grid.

Yardsticks: the unchanged stream form (f16x6-stream, bit for bit) and the fp32 kernel (2e-6, the bound of tests/test_edge_cases_gpu.py
for this pair).  Inputs: the fan of tests/test_dvis_tail_rounds_gpu.py, which gives every point an exact count S of front-facing
directions."""
import math

import pytest
import torch

from test_dvis_tail_rounds_gpu import _inputs, dev, split  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

S_SET = (0, 1, 16, 63, 64, 65, 127, 128, 129, 192, 193, 257)


def _run(x, split, form, argmax, cid=None):
    from robir_amd import ops
    out = ops.dvis_fused(x["nrm"], cid, x["A"], x["Bd"], x["dirs"], x["wdir"], x["wsum"], split, x["L"], x["nsamp"], argmax, None,
                         precision=form)
    torch.cuda.synchronize()
    return out.cpu()


def _run_pt(x, split, argmax, workgroups, cid=None):
    from robir_amd import ops
    old = ops.DVIS_PT_WORKGROUPS
    try:
        ops.DVIS_PT_WORKGROUPS = workgroups
        return _run(x, split, "f16x6-pt", argmax, cid)
    finally:
        ops.DVIS_PT_WORKGROUPS = old


def _check(pt, st, ref, tag):
    print(tag, "max |pt - fp32| %.3g" % float((pt - ref).abs().max()))
    assert bool(torch.isfinite(pt).all()), tag
    if st is not None:
        assert torch.equal(pt, st), tag
    assert float((pt - ref).abs().max()) <= 2e-6, tag


def _shuffled_counts():
    """40 counts from S_SET: each value three times in a shuffled order, S = 0 first and last and a pair of S = 0 in the middle."""
    g = torch.Generator().manual_seed(11)
    mid = [S_SET[i] for i in (torch.randperm(36, generator=g) % 12).tolist()]
    return [0] + mid[:18] + [0, 0] + mid[18:] + [0]


def test_workgroup_counts(dev, split):
    """40 points with S on both sides of every tile and round boundary, with 1, 2, 3 and the default number of workgroups."""
    counts = _shuffled_counts()
    x, S = _inputs(dev, split, 16, 32, counts)
    assert S == counts and len(S) == 40 and set(S) == set(S_SET)
    for am in (False, True):
        st, ref = _run(x, split, "f16x6-stream", am), _run(x, split, "fp32", am)
        for w in (1, 2, 3, 0):
            pt = _run_pt(x, split, am, w)
            assert pt.shape == (40, 16)
            _check(pt, st, ref, f"argmax {am} workgroups {w}")
            zero = torch.tensor(S) == 0
            assert float(pt[zero].abs().max()) == 0.0                 # S = 0: nothing evaluated
        assert float(st[~zero].abs().max()) > 0.0                     # (the comparison is not one of zeros)


@pytest.mark.parametrize("counts", [(129, 0, 64), (193,), (0,)])
def test_fewer_points_than_workgroups(dev, split, counts):
    x, S = _inputs(dev, split, 16, 32, list(counts), seed=3)
    assert S == list(counts)
    for am in (False, True):
        st, ref = _run(x, split, "f16x6-stream", am), _run(x, split, "fp32", am)
        for w in (0, 2):
            _check(_run_pt(x, split, am, w), st, ref, f"n {len(counts)} argmax {am} workgroups {w}")


def test_several_chunks(dev, split):
    """Points of three chunks (ascending chunk ids, a direction table each) in one launch: a workgroup's next point may lie in another
    chunk's table."""
    spans = (math.pi / 2, math.pi / 3, math.pi / 4)
    per_chunk = ([257, 0, 64, 129, 1], [65, 193, 0, 128], [16, 127, 192, 63, 0, 257])
    xs = []
    for c, (span, counts) in enumerate(zip(spans, per_chunk)):
        xc, S = _inputs(dev, split, 16, 32, counts, span=span, seed=20 + c)
        assert S == counts
        xs.append(xc)
    x = {k: torch.cat([xc[k] for xc in xs]).contiguous() for k in ("nrm", "A", "Bd", "dirs", "wdir", "wsum")}
    x.update(L=16, nsamp=32)
    cid = torch.cat([torch.full((len(c),), i, dtype=torch.int32) for i, c in enumerate(per_chunk)]).to(dev)
    n = cid.numel()
    for am in (False, True):
        st, ref = _run(x, split, "f16x6-stream", am, cid), _run(x, split, "fp32", am, cid)
        for w in (1, 2, 0):
            pt = _run_pt(x, split, am, w, cid)
            assert pt.shape == (n, 16)
            _check(pt, st, ref, f"chunks argmax {am} workgroups {w}")
        # a point's values are those of its chunk's table alone
        lo = len(per_chunk[0])
        alone = _run_pt(xs[1], split, am, 1)
        assert torch.equal(pt[lo:lo + len(per_chunk[1])], alone)


def test_list_not_a_multiple_of_16(dev, split):
    """L * nsamp = 45: the tile-list form does not take it; against fp32 only."""
    L, nsamp = 5, 9
    counts = [45, 0, 17, 45, 1, 30, 0, 44]
    x, S = _inputs(dev, split, L, nsamp, counts, span=math.pi / 4, seed=4)
    assert S == counts
    for am in (False, True):
        ref = _run(x, split, "fp32", am)
        res = [_run_pt(x, split, am, w) for w in (1, 3, 0)]
        for pt in res:
            assert pt.shape == (len(counts), L)
            _check(pt, None, ref, f"L*nsamp 45 argmax {am}")
            assert torch.equal(pt, res[0])


def test_ring_soak_one_workgroup(dev, split):
    """300 points on ONE workgroup: the ring runs across 299 boundaries of every kind."""
    counts = [S_SET[(7 * i + i // 12) % 12] for i in range(300)]
    x, S = _inputs(dev, split, 16, 32, counts, seed=6)
    assert S == counts
    for am in (False, True):
        st, ref = _run(x, split, "f16x6-stream", am), _run(x, split, "fp32", am)
        one = [_run_pt(x, split, am, 1) for _ in range(2)]
        assert torch.equal(one[0], one[1])
        _check(one[0], st, ref, f"soak argmax {am}")
        assert torch.equal(_run_pt(x, split, am, 0), st)
