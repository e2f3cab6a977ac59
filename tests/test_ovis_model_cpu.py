"""tests/ovis_model.py pinned to the oracle's own pair-materialising path (robir_oracle.sg.diffuse_visibility with
octree_vis_logits as the VisModel), so that the model the device's stage tests compare with cannot drift with the kernels.
No GPU: analytic two-sphere tree, oracle on the CPU."""
import numpy as np
import pytest
import torch

import ovis_model as om
from robir_oracle import octree as ooct, sg as osg


@pytest.fixture(scope="module")
def tree():
    torch.set_num_threads(8)
    return om.two_sphere_tree()


def _scene(seed, n, L, nsamp, chunk_ids, C):
    """Points on the spheres (a few with a zero normal) + per-chunk light SGs and uniform draws."""
    gen = torch.Generator().manual_seed(seed)
    pts, nrm = om.surface_points(gen, n)
    nrm[::17] = 0.0                                                # points with no front-facing direction
    lobes = om.unit_rows(gen, L)
    lam = torch.rand(L, 1, generator=gen) * 30 + 0.5
    u = torch.rand(2, C, L, nsamp, generator=gen)
    cid = None if chunk_ids is None else torch.tensor(chunk_ids)[(torch.arange(n) * len(chunk_ids)) // n]
    return pts, nrm, lobes, lam, u, cid


def _oracle_chunk(tree, pts, nrm, lobes, lam, ut, up, batch):
    """diffuse_visibility of one chunk -> vis [n,L], flat dirs, the weights it derives, and what it handed its VisModel."""
    seen = []

    def vis_fn(p, d):
        seen.append((p.clone(), d.clone()))
        return ooct.octree_vis_logits(tree, p, d)

    out, dirs, cnt = osg.diffuse_visibility(pts, nrm, vis_fn, lobes, lam, ut, up, batch=batch, return_dirs=True)
    axis = osg.unit_eps(lobes.unsqueeze(-2))
    w = torch.exp(lam.unsqueeze(-2) * ((dirs * axis).sum(-1, keepdim=True) - 1.0))[..., 0]         # sg.py: w, [L,nsamp]
    assert sum(p.shape[0] for p, _ in seen) == cnt
    return out.t(), dirs.reshape(-1, 3), w.reshape(-1), w.sum(1) + osg.TINY, seen


# (L, nsamp, n, chunk ids in use, n_chunks, batch_pairs)
CASES = {
    "one_chunk": (5, 3, 37, None, 1, 2000000),
    "empty_chunks_uneven_batch": (20, 13, 70, (0, 2), 4, 1700),       # LS = 260 <= 1700, 1700 divides no chunk total
    "step_switch": (128, 32, 64, None, 1, 120000),                    # ~131 k pairs: one group above 100 000 rays, the rest below
}


@pytest.fixture(scope="module", params=list(CASES))
def case(request, tree):
    L, nsamp, n, ids, C, batch = CASES[request.param]
    pts, nrm, lobes, lam, u, cid = _scene(5, n, L, nsamp, ids, C)
    per_chunk = []
    dirs, wdir, wsum = [], [], []
    for c in range(C):
        sel = torch.arange(n) if cid is None else (cid == c).nonzero()[:, 0]
        vis, d, w, ws, seen = _oracle_chunk(tree, pts[sel], nrm[sel], lobes, lam, u[0, c], u[1, c], batch)
        per_chunk.append((sel, vis, seen))
        dirs.append(d), wdir.append(w), wsum.append(ws)
    dirs, wdir, wsum = torch.cat(dirs), torch.cat(wdir), torch.cat(wsum)
    m = om.dvis_octree_model(tree, pts, nrm, cid, C, dirs, wdir, wsum, L, nsamp, batch, 32, False)
    return dict(name=request.param, L=L, nsamp=nsamp, n=n, C=C, batch=batch, pts=pts, nrm=nrm, cid=cid, dirs=dirs, m=m,
                per_chunk=per_chunk)


def test_vis_equals_the_oracles_pair_path(case):
    """Tolerance: the oracle forms softmax (exp, add, divide: 3 roundings), one product per sample, nsamp-1 additions and one
    division in float32 on non-negative terms, the model in float64: |oracle - model| <= (nsamp + 4) 2^-24 model, first order;
    one more unit covers the second-order terms."""
    m, nsamp = case["m"], case["nsamp"]
    for sel, vis, _ in case["per_chunk"]:
        ref = m.vis[sel.numpy()]
        err = np.abs(vis.double().numpy() - ref)
        assert (err <= (nsamp + 5) * 2.0 ** -24 * ref).all(), (case["name"], float((err / np.maximum(ref, 1e-30)).max()))
    assert 0.05 < m.hit.mean() < 0.95                              # both kinds of pair occur
    assert (m.vis[(case["nrm"] == 0).all(-1).numpy()] == 0).all()


def test_pair_order_equals_front_nonzero(case):
    m = case["m"]
    for c, (sel, _, seen) in enumerate(case["per_chunk"]):
        a, b = int(m.coff[c]), int(m.coff[c] + m.ctotal[c])
        p = torch.cat([s[0] for s in seen]) if seen else torch.zeros(0, 3)
        d = torch.cat([s[1] for s in seen]) if seen else torch.zeros(0, 3)
        assert p.shape[0] == b - a
        assert torch.equal(case["pts"][m.pair_p[a:b]], p) and torch.equal(case["dirs"][m.row[a:b]], d)
        # and as indices: front.nonzero(as_tuple=True) of the chunk
        front = om.front_facing(case["nrm"][sel], case["dirs"][c * m.LS:(c + 1) * m.LS])
        pi, di = torch.from_numpy(front).nonzero(as_tuple=True)
        assert np.array_equal(m.pair_p[a:b], sel[pi].numpy()) and np.array_equal(m.pair_j[a:b], di.numpy())


def test_group_cuts_equal_run_vis_batches(case):
    m = case["m"]
    g = 0
    for c, (_, _, seen) in enumerate(case["per_chunk"]):
        assert m.goff[c] == g
        at = int(m.coff[c])
        for p, _ in seen:                                          # one _run_vis batch = one lock-step group
            assert m.gstart[g] == at and m.gsize[g] == p.shape[0]
            assert (m.grp[at:at + p.shape[0]] == g).all()
            at += p.shape[0]
            g += 1
        assert at == m.coff[c] + m.ctotal[c]
    assert g == m.total_groups and m.grp.shape[0] == m.total_pairs
    if case["name"] == "step_switch":
        assert m.gsize[0] == 120000 and 0 < m.gsize[1] < 100000
    if case["name"] == "empty_chunks_uneven_batch":
        assert (m.ctotal % case["batch"] != 0)[[0, 2]].all() and m.total_groups > 4


def test_layout_properties(case):
    m = case["m"]
    if case["name"] == "empty_chunks_uneven_batch":                # chunks 1 and 3 hold no point
        assert m.ctotal[1] == 0 and m.ctotal[3] == 0 and m.cstart[1] == m.cstart[2] and m.cstart[3] == m.cstart[4] == m.n
        assert m.coff[1] == m.coff[2] and m.goff[1] == m.goff[2] and m.goff[3] == m.total_groups
    zero = (case["nrm"] == 0).all(-1).numpy()
    assert zero.sum() >= 3 and (m.pcount[zero] == 0).all() and (m.point_span[zero, 1] == 0).all()
    assert m.pcount.sum() == m.total_pairs == m.gsize.sum() == m.ctotal.sum()
    assert np.array_equal(m.point_span[:, 1], m.pcount)
    for p in range(m.n):                                           # a point's span holds exactly its pairs, directions ascending
        a, k = m.point_span[p]
        assert (m.pair_p[a:a + k] == p).all() and (np.diff(m.pair_j[a:a + k]) > 0).all()
    assert np.array_equal(np.bincount(m.grp, minlength=m.total_groups), m.gsize)
    assert (np.diff(m.grp) >= 0).all() and (m.gsize > 0).all() and (m.gsize <= case["batch"]).all()
    # counters: iteration 0 counts the rays active after set-up, never more than the group; a finished schedule ends in 0
    assert (m.counters[:, 0] <= m.gsize).all() and (m.counters[:, 1:] <= m.counters[:, :-1]).all() and (m.counters[:, 33] == 0).all()


def test_cull_is_strict_and_in_float32():
    """dot == 1e-6f exactly is culled; one ulp above is kept; the order (x + y) + z decides a sum that x + (y + z) rounds differently."""
    tiny = np.float32(1e-6)
    nr = np.array([[tiny, 0, 0], [np.nextafter(tiny, np.float32(1)), 0, 0], [0, 0, 0], [1.0, 1.0, 1.0]], dtype=np.float32)
    # (32 + 2^-19) rounds to 32 (tie to even), + (-32) = 0: culled.  32 + (2^-19 - 32) would be 2^-19 = 1.9e-6: kept.
    d = np.array([[1, 0, 0], [32.0, 2.0 ** -19, -32.0]], dtype=np.float32)
    f = om.front_facing(nr, d)
    assert f[:, 0].tolist() == [False, True, False, True] and f[:, 1].tolist() == [True, True, False, False]
    m = om.dvis_octree_model(None, np.zeros((4, 3), np.float32), nr, None, 1, d, np.ones(2, np.float32), np.ones(1, np.float32), 1, 2,
                             with_cast=False)
    assert m.pcount.tolist() == [1, 2, 0, 1] and m.pair_p.tolist() == [0, 1, 1, 3] and m.pair_j.tolist() == [1, 0, 1, 0]


def test_step_switch_is_strictly_above_100000(tree, monkeypatch):
    """The model leaves the step to the oracle's cast: a group of exactly 100 000 rays marches with 0.005, 100 001 rays with 0.01."""
    gen = torch.Generator().manual_seed(9)
    pts, _ = om.surface_points(gen, 100001)
    d = om.unit_rows(gen, 100001)
    steps = []
    real = ooct._fine_march
    monkeypatch.setattr(ooct, "_fine_march", lambda T, pos, dd, mm, step: (steps.append(step), real(T, pos, dd, mm, step))[1])
    om.group_counters(tree, pts[:100000], d[:100000], 32)
    assert steps and set(steps) == {0.005}
    del steps[:]
    om.group_counters(tree, pts, d, 32)
    assert steps and set(steps) == {0.01}


def test_cut_off_count_and_grouped_model(tree):
    """max_iter = 3 cuts the schedule: the slot after the last logged iteration holds the rays still active, and every one of them is
    among the hits; explicit groups equal separate casts."""
    gen = torch.Generator().manual_seed(2)
    pts, _ = om.surface_points(gen, 600)
    d = om.unit_rows(gen, 600)
    t, hit, row = om.group_counters(tree, pts, d, 3)
    _, hit_full, row_full = om.group_counters(tree, pts, d, 32)
    assert np.array_equal(row[:5], row_full[:5]) and row[4] > 0 and (row[5:] == 0).all()
    assert int(hit.sum()) >= row[4] and bool((hit | ~hit_full).all())      # a ray that hits later was active at the cut-off: a hit
    assert int((hit & ~hit_full).sum()) > 0
    off = [0, 1, 300, 300, 600, 600]
    g = om.cast_grouped_model(tree, pts, d, off, 32)
    assert g.gsize.tolist() == [1, 299, 0, 300, 0] and g.grp[0] == 0 and g.grp[1] == 1 and g.grp[300] == 3
    for k, (a, b) in enumerate(zip(off[:-1], off[1:])):
        if b > a:
            log = []
            tt, hh = ooct.cast(tree, pts[a:b], d[a:b], 32, trace=log)
            assert torch.equal(g.t[a:b], tt) and np.array_equal(g.hit[a:b], hh.numpy())
            assert g.counters[k, :len(log)].tolist() == [x for x, _ in log] and (g.counters[k, len(log):] == 0).all()
        else:
            assert (g.counters[k] == 0).all()
    assert torch.equal(g.x, g.t[:, None] * d + pts)
