"""Stage-level tests of the traced-visibility kernels (csrc/octree_vis.hip): after ONE call of rb_dvis_octree every scratch array
the header documents as caller-owned is read back and compared -- exactly -- with the plain model of tests/ovis_model.py (pinned to
the oracle by tests/test_ovis_model_cpu.py); vis_out against the model's float64 sums within a derived rounding bound; the plain and
the compacted form bit for bit; rb_octree_cast_grouped against one oracle cast per group.  Analytic two-sphere tree, no network."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_err
import ovis_model as om

pytestmark = pytest.mark.gpu

c_long, c_int, c_float = ctypes.c_long, ctypes.c_int, ctypes.c_float
N_SLOTS = 4096                      # per-workgroup statistics slots behind the four layout scalars


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tree():
    torch.set_num_threads(8)
    return om.two_sphere_tree()


@pytest.fixture(scope="module")
def tabs(tree, dev):
    from robir_amd.octree_tracing import OctreeSDF
    return OctreeSDF.from_host_tables(tree, dev, 32).tables


# ---------------------------------------------------------------------------------------------------------------- scenes
def _scene(seed, n, L, nsamp, C=1, cid=None, batch=2000000, max_iter=32, argmax=False, odd_points=False, towards=None):
    gen = torch.Generator().manual_seed(seed)
    pts, nrm = om.surface_points(gen, n)
    if odd_points:
        nrm[[3, 11, 36, 40, 69]] = 0.0                                     # no front-facing pair: visibility 0
        pts[[5, 20, 50]] = torch.tensor([[0.7, 0.1, 0.0], [-0.65, -0.2, 0.3], [0.1, 0.9, 0.1]])      # outside the root box
        nrm[[5, 20, 50]] = -pts[[5, 20, 50]] / pts[[5, 20, 50]].norm(dim=-1, keepdim=True)           # ... facing it
        ctr = torch.tensor([c for c, _ in om.SPHERES])
        pts[[8, 9, 44, 45]] = ctr[[0, 1, 0, 1]] + torch.tensor([[0.02, 0, 0], [0, 0.03, 0], [0, 0, -0.05], [0.01, 0.01, 0.01]])   # in a hit cell
    dirs, wdir, wsum = om.direction_tables(gen, C, L, nsamp, towards)
    return dict(pts=pts, nrm=nrm, cid=cid, C=C, dirs=dirs, wdir=wdir, wsum=wsum, L=L, nsamp=nsamp, batch=batch, max_iter=max_iter,
                argmax=argmax)


def _cid_b():
    return torch.tensor([0] * 35 + [2] * 35, dtype=torch.int32)            # chunks 1 and 3 of 4 are empty


SCENES = {
    "A": lambda: _scene(1, 37, 5, 3),
    "B": lambda: _scene(2, 70, 20, 13, C=4, cid=_cid_b(), odd_points=True),
    "C": lambda: _scene(3, 1500, 5, 3),
    "D_3chunks_batch30011": lambda: _scene(4, 64, 128, 32, C=3, cid=(torch.arange(64) * 3 // 64).to(torch.int32), batch=30011),
    "D_1chunk_batch120000": lambda: _scene(4, 64, 128, 32, batch=120000),
    "E_max_iter3": lambda: _scene(2, 70, 20, 13, C=4, cid=_cid_b(), odd_points=True, max_iter=3),
    "F_argmax_A": lambda: _scene(1, 37, 5, 3, argmax=True),
    "F_argmax_D": lambda: _scene(4, 64, 128, 32, C=3, cid=(torch.arange(64) * 3 // 64).to(torch.int32), batch=30011, argmax=True),
}


# ------------------------------------------------------------------------------------------------------------ the call
def _max_groups(sc):
    n, LS = sc["pts"].shape[0], sc["L"] * sc["nsamp"]
    per_chunk = n if sc["cid"] is None else int(torch.bincount(sc["cid"].long()).max())
    return sc["C"] * (-(-per_chunk * LS // sc["batch"])) + 1


def _call_dvis(tabs, dev, sc, compact, keep_on_device=False, stash=None):
    """rb_dvis_octree through the C ABI with scratch this test owns, sized as include/robir_hip.h says and filled with a
    sentinel first.  -> dict of what came back (host tensors unless keep_on_device); stash receives the device tensors before the call."""
    from robir_amd import _lib
    ptr = _lib.ptr
    n, L, nsamp, C = sc["pts"].shape[0], sc["L"], sc["nsamp"], sc["C"]
    cap, mg = n * L * nsamp, _max_groups(sc)
    full = lambda m, dt, v: torch.full((m,), v, dtype=dt, device=dev)
    s = dict(pcount=full(n, torch.int32, -7), prank=full(n, torch.int32, -7), chunk_tab=full(4 * C + 4, torch.int64, -7),
             group_tab=full(2 * mg, torch.int64, -7), counters=full(34 * mg, torch.int32, -7), pair_p=full(cap, torch.int32, -7),
             pair_j=full(cap, torch.int16, -7), t_st=full(cap, torch.float32, -7.0), leaf_st=full(cap, torch.int32, -7),
             act_st=full(cap, torch.uint8, 7), grp=full(cap, torch.int32, -7), point_span=full(2 * n, torch.int64, -7),
             layout=full(4 + 2 * N_SLOTS, torch.int64, -7), vis=full(n * L, torch.float32, -7.0).view(n, L))
    nblk = cap // 2048 + 2
    cmp = [full(cap, torch.int32, -7), full(cap, torch.int32, -7), full(cap + 8, torch.uint8, 7), full(nblk, torch.int32, -7),
           full(nblk, torch.int64, -7), full(40, torch.int64, -7)] if compact else [None] * 6
    d = {k: sc[k].to(dev).contiguous() for k in ("pts", "nrm", "dirs", "wdir", "wsum")}
    cid = None if sc["cid"] is None else sc["cid"].to(dev)
    if stash is not None:
        stash.update(s, **{"cmp%d" % i: t for i, t in enumerate(cmp) if t is not None})
    try:
        _lib.call("rb_dvis_octree", *tabs.args(), ptr(d["pts"]), ptr(d["nrm"]), ptr(cid), c_long(n), c_int(C), ptr(d["dirs"]),
                  ptr(d["wdir"]), ptr(d["wsum"]), c_int(L), c_int(nsamp), c_int(1 if sc["argmax"] else 0),
                  c_long(sc["batch"]), c_int(sc["max_iter"]), ptr(s["pcount"]), ptr(s["prank"]),
                  ptr(s["chunk_tab"]), ptr(s["group_tab"]), c_int(mg), ptr(s["counters"]), ptr(s["pair_p"]), ptr(s["pair_j"]),
                  ptr(s["t_st"]), ptr(s["leaf_st"]), ptr(s["act_st"]), ptr(s["grp"]), ptr(s["point_span"]), ptr(s["layout"]),
                  *[ptr(t) for t in cmp], ptr(s["vis"]), ptr(None), _lib.stream_ptr())
    finally:
        torch.cuda.synchronize()
    s["max_groups"] = mg
    lay = s["layout"].cpu()
    s["total_pairs"], s["total_groups"] = int(lay[0]), int(lay[:2].view(torch.int32)[2])        # long, then int (+ an unwritten pad)
    s["node_fetches"], s["ray_steps"] = (int(v) for v in lay[4:].view(N_SLOTS, 2).sum(0))
    if not keep_on_device:
        s = {k: v.cpu() if isinstance(v, torch.Tensor) else v for k, v in s.items()}
    return s


@pytest.fixture(scope="module", params=list(SCENES))
def case(request, tree, tabs, dev):
    """The model (once) and the device's plain and compacted calls (once each) of a scene; the tests below only compare."""
    sc = SCENES[request.param]()
    m = om.dvis_octree_model(tree, sc["pts"], sc["nrm"], None if sc["cid"] is None else sc["cid"].numpy(), sc["C"], sc["dirs"],
                             sc["wdir"], sc["wsum"], sc["L"], sc["nsamp"], sc["batch"], sc["max_iter"], sc["argmax"])
    return dict(name=request.param, sc=sc, m=m, plain=_call_dvis(tabs, dev, sc, False), compact=_call_dvis(tabs, dev, sc, True))


def _eq(got, want, what):
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, "%d of %d differ, first at %d: got %d, model %d" % (bad.size, got.size, bad[0], got[bad[0]], want[bad[0]]))


# ------------------------------------------------------------------------------------------------------- model parity
def test_count_scan_and_layout_arrays(case):
    """k_ovis_count, k_ovis_scan (carry between strips of 1024 points in case C; empty chunks in B), k_ovis_layout."""
    m, C = case["m"], case["m"].C
    for form in ("plain", "compact"):
        s = case[form]
        _eq(s["pcount"], m.pcount, form + " pcount")
        _eq(s["prank"], m.prank, form + " prank")
        ct = s["chunk_tab"]
        _eq(ct[:C + 1], m.cstart, form + " cstart")
        _eq(ct[C + 1:2 * C + 1], m.ctotal, form + " ctotal")
        _eq(ct[2 * C + 1:3 * C + 1], m.coff, form + " coff")
        _eq(ct[3 * C + 1:].view(torch.int32)[:C], m.goff, form + " goff")             # int32, packed behind coff
        assert s["total_pairs"] == m.total_pairs and s["total_groups"] == m.total_groups, (form, s["total_pairs"], s["total_groups"])
        assert m.total_groups <= s["max_groups"]
        G = m.total_groups
        _eq(s["group_tab"][:G], m.gstart, form + " gstart")
        _eq(s["group_tab"][s["max_groups"]:s["max_groups"] + G], m.gsize, form + " gsize")
    name = case["name"]
    if name == "C":
        assert m.n > 1024 and m.prank[1024] > 0                    # the scan really carried into a second strip
    if name in ("B", "E_max_iter3"):
        assert m.ctotal[1] == 0 and m.ctotal[3] == 0 and (m.pcount == 0).sum() >= 5
    if name.startswith("D_3chunks"):
        assert m.total_groups >= 6
        inside = [g for g in m.gstart[1:] if ((m.point_span[:, 0] < g) & (g < m.point_span[:, 0] + m.point_span[:, 1])).any()]
        assert inside and any(g % 64 for g in m.gstart)            # group boundaries inside a point and inside a wave
    if name.startswith("D_1chunk"):
        assert m.gsize.tolist()[0] == 120000 and 0 < m.gsize[1] < 100000 and m.total_groups == 2


def test_pair_arrays(case):
    """k_ovis_fill's ordered compaction (strips of 256 directions: LS = 260 in B, 4096 in D): pair_p, pair_j, grp, point_span."""
    m = case["m"]
    for form in ("plain", "compact"):
        s, tp = case[form], m.total_pairs
        _eq(s["pair_p"][:tp], m.pair_p, form + " pair_p")
        _eq(s["pair_j"][:tp].view(torch.int16).to(torch.int32) & 0xFFFF, m.pair_j, form + " pair_j")
        _eq(s["grp"][:tp], m.grp, form + " grp")
        _eq(s["point_span"].view(-1, 2).reshape(-1), m.point_span.reshape(-1), form + " point_span")
        assert bool((s["pair_p"][tp:] == -7).all()) and bool((s["grp"][tp:] == -7).all())          # nothing written past the pairs


def test_counters_hits_and_ray_steps(case):
    """Per-group lock-step counters at every iteration == the oracle's schedule of a cast of that group alone; leaf_st >= 0 == the
    oracle's hit for every pair; ray_steps == the sum of the counters of the iterations that ran."""
    m, mi = case["m"], case["sc"]["max_iter"]
    for form in ("plain", "compact"):
        s, tp, G = case[form], m.total_pairs, m.total_groups
        cnt = s["counters"].view(-1, 34)[:G]
        _eq(cnt.reshape(-1), m.counters.reshape(-1), form + " counters")
        _eq(s["leaf_st"][:tp] >= 0, m.hit, form + " hit")
        assert s["ray_steps"] == int(cnt[:, :mi + 1].sum()), (form, s["ray_steps"], int(cnt[:, :mi + 1].sum()))
    if case["name"] == "E_max_iter3":
        still = int(m.counters[:, mi + 1].sum())
        assert still > 0                                           # the model really has rays active at the cut-off
        act = case["plain"]["act_st"][:m.total_pairs] != 0         # (the plain form keeps the active flag per pair)
        assert int(act.sum()) == still
        assert bool((case["plain"]["leaf_st"][:m.total_pairs][act] >= 0).all()) and bool(m.hit[act.numpy()].all())     # ... and they are hits
    else:
        assert (m.counters[:, mi + 1] == 0).all()
    if case["name"] in ("B", "E_max_iter3"):
        inside = np.isin(m.pair_p, [8, 9, 44, 45])
        assert inside.any() and m.hit[inside].all()                # rays that start inside a sphere never leave it
        assert m.counters[:, 0].sum() < m.total_pairs              # rays from outside the box that miss it are never active


def test_vis_out_within_the_rounding_bound(case):
    """|got - ref| <= (nsamp + 3) 2^-24 ref element-wise against the float64 model: all terms are non-negative; nsamp - 1 additions,
    one product, one division and the rounded softmax constant (derived, not measured)."""
    m, nsamp = case["m"], case["sc"]["nsamp"]
    got = case["plain"]["vis"].double().numpy()
    err = np.abs(got - m.vis)
    print(case["name"], "max |got - ref| / ref in units of 2^-24:", float((err / np.maximum(m.vis, 1e-300)).max() * 2 ** 24))
    assert (err <= (nsamp + 3) * 2.0 ** -24 * m.vis).all(), float((err / np.maximum(m.vis, 1e-300)).max() * 2 ** 24)
    assert (got[m.pcount == 0] == 0).all() and 0.0 < got.mean() < 1.0
    if case["sc"]["argmax"]:
        assert (m.vis.max() <= 1.0 + 1e-12) and case["name"].startswith("F_")


def test_compacted_form_equals_plain_bit_for_bit(case):
    p, c, tp = case["plain"], case["compact"], case["m"].total_pairs
    assert torch.equal(p["vis"].view(torch.int32), c["vis"].view(torch.int32))
    assert torch.equal(p["t_st"][:tp].view(torch.int32), c["t_st"][:tp].view(torch.int32))
    assert torch.equal(p["leaf_st"][:tp], c["leaf_st"][:tp])
    G = case["m"].total_groups
    assert torch.equal(p["counters"][:34 * G], c["counters"][:34 * G])
    for k in ("total_pairs", "total_groups", "node_fetches", "ray_steps"):
        assert p[k] == c[k], (k, p[k], c[k])


# ------------------------------------------------------------------------------------------------- G: device-only, 2.1 M pairs
def test_two_million_pairs_plain_equals_compacted(tabs, dev):
    """520 points x 4096 directions, all front-facing: 2 129 920 pairs = 1040 compaction blocks of 2048, so k_cmp_scan walks a
    second strip of 1024 blocks with a carry, at the first list and -- every ray starts active in free space -- at the next one.
    Plain against compacted only (an oracle cast of 2 M rays is no few-second test)."""
    gen = torch.Generator().manual_seed(7)
    x = torch.rand(4000, 3, generator=gen) - 0.5
    x = x[om.two_sphere_sdf(x) > 0.12][:520]                       # free space: every ray is active after set-up and after one step
    assert x.shape[0] == 520
    sc = _scene(7, 520, 128, 32, towards=(0.0, 0.0, 1.0))
    sc["pts"], sc["nrm"] = x.contiguous(), torch.tensor([[0.0, 0.0, 1.0]]).repeat(520, 1)
    p = _call_dvis(tabs, dev, sc, False, keep_on_device=True)
    c = _call_dvis(tabs, dev, sc, True, keep_on_device=True)
    tp = 520 * 4096
    for s in (p, c):
        assert s["total_pairs"] == tp and s["total_groups"] == 2
        assert s["group_tab"][:2].tolist() == [0, 2000000] and s["group_tab"][s["max_groups"]:s["max_groups"] + 2].tolist() == [2000000, 129920]
        assert bool((s["pcount"] == 4096).all())
        cnt = s["counters"].view(-1, 34)[:2].cpu()
        assert int(cnt[:, 0].sum()) > 1024 * 2048 and int(cnt[:, 1].sum()) > 1024 * 2048       # live lists longer than one strip of blocks
        assert s["ray_steps"] == int(cnt[:, :33].sum())
        assert bool((s["grp"][:2000000] == 0).all()) and bool((s["grp"][2000000:tp] == 1).all())
    assert torch.equal(p["vis"].view(torch.int32), c["vis"].view(torch.int32))
    assert torch.equal(p["t_st"].view(torch.int32), c["t_st"].view(torch.int32)) and torch.equal(p["leaf_st"], c["leaf_st"])
    assert torch.equal(p["counters"][:68], c["counters"][:68])
    assert torch.equal(p["pair_p"], c["pair_p"]) and torch.equal(p["pair_j"], c["pair_j"])
    assert torch.equal(p["pair_p"].view(520, 4096)[:, 0].cpu(), torch.arange(520, dtype=torch.int32))
    for k in ("node_fetches", "ray_steps"):
        assert p[k] == c[k], (k, p[k], c[k])
    hit = (p["leaf_st"] >= 0).float().mean().item()
    assert 0.0 < hit < 0.9 and bool(torch.isfinite(p["vis"]).all())


# ----------------------------------------------------------------------------------------------------------- the guard
@pytest.mark.parametrize("compact", [False, True])
def test_batch_below_all_directions_of_a_point_is_refused(tabs, dev, compact):
    """k_ovis_fill credits a point's active rays to at most two consecutive groups, which needs batch_pairs >= L*nsamp: a smaller
    batch is refused before anything is launched (no scratch array and not vis_out is written)."""
    from robir_amd import _lib
    sc = SCENES["A"]()
    sc["batch"] = 14                                               # L*nsamp = 15
    held = {}
    with pytest.raises(_lib.RobirHipError) as e:
        _call_dvis(tabs, dev, sc, compact, stash=held)
    assert "batch_pairs = 14" in str(e.value) and "L*nsamp = 15" in str(e.value)
    assert len(held) == (20 if compact else 14)
    for k, t in held.items():                                      # every scratch array and vis_out still hold the sentinel
        assert bool((t == (7 if t.dtype == torch.uint8 else -7)).all()), k
    sc["batch"] = 15                                               # the smallest batch allowed runs
    ok = _call_dvis(tabs, dev, sc, compact)
    assert ok["total_groups"] > 2 and bool((ok["vis"] >= 0).all())


# --------------------------------------------------------------------------------------------------- explicit rays in groups
GROUPED = {
    "R2561": (2561, [0, 1, 300, 300, 1500, 2561, 2561]),          # a group of one ray, two empty groups, R no multiple of 256
    "R3_G5": (3, [0, 0, 1, 1, 3, 3]),                              # more groups than rays
}


@pytest.fixture(scope="module")
def grouped_rays():
    sc = SCENES["B"]()                                             # B's points: on the spheres, outside the box, inside a sphere
    gen = torch.Generator().manual_seed(12)
    idx = torch.randint(0, 70, (2561,), generator=gen)
    idx[:3] = torch.tensor([5, 8, 0])                              # the three-ray case: outside the box, in a hit cell, on a sphere
    d = om.unit_rows(gen, 2561)
    d[0] = -sc["pts"][5] / sc["pts"][5].norm()
    return sc["pts"][idx].contiguous(), d.contiguous()


@pytest.mark.parametrize("max_iter", [32, 3])
@pytest.mark.parametrize("which", list(GROUPED))
def test_grouped_cast_against_one_oracle_cast_per_group(tree, tabs, dev, grouped_rays, which, max_iter):
    from robir_amd import _lib, ops
    ptr = _lib.ptr
    R, off = GROUPED[which]
    o, d = grouped_rays[0][:R].contiguous(), grouped_rays[1][:R].contiguous()
    m = om.cast_grouped_model(tree, o, d, off, max_iter)
    G = len(off) - 1
    od, dd, gs = o.to(dev), d.to(dev), torch.tensor(off, dtype=torch.int64, device=dev)
    x, hit, t = ops.octree_cast_grouped(tabs, od, dd, gs, max_iter)
    # and through the C ABI, for the scratch
    full = lambda n, dt, v: torch.full((n,), v, dtype=dt, device=dev)
    gsize, grp, leaf, t_st = full(G, torch.int64, -7), full(R, torch.int32, -7), full(R, torch.int32, -7), full(R, torch.float32, -7.0)
    act, cnt = full(R, torch.uint8, 7), full(34 * G, torch.int32, -7)
    x2, hit2, t2 = torch.empty(R, 3, device=dev), full(R, torch.uint8, 7), torch.empty(R, device=dev)
    _lib.call("rb_octree_cast_grouped", *tabs.args(), ptr(od), ptr(dd), c_long(R), ptr(gs), c_int(G), c_int(max_iter),
              c_float(tabs.clamp_dt), ptr(gsize), ptr(grp), ptr(t_st), ptr(leaf), ptr(act), ptr(cnt), ptr(x2), ptr(hit2), ptr(t2),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    # bit for bit (ray 0 of either case lies in a cell face with a zero direction component: 0 * inf, NaN in the oracle and here)
    assert torch.equal(x.view(torch.int32), x2.view(torch.int32)) and torch.equal(t.view(torch.int32), t2.view(torch.int32))
    assert torch.equal(hit, hit2.bool())
    _eq(gsize.cpu(), m.gsize, "gsize")
    _eq(grp.cpu(), m.grp, "grp")
    _eq(cnt.cpu(), m.counters.reshape(-1), "counters")
    _eq(hit.cpu(), m.hit, "hit")
    assert bool(((leaf >= 0) == hit).all())
    assert rel_err(t.cpu(), m.t) <= 1e-6 and rel_err(x.cpu(), m.x) <= 1e-6
    if max_iter == 3 and which == "R2561":
        assert m.counters[:, 4].sum() > 0 and int((act != 0).sum()) == int(m.counters[:, 4].sum())      # the cut-off is taken
        assert bool(hit[act != 0].all())
    if which == "R2561":
        assert 0.05 < m.hit.mean() < 0.95
