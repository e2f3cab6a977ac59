"""A plain numpy / torch-CPU model of what rb_dvis_octree and rb_octree_cast_grouped are documented to compute
(include/robir_hip.h, "Traced light visibility"), every scratch array included.  Written from that header comment and the
reference's semantics (get_diffuse_visibility, model/sg_render.py:111-195, with OctreeVisModel as the VisModel): it shares no code
with csrc/octree_vis.hip, and tests/test_ovis_model_cpu.py pins it to the oracle's own pair-materialising path.

Everything about a ray is left to robir_oracle.octree.cast, called ONCE PER LOCK-STEP GROUP on that group's rays alone: the
0.005 secondary offset, the step switch at R > 100000 and the per-iteration fine-march count live there."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from robir_oracle import octree as ooct

N_ITERS = 34                      # counter slots per group (iterations 0 .. max_iter + 1, max_iter <= 32)
TINY = np.float32(1e-6)


def front_facing(normals, dirs_rows):
    """The cull: ((nx*dx + ny*dy) + nz*dz) > 1e-6 in float32, in exactly that order.  normals [m,3], dirs_rows [LS,3] -> bool [m,LS]."""
    nr, d = np.asarray(normals, dtype=np.float32), np.asarray(dirs_rows, dtype=np.float32)
    dot = (nr[:, None, 0] * d[None, :, 0] + nr[:, None, 1] * d[None, :, 1]) + nr[:, None, 2] * d[None, :, 2]
    assert dot.dtype == np.float32
    return dot > TINY


def group_counters(T, o, d, max_iter):
    """One lock-step cast of the rays (o, d) -> t, hit, counters[N_ITERS]: the oracle's logged n_active per iteration, then the
    number of rays still active when it left its loop (0 unless max_iter cut it off), then zeros."""
    row = np.zeros(N_ITERS, dtype=np.int64)
    log = []
    t, hit = ooct.cast(T, o, d, max_iter, trace=log)
    row[:len(log)] = [a for a, _ in log]
    if len(log) == max_iter + 1:
        # the loop may have been cut off.  The schedule of a cast does not depend on max_iter, so the same cast allowed one more
        # iteration logs, as that iteration's n_active, exactly the rays that were still active here.
        log2 = []
        ooct.cast(T, o, d, max_iter + 1, trace=log2)
        assert [a for a, _ in log2[:len(log)]] == [a for a, _ in log]
        if len(log2) > len(log):
            row[len(log)] = log2[len(log)][0]
    return t, hit, row


def dvis_octree_model(T, points, normals, chunk_id, n_chunks, dirs, wdir, wsum, L, nsamp, batch_pairs=2000000, max_iter=32,
                      argmax_vis=False, with_cast=True):
    """points, normals [n,3] f32; chunk_id [n] ascending ints or None (one chunk); dirs [C*LS,3], wdir [C*LS], wsum [C*L] f32.
    with_cast=False stops after the layout (no oracle casts: hit, counters and vis are None)."""
    points, normals = torch.as_tensor(points).float(), torch.as_tensor(normals).float()
    dirs = torch.as_tensor(dirs).float()
    n, C, LS = points.shape[0], int(n_chunks), L * nsamp
    cid = np.zeros(n, dtype=np.int64) if chunk_id is None else np.asarray(chunk_id, dtype=np.int64)
    assert (np.diff(cid) >= 0).all() and (cid >= 0).all() and (cid < C).all()
    dnp, nnp = dirs.numpy(), normals.numpy()

    m = SimpleNamespace(n=n, C=C, LS=LS)
    m.cstart = np.searchsorted(cid, np.arange(C + 1), side="left").astype(np.int64)      # points of chunk c: cstart[c] .. cstart[c+1]
    m.pcount = np.zeros(n, dtype=np.int64)
    m.prank = np.zeros(n, dtype=np.int64)
    m.ctotal = np.zeros(C, dtype=np.int64)
    m.coff = np.zeros(C, dtype=np.int64)
    m.goff = np.zeros(C, dtype=np.int64)
    pair_p, pair_j, grp, gstart, gsize = [], [], [], [], []
    m.point_span = np.zeros((n, 2), dtype=np.int64)
    po = go = 0
    for c in range(C):
        a, b = int(m.cstart[c]), int(m.cstart[c + 1])
        front = front_facing(nnp[a:b], dnp[c * LS:(c + 1) * LS])
        cnt = front.sum(1).astype(np.int64)
        m.pcount[a:b] = cnt
        m.prank[a:b] = np.cumsum(cnt) - cnt                       # exclusive scan inside the chunk
        tot = int(cnt.sum())
        m.ctotal[c], m.coff[c], m.goff[c] = tot, po, go
        pp, jj = np.nonzero(front)                                # point-major, direction-minor
        pair_p.append(pp + a)
        pair_j.append(jj)
        rank = np.arange(tot, dtype=np.int64)
        grp.append(go + rank // batch_pairs)
        m.point_span[a:b, 0] = po + m.prank[a:b]
        m.point_span[a:b, 1] = cnt
        ng = -(-tot // batch_pairs)
        for k in range(ng):
            gstart.append(po + k * batch_pairs)
            gsize.append(min(batch_pairs, tot - k * batch_pairs))
        po += tot
        go += ng
    m.total_pairs, m.total_groups = po, go
    cat = lambda xs: np.concatenate(xs).astype(np.int64) if xs else np.zeros(0, dtype=np.int64)
    m.pair_p, m.pair_j, m.grp = cat(pair_p), cat(pair_j), cat(grp)
    m.gstart, m.gsize = np.asarray(gstart, dtype=np.int64), np.asarray(gsize, dtype=np.int64)
    m.row = cid[m.pair_p] * LS + m.pair_j                         # row of the direction table each pair reads
    m.hit = m.counters = m.vis = None
    if not with_cast:
        return m

    m.hit = np.zeros(po, dtype=bool)
    m.counters = np.zeros((go, N_ITERS), dtype=np.int64)
    pp_t, row_t = torch.from_numpy(m.pair_p), torch.from_numpy(m.row)
    for g in range(go):
        s = slice(int(m.gstart[g]), int(m.gstart[g] + m.gsize[g]))
        _, hit, m.counters[g] = group_counters(T, points[pp_t[s]], dirs[row_t[s]], max_iter)
        m.hit[s] = hit.numpy()

    e1 = math.exp(-1.0)
    v_hit, v_free = (0.0, 1.0) if argmax_vis else (e1 / (1.0 + e1), 1.0 / (1.0 + e1))    # softmax([hit, ~hit])[1] / argmax
    tab = np.zeros((n, LS), dtype=np.float64)                     # a culled pair contributes 0
    tab[m.pair_p, m.pair_j] = np.where(m.hit, v_hit, v_free)
    w = np.asarray(wdir, dtype=np.float64).reshape(C, L, nsamp)[cid]
    ws = np.asarray(wsum, dtype=np.float64).reshape(C, L)[cid]
    m.vis = (tab.reshape(n, L, nsamp) * w).sum(-1) / ws
    return m


def cast_grouped_model(T, origins, dirs, offsets, max_iter=32):
    """Explicit rays in groups: group g = rays offsets[g] .. offsets[g+1]-1, one oracle cast per non-empty group."""
    origins, dirs = torch.as_tensor(origins).float(), torch.as_tensor(dirs).float()
    off = np.asarray(offsets, dtype=np.int64)
    G, R = len(off) - 1, origins.shape[0]
    assert off[0] == 0 and off[-1] == R and (np.diff(off) >= 0).all()
    m = SimpleNamespace(gsize=np.diff(off), grp=np.repeat(np.arange(G, dtype=np.int64), np.diff(off)))
    m.hit = np.zeros(R, dtype=bool)
    m.t = torch.zeros(R)
    m.counters = np.zeros((G, N_ITERS), dtype=np.int64)
    for g in range(G):
        a, b = int(off[g]), int(off[g + 1])
        if b > a:
            t, hit, m.counters[g] = group_counters(T, origins[a:b], dirs[a:b], max_iter)
            m.t[a:b] = t
            m.hit[a:b] = hit.numpy()
    m.x = m.t[:, None] * dirs + origins                           # from the un-offset origin (OctreeTracing.forward)
    return m


# ---- the analytic scene the model's tests and the device's stage tests share: two spheres, no network anywhere
SPHERES = (((-0.12, 0.0, 0.05), 0.22), ((0.2, 0.1, -0.05), 0.15))


def _sphere_dist(x):
    return torch.stack([(x - torch.tensor(c)).norm(dim=-1) - r for c, r in SPHERES], -1)


def two_sphere_sdf(x):
    return _sphere_dist(x).min(-1).values


def two_sphere_grad(x):
    k = _sphere_dist(x).argmin(-1)
    v = x - torch.tensor([c for c, _ in SPHERES])[k]
    return v / v.norm(dim=-1, keepdim=True).clamp(min=1e-12)


def two_sphere_tree():
    """The oracle's octree of the union of the two spheres in [-0.6, 0.6]^3 (428 104 nodes at 4 levels, about a second)."""
    return ooct.build(two_sphere_sdf, two_sphere_grad, [-0.6] * 3, [0.6] * 3)


def unit_rows(gen, m):
    v = torch.randn(m, 3, generator=gen)
    return v / v.norm(dim=-1, keepdim=True)


def surface_points(gen, n):
    """n points on the two spheres with their outward normals (alternating spheres)."""
    nr = unit_rows(gen, n)
    k = torch.arange(n) % 2
    ctr = torch.tensor([c for c, _ in SPHERES])[k]
    rad = torch.tensor([r for _, r in SPHERES])[k]
    return (ctr + nr * rad[:, None]).contiguous(), nr.contiguous()


def direction_tables(gen, C, L, nsamp, towards=None):
    """dirs[C*LS,3] unit (spread over the sphere, or within 60 degrees of `towards`), wdir[C*LS] in (0.1, 1.1), wsum[C*L] = sum + 1e-6."""
    d = unit_rows(gen, C * L * nsamp)
    if towards is not None:
        a = torch.tensor(towards, dtype=torch.float32)
        d = d * 0.8 + a                                           # |0.8 u + a| direction stays within asin(0.8) of a
        d = d / d.norm(dim=-1, keepdim=True)
    wdir = torch.rand(C * L * nsamp, generator=gen) + 0.1
    wsum = wdir.reshape(C * L, nsamp).sum(-1) + 1e-6
    return d.contiguous(), wdir.contiguous(), wsum.contiguous()
