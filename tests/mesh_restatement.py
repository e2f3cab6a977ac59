"""numpy restatement of the marching-tetrahedra conventions of include/robir_hip.h ("Isosurface extraction"), in plain loops and
float32, independent of robir_amd/csrc/mesh.hip: the table is built geometrically here (floating-point cross products on the unit
cube), the mesh cell by cell.  Also the mesh measures the tests share (canonical form, edge pairing, Euler characteristic, area,
volume).  Not a test module."""
import itertools

import numpy as np

DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]      # edge slots of an owner
PERMS = list(itertools.permutations(range(3)))
EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]                                   # tet edge ids


def tet_corners(t):
    """Cell corners (dx,dy,dz) of tetrahedron t: the path 000 -> e_p -> e_p+e_q -> 111."""
    p, q, _ = PERMS[t]
    c1 = [0, 0, 0]
    c1[p] = 1
    c2 = list(c1)
    c2[q] = 1
    return [(0, 0, 0), tuple(c1), tuple(c2), (1, 1, 1)]


def tet_triangles(t, mask):
    """Triangles of tetrahedron t for the 4-bit inside mask: a list of triangles, each three tet edges (i, j), i < j."""
    ins = [i for i in range(4) if mask >> i & 1]
    outs = [i for i in range(4) if not mask >> i & 1]
    pair = lambda i, j: (min(i, j), max(i, j))
    if len(ins) == 1:
        tris = [[pair(ins[0], o) for o in outs]]
    elif len(ins) == 3:
        tris = [[pair(outs[0], i) for i in ins]]
    elif len(ins) == 2:
        (a, b), (c, d) = ins, outs
        q = [pair(a, c), pair(a, d), pair(b, d), pair(b, c)]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    else:
        return []
    # orientation: corner values -1 inside / +1 outside, crossings at the edge midpoints; (B-A)x(C-A) must point towards increasing f
    P = np.array(tet_corners(t), dtype=np.float64)
    g = P[outs].mean(0) - P[ins].mean(0)
    out = []
    for tri in tris:
        A, B, C = (0.5 * (P[i] + P[j]) for i, j in tri)
        n = np.cross(B - A, C - A)
        assert abs(float(n @ g)) > 1e-9
        out.append(tri if float(n @ g) > 0 else [tri[0], tri[2], tri[1]])
    return out


def table():
    """[6][16] rows of 7 ints: triangle count, then six tet edge ids (-1 padding) -- the layout of rb_mesh_table."""
    T = []
    for t in range(6):
        rows = []
        for m in range(16):
            tris = tet_triangles(t, m)
            ids = [EDGES.index(e) for tri in tris for e in tri]
            rows.append([len(tris)] + ids + [-1] * (6 - len(ids)))
        T.append(rows)
    return T


def marching_tets(f, xs, ys, zs, iso=0.0):
    """f [nx,ny,nz] float32 -> (verts [V,3] float32, faces [F,3] int32): vertices by owner linear index then edge slot, faces by cell
    linear index, tetrahedron, triangle."""
    f = np.asarray(f, dtype=np.float32)
    xs, ys, zs = (np.asarray(a, dtype=np.float32) for a in (xs, ys, zs))
    nx, ny, nz = f.shape
    iso = np.float32(iso)
    inside = f < iso
    axes = (xs, ys, zs)
    index, verts = {}, []
    cand = np.zeros(f.shape, dtype=bool)          # owners with at least one crossing edge (numpy only narrows the loop)
    for dx, dy, dz in DIRS:
        a = inside[:nx - dx, :ny - dy, :nz - dz]
        b = inside[dx:, dy:, dz:]
        cand[:nx - dx, :ny - dy, :nz - dz] |= a != b
    for ix, iy, iz in np.argwhere(cand):
        fa = f[ix, iy, iz]
        for k, (dx, dy, dz) in enumerate(DIRS):
            jx, jy, jz = ix + dx, iy + dy, iz + dz
            if jx >= nx or jy >= ny or jz >= nz or inside[ix, iy, iz] == inside[jx, jy, jz]:
                continue
            fb = f[jx, jy, jz]
            t = np.float32(np.float32(iso - fa) / np.float32(fb - fa))
            pos = []
            for ax, i, j in zip(axes, (ix, iy, iz), (jx, jy, jz)):
                a, b = ax[i], ax[j]
                pos.append(np.float32(a + np.float32(t * np.float32(b - a))))
            index[(int(ix), int(iy), int(iz), k)] = len(verts)
            verts.append(pos)
    tabs = [[tet_triangles(t, m) for m in range(16)] for t in range(6)]
    corners = [tet_corners(t) for t in range(6)]
    mixed = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int32)
    for dx, dy, dz in [(0, 0, 0)] + DIRS:
        mixed += inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]
    faces = []
    for ix, iy, iz in np.argwhere((mixed > 0) & (mixed < 8)):
        for t in range(6):
            C = corners[t]
            m = 0
            for i, (dx, dy, dz) in enumerate(C):
                m |= int(inside[ix + dx, iy + dy, iz + dz]) << i
            for tri in tabs[t][m]:
                row = []
                for i, j in tri:
                    o = (int(ix) + C[i][0], int(iy) + C[i][1], int(iz) + C[i][2])
                    d = (C[j][0] - C[i][0], C[j][1] - C[i][1], C[j][2] - C[i][2])
                    row.append(index[o + (DIRS.index(d),)])
                faces.append(row)
    return (np.array(verts, dtype=np.float32).reshape(-1, 3), np.array(faces, dtype=np.int32).reshape(-1, 3))


# ------------------------------------------------------------------------------------------------- shared mesh measures
def canonical(verts, faces):
    """[F,9] uint32: every triangle as the bit patterns of its three corner positions, rotated (never reflected) to the smallest of its
    three rotations, rows sorted.  Two meshes with the same triangles in any vertex / face order give the same array."""
    bits = np.ascontiguousarray(np.asarray(verts, dtype=np.float32)).view(np.uint32).reshape(-1, 3)
    tri = bits[np.asarray(faces, dtype=np.int64)].reshape(-1, 9)
    rows = []
    for r in tri.tolist():
        rows.append(min(tuple(r), tuple(r[3:] + r[:3]), tuple(r[6:] + r[:6])))
    rows.sort()
    return np.array(rows, dtype=np.uint32).reshape(-1, 9)


def edge_report(faces):
    """(every directed edge occurs exactly once, every directed edge has its reverse, number of undirected edges)."""
    fc = np.asarray(faces, dtype=np.int64)
    if fc.shape[0] == 0:
        return True, True, 0
    n = int(fc.max()) + 1
    a = np.concatenate([fc[:, 0], fc[:, 1], fc[:, 2]])
    b = np.concatenate([fc[:, 1], fc[:, 2], fc[:, 0]])
    fwd, cnt = np.unique(a * n + b, return_counts=True)
    rev = np.unique(b * n + a)
    und = np.unique(np.minimum(a, b) * n + np.maximum(a, b))
    return bool((cnt == 1).all()), bool(fwd.shape == rev.shape and (fwd == rev).all()), int(und.shape[0])


def euler(n_verts, faces):
    return n_verts - edge_report(faces)[2] + int(np.asarray(faces).shape[0])


def area_volume(verts, faces):
    v = np.asarray(verts, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    return 0.5 * np.linalg.norm(n, axis=1).sum(), (v[:, 0] * n).sum() / 6.0


# ------------------------------------------------------------------------------------------------- analytic fields (float32)
def lattice(shape, lo=-1.0, hi=1.0):
    return tuple(np.linspace(lo, hi, n, dtype=np.float32) for n in shape)


def field(name, xs, ys, zs):
    X, Y, Z = (a.astype(np.float32) for a in np.meshgrid(xs, ys, zs, indexing="ij"))
    if name == "sphere":
        f = np.sqrt(X * X + Y * Y + Z * Z) - np.float32(0.7)
    elif name == "torus":
        q = np.sqrt(X * X + Y * Y) - np.float32(0.55)
        f = np.sqrt(q * q + Z * Z) - np.float32(0.25)
    elif name == "union":       # two spheres and a ring
        s1 = np.sqrt((X - np.float32(0.35)) ** 2 + Y * Y + Z * Z) - np.float32(0.4)
        s2 = np.sqrt((X + np.float32(0.4)) ** 2 + (Y - np.float32(0.1)) ** 2 + Z * Z) - np.float32(0.3)
        q = np.sqrt(Y * Y + Z * Z) - np.float32(0.6)
        ring = np.sqrt(q * q + X * X) - np.float32(0.12)
        f = np.minimum(np.minimum(s1, s2), ring)
    elif name == "sines":       # smooth, not a distance
        f = np.sin(np.float32(3.1) * X + np.float32(0.3)) + np.sin(np.float32(2.3) * Y) * np.cos(np.float32(1.7) * Z) + np.float32(0.2) * X * Z
    elif name == "box":         # Chebyshev box of half width 0.5: lattices that contain +-0.5 hit the threshold 0 exactly
        f = np.maximum(np.maximum(np.abs(X), np.abs(Y)), np.abs(Z)) - np.float32(0.5)
    elif name == "plane":       # leaves the lattice box
        f = np.float32(0.6) * X + np.float32(0.3) * Y + np.float32(0.74) * Z - np.float32(0.1)
    elif name == "outside":
        f = np.ones_like(X)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(f.astype(np.float32))
