// Isosurface extraction on the device: marching tetrahedra on the Kuhn (six-tetrahedra) split of every lattice cell, and the three
// small kernels of the block-sparse lattice fill.
// Reference: neus/optimization/extraction.py:12-49 (extract_fields / extract_geometry / extract_mesh: 512^3 values copied to the host
// in 64^3 blocks, mcubes.marching_cubes + trimesh on the CPU).  No marching-cubes table is used here: the tetrahedron tables below are
// GENERATED at compile time (constexpr builder, orientation fixed by a geometric test on the unit cube) and exported through
// rb_mesh_table so that a test can compare them with an independent restatement.
//
// Conventions (include/robir_hip.h repeats them):
//   field f[nx][ny][nz] fp32, z fastest; lattice vertex v = (ix*ny + iy)*nz + iz at (xs[ix], ys[iy], zs[iz]); INSIDE iff f < iso.
//   A lattice vertex OWNS the edges to v + d, d = slot 0..6: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1), where the far
//   end is in the lattice.  A mesh vertex sits on every owned edge whose ends differ in inside-ness, at a + t (b - a) per component,
//   t = (iso - f_a) / (f_b - f_a), a = the owner (plain fp32, -ffp-contract=off: the Makefile's default).
//   Cell (ix,iy,iz) (ix < nx-1, ...) is cut into six tetrahedra, one per permutation (p,q,r) of the axes in
//   itertools.permutations(range(3)) order: corners 000, e_p, e_p+e_q, 111 (tet corner 0..3).  Per tetrahedron and 4-bit inside mask
//   (bit i = corner i inside) the table holds 0, 1 or 2 triangles of tet edges (i,j), i < j, edge id 0..5 = 01 02 03 12 13 23:
//     one corner a on its own side, the others o1 < o2 < o3:   (a,o1) (a,o2) (a,o3)
//     two inside a < b, two outside c < d: the quad (a,c) (a,d) (b,d) (b,c) as triangles (q0,q1,q2), (q0,q2,q3)
//   and the 2nd and 3rd vertex of a triangle are swapped where (B-A)x(C-A) would point from outside to inside.
// Output order: mesh vertices by owner linear index, then edge slot; faces by cell linear index (= linear index of the cell's lowest
// corner), then tetrahedron, then triangle.  No atomics: count per workgroup -> host prefix -> recount + in-workgroup scan, so the
// same inputs give the same bytes on every run.
#include "../../include/robir_hip.h"
#include "common.h"

namespace rb {
namespace {

constexpr int MESH_GROUP = 256;      // lattice vertices per workgroup: a fixed run of the linear index, one per thread

struct MeshTables {
  signed char corner[6][4];          // cube corner (bit 0 = +x, 1 = +y, 2 = +z) of tet corner i
  signed char ntri[6][16];
  signed char tri[6][16][6];         // edge ids, 3 per triangle
  signed char own[6][6];             // tet edge e: cube corner that owns it
  signed char slot[6][6];            //             and its slot among the owner's seven edges
};

constexpr int EDGE_I[6] = {0, 0, 0, 1, 1, 2}, EDGE_J[6] = {1, 2, 3, 2, 3, 3};
constexpr int SLOT_DIR[7] = {1, 2, 4, 3, 5, 6, 7};        // direction bits of slot k
constexpr int DIR_SLOT[8] = {-1, 0, 1, 3, 2, 4, 5, 6};
constexpr int PERMS[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

constexpr int edge_id(int i, int j) {
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  return lo == 0 ? hi - 1 : (lo == 1 ? hi + 1 : 5);
}

constexpr MeshTables build_tables() {
  MeshTables T{};
  for (int t = 0; t < 6; ++t) {
    const int p = PERMS[t][0], q = PERMS[t][1];
    T.corner[t][0] = 0;
    T.corner[t][1] = (signed char)(1 << p);
    T.corner[t][2] = (signed char)((1 << p) | (1 << q));
    T.corner[t][3] = 7;
    for (int e = 0; e < 6; ++e) {
      T.own[t][e] = T.corner[t][EDGE_I[e]];
      T.slot[t][e] = (signed char)DIR_SLOT[T.corner[t][EDGE_J[e]] ^ T.corner[t][EDGE_I[e]]];
    }
    for (int m = 0; m < 16; ++m) {
      int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, nin = 0, nout = 0;
      for (int i = 0; i < 4; ++i) {
        if (m >> i & 1) in[nin++] = i;
        else out[nout++] = i;
      }
      int tri[2][3] = {{0, 0, 0}, {0, 0, 0}}, n = 0;
      if (nin == 1) {
        n = 1;
        for (int k = 0; k < 3; ++k) tri[0][k] = edge_id(in[0], out[k]);
      } else if (nin == 3) {
        n = 1;
        for (int k = 0; k < 3; ++k) tri[0][k] = edge_id(out[0], in[k]);
      } else if (nin == 2) {
        n = 2;
        const int q0 = edge_id(in[0], out[0]), q1 = edge_id(in[0], out[1]), q2 = edge_id(in[1], out[1]), q3 = edge_id(in[1], out[0]);
        tri[0][0] = q0; tri[0][1] = q1; tri[0][2] = q2;
        tri[1][0] = q0; tri[1][1] = q2; tri[1][2] = q3;
      }
      // orientation on the unit cube with corner values -1 (inside) / +1 (outside): crossings are the edge midpoints; everything x 2
      // and x nin x nout to stay in integers.  g = direction of increasing f = mean(outside corners) - mean(inside corners).
      int g[3] = {0, 0, 0};
      for (int c = 0; c < 3; ++c) {
        int so = 0, si = 0;
        for (int i = 0; i < nout; ++i) so += T.corner[t][out[i]] >> c & 1;
        for (int i = 0; i < nin; ++i) si += T.corner[t][in[i]] >> c & 1;
        g[c] = nin * so - nout * si;
      }
      for (int k = 0; k < n; ++k) {
        int P[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        for (int v = 0; v < 3; ++v)
          for (int c = 0; c < 3; ++c)
            P[v][c] = (T.corner[t][EDGE_I[tri[k][v]]] >> c & 1) + (T.corner[t][EDGE_J[tri[k][v]]] >> c & 1);
        int u[3] = {0, 0, 0}, w[3] = {0, 0, 0};
        for (int c = 0; c < 3; ++c) {
          u[c] = P[1][c] - P[0][c];
          w[c] = P[2][c] - P[0][c];
        }
        const int dot = (u[1] * w[2] - u[2] * w[1]) * g[0] + (u[2] * w[0] - u[0] * w[2]) * g[1] + (u[0] * w[1] - u[1] * w[0]) * g[2];
        if (dot < 0) {
          const int s = tri[k][1];
          tri[k][1] = tri[k][2];
          tri[k][2] = s;
        }
      }
      T.ntri[t][m] = (signed char)n;
      for (int k = 0; k < 2; ++k)
        for (int v = 0; v < 3; ++v) T.tri[t][m][3 * k + v] = (signed char)tri[k][v];
    }
  }
  return T;
}

constexpr MeshTables H_TAB = build_tables();
__constant__ MeshTables D_TAB = build_tables();

struct Lat {
  const float* f;
  int nx, ny, nz;
  float iso;
};

__device__ __forceinline__ long lat_index(const Lat& L, int ix, int iy, int iz) { return ((long)ix * L.ny + iy) * L.nz + iz; }

// crossing mask of the edge slots < kmax owned by lattice vertex (ix,iy,iz)
__device__ __forceinline__ int edge_mask(const Lat& L, int ix, int iy, int iz, int kmax) {
  const long v = lat_index(L, ix, iy, iz);
  const bool a = L.f[v] < L.iso;
  int mask = 0;
  for (int k = 0; k < kmax; ++k) {
    const int d = SLOT_DIR[k], dx = d & 1, dy = d >> 1 & 1, dz = d >> 2 & 1;
    if (ix + dx < L.nx && iy + dy < L.ny && iz + dz < L.nz) {
      const bool b = L.f[v + ((long)dx * L.ny + dy) * L.nz + dz] < L.iso;
      mask |= (int)(a != b) << k;
    }
  }
  return mask;
}

// the thread's lattice vertex: its owned-edge crossing mask, the cell's 8-bit inside mask (-1: the vertex owns no cell)
struct Site {
  int ix, iy, iz;
  int vmask, cube;
  float fa, fb[7];
};

__device__ __forceinline__ Site load_site(const Lat& L, long v) {
  Site s;
  const unsigned u = (unsigned)v;          // rb_mesh_groups bounds the lattice to 2^30 vertices: 32-bit division, a fraction of the 64-bit cost
  s.iz = (int)(u % (unsigned)L.nz);
  const unsigned r = u / (unsigned)L.nz;
  s.iy = (int)(r % (unsigned)L.ny);
  s.ix = (int)(r / (unsigned)L.ny);
  s.fa = L.f[v];
  const bool a = s.fa < L.iso;
  s.vmask = 0;
  int cube = a ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const int d = SLOT_DIR[k], dx = d & 1, dy = d >> 1 & 1, dz = d >> 2 & 1;
    s.fb[k] = 0.f;
    if (s.ix + dx < L.nx && s.iy + dy < L.ny && s.iz + dz < L.nz) {
      s.fb[k] = L.f[v + ((long)dx * L.ny + dy) * L.nz + dz];
      const bool b = s.fb[k] < L.iso;
      s.vmask |= (int)(a != b) << k;
      cube |= (int)b << d;
    }
  }
  s.cube = (s.ix + 1 < L.nx && s.iy + 1 < L.ny && s.iz + 1 < L.nz) ? cube : -1;
  return s;
}

__device__ __forceinline__ int tet_mask(int cube, int t) {
  return (cube >> D_TAB.corner[t][0] & 1) | (cube >> D_TAB.corner[t][1] & 1) << 1 | (cube >> D_TAB.corner[t][2] & 1) << 2 |
         (cube >> D_TAB.corner[t][3] & 1) << 3;
}

__device__ __forceinline__ int cell_triangles(int cube) {
  if (cube <= 0 || cube == 255) return 0;
  int n = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) n += D_TAB.ntri[t][tet_mask(cube, t)];
  return n;
}

// exclusive scan of one int per thread over the 256-thread workgroup, in thread order; total = the workgroup's sum
__device__ __forceinline__ int group_scan(int v, int* s_w, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < MESH_GROUP / 64; ++i) {
    if (i < w) base += s_w[i];
    total += s_w[i];
  }
  return base + inc - v;
}

__global__ __launch_bounds__(MESH_GROUP) void k_mesh_count(Lat L, long N, int* __restrict__ counts) {
  __shared__ int s_v[MESH_GROUP / 64], s_f[MESH_GROUP / 64];
  const long v = (long)blockIdx.x * MESH_GROUP + threadIdx.x;
  int nv = 0, nf = 0;
  if (v < N) {
    const Site s = load_site(L, v);
    nv = __popc(s.vmask);
    nf = cell_triangles(s.cube);
  }
  int tv, tf;
  group_scan(nv, s_v, tv);
  group_scan(nf, s_f, tf);
  if (threadIdx.x == 0) {
    counts[2 * (long)blockIdx.x] = tv;
    counts[2 * (long)blockIdx.x + 1] = tf;
  }
}

__global__ __launch_bounds__(MESH_GROUP) void k_mesh_verts(Lat L, const float* __restrict__ xs, const float* __restrict__ ys,
                                                            const float* __restrict__ zs, long N, const long* __restrict__ group_base,
                                                            long V, float* __restrict__ verts, int* __restrict__ vbase) {
  __shared__ int s_v[MESH_GROUP / 64];
  const long v = (long)blockIdx.x * MESH_GROUP + threadIdx.x;
  Site s;
  s.vmask = 0;
  if (v < N) s = load_site(L, v);
  int total;
  const int excl = group_scan(__popc(s.vmask), s_v, total);
  if (v >= N) return;
  long o = group_base[blockIdx.x] + excl;
  vbase[v] = (int)o;
  if (!s.vmask) return;
  const float ax = xs[s.ix], ay = ys[s.iy], az = zs[s.iz];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    if (!(s.vmask >> k & 1)) continue;
    const int d = SLOT_DIR[k];
    const float t = (L.iso - s.fa) / (s.fb[k] - s.fa);
    const float bx = (d & 1) ? xs[s.ix + 1] : ax, by = (d & 2) ? ys[s.iy + 1] : ay, bz = (d & 4) ? zs[s.iz + 1] : az;
    if (o < V) {                    // never past the buffer, even if the field changed since the count
      verts[3 * o] = ax + t * (bx - ax);
      verts[3 * o + 1] = ay + t * (by - ay);
      verts[3 * o + 2] = az + t * (bz - az);
    }
    ++o;
  }
}

__global__ __launch_bounds__(MESH_GROUP) void k_mesh_faces(Lat L, long N, const long* __restrict__ group_base,
                                                            const int* __restrict__ vbase, long F, int* __restrict__ faces) {
  __shared__ int s_f[MESH_GROUP / 64];
  const long v = (long)blockIdx.x * MESH_GROUP + threadIdx.x;
  Site s;
  s.cube = -1;
  if (v < N) s = load_site(L, v);
  const int nf = cell_triangles(s.cube);
  int total;
  const int excl = group_scan(nf, s_f, total);
  if (nf == 0) return;
  long o = group_base[blockIdx.x] + excl;
  for (int t = 0; t < 6; ++t) {
    const int m = tet_mask(s.cube, t);
    const int n = D_TAB.ntri[t][m];
    if (n == 0) continue;
    // mesh vertex index on each tet edge that the triangles use
    int idx[6];
    int used = 0;
    for (int j = 0; j < 3 * n; ++j) used |= 1 << D_TAB.tri[t][m][j];
    for (int e = 0; e < 6; ++e) {
      idx[e] = 0;
      if (!(used >> e & 1)) continue;
      const int c = D_TAB.own[t][e], k = D_TAB.slot[t][e];
      const int ox = s.ix + (c & 1), oy = s.iy + (c >> 1 & 1), oz = s.iz + (c >> 2 & 1);
      idx[e] = vbase[lat_index(L, ox, oy, oz)] + __popc(edge_mask(L, ox, oy, oz, k));
    }
    for (int j = 0; j < n; ++j, ++o) {
      if (o >= F) continue;
      faces[3 * o] = idx[D_TAB.tri[t][m][3 * j]];
      faces[3 * o + 1] = idx[D_TAB.tri[t][m][3 * j + 1]];
      faces[3 * o + 2] = idx[D_TAB.tri[t][m][3 * j + 2]];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Block-sparse lattice fill: blocks of B lattice vertices per axis (the last block of an axis is shorter), block id
// (bx*nby + by)*nbz + bz, vertex l of a block = (lx*B + ly)*B + lz.
// ---------------------------------------------------------------------------------------------------------
struct Blk {
  int nx, ny, nz, B, nbx, nby, nbz;
};

// lattice coordinates of element i of the block list (unclamped); false: block id outside the lattice
__device__ __forceinline__ bool block_site(const Blk& G, const int* blocks, long i, int& ix, int& iy, int& iz) {
  const int B3 = G.B * G.B * G.B;
  const int b = blocks[i / B3], l = (int)(i % B3);
  if (b < 0 || (long)b >= (long)G.nbx * G.nby * G.nbz) return false;
  ix = (b / (G.nby * G.nbz)) * G.B + l / (G.B * G.B);
  iy = (b / G.nbz % G.nby) * G.B + l / G.B % G.B;
  iz = (b % G.nbz) * G.B + l % G.B;
  return true;
}

__global__ void k_block_points(Blk G, const int* __restrict__ blocks, long n, const float* __restrict__ xs, const float* __restrict__ ys,
                               const float* __restrict__ zs, float* __restrict__ pts) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  int ix = 0, iy = 0, iz = 0;
  block_site(G, blocks, i, ix, iy, iz);           // an invalid id evaluates vertex 0: harmless, never stored
  pts[3 * i] = xs[min(ix, G.nx - 1)];
  pts[3 * i + 1] = ys[min(iy, G.ny - 1)];
  pts[3 * i + 2] = zs[min(iz, G.nz - 1)];
}

// per_block = 0: vals[n] one value per block vertex; 1: vals[n / B^3] one value per block
__global__ void k_block_store(Blk G, const int* __restrict__ blocks, long n, const float* __restrict__ vals, int per_block,
                              float* __restrict__ field) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  int ix, iy, iz;
  if (!block_site(G, blocks, i, ix, iy, iz)) return;
  if (ix >= G.nx || iy >= G.ny || iz >= G.nz) return;
  field[((long)ix * G.ny + iy) * G.nz + iz] = vals[per_block ? i / (G.B * G.B * G.B) : i];
}

int make_blk(int nx, int ny, int nz, int B, Blk& G) {
  if (nx < 2 || ny < 2 || nz < 2) return 1;
  if (B < 2 || B > 16) return 2;
  G = Blk{nx, ny, nz, B, (nx + B - 1) / B, (ny + B - 1) / B, (nz + B - 1) / B};
  return 0;
}

}  // namespace
}  // namespace rb

using namespace rb;

extern "C" {

long rb_mesh_groups(int nx, int ny, int nz) {
  if (nx < 2 || ny < 2 || nz < 2) {
    fail(__func__, "nx, ny, nz must be >= 2");
    return -1;
  }
  const long groups = ((long)nx * ny * nz + MESH_GROUP - 1) / MESH_GROUP;
  if (groups > RB_MAX_BLOCKS) {
    fail(__func__, "lattice too large for one launch");
    return -1;
  }
  return groups;
}

int rb_mesh_table(int* table) {
  RB_REQUIRE(table, "null pointer");
  for (int t = 0; t < 6; ++t)
    for (int m = 0; m < 16; ++m) {
      int* row = table + (t * 16 + m) * 7;
      row[0] = H_TAB.ntri[t][m];
      for (int j = 0; j < 6; ++j) row[1 + j] = j < 3 * H_TAB.ntri[t][m] ? H_TAB.tri[t][m][j] : -1;
    }
  return 0;
}

int rb_mesh_count(const float* f, int nx, int ny, int nz, float iso, int* counts, long n_counts, rb_stream_t stream) {
  RB_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "nx, ny, nz must be >= 2");
  RB_REQUIRE(f && counts, "null pointer");
  const long groups = rb_mesh_groups(nx, ny, nz);
  RB_REQUIRE(groups > 0, "lattice too large for one launch");
  RB_REQUIRE(n_counts >= 2 * groups, "counts buffer too small: 2 * rb_mesh_groups() ints");
  hipLaunchKernelGGL(k_mesh_count, dim3((unsigned)groups), dim3(MESH_GROUP), 0, (hipStream_t)stream, Lat{f, nx, ny, nz, iso},
                     (long)nx * ny * nz, counts);
  return check_launch("k_mesh_count");
}

int rb_mesh_emit_vertices(const float* f, const float* xs, const float* ys, const float* zs, int nx, int ny, int nz, float iso,
                          const long* group_base, long V, float* verts, int* vbase, rb_stream_t stream) {
  RB_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "nx, ny, nz must be >= 2");
  RB_REQUIRE(V >= 0 && V < (1L << 31), "vertex total outside [0, 2^31)");
  if (V == 0) return 0;
  RB_REQUIRE(f && xs && ys && zs && group_base && verts && vbase, "null pointer");
  const long groups = rb_mesh_groups(nx, ny, nz);
  RB_REQUIRE(groups > 0, "lattice too large for one launch");
  hipLaunchKernelGGL(k_mesh_verts, dim3((unsigned)groups), dim3(MESH_GROUP), 0, (hipStream_t)stream, Lat{f, nx, ny, nz, iso}, xs, ys,
                     zs, (long)nx * ny * nz, group_base, V, verts, vbase);
  return check_launch("k_mesh_verts");
}

int rb_mesh_emit_faces(const float* f, int nx, int ny, int nz, float iso, const long* group_base, const int* vbase, long V, long F,
                       int* faces, rb_stream_t stream) {
  RB_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "nx, ny, nz must be >= 2");
  RB_REQUIRE(V >= 0 && V < (1L << 31), "vertex total outside [0, 2^31)");
  RB_REQUIRE(F >= 0 && F < (1L << 31), "face total outside [0, 2^31)");
  if (F == 0) return 0;
  RB_REQUIRE(V >= 3, "faces without vertices");
  RB_REQUIRE(f && group_base && vbase && faces, "null pointer");
  const long groups = rb_mesh_groups(nx, ny, nz);
  RB_REQUIRE(groups > 0, "lattice too large for one launch");
  hipLaunchKernelGGL(k_mesh_faces, dim3((unsigned)groups), dim3(MESH_GROUP), 0, (hipStream_t)stream, Lat{f, nx, ny, nz, iso},
                     (long)nx * ny * nz, group_base, vbase, F, faces);
  return check_launch("k_mesh_faces");
}

int rb_mesh_block_points(const int* blocks, long nb, int B, const float* xs, const float* ys, const float* zs, int nx, int ny, int nz,
                         float* pts, long n_pts, rb_stream_t stream) {
  Blk G;
  const int bad = make_blk(nx, ny, nz, B, G);
  RB_REQUIRE(bad != 1, "nx, ny, nz must be >= 2");
  RB_REQUIRE(bad != 2, "block size outside 2..16");
  if (nb <= 0) return 0;
  RB_REQUIRE(blocks && xs && ys && zs && pts, "null pointer");
  const long n = nb * B * B * B;
  RB_REQUIRE(n_pts >= n, "points buffer too small: nb * B^3 rows");
  hipLaunchKernelGGL(k_block_points, grid1d(n, 256), dim3(256), 0, (hipStream_t)stream, G, blocks, n, xs, ys, zs, pts);
  return check_launch("k_block_points");
}

int rb_mesh_block_store(const int* blocks, long nb, int B, const float* vals, long n_vals, int nx, int ny, int nz, float* field,
                        rb_stream_t stream) {
  Blk G;
  const int bad = make_blk(nx, ny, nz, B, G);
  RB_REQUIRE(bad != 1, "nx, ny, nz must be >= 2");
  RB_REQUIRE(bad != 2, "block size outside 2..16");
  if (nb <= 0) return 0;
  RB_REQUIRE(blocks && vals && field, "null pointer");
  const long n = nb * B * B * B;
  RB_REQUIRE(n_vals >= n, "values buffer too small: nb * B^3 values");
  hipLaunchKernelGGL(k_block_store, grid1d(n, 256), dim3(256), 0, (hipStream_t)stream, G, blocks, n, vals, 0, field);
  return check_launch("k_block_store");
}

int rb_mesh_block_fill(const int* blocks, long nb, int B, const float* vals, int nx, int ny, int nz, float* field, rb_stream_t stream) {
  Blk G;
  const int bad = make_blk(nx, ny, nz, B, G);
  RB_REQUIRE(bad != 1, "nx, ny, nz must be >= 2");
  RB_REQUIRE(bad != 2, "block size outside 2..16");
  if (nb <= 0) return 0;
  RB_REQUIRE(blocks && vals && field, "null pointer");
  const long n = nb * B * B * B;
  hipLaunchKernelGGL(k_block_store, grid1d(n, 256), dim3(256), 0, (hipStream_t)stream, G, blocks, n, vals, 1, field);
  return check_launch("k_block_store(fill)");
}

}  // extern "C"
