// librobir_hip_raster.so: drawing a triangle mesh into a camera's image on the device (include/robir_hip_raster.h) -- the
// projection of the vertices, tile binning, the camera-space rasteriser with its depth test and perspective-correct weights, and the G-buffer
// that robir_amd/meshrender.py shades.  The per-vertex, per-face and per-pixel arithmetic is raster_math.h; this file holds the loops, the
// LDS staging of a tile's faces, the argument checks and the launches.
//
// The style is ../texbake/texbake.hip's: gather kernels, no atomics, plain fp32 (-ffp-contract=off: the Makefile's default).  Binning is the
// same count kernel, exclusive prefix on the caller's side, emit kernel.
#include "../../../include/robir_hip_raster.h"
#include <hip/hip_runtime.h>
#include "raster_math.h"
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

namespace {

using namespace rb::rs;

static_assert(TILE == RB_RS_TILE && BATCH == RB_RS_BATCH && MAX_CHANNELS == RB_RS_MAX_CHANNELS, "the header names the constants");
static_assert(BATCH == TILE * TILE, "one lane per pixel sets up one face of a batch");
constexpr long MAX_INDEX = (1L << 31) - 1, MAX_PAIRS = (1L << 31) - 1;

thread_local char g_err[512] = "";

int fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return 1;
}

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s: %s", what, hipGetErrorString(e));
}

unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

int check_image(int H, int W) {
  if (H < 1 || W < 1) return fail("empty image: %d x %d", H, W);
  if (H > RB_RS_MAX_RESOLUTION || W > RB_RS_MAX_RESOLUTION) return fail("image %d x %d: more than %d pixels per side", H, W, RB_RS_MAX_RESOLUTION);
  return 0;
}

int check_mesh(long V, long F, int H, int W, float near, int cull) {
  if (V < 0 || F < 0) return fail("negative size: V = %ld, F = %ld", V, F);
  if (V > MAX_INDEX || F > MAX_INDEX) return fail("V = %ld, F = %ld: indices do not fit 32 bits", V, F);
  if (check_image(H, W)) return 1;
  if (!(near > 0.0f) || !finite_f(near)) return fail("near = %g: a positive finite distance is needed", (double)near);
  if (cull < 0 || cull > 2) return fail("cull = %d outside 0 .. 2", cull);
  return 0;
}

int check_pairs(long P) {
  if (P < 0) return fail("P = %ld is negative", P);
  if (P > MAX_PAIRS) return fail("P = %ld: 2^31 or more (tile, face) pairs", P);
  return 0;
}

// face f ready for its pixels; an index out of [0, V) gives the empty face
__device__ __forceinline__ Face load_face(const float* __restrict__ screen, long V, const int* __restrict__ faces, long f, int H, int W,
                                          float near, int cull) {
  const long v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
  const bool ok = v0 >= 0 && v0 < V && v1 >= 0 && v1 < V && v2 >= 0 && v2 < V;
  float s[3][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    s[0][k] = ok ? screen[4 * v0 + k] : NAN;
    s[1][k] = ok ? screen[4 * v1 + k] : NAN;
    s[2][k] = ok ? screen[4 * v2 + k] : NAN;
  }
  return face_of(s[0], s[1], s[2], H, W, near, cull);
}

// ---------------------------------------------------------------------------------------------------------------- projection
__global__ __launch_bounds__(256) void k_rs_project(const float* __restrict__ vertices, long V, const float* __restrict__ pose_inv,
                                                    const float* __restrict__ K, float* __restrict__ screen) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per vertex
  if (i >= V) return;
  float P[12], Kc[6], x[3] = {vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]}, s[4];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = pose_inv[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) Kc[k] = K[k];
  project(x, P, Kc, s);
#pragma unroll
  for (int k = 0; k < 4; ++k) screen[4 * i + k] = s[k];
}

// ---------------------------------------------------------------------------------------------------------------- binning
__global__ __launch_bounds__(256) void k_rs_bin_count(const float* __restrict__ screen, long V, const int* __restrict__ faces, long F, int H,
                                                      int W, float near, int cull, int* __restrict__ counts) {
  const long f = (long)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  int tx0, ty0, tw;
  counts[f] = (int)face_tiles(load_face(screen, V, faces, f, H, W, near, cull), tx0, ty0, tw);
}

__global__ __launch_bounds__(256) void k_rs_bin_emit(const float* __restrict__ screen, long V, const int* __restrict__ faces, long F, int H,
                                                     int W, float near, int cull, const long* __restrict__ base, long P,
                                                     int* __restrict__ pair_tile, int* __restrict__ pair_face) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per pair
  if (p >= P) return;
  long lo = 0, hi = F;                                      // the last face with base[f] <= p: base is non-decreasing, base[0] = 0
  while (hi - lo > 1) {
    const long mid = lo + (hi - lo) / 2;
    if (base[mid] <= p) lo = mid; else hi = mid;
  }
  int tx0, ty0, tw;
  const long count = face_tiles(load_face(screen, V, faces, lo, H, W, near, cull), tx0, ty0, tw), k = p - base[lo];
  const int ntx = (W + TILE - 1) / TILE;
  int tile = -1, face = -1;
  if (k >= 0 && k < count) {                                // count > 0, hence tw > 0
    tile = (ty0 + (int)(k / tw)) * ntx + tx0 + (int)(k % tw);
    face = (int)lo;
  }
  pair_tile[p] = tile;
  pair_face[p] = face;
}

// ---------------------------------------------------------------------------------------------------------------- raster
__global__ __launch_bounds__(BATCH) void k_rs_raster(const float* __restrict__ screen, long V, const int* __restrict__ faces, long F, int H,
                                                     int W, float near, int cull, const int* __restrict__ tile_start,
                                                     const int* __restrict__ pair_face, long P, int* __restrict__ face_id,
                                                     float* __restrict__ bary, float* __restrict__ depth) {
  __shared__ Face rec[BATCH];
  const int ntx = (W + TILE - 1) / TILE;
  const int tile = blockIdx.y * ntx + blockIdx.x, lane = threadIdx.x;
  const int r = blockIdx.y * TILE + lane / TILE, c = blockIdx.x * TILE + lane % TILE;
  long a = 0, b = 0;
  if (P > 0) {                                              // a list out of [0, P] is clipped, never followed
    a = tile_start[tile];
    b = tile_start[tile + 1];
    a = a < 0 ? 0 : a;
    b = b > P ? P : b;
  }
  int hit = -1;
  float best = 0.0f, w[2] = {0.0f, 0.0f};
  for (long base = a; base < b; base += BATCH) {            // wave-uniform bounds: every lane meets every barrier
    const long i = base + lane;
    const int f = i < b ? pair_face[i] : -1;
    Face mine{};
    if (f >= 0 && f < F) {
      mine = load_face(screen, V, faces, f, H, W, near, cull);
    } else {
      mine.c0 = mine.r0 = 0;
      mine.c1 = mine.r1 = -1;
    }
    mine.id = f;
    rec[lane] = mine;
    __syncthreads();
    const int n = b - base < BATCH ? (int)(b - base) : BATCH;
    for (int j = 0; j < n; ++j) {                           // ascending faces; the same LDS address for all lanes: a broadcast
      if (c < rec[j].c0 || c > rec[j].c1 || r < rec[j].r0 || r > rec[j].r1) continue;
      float d, b01[2];
      if (sample(rec[j], r, c, d, b01) && d > best) {       // strictly larger: an equal depth stays with the lower index
        best = d;
        hit = rec[j].id;
        w[0] = b01[0];
        w[1] = b01[1];
      }
    }
    __syncthreads();
  }
  if (r >= H || c >= W) return;
  const long t = (long)r * W + c;
  face_id[t] = hit;
  bary[2 * t] = hit < 0 ? 0.0f : w[0];
  bary[2 * t + 1] = hit < 0 ? 0.0f : w[1];
  depth[t] = hit < 0 ? 0.0f : 1.0f / best;
}

// ---------------------------------------------------------------------------------------------------------------- G-buffer
__global__ __launch_bounds__(256) void k_rs_gbuffer(const int* __restrict__ face_id, const float* __restrict__ bary, long n_pixels,
                                                    const long* __restrict__ index, long n, const int* __restrict__ faces, long F,
                                                    const float* __restrict__ vertices, long V, const float* __restrict__ uv,
                                                    const float* __restrict__ vnormals, const float* __restrict__ cam_loc,
                                                    const float* __restrict__ planes, int R, int C, int filter, float* __restrict__ position,
                                                    float* __restrict__ uv_out, float* __restrict__ view_dir, float* __restrict__ tex,
                                                    float* __restrict__ normal) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per output row
  if (i >= n) return;
  const float cam[3] = {cam_loc[0], cam_loc[1], cam_loc[2]};
  gbuffer_row(index ? index[i] : i, n_pixels, face_id, bary, faces, F, vertices, V, uv, vnormals, cam, planes, R, C, filter, position + 3 * i,
              uv_out + 2 * i, view_dir + 3 * i, tex ? tex + (long)C * i : nullptr, normal ? normal + 3 * i : nullptr);
}

}  // namespace

extern "C" {

int rb_rs_abi_version(void) { return RB_RS_ABI_VERSION; }

const char* rb_rs_last_error(void) { return g_err; }

int rb_rs_project(const float* vertices, long V, const float* pose_inv, const float* K, float* screen, rb_rs_stream_t stream) {
  if (V < 0) return fail("V = %ld is negative", V);
  if (V > MAX_INDEX) return fail("V = %ld: vertex indices do not fit 32 bits", V);
  if (V == 0) return 0;
  if (!vertices || !pose_inv || !K || !screen) return fail("null pointer: vertices / pose_inv / K / screen");
  hipLaunchKernelGGL(k_rs_project, dim3(blocks_of(V)), dim3(256), 0, (hipStream_t)stream, vertices, V, pose_inv, K, screen);
  return launched("k_rs_project");
}

int rb_rs_bin_count(const float* screen, long V, const int* faces, long F, int H, int W, float near, int cull, int* counts,
                    rb_rs_stream_t stream) {
  if (check_mesh(V, F, H, W, near, cull)) return 1;
  if (F == 0) return 0;
  if (!faces || !counts || (V > 0 && !screen)) return fail("null pointer: screen / faces / counts");
  hipLaunchKernelGGL(k_rs_bin_count, dim3(blocks_of(F)), dim3(256), 0, (hipStream_t)stream, screen, V, faces, F, H, W, near, cull, counts);
  return launched("k_rs_bin_count");
}

int rb_rs_bin_emit(const float* screen, long V, const int* faces, long F, int H, int W, float near, int cull, const long* base, long P,
                   int* pair_tile, int* pair_face, rb_rs_stream_t stream) {
  if (check_mesh(V, F, H, W, near, cull) || check_pairs(P)) return 1;
  if (P == 0) return 0;
  if (F == 0) return fail("P = %ld pairs of no face", P);
  if (!faces || !base || !pair_tile || !pair_face || (V > 0 && !screen)) return fail("null pointer: screen / faces / base / pair_tile / pair_face");
  hipLaunchKernelGGL(k_rs_bin_emit, dim3(blocks_of(P)), dim3(256), 0, (hipStream_t)stream, screen, V, faces, F, H, W, near, cull, base, P,
                     pair_tile, pair_face);
  return launched("k_rs_bin_emit");
}

int rb_rs_raster(const float* screen, long V, const int* faces, long F, int H, int W, float near, int cull, const int* tile_start,
                 const int* pair_face, long P, int* face_id, float* bary, float* depth, rb_rs_stream_t stream) {
  if (check_mesh(V, F, H, W, near, cull) || check_pairs(P)) return 1;
  if (F == 0 || V == 0) P = 0;
  if (!face_id || !bary || !depth) return fail("null pointer: face_id / bary / depth");
  if (P > 0 && (!screen || !faces || !tile_start || !pair_face)) return fail("null pointer: screen / faces / tile_start / pair_face");
  const int ntx = (W + TILE - 1) / TILE, nty = (H + TILE - 1) / TILE;
  hipLaunchKernelGGL(k_rs_raster, dim3(ntx, nty), dim3(BATCH), 0, (hipStream_t)stream, screen, V, faces, F, H, W, near, cull, tile_start,
                     pair_face, P, face_id, bary, depth);
  return launched("k_rs_raster");
}

int rb_rs_gbuffer(const int* face_id, const float* bary, int H, int W, const long* index, long n, const int* faces, long F,
                  const float* vertices, long V, const float* uv, const float* vnormals, const float* cam_loc, const float* planes, int R,
                  int C, int filter, float* position, float* uv_out, float* view_dir, float* tex, float* normal, rb_rs_stream_t stream) {
  if (check_image(H, W)) return 1;
  const long n_pixels = (long)H * W;
  if (n < 0 || F < 0 || V < 0) return fail("negative size: n = %ld, F = %ld, V = %ld", n, F, V);
  if (F > MAX_INDEX || V > MAX_INDEX) return fail("F = %ld, V = %ld: indices do not fit 32 bits", F, V);
  if (!index && n != n_pixels) return fail("image form: n = %ld must equal H W = %ld", n, n_pixels);
  if (n > n_pixels) return fail("n = %ld rows of %ld pixels", n, n_pixels);
  if (filter < 0 || filter > 1) return fail("filter = %d outside 0 .. 1", filter);
  if (planes || tex) {
    if (C < 1 || C > RB_RS_MAX_CHANNELS) return fail("C = %d outside 1 .. %d", C, RB_RS_MAX_CHANNELS);
    if (R < 1 || R > RB_RS_MAX_RESOLUTION) return fail("R = %d outside 1 .. %d", R, RB_RS_MAX_RESOLUTION);
    if (!planes || !tex) return fail("null pointer: planes / tex (both or neither)");
  }
  if ((vnormals == nullptr) != (normal == nullptr)) return fail("null pointer: vnormals / normal (both or neither)");
  if (n == 0) return 0;
  if (!face_id || !bary || !cam_loc || !position || !uv_out || !view_dir) return fail("null pointer: face_id / bary / cam_loc / position / uv_out / view_dir");
  if (F > 0 && V > 0 && (!faces || !vertices || !uv)) return fail("null pointer: faces / vertices / uv");
  if (!faces || !vertices || !uv) F = 0;
  hipLaunchKernelGGL(k_rs_gbuffer, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, face_id, bary, n_pixels, index, n, faces, F, vertices,
                     V, uv, vnormals, cam_loc, planes, R, C, filter, position, uv_out, view_dir, tex, normal);
  return launched("k_rs_gbuffer");
}

}  // extern "C"
