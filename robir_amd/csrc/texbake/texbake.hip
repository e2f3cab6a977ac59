// librobir_hip_texbake.so: baking into texture space on the device (include/robir_hip_texbake.h) -- the per-triangle atlas,
// the UV-space rasteriser that stands in for the reference's OpenGL pass (model/rasterizor.py), attribute interpolation, one ring of
// erode_map (model/texture_model.py:24-45) and TexSampler.sample's arithmetic (texture_model.py:135-160).  The per-face and per-texel
// arithmetic is texbake_math.h; this file holds the loops, the argument checks and the launches.
//
// The style is ../mesh.hip's: gather kernels, one thread per output element, no atomics, plain fp32 (-ffp-contract=off: the Makefile's
// default).  Binning is k_mesh_count / k_mesh_verts' pattern: a count kernel, an exclusive prefix on the caller's side, an emit kernel.
#include "../../../include/robir_hip_texbake.h"
#include <hip/hip_runtime.h>
#include "texbake_math.h"
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

namespace {

using namespace rb::tb;

static_assert(TILE == RB_TB_TILE, "the header names the tile size");
constexpr long MAX_FACES = (1L << 31) - 1, MAX_PAIRS = (1L << 31) - 1;
constexpr int MAX_CHANNELS = 64;

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

int check_texture(long F, int R) {
  if (F < 0) return fail("F = %ld is negative", F);
  if (F > MAX_FACES) return fail("F = %ld: face indices do not fit 32 bits", F);
  if (R < 1) return fail("R = %d: empty texture", R);
  if (R > RB_TB_MAX_RESOLUTION) return fail("R = %d: more than %d texels per side", R, RB_TB_MAX_RESOLUTION);
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------- atlas
__global__ __launch_bounds__(256) void k_tb_atlas(long F, long ncols, int S, int R, float* __restrict__ uv) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per face corner
  if (i >= 3 * F) return;
  float o[2];
  atlas_corner(i / 3, (int)(i % 3), ncols, S, R, o);
  uv[2 * i] = o[0];
  uv[2 * i + 1] = o[1];
}

// ---------------------------------------------------------------------------------------------------------------- binning
__global__ __launch_bounds__(256) void k_tb_bin_count(const float* __restrict__ uv, long F, int R, int* __restrict__ counts) {
  const long f = (long)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  int tx0, ty0, tw;
  counts[f] = (int)face_tiles(face_of(uv + 6 * f, R), tx0, ty0, tw);
}

__global__ __launch_bounds__(256) void k_tb_bin_emit(const float* __restrict__ uv, long F, int R, const long* __restrict__ base, long P,
                                                     int* __restrict__ pair_tile, int* __restrict__ pair_face) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per pair
  if (p >= P) return;
  long lo = 0, hi = F;                                      // the last face with base[f] <= p: base is non-decreasing, base[0] = 0
  while (hi - lo > 1) {
    const long mid = lo + (hi - lo) / 2;
    if (base[mid] <= p) lo = mid; else hi = mid;
  }
  int tx0, ty0, tw;
  const long count = face_tiles(face_of(uv + 6 * lo, R), tx0, ty0, tw), k = p - base[lo];
  const int ntiles = (R + TILE - 1) / TILE;
  int tile = -1, face = -1;
  if (k >= 0 && k < count) {                                // count > 0, hence tw > 0
    tile = (ty0 + (int)(k / tw)) * ntiles + tx0 + (int)(k % tw);
    face = (int)lo;
  }
  pair_tile[p] = tile;
  pair_face[p] = face;
}

// ---------------------------------------------------------------------------------------------------------------- raster
__global__ __launch_bounds__(TILE* TILE) void k_tb_raster(const float* __restrict__ uv, long F, int R, const int* __restrict__ tile_start,
                                                          const int* __restrict__ pair_face, long P, int* __restrict__ face_id,
                                                          float* __restrict__ bary) {
  const int ntiles = (R + TILE - 1) / TILE;
  const int tile = blockIdx.y * ntiles + blockIdx.x;
  const int r = blockIdx.y * TILE + threadIdx.x / TILE, c = blockIdx.x * TILE + threadIdx.x % TILE;
  if (r >= R || c >= R) return;
  long a = 0, b = 0;
  if (P > 0) {                                              // a list out of [0, P] is clipped, never followed
    a = tile_start[tile];
    b = tile_start[tile + 1];
    a = a < 0 ? 0 : a;
    b = b > P ? P : b;
  }
  int hit = -1;
  float w[2] = {0.0f, 0.0f};
  for (long i = a; i < b; ++i) {                            // wave-uniform bounds and loads; ascending faces: the first that covers wins
    const int f = pair_face[i];
    if (f < 0 || f >= F) continue;
    if (covers(face_of(uv + 6 * (long)f, R), r, c, w)) {
      hit = f;
      break;
    }
  }
  const long t = (long)r * R + c;
  face_id[t] = hit;
  bary[2 * t] = hit < 0 ? 0.0f : w[0];
  bary[2 * t + 1] = hit < 0 ? 0.0f : w[1];
}

// ---------------------------------------------------------------------------------------------------------------- interpolation
__global__ __launch_bounds__(256) void k_tb_interp(const int* __restrict__ face_id, const float* __restrict__ bary, long n_texels,
                                                   const long* __restrict__ index, long n, const int* __restrict__ faces, long F,
                                                   const float* __restrict__ attr, long V, int C, float* __restrict__ out) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per output element
  if (e >= n * C) return;
  const long i = e / C;
  const int ch = (int)(e % C);
  const long t = index ? index[i] : i;
  float o = 0.0f;
  if (t >= 0 && t < n_texels) {
    const int f = face_id[t];
    if (f >= 0 && f < F) {
      const long v0 = faces[3 * (long)f], v1 = faces[3 * (long)f + 1], v2 = faces[3 * (long)f + 2];
      if (v0 >= 0 && v0 < V && v1 >= 0 && v1 < V && v2 >= 0 && v2 < V) {
        const float b0 = bary[2 * t], b1 = bary[2 * t + 1], b2 = (1.0f - b0) - b1;
        o = (b0 * attr[v0 * C + ch] + b1 * attr[v1 * C + ch]) + b2 * attr[v2 * C + ch];
      }
    }
  }
  out[e] = o;
}

// ---------------------------------------------------------------------------------------------------------------- dilation
__global__ __launch_bounds__(256) void k_tb_dilate(const float* __restrict__ image, const unsigned char* __restrict__ mask, int H, int W, int C,
                                                   float* __restrict__ dst, unsigned char* __restrict__ mask_out) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per output element
  if (e >= (long)H * W * C) return;
  const long t = e / C;
  const int ch = (int)(e % C), r = (int)(t / W), c = (int)(t % W);
  if (mask[t]) {
    dst[e] = image[e];
    if (ch == 0) mask_out[t] = mask[t];
    return;
  }
  float sum = 0.0f;
  int count = 0;
  for (int dr = -1; dr <= 1; ++dr)
    for (int dc = -1; dc <= 1; ++dc) {
      const int rr = r + dr, cc = c + dc;
      if ((dr == 0 && dc == 0) || rr < 0 || rr >= H || cc < 0 || cc >= W) continue;
      const long u = (long)rr * W + cc;
      if (mask[u]) {
        sum += image[u * C + ch];
        ++count;
      }
    }
  dst[e] = count ? sum / (float)count : image[e];
  if (ch == 0) mask_out[t] = count ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------- sampler
// grid_sample, bilinear, zeros padding, align_corners=False, of a [R, R, C] image at texel coordinates (x, y): texels out of the image count
// as +0 and every product is formed, so the association is the same at the border
template <int C>
__device__ __forceinline__ void fetch(const float* __restrict__ img, int R, float x, float y, float* o) {
  const float x0 = floorf(x), y0 = floorf(y);
  const float wx1 = x - x0, wx0 = (x0 + 1.0f) - x, wy1 = y - y0, wy0 = (y0 + 1.0f) - y;
  const float nw = wx0 * wy0, ne = wx1 * wy0, sw = wx0 * wy1, se = wx1 * wy1;
  // x0, y0 beyond the image by more than a texel contribute nothing: clamp before the conversion so that it cannot overflow
  const int c0 = (int)fminf(fmaxf(x0, -2.0f), (float)R + 1.0f), r0 = (int)fminf(fmaxf(y0, -2.0f), (float)R + 1.0f);
  const bool cin0 = c0 >= 0 && c0 < R, cin1 = c0 + 1 >= 0 && c0 + 1 < R, rin0 = r0 >= 0 && r0 < R, rin1 = r0 + 1 >= 0 && r0 + 1 < R;
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const float a = rin0 && cin0 ? img[((long)r0 * R + c0) * C + ch] : 0.0f;
    const float b = rin0 && cin1 ? img[((long)r0 * R + c0 + 1) * C + ch] : 0.0f;
    const float c = rin1 && cin0 ? img[((long)(r0 + 1) * R + c0) * C + ch] : 0.0f;
    const float d = rin1 && cin1 ? img[((long)(r0 + 1) * R + c0 + 1) * C + ch] : 0.0f;
    o[ch] = ((a * nw + b * ne) + c * sw) + d * se;
  }
}

__device__ __forceinline__ void unit_clamped(const float* v, float* __restrict__ o) {
  const float len = fmaxf(sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]), 1e-4f);
  o[0] = v[0] / len;
  o[1] = v[1] / len;
  o[2] = v[2] / len;
}

__global__ __launch_bounds__(256) void k_tb_sample(const float* __restrict__ position, const float* __restrict__ normal,
                                                   const float* __restrict__ mask, int R, const float* __restrict__ uv, long n, float scale,
                                                   float* __restrict__ x, float* __restrict__ normal_out,
                                                   unsigned char* __restrict__ object_mask, float* __restrict__ tangent_u,
                                                   float* __restrict__ tangent_v) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per sample
  if (i >= n) return;
  const float fr = (float)R, u = uv[2 * i], v = uv[2 * i + 1];
  const float tx = u * fr - 0.5f, ty = (1.0f - v) * fr - 0.5f;
  const float txu = (u + 0.001f) * fr - 0.5f, tyv = (1.0f - (v + 0.001f)) * fr - 0.5f;
  float p[3], nr[3], m[1], pu[3], pv[3], du[3], dv[3];
  fetch<3>(position, R, tx, ty, p);
  fetch<3>(normal, R, tx, ty, nr);
  fetch<1>(mask, R, tx, ty, m);
  fetch<3>(position, R, txu, ty, pu);
  fetch<3>(position, R, tx, tyv, pv);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    x[3 * i + k] = p[k] * scale;
    du[k] = pu[k] - p[k];
    dv[k] = pv[k] - p[k];
  }
  unit_clamped(nr, normal_out + 3 * i);
  unit_clamped(dv, tangent_u + 3 * i);                      // the reference's assignment: tangent_u is the v-difference
  unit_clamped(du, tangent_v + 3 * i);
  object_mask[i] = m[0] > 0.1f ? 1 : 0;
}

}  // namespace

extern "C" {

int rb_tb_abi_version(void) { return RB_TB_ABI_VERSION; }

const char* rb_tb_last_error(void) { return g_err; }

long rb_tb_atlas_cell(long F, int R) {
  if (check_texture(F, R)) return -1;
  if (F < 1) return fail("F = %ld: an atlas needs at least one face", F), -1;
  const long ncols = atlas_ncols(F), S = R / ncols;
  if (S < 6)
    return fail("R = %d gives cells of %ld texels for %ld faces (%ld columns): the smallest resolution at which every face owns a texel is %ld",
                R, S, F, ncols, 6 * ncols), -1;
  return S;
}

int rb_tb_atlas_uv(long F, int R, float* uv, rb_tb_stream_t stream) {
  const long S = rb_tb_atlas_cell(F, R);
  if (S < 0) return 1;
  if (!uv) return fail("null pointer: uv");
  hipLaunchKernelGGL(k_tb_atlas, dim3(blocks_of(3 * F)), dim3(256), 0, (hipStream_t)stream, F, atlas_ncols(F), (int)S, R, uv);
  return launched("k_tb_atlas");
}

int rb_tb_bin_count(const float* uv, long F, int R, int* counts, rb_tb_stream_t stream) {
  if (check_texture(F, R)) return 1;
  if (F == 0) return 0;
  if (!uv || !counts) return fail("null pointer: uv / counts");
  hipLaunchKernelGGL(k_tb_bin_count, dim3(blocks_of(F)), dim3(256), 0, (hipStream_t)stream, uv, F, R, counts);
  return launched("k_tb_bin_count");
}

int rb_tb_bin_emit(const float* uv, long F, int R, const long* base, long P, int* pair_tile, int* pair_face, rb_tb_stream_t stream) {
  if (check_texture(F, R)) return 1;
  if (P < 0) return fail("P = %ld is negative", P);
  if (P > MAX_PAIRS) return fail("P = %ld: 2^31 or more (tile, face) pairs", P);
  if (P == 0) return 0;
  if (F == 0) return fail("P = %ld pairs of no face", P);
  if (!uv || !base || !pair_tile || !pair_face) return fail("null pointer: uv / base / pair_tile / pair_face");
  hipLaunchKernelGGL(k_tb_bin_emit, dim3(blocks_of(P)), dim3(256), 0, (hipStream_t)stream, uv, F, R, base, P, pair_tile, pair_face);
  return launched("k_tb_bin_emit");
}

int rb_tb_raster(const float* uv, long F, int R, const int* tile_start, const int* pair_face, long P, int* face_id, float* bary,
                 rb_tb_stream_t stream) {
  if (check_texture(F, R)) return 1;
  if (P < 0) return fail("P = %ld is negative", P);
  if (P > MAX_PAIRS) return fail("P = %ld: 2^31 or more (tile, face) pairs", P);
  if (F == 0) P = 0;
  if (!face_id || !bary) return fail("null pointer: face_id / bary");
  if (P > 0 && (!uv || !tile_start || !pair_face)) return fail("null pointer: uv / tile_start / pair_face");
  const int ntiles = (R + TILE - 1) / TILE;
  hipLaunchKernelGGL(k_tb_raster, dim3(ntiles, ntiles), dim3(TILE * TILE), 0, (hipStream_t)stream, uv, F, R, tile_start, pair_face, P, face_id,
                     bary);
  return launched("k_tb_raster");
}

int rb_tb_interp(const int* face_id, const float* bary, long n_texels, const long* index, long n, const int* faces, long F,
                 const float* attr, long V, int C, float* out, rb_tb_stream_t stream) {
  if (n < 0 || n_texels < 0 || F < 0 || V < 0) return fail("negative size: n = %ld, n_texels = %ld, F = %ld, V = %ld", n, n_texels, F, V);
  if (F > MAX_FACES || V > MAX_FACES) return fail("F = %ld, V = %ld: indices do not fit 32 bits", F, V);
  if (n_texels > (long)RB_TB_MAX_RESOLUTION * RB_TB_MAX_RESOLUTION) return fail("n_texels = %ld: more than 16384^2", n_texels);
  if (C < 1 || C > MAX_CHANNELS) return fail("C = %d outside 1 .. %d", C, MAX_CHANNELS);
  if (!index && n != n_texels) return fail("image form: n = %ld must equal n_texels = %ld", n, n_texels);
  if (n > n_texels) return fail("n = %ld outputs of %ld texels", n, n_texels);
  if (n == 0) return 0;
  if (!face_id || !bary || !out) return fail("null pointer: face_id / bary / out");
  if (F > 0 && V > 0 && (!faces || !attr)) return fail("null pointer: faces / attr");
  if (!faces || !attr) F = 0;
  hipLaunchKernelGGL(k_tb_interp, dim3(blocks_of(n * C)), dim3(256), 0, (hipStream_t)stream, face_id, bary, n_texels, index, n, faces, F, attr,
                     V, C, out);
  return launched("k_tb_interp");
}

int rb_tb_dilate(const float* image, const unsigned char* mask, int H, int W, int C, float* dst, unsigned char* mask_out,
                 rb_tb_stream_t stream) {
  if (H < 1 || W < 1) return fail("empty image: %d x %d", H, W);
  if (H > RB_TB_MAX_RESOLUTION || W > RB_TB_MAX_RESOLUTION) return fail("image %d x %d: more than %d texels per side", H, W, RB_TB_MAX_RESOLUTION);
  if (C < 1 || C > MAX_CHANNELS) return fail("C = %d outside 1 .. %d", C, MAX_CHANNELS);
  if (!image || !mask || !dst || !mask_out) return fail("null pointer: image / mask / dst / mask_out");
  if ((const void*)image == (const void*)dst || mask == mask_out) return fail("dst / mask_out alias image / mask: dilation is ping-pong");
  hipLaunchKernelGGL(k_tb_dilate, dim3(blocks_of((long)H * W * C)), dim3(256), 0, (hipStream_t)stream, image, mask, H, W, C, dst, mask_out);
  return launched("k_tb_dilate");
}

int rb_tb_sample(const float* position, const float* normal, const float* mask, int R, const float* uv, long n, float scale, float* x,
                 float* normal_out, unsigned char* object_mask, float* tangent_u, float* tangent_v, rb_tb_stream_t stream) {
  if (check_texture(0, R)) return 1;
  if (n < 0) return fail("n = %ld is negative", n);
  if (n > (1L << 36)) return fail("n = %ld: more than 2^36 samples", n);
  if (n == 0) return 0;
  if (!position || !normal || !mask || !uv) return fail("null pointer: position / normal / mask / uv");
  if (!x || !normal_out || !object_mask || !tangent_u || !tangent_v) return fail("null pointer: x / normal / object_mask / tangent_u / tangent_v");
  hipLaunchKernelGGL(k_tb_sample, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, position, normal, mask, R, uv, n, scale, x, normal_out,
                     object_mask, tangent_u, tangent_v);
  return launched("k_tb_sample");
}

}  // extern "C"
