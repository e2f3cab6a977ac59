// librobir_hip_lightfit.so: fitting the light SGs to an environment map on the device (include/robir_hip_lightfit.h) -- the
// reverse mode of k_envmap_sg (../sg_shade.hip), the fused steps of the reference's fit (envmaps/fit_envmap_with_sg.py:50-55: forward, MSE,
// gradient, Adam) and the area down-sample of the target.  The per-(pixel, lobe) arithmetic is lightfit_math.h; this file holds the loops,
// the reductions, the argument checks and the launch order.
//
// The work shape is k_sg_shade_bwd's (../sg_shade_bwd.hip, DESIGN 4.1 "The two sums over points"): a persistent grid of G = min(ceil(n / 4),
// 512) workgroups of four waves, wave w of workgroup b takes the pixels 4 b + w, 4 b + w + 4 G, ...; a lane owns lobes k and k + 64 of a
// 128-lobe tile (blockIdx.y) and keeps their seven fp64 partial sums in registers across its pixels; the four waves are added through LDS in
// wave order; every workgroup stores one slab [7 M + 1] of doubles with plain stores (the last entry is its share of the squared error);
// k_lf_finish adds the G slabs in index order, applies the chain to the raw rows and, in the fit, the Adam update.  No atomics: the
// association of every sum is a function of (n, M) alone.
#include "../../../include/robir_hip_lightfit.h"
#include <hip/hip_runtime.h>
#include "lightfit_math.h"
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

namespace {

using namespace rb::lf;

constexpr int WAVES = 4, MAX_GROUPS = 512, TILE = 128;      // TILE: lobes whose partials one workgroup keeps, two per lane
constexpr int FIN_LOBES = 32, FIN_ELEMS = FIN_LOBES * 7;    // lobes and slab entries of one finishing workgroup
constexpr int MAX_TILES = 65535;                            // grid.y
constexpr long MAX_PIXELS = 1L << 36;                       // of a fit: 3 n and the first pass's grid stay in range
constexpr long MAX_SRC_PIXELS = 1L << 31;                   // of rb_lf_area_resize's source: one thread per destination pixel

thread_local char g_err[512] = "";

int fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return 1;
}

__device__ __forceinline__ double wave_sum_d(double v) {      // sg_common.h's wave_sum on doubles: every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

enum { UP_GIVEN = 0, FIT_WAVE = 1, FIT_RGB_IN = 2 };

// MODE UP_GIVEN:   `up` is the upstream gradient g_rgb [n,3] (rb_lf_envmap_sg_bwd)
//      FIT_WAVE:   `up` is the target [n,3]; one lobe tile: rgb[p] is a wave reduction of the lanes' lobes
//      FIT_RGB_IN: `up` is the target; several tiles: rgb[p] comes from k_lf_rgb's pass (rgb_in [n,3] fp64), tile 0 carries the loss
template <int MODE>
__global__ __launch_bounds__(256) void k_lf_accum(const float* __restrict__ lgt, int M, const float* __restrict__ dirs, long n,
                                                  const float* __restrict__ up, const double* __restrict__ rgb_in, double inv_3n,
                                                  double* __restrict__ slabs, long stride) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, tile = blockIdx.y;
  Lobe L[2];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const long k = (long)tile * TILE + jj * 64 + lane;
    L[jj] = k < M ? lobe_of(lgt + 7 * k) : no_lobe();
  }
  double acc[2][7], sq = 0.0;
#pragma unroll
  for (int jj = 0; jj < 2; ++jj)
#pragma unroll
    for (int i = 0; i < 7; ++i) acc[jj][i] = 0.0;
  const long step = (long)WAVES * gridDim.x;
  for (long p = (long)WAVES * blockIdx.x + w; p < n; p += step) {      // wave-uniform: the shuffles below run on whole waves
    const double d[3] = {(double)dirs[3 * p], (double)dirs[3 * p + 1], (double)dirs[3 * p + 2]};
    double e[2], cm1[2], r[3];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) e[jj] = lobe_e(L[jj], d, cm1[jj]);
    if (MODE == UP_GIVEN) {
#pragma unroll
      for (int c = 0; c < 3; ++c) r[c] = (double)up[3 * p + c];
    } else {
      double rgb[3] = {0.0, 0.0, 0.0};
      if (MODE == FIT_WAVE) {
        lobe_rgb(L[0], e[0], rgb);
        lobe_rgb(L[1], e[1], rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = wave_sum_d(rgb[c]);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = rgb_in[3 * p + c];
      }
      sq += mse_upstream(rgb, up + 3 * p, inv_3n, r);
    }
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) lobe_accum(L[jj], d, cm1[jj], e[jj], r, acc[jj]);
  }
  // ---- the four waves of the workgroup, in wave order, then one slab per workgroup
  __shared__ double lds[WAVES][TILE * 7];
  __shared__ double lds_sq[WAVES];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj)
#pragma unroll
    for (int i = 0; i < 7; ++i) lds[w][(jj * 64 + lane) * 7 + i] = acc[jj][i];
  if (lane == 0) lds_sq[w] = sq;
  __syncthreads();
  double* slab = slabs + blockIdx.x * stride;
  for (int e = threadIdx.x; e < TILE * 7; e += 256) {
    const long g = (long)tile * TILE * 7 + e;
    if (g < (long)M * 7) slab[g] = ((lds[0][e] + lds[1][e]) + lds[2][e]) + lds[3][e];
  }
  if (tile == 0 && threadIdx.x == 0) slab[stride - 1] = ((lds_sq[0] + lds_sq[1]) + lds_sq[2]) + lds_sq[3];
}

// rgb[p] = the lobes' shares added in lobe order, fp64 (the first pass of a fit with more than one lobe tile)
__global__ __launch_bounds__(256) void k_lf_rgb(const float* __restrict__ lgt, int M, const float* __restrict__ dirs, long n,
                                                double* __restrict__ rgb) {
  __shared__ Lobe sh[TILE];
  const long p = blockIdx.x * 256L + threadIdx.x;
  double d[3] = {0.0, 0.0, 1.0}, acc[3] = {0.0, 0.0, 0.0};
  if (p < n)
    for (int c = 0; c < 3; ++c) d[c] = (double)dirs[3 * p + c];
  for (int k0 = 0; k0 < M; k0 += TILE) {
    __syncthreads();
    if (threadIdx.x < TILE && k0 + (int)threadIdx.x < M) sh[threadIdx.x] = lobe_of(lgt + 7L * (k0 + threadIdx.x));
    __syncthreads();
    const int m = M - k0 < TILE ? M - k0 : TILE;
    for (int k = 0; k < m; ++k) {
      double cm1;
      const double e = lobe_e(sh[k], d, cm1);
      lobe_rgb(sh[k], e, acc);
    }
  }
  if (p < n)
    for (int c = 0; c < 3; ++c) rgb[3 * p + c] = acc[c];
}

struct Adam {
  double lr, beta1, beta2, eps, bc1, bc2;
};

// A workgroup owns FIN_LOBES lobes: thread t < FIN_ELEMS adds slab entry blockIdx.x FIN_ELEMS + t over the G slabs in index order, then
// forms element t % 7 of lobe t / 7's raw-row gradient from the lobe's seven sums and stores it (d_lgt) or applies Adam's step to that
// element.  The rows are read before the barrier and written after it; no other workgroup touches them.
template <bool ADAM>
__global__ __launch_bounds__(256) void k_lf_finish(const double* __restrict__ slabs, int G, long stride, int M, float* lgt, float* d_lgt,
                                                   float* adam_m, float* adam_v, Adam A, double inv_3n, double* loss_out) {
  __shared__ double S[FIN_ELEMS];
  const int t = threadIdx.x;
  const long e = (long)blockIdx.x * FIN_ELEMS + t;
  const bool live = t < FIN_ELEMS && e < 7L * M;
  const long k = (long)blockIdx.x * FIN_LOBES + t / 7;
  const int comp = t % 7;
  float row[7] = {0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += slabs[g * stride + e];
    S[t] = s;
#pragma unroll
    for (int i = 0; i < 7; ++i) row[i] = lgt[7 * k + i];
  }
  if (ADAM && blockIdx.x == 0 && t == FIN_ELEMS) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += slabs[g * stride + stride - 1];
    loss_out[0] = s * inv_3n;
  }
  __syncthreads();
  if (!live) return;
  const Lobe L = lobe_of(row);
  double g7[7], g = 0.0;
  lobe_chain(row, L, S + (t / 7) * 7, g7);
#pragma unroll
  for (int i = 0; i < 7; ++i) g = i == comp ? g7[i] : g;
  if (ADAM)
    adam_element(lgt[e], adam_m[e], adam_v[e], g, A.lr, A.beta1, A.beta2, A.eps, A.bc1, A.bc2);
  else
    d_lgt[e] = (float)g;
}

// one thread per destination pixel; the overlaps of footprint and source pixels are integers in units of 1 / (H W) of a source pixel
__global__ void k_lf_area_resize(const float* __restrict__ src, int H0, int W0, float* __restrict__ dst, int H, int W) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)H * W) return;
  const long y = i / W, x = i % W;
  const long ya = y * H0, yb = ya + H0, xa = x * W0, xb = xa + W0;      // source pixel j covers [j H, (j + 1) H) on this scale
  double acc[3] = {0.0, 0.0, 0.0};
  for (long j = ya / H; j <= (yb - 1) / H; ++j) {
    const long oy = (yb < (j + 1) * H ? yb : (j + 1) * H) - (ya > j * H ? ya : j * H);
    for (long q = xa / W; q <= (xb - 1) / W; ++q) {
      const long ox = (xb < (q + 1) * W ? xb : (q + 1) * W) - (xa > q * W ? xa : q * W);
      const double wgt = (double)(oy * ox);
      const float* s = src + (j * W0 + q) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += wgt * (double)s[c];
    }
  }
  const double area = (double)H0 * (double)W0;
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[3 * i + c] = (float)(acc[c] / area);
}

long groups(long n) {
  const long g = (n + WAVES - 1) / WAVES;
  return g < MAX_GROUPS ? g : MAX_GROUPS;
}

int tiles(int M) { return (M + TILE - 1) / TILE; }

long scratch_doubles(long n, int M) { return groups(n) * (7L * M + 1) + (M > TILE ? 3 * n : 0L); }

// what both entry points check of (n, M) and of their scratch
int check_shape(long n, int M) {
  if (n < 0) return fail("n = %ld is negative", n);
  if (n > MAX_PIXELS) return fail("n = %ld: more than 2^36 pixels", n);
  if (M < 1) return fail("M = %d: need at least one lobe", M);
  if (tiles(M) > MAX_TILES) return fail("M = %d: more than %d lobe tiles of %d", M, MAX_TILES, TILE);
  return 0;
}

int check_scratch(const void* scratch, long scratch_bytes, long n, int M) {
  const long need = scratch_doubles(n, M) * (long)sizeof(double);
  if (!scratch) return fail("null pointer: scratch");
  if ((uintptr_t)scratch % 8) return fail("scratch is not 8-byte aligned");
  if (scratch_bytes < need) return fail("scratch too small: %ld bytes given, %ld needed (rb_lf_scratch_bytes)", scratch_bytes, need);
  return 0;
}

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s: %s", what, hipGetErrorString(e));
}

}  // namespace

extern "C" {

int rb_lf_abi_version(void) { return RB_LF_ABI_VERSION; }

const char* rb_lf_last_error(void) { return g_err; }

long rb_lf_groups(long n) {
  if (n < 0) return fail("n = %ld is negative", n), -1;
  return groups(n);
}

long rb_lf_scratch_bytes(long n, int M) {
  if (check_shape(n, M)) return -1;
  return scratch_doubles(n, M) * (long)sizeof(double);
}

int rb_lf_envmap_sg_bwd(const float* lgt, int M, const float* dirs, long n, const float* g_rgb, float* d_lgt, void* scratch,
                        long scratch_bytes, rb_lf_stream_t stream) {
  if (check_shape(n, M)) return 1;
  if (n == 0) return 0;
  if (!lgt || !dirs || !g_rgb || !d_lgt) return fail("null pointer: lgt / dirs / g_rgb / d_lgt");
  if (check_scratch(scratch, scratch_bytes, n, M)) return 1;
  hipStream_t st = (hipStream_t)stream;
  const int G = (int)groups(n);
  const long stride = 7L * M + 1;
  double* slabs = (double*)scratch;
  hipLaunchKernelGGL(k_lf_accum<UP_GIVEN>, dim3(G, tiles(M)), dim3(256), 0, st, lgt, M, dirs, n, g_rgb, (const double*)nullptr, 0.0, slabs,
                     stride);
  if (launched("k_lf_accum")) return 1;
  hipLaunchKernelGGL(k_lf_finish<false>, dim3((M + FIN_LOBES - 1) / FIN_LOBES), dim3(256), 0, st, (const double*)slabs, G, stride, M,
                     const_cast<float*>(lgt), d_lgt, (float*)nullptr, (float*)nullptr, Adam{}, 0.0, (double*)nullptr);
  return launched("k_lf_finish");
}

int rb_lf_fit_steps(float* lgt, float* adam_m, float* adam_v, int M, const float* dirs, const float* target, long n, long first_step,
                    long n_steps, double lr, double beta1, double beta2, double eps, double* loss_hist, void* scratch, long scratch_bytes,
                    rb_lf_stream_t stream) {
  if (check_shape(n, M)) return 1;
  if (n_steps < 0) return fail("n_steps = %ld is negative", n_steps);
  if (first_step < 0) return fail("first_step = %ld is negative", first_step);
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail("beta1 = %g, beta2 = %g outside [0, 1)", beta1, beta2);
  if (!(eps >= 0.0)) return fail("eps = %g is negative", eps);
  if (!(lr == lr)) return fail("lr is not a number");
  if (n == 0 || n_steps == 0) return 0;
  if (!lgt || !adam_m || !adam_v || !dirs || !target || !loss_hist) return fail("null pointer: lgt / adam_m / adam_v / dirs / target / loss_hist");
  if (check_scratch(scratch, scratch_bytes, n, M)) return 1;
  hipStream_t st = (hipStream_t)stream;
  const int G = (int)groups(n), T = tiles(M);
  const long stride = 7L * M + 1;
  double* slabs = (double*)scratch;
  double* rgb = slabs + G * stride;                      // [n, 3], only with T > 1
  const double inv_3n = 1.0 / (3.0 * (double)n);
  for (long i = 0; i < n_steps; ++i) {
    const double t = (double)(first_step + i + 1);
    const Adam A{lr, beta1, beta2, eps, 1.0 - pow(beta1, t), 1.0 - pow(beta2, t)};
    if (T > 1) {
      hipLaunchKernelGGL(k_lf_rgb, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)lgt, M, dirs, n, rgb);
      hipLaunchKernelGGL(k_lf_accum<FIT_RGB_IN>, dim3(G, T), dim3(256), 0, st, (const float*)lgt, M, dirs, n, target, (const double*)rgb,
                         inv_3n, slabs, stride);
    } else {
      hipLaunchKernelGGL(k_lf_accum<FIT_WAVE>, dim3(G, 1), dim3(256), 0, st, (const float*)lgt, M, dirs, n, target, (const double*)nullptr,
                         inv_3n, slabs, stride);
    }
    hipLaunchKernelGGL(k_lf_finish<true>, dim3((M + FIN_LOBES - 1) / FIN_LOBES), dim3(256), 0, st, (const double*)slabs, G, stride, M, lgt,
                       (float*)nullptr, adam_m, adam_v, A, inv_3n, loss_hist + i);
    if (launched("rb_lf_fit_steps")) return 1;
  }
  return 0;
}

int rb_lf_area_resize(const float* src, int H0, int W0, float* dst, int H, int W, rb_lf_stream_t stream) {
  if (H < 1 || W < 1 || H0 < 1 || W0 < 1) return fail("empty image: %d x %d -> %d x %d", H0, W0, H, W);
  if ((long)H0 * W0 > MAX_SRC_PIXELS) return fail("source %d x %d: more than 2^31 pixels", H0, W0);
  if (H > H0 || W > W0) return fail("up-sampling refused: %d x %d -> %d x %d (an area mean only shrinks)", H0, W0, H, W);
  if (!src || !dst) return fail("null pointer: src / dst");
  const long count = (long)H * W;
  hipLaunchKernelGGL(k_lf_area_resize, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, H0, W0, dst, H, W);
  return launched("k_lf_area_resize");
}

}  // extern "C"
