// librobir_hip_texfit.so: fitting the texels of a baked atlas through the mesh view (include/robir_hip_texfit.h) -- the taps
// that linearise the view's plane fetch, the fetch formed from them, its transpose as a gather over (row, tap) pairs sorted by texel, and a
// lazy Adam step on the touched texels.  The per-row, per-segment and per-element arithmetic is texfit_math.h; this file holds the loops, the
// argument checks and the launches.
//
// The style is ../raster/raster.hip's: gather kernels, no atomics, -ffp-contract=off (the Makefile's default), wave64, 256-thread workgroups.
#include "../../../include/robir_hip_texfit.h"
#include <hip/hip_runtime.h>
#include "texfit_math.h"
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

namespace {

using namespace rb::tf;

static_assert(MAX_CHANNELS == RB_TF_MAX_CHANNELS, "the header names the constant");

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

int check_atlas(int R, int Cs, int C) {
  if (R < 1 || R > RB_TF_MAX_RESOLUTION) return fail("R = %d outside 1 .. %d", R, RB_TF_MAX_RESOLUTION);
  if (Cs < 1 || Cs > RB_TF_MAX_CHANNELS) return fail("Cs = %d outside 1 .. %d", Cs, RB_TF_MAX_CHANNELS);
  if (C < 1 || C > Cs) return fail("C = %d outside 1 .. Cs = %d", C, Cs);
  return 0;
}

int check_rows(long n) {
  if (n < 0) return fail("negative size: n = %ld", n);
  if (n > RB_TF_MAX_ROWS) return fail("n = %ld: 2^29 or more rows, 4 n does not fit 32 bits", n);
  return 0;
}

struct PerChannel {
  double lr[MAX_CHANNELS], lo[MAX_CHANNELS], hi[MAX_CHANNELS];
};

// ---------------------------------------------------------------------------------------------------------------- taps, fetch
__global__ __launch_bounds__(256) void k_tf_taps(const float* __restrict__ uv, long n, int R, int filter, int* __restrict__ tap_texel,
                                                 float* __restrict__ tap_weight) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per row
  if (i >= n) return;
  int t[4];
  float w[4];
  taps_row(uv[2 * i], uv[2 * i + 1], R, filter, t, w);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    tap_texel[4 * i + k] = t[k];
    tap_weight[4 * i + k] = w[k];
  }
}

__global__ __launch_bounds__(256) void k_tf_fetch(const float* __restrict__ planes, int R, int Cs, const int* __restrict__ tap_texel,
                                                  const float* __restrict__ tap_weight, long n, int C, float* __restrict__ tex) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per row
  if (i >= n) return;
  int t[4];
  float w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    t[k] = tap_texel[4 * i + k];
    w[k] = tap_weight[4 * i + k];
  }
  fetch_row(planes, R, Cs, t, w, C, tex + (long)C * i);
}

// ---------------------------------------------------------------------------------------------------------------- the transpose
// One thread per segment.  Neighbouring threads own neighbouring pair ranges, so for short segments (a fine atlas under a coarse view: one
// to a few pairs each) a wave reads pair_row / pair_weight from one contiguous stretch.  VEC4: C == 4 and g_tex 16-byte aligned, a row of
// g_tex is one vector load; the sums are the same numbers in the same order as gather_segment's.
template <bool VEC4>
__global__ __launch_bounds__(256) void k_tf_scatter(const int* __restrict__ pair_row, const float* __restrict__ pair_weight, long P,
                                                    const int* __restrict__ seg_start, long T, const float* __restrict__ g_tex, long n, int C,
                                                    float* __restrict__ grad) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= T) return;
  long p0 = seg_start[s], p1 = seg_start[s + 1];
  p0 = p0 < 0 ? 0 : p0;
  p1 = p1 > P ? P : p1;
  if (VEC4) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (long p = p0; p < p1; ++p) {
      const long row = pair_row[p];
      if (row < 0 || row >= n) continue;
      const double w = (double)pair_weight[p];
      const float4 g = reinterpret_cast<const float4*>(g_tex)[row];
      a0 += w * (double)g.x;
      a1 += w * (double)g.y;
      a2 += w * (double)g.z;
      a3 += w * (double)g.w;
    }
    float* o = grad + 4 * s;
    o[0] = (float)a0;
    o[1] = (float)a1;
    o[2] = (float)a2;
    o[3] = (float)a3;
  } else {
    gather_segment(pair_row, pair_weight, p0, p1, g_tex, n, C, grad + (long)C * s);
  }
}

// ---------------------------------------------------------------------------------------------------------------- lazy Adam
__global__ __launch_bounds__(256) void k_tf_adam(float* __restrict__ planes, float* __restrict__ adam_m, float* __restrict__ adam_v,
                                                 const int* __restrict__ seg_texel, const float* __restrict__ grad, long T, int R, int Cs, int C,
                                                 PerChannel pc, double beta1, double beta2, double eps, double bc1, double bc2) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per (segment, channel)
  if (e >= T * C) return;
  const long s = e / C;
  const int c = (int)(e - s * C);
  const long texel = seg_texel[s];
  if (texel < 0 || texel >= (long)R * R) return;
  float p = planes[texel * Cs + c], m = adam_m[texel * C + c], v = adam_v[texel * C + c];
  double lr = 0.0, lo = 0.0, hi = 0.0;
#pragma unroll
  for (int k = 0; k < MAX_CHANNELS; ++k)                     // a select chain over kernel arguments: no indexed private array
    if (k == c) {
      lr = pc.lr[k];
      lo = pc.lo[k];
      hi = pc.hi[k];
    }
  adam_element(p, m, v, (double)grad[e], lr, lo, hi, beta1, beta2, eps, bc1, bc2);
  planes[texel * Cs + c] = p;
  adam_m[texel * C + c] = m;
  adam_v[texel * C + c] = v;
}

}  // namespace

extern "C" {

int rb_tf_abi_version(void) { return RB_TF_ABI_VERSION; }

const char* rb_tf_last_error(void) { return g_err; }

int rb_tf_taps(const float* uv, long n, int R, int filter, int* tap_texel, float* tap_weight, rb_tf_stream_t stream) {
  if (check_rows(n)) return 1;
  if (R < 1 || R > RB_TF_MAX_RESOLUTION) return fail("R = %d outside 1 .. %d", R, RB_TF_MAX_RESOLUTION);
  if (filter < 0 || filter > 1) return fail("filter = %d outside 0 .. 1", filter);
  if (n == 0) return 0;
  if (!uv || !tap_texel || !tap_weight) return fail("null pointer: uv / tap_texel / tap_weight");
  hipLaunchKernelGGL(k_tf_taps, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, uv, n, R, filter, tap_texel, tap_weight);
  return launched("k_tf_taps");
}

int rb_tf_fetch(const float* planes, int R, int Cs, const int* tap_texel, const float* tap_weight, long n, int C, float* tex,
                rb_tf_stream_t stream) {
  if (check_rows(n) || check_atlas(R, Cs, C)) return 1;
  if (n == 0) return 0;
  if (!planes || !tap_texel || !tap_weight || !tex) return fail("null pointer: planes / tap_texel / tap_weight / tex");
  hipLaunchKernelGGL(k_tf_fetch, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, planes, R, Cs, tap_texel, tap_weight, n, C, tex);
  return launched("k_tf_fetch");
}

int rb_tf_scatter(const int* pair_row, const float* pair_weight, long P, const int* seg_start, long T, const float* g_tex, long n, int C,
                  float* grad, rb_tf_stream_t stream) {
  if (check_rows(n)) return 1;
  if (P < 0 || T < 0) return fail("negative size: P = %ld, T = %ld", P, T);
  if (P > 4 * n) return fail("P = %ld pairs of n = %ld rows: more than 4 n", P, n);
  if (T > P) return fail("T = %ld segments of P = %ld pairs", T, P);
  if (C < 1 || C > RB_TF_MAX_CHANNELS) return fail("C = %d outside 1 .. %d", C, RB_TF_MAX_CHANNELS);
  if (T == 0 || P == 0) return 0;
  if (!pair_row || !pair_weight || !seg_start || !g_tex || !grad) return fail("null pointer: pair_row / pair_weight / seg_start / g_tex / grad");
  const dim3 grid(blocks_of(T)), block(256);
  if (C == 4 && ((uintptr_t)g_tex & 15) == 0)
    hipLaunchKernelGGL(k_tf_scatter<true>, grid, block, 0, (hipStream_t)stream, pair_row, pair_weight, P, seg_start, T, g_tex, n, C, grad);
  else
    hipLaunchKernelGGL(k_tf_scatter<false>, grid, block, 0, (hipStream_t)stream, pair_row, pair_weight, P, seg_start, T, g_tex, n, C, grad);
  return launched("k_tf_scatter");
}

int rb_tf_adam(float* planes, float* adam_m, float* adam_v, const int* seg_texel, const float* grad, long T, int R, int Cs, int C,
               const double* lr, const double* lo, const double* hi, double beta1, double beta2, double eps, double bc1, double bc2,
               rb_tf_stream_t stream) {
  if (check_atlas(R, Cs, C)) return 1;
  if (T < 0) return fail("negative size: T = %ld", T);
  if (T > (long)R * R) return fail("T = %ld touched texels of an atlas of %ld", T, (long)R * R);
  if (!lr || !lo || !hi) return fail("null pointer: lr / lo / hi (host arrays of C doubles)");
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail("beta = (%g, %g) outside [0, 1)", beta1, beta2);
  if (!(bc1 > 0.0 && bc1 <= 1.0) || !(bc2 > 0.0 && bc2 <= 1.0)) return fail("bias corrections (%g, %g) outside (0, 1]", bc1, bc2);
  if (!(eps >= 0.0)) return fail("eps = %g is negative", eps);
  PerChannel pc{};
  for (int c = 0; c < C; ++c) {
    if (!(lr[c] >= 0.0) || !(lo[c] <= hi[c])) return fail("channel %d: lr = %g, clamp [%g, %g]", c, lr[c], lo[c], hi[c]);
    pc.lr[c] = lr[c];
    pc.lo[c] = lo[c];
    pc.hi[c] = hi[c];
  }
  if (T == 0) return 0;
  if (!planes || !adam_m || !adam_v || !seg_texel || !grad) return fail("null pointer: planes / adam_m / adam_v / seg_texel / grad");
  hipLaunchKernelGGL(k_tf_adam, dim3(blocks_of(T * C)), dim3(256), 0, (hipStream_t)stream, planes, adam_m, adam_v, seg_texel, grad, T, R, Cs, C,
                     pc, beta1, beta2, eps, bc1, bc2);
  return launched("k_tf_adam");
}

}  // extern "C"
