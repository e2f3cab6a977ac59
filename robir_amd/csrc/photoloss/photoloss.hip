// librobir_hip_photoloss.so: the photometric loss on the device (include/robir_hip_photoloss.h) -- the reverse mode of
// ACESToneMapping's curves (model/color_correction.py:31-73,116-137) and the fused image loss of InvLoss.forward (model/loss.py:31-42,
// 97-110).  The arithmetic is photoloss_math.h; this file holds the thread indexing, the two-stage reductions, the argument checks and the
// launches.
//
// Element-wise kernels with one thread per row, no atomics; a scalar sum is G block partials in fp64 (plain stores) that a second launch
// adds in index order.
#include "../../../include/robir_hip_photoloss.h"
#include <hip/hip_runtime.h>
#include "photoloss_math.h"
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

namespace {

using namespace rb::pl;

static_assert(MAX_GROUPS == RB_PL_MAX_GROUPS, "the header names the partial count");
static_assert(CURVE_RATIONAL == RB_PL_CURVE_RATIONAL && CURVE_IDENTITY == RB_PL_CURVE_IDENTITY, "the header names the curves");
constexpr long MAX_ROWS = (1L << 31) - 1;

thread_local char g_err[512] = "";

int fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return 1;
}

// the default library's idiom (csrc/common.h) on this library's own error text
#define RB_REQUIRE(cond, ...)                 \
  do {                                        \
    if (!(cond)) return fail(__VA_ARGS__);    \
  } while (0)

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s: %s", what, hipGetErrorString(e));
}

long groups_of(long n) {
  const long g = (n + 255) / 256;
  return g < MAX_GROUPS ? g : MAX_GROUPS;
}

// the 256 fp64 registers of a workgroup added by a fixed tree; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(256) void k_pl_tonemap(const float* __restrict__ x, long n, const float* __restrict__ shift, int shift_stride,
                                                    int curve, int inverse, float* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per element
  if (i >= 3 * n) return;
  const float t = curve_reads_shift(curve) ? shift[(i / 3) * shift_stride] : 1.f;
  y[i] = value_f32(x[i], t, curve, inverse != 0);
}

// gridDim.x = G workgroups; thread j of workgroup b: rows 256 b + j + 256 G k, k = 0, 1, ...   part: [G][2] doubles, slot 1 unused here.
// WANT_X / WANT_T: which derivative is formed at all -- with one of them off, its arithmetic is dead code of the inlined value_d1 and the
// compiler removes it (the other's operations, and so its bits, stay as they are).
template <bool WANT_X, bool WANT_T>
__global__ __launch_bounds__(256) void k_pl_tonemap_bwd(const float* __restrict__ x, long n, const float* __restrict__ shift,
                                                        int shift_stride, int curve, int inverse, const float* __restrict__ gy,
                                                        float* __restrict__ gx, float* __restrict__ gshift, double* __restrict__ part) {
  __shared__ double red[256];
  const bool reads = curve_reads_shift(curve);
  double acc = 0.0;
  for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < n; r += (long)gridDim.x * 256) {
    const float t = reads ? shift[r * shift_stride] : 1.f;
    double gs = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const D1 v = value_d1((double)x[3 * r + c], t, curve, inverse != 0);
      const double g = (double)gy[3 * r + c];
      if (WANT_X) gx[3 * r + c] = (float)(g * v.dx);
      if (WANT_T) gs += g * v.dt;
    }
    if (WANT_T) {
      if (shift_stride == 1) gshift[r] = (float)gs;
      acc += gs;
    }
  }
  if (WANT_T && part) {      // uniform over the grid
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) part[2 * blockIdx.x] = s;
  }
}

// part: [G][2] doubles: the loss's sum and the single-value shift's gradient sum.  WANT_X / WANT_T as above: the value alone forms no derivative.
template <bool WANT_X, bool WANT_T>
__global__ __launch_bounds__(256) void k_pl_image_loss(const float* __restrict__ sg, const float* __restrict__ indir,
                                                       const float* __restrict__ gt, const unsigned char* __restrict__ m1,
                                                       const unsigned char* __restrict__ m2, long N, const float* __restrict__ shift,
                                                       int shift_stride, int curve, int l2, float* __restrict__ g_rgb,
                                                       float* __restrict__ g_shift, double* __restrict__ part) {
  __shared__ double red[256];
  const bool reads = curve_reads_shift(curve);
  const double inv_n = 1.0 / (double)N;
  double acc = 0.0, acc_t = 0.0;
  for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < N; r += (long)gridDim.x * 256) {
    double gx[3] = {0.0, 0.0, 0.0}, gs = 0.0;
    if (m1[r] && m2[r]) {
      const float t = reads ? shift[r * shift_stride] : 1.f;
      acc += loss_row(sg + 3 * r, indir ? indir + 3 * r : nullptr, gt + 3 * r, t, curve, l2 != 0, gx, gs);
      if (WANT_T) acc_t += gs;
    }
    if (WANT_X) {
#pragma unroll
      for (int c = 0; c < 3; ++c) g_rgb[3 * r + c] = (float)(gx[c] * inv_n);
    }
    if (WANT_T && shift_stride == 1) g_shift[r] = (float)(gs * inv_n);
  }
  const double s = block_sum(acc, red);
  __syncthreads();
  const double st = WANT_T ? block_sum(acc_t, red) : 0.0;
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = s;
    part[2 * blockIdx.x + 1] = st;
  }
}

// the G partials of both slots added in index order by one thread (its loads come from LDS); out_k = (float)(sum_k * scale_k), NULL: skipped
__global__ __launch_bounds__(256) void k_pl_finish(const double* __restrict__ part, int G, float* __restrict__ out0, double scale0,
                                                   float* __restrict__ out1, double scale1) {
  __shared__ double buf[2 * MAX_GROUPS];
  for (int i = threadIdx.x; i < 2 * G; i += 256) buf[i] = part[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (out0) {
    double s = 0.0;
    for (int b = 0; b < G; ++b) s += buf[2 * b];
    out0[0] = (float)(s * scale0);
  }
  if (out1) {
    double s = 0.0;
    for (int b = 0; b < G; ++b) s += buf[2 * b + 1];
    out1[0] = (float)(s * scale1);
  }
}

int check_rows(long n) {
  RB_REQUIRE(n >= 0, "n = %ld is negative", n);
  RB_REQUIRE(n <= MAX_ROWS, "n = %ld: 2^31 or more rows", n);
  return 0;
}

int check_curve(int curve, int inverse, const float* shift, int shift_stride) {
  RB_REQUIRE(curve_known(curve), "curve = %d: 0 (scale_aces), 1 (warp_aces), 2 (ln_space), 3 (identity) or 4 (x / (x + 1))", curve);
  RB_REQUIRE(inverse != 2, "inverse = 2: ldr2hdr(x^2.2) (rb_tonemap's op 2) has no counterpart and no backward here");
  RB_REQUIRE(inverse == 0 || inverse == 1, "inverse = %d: 0 (hdr2ldr) or 1 (ldr2hdr)", inverse);
  RB_REQUIRE(!(curve == CURVE_RATIONAL && inverse), "curve 4 (x / (x + 1)) has no inverse");
  RB_REQUIRE(shift_stride == 0 || shift_stride == 1, "shift_stride = %d: 0 (a single value) or 1 (one per row)", shift_stride);
  RB_REQUIRE(shift || !curve_reads_shift(curve), "null pointer: shift (curve %d reads it)", curve);
  return 0;
}

int check_scratch(long n, const void* scratch, long scratch_bytes) {
  RB_REQUIRE(scratch, "null pointer: scratch");
  RB_REQUIRE(((uintptr_t)scratch & 7) == 0, "scratch is not 8-byte aligned");
  RB_REQUIRE(scratch_bytes >= 16 * groups_of(n), "scratch_bytes = %ld: rb_pl_scratch_bytes(%ld) = %ld", scratch_bytes, n, 16 * groups_of(n));
  return 0;
}

}  // namespace

extern "C" {

int rb_pl_abi_version(void) { return RB_PL_ABI_VERSION; }

const char* rb_pl_last_error(void) { return g_err; }

long rb_pl_groups(long n) { return n < 0 ? -1 : groups_of(n); }

long rb_pl_scratch_bytes(long n) { return n < 0 ? -1 : 16 * groups_of(n); }

int rb_pl_tonemap(const float* x, long n, const float* shift, int shift_stride, int curve, int inverse, float* y, rb_pl_stream_t stream) {
  if (check_rows(n) || check_curve(curve, inverse, shift, shift_stride)) return 1;
  if (n == 0) return 0;
  RB_REQUIRE(x && y, "null pointer: x / y");
  hipLaunchKernelGGL(k_pl_tonemap, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n, shift, shift_stride, curve,
                     inverse, y);
  return launched("k_pl_tonemap");
}

int rb_pl_tonemap_bwd(const float* x, long n, const float* shift, int shift_stride, int curve, int inverse, const float* gy, float* gx,
                      float* gshift, void* scratch, long scratch_bytes, rb_pl_stream_t stream) {
  if (check_rows(n) || check_curve(curve, inverse, shift, shift_stride)) return 1;
  if (n == 0) return 0;
  RB_REQUIRE(x && gy, "null pointer: x / gy");
  const bool reduce = gshift && shift_stride == 0;
  if (reduce && check_scratch(n, scratch, scratch_bytes)) return 1;
  if (!gx && !gshift) return 0;
  const int G = (int)groups_of(n);
  double* part = reduce ? (double*)scratch : nullptr;
  auto* kernel = gx ? (gshift ? k_pl_tonemap_bwd<true, true> : k_pl_tonemap_bwd<true, false>) : k_pl_tonemap_bwd<false, true>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, x, n, shift, shift_stride, curve, inverse, gy, gx, gshift,
                     part);
  if (launched("k_pl_tonemap_bwd")) return 1;
  if (!reduce) return 0;
  hipLaunchKernelGGL(k_pl_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)part, G, gshift, 1.0, (float*)nullptr, 0.0);
  return launched("k_pl_finish");
}

int rb_pl_image_loss(const float* sg_rgb, const float* indir_rgb, const float* gt, const unsigned char* net_mask,
                     const unsigned char* obj_mask, long N, const float* shift, int shift_stride, int curve, int l2, float* loss,
                     float* g_rgb, float* g_shift, void* scratch, long scratch_bytes, rb_pl_stream_t stream) {
  if (check_rows(N) || check_curve(curve, 0, shift, shift_stride)) return 1;
  RB_REQUIRE(l2 == 0 || l2 == 1, "l2 = %d: 0 (L1) or 1 (L2)", l2);
  if (N == 0) return 0;
  RB_REQUIRE(sg_rgb && gt && net_mask && obj_mask, "null pointer: sg_rgb / gt / net_mask / obj_mask");
  RB_REQUIRE(loss, "null pointer: loss");
  if (check_scratch(N, scratch, scratch_bytes)) return 1;
  const int G = (int)groups_of(N);
  double* part = (double*)scratch;
  auto* kernel = g_rgb ? (g_shift ? k_pl_image_loss<true, true> : k_pl_image_loss<true, false>)
                       : (g_shift ? k_pl_image_loss<false, true> : k_pl_image_loss<false, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, sg_rgb, indir_rgb, gt, net_mask, obj_mask, N, shift,
                     shift_stride, curve, l2, g_rgb, g_shift, part);
  if (launched("k_pl_image_loss")) return 1;
  const double inv_n = 1.0 / (double)N;
  hipLaunchKernelGGL(k_pl_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)part, G, loss, inv_n,
                     (g_shift && shift_stride == 0) ? g_shift : (float*)nullptr, inv_n);
  return launched("k_pl_finish");
}

}  // extern "C"
