// librobir_hip_observe.so: multi-view observations of surface points on the device (include/robir_hip_observe.h) -- the
// per-pair arithmetic of the reference's inv_camera_params + FocusSampler.scatter_sample (model/focus_sampler.py:17-30,63-101), the choice
// of n_obs views per point (training/tex_module.py:50-53 without the full sort) and the fused weighted colour statistics of the bake.  The
// arithmetic is observe_math.h; this file holds the thread indexing, the argument checks and the launches.
//
// The style is ../texbake/texbake.hip's: gather kernels, no atomics, plain fp32 (-ffp-contract=off: the Makefile's default).
#include "../../../include/robir_hip_observe.h"
#include <hip/hip_runtime.h>
#include "observe_math.h"
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

namespace {

using namespace rb::ob;

static_assert(MAX_OBS == RB_OB_MAX_OBS, "the header names the candidate count");
constexpr long MAX_POINTS = (1L << 31) - 1;

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

int check_points(long N) {
  if (N < 0) return fail("N = %ld is negative", N);
  if (N > MAX_POINTS) return fail("N = %ld: 2^31 or more points", N);
  return 0;
}

int check_cameras(int M) {
  if (M < 1) return fail("M = %d: no camera", M);
  if (M > RB_OB_MAX_CAMERAS) return fail("M = %d: more than %d cameras", M, RB_OB_MAX_CAMERAS);
  return 0;
}

int check_images(int H, int W, int C) {
  if (H < 2 || W < 2) return fail("images of %d x %d: H and W must be at least 2", H, W);
  if ((long)H * W > (1L << 28)) return fail("images of %d x %d: more than 2^28 pixels", H, W);
  if (C != 1 && C != 3) return fail("C = %d: 1 or 3 channels", C);
  return 0;
}

// blockIdx.y is the camera: its 24 constants are wave-uniform
template <int C>
__global__ __launch_bounds__(256) void k_ob_scatter(const float* __restrict__ x, long N, const float* __restrict__ cam_loc,
                                                    const float* __restrict__ pose_inv, const float* __restrict__ K,
                                                    const float* __restrict__ images, const float* __restrict__ masks, int H, int W,
                                                    float* __restrict__ uv, float* __restrict__ view_dir, float* __restrict__ rgb,
                                                    unsigned char* __restrict__ valid) {
  const long n = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per (camera, point) pair
  if (n >= N) return;
  scatter_pair<C>((int)blockIdx.y, n, (long)blockIdx.y * N + n, x, cam_loc, pose_inv, K, images, masks, H, W, uv, view_dir, rgb, valid);
}

// blockIdx.y is the camera; uv [M][N][2] -> out [M][N][C]
template <int C>
__global__ __launch_bounds__(256) void k_ob_fetch(const float* __restrict__ images, int H, int W, const float* __restrict__ uv, long N,
                                                  float* __restrict__ out) {
  const long n = (long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const long e = (long)blockIdx.y * N + n;
  float col[C];
  fetch<C>(images + (long)blockIdx.y * H * W * C, H, W, uv[2 * e], uv[2 * e + 1], col);
#pragma unroll
  for (int ch = 0; ch < C; ++ch) out[C * e + ch] = col[ch];
}

// blockIdx.y is the row k of the index
template <int C>
__global__ __launch_bounds__(256) void k_ob_gather(const int* __restrict__ index, const float* __restrict__ x, long N,
                                                   const float* __restrict__ cam_loc, const float* __restrict__ pose_inv,
                                                   const float* __restrict__ K, int M, const float* __restrict__ images,
                                                   const float* __restrict__ masks, int H, int W, float* __restrict__ uv,
                                                   float* __restrict__ view_dir, float* __restrict__ rgb, unsigned char* __restrict__ valid) {
  const long n = (long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  gather_pair<C>((int)blockIdx.y, n, N, M, index, x, cam_loc, pose_inv, K, images, masks, H, W, uv, view_dir, rgb, valid);
}

__global__ __launch_bounds__(256) void k_ob_select(const unsigned char* __restrict__ vis, const float* __restrict__ draws, int M, long N,
                                                   int n_obs, int* __restrict__ index, int* __restrict__ count) {
  const long n = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per point
  if (n >= N) return;
  select_point(n, N, M, n_obs, vis, draws, index, count);
}

template <int C>
__global__ __launch_bounds__(256) void k_ob_accumulate(const float* __restrict__ x, const float* __restrict__ normals, long N,
                                                       const float* __restrict__ cam_loc, const float* __restrict__ pose_inv,
                                                       const float* __restrict__ K, int M, const float* __restrict__ images, int H, int W,
                                                       const unsigned char* __restrict__ vis, float* __restrict__ weight,
                                                       float* __restrict__ mean, float* __restrict__ var, int* __restrict__ count) {
  const long n = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per point
  if (n >= N) return;
  accumulate_point<C>(n, N, M, x, normals, cam_loc, pose_inv, K, images, H, W, vis, weight, mean, var, count);
}

}  // namespace

extern "C" {

int rb_ob_abi_version(void) { return RB_OB_ABI_VERSION; }

const char* rb_ob_last_error(void) { return g_err; }

int rb_ob_scatter(const float* x, long N, const float* cam_loc, const float* pose_inv, const float* K, int M, const float* images,
                  const float* masks, int H, int W, int C, float* uv, float* view_dir, float* rgb, unsigned char* valid,
                  rb_ob_stream_t stream) {
  if (check_points(N) || check_cameras(M) || check_images(H, W, C)) return 1;
  if (N == 0) return 0;
  if (!x || !cam_loc || !pose_inv || !K || !images) return fail("null pointer: x / cam_loc / pose_inv / K / images");
  if (!uv || !view_dir || !rgb || !valid) return fail("null pointer: uv / view_dir / rgb / valid");
  const dim3 grid(blocks_of(N), (unsigned)M);
  if (C == 3)
    hipLaunchKernelGGL(k_ob_scatter<3>, grid, dim3(256), 0, (hipStream_t)stream, x, N, cam_loc, pose_inv, K, images, masks, H, W, uv, view_dir,
                       rgb, valid);
  else
    hipLaunchKernelGGL(k_ob_scatter<1>, grid, dim3(256), 0, (hipStream_t)stream, x, N, cam_loc, pose_inv, K, images, masks, H, W, uv, view_dir,
                       rgb, valid);
  return launched("k_ob_scatter");
}

int rb_ob_fetch(const float* images, int M, int H, int W, int C, const float* uv, long N, float* out, rb_ob_stream_t stream) {
  if (check_points(N) || check_cameras(M) || check_images(H, W, C)) return 1;
  if (N == 0) return 0;
  if (!images || !uv || !out) return fail("null pointer: images / uv / out");
  const dim3 grid(blocks_of(N), (unsigned)M);
  if (C == 3)
    hipLaunchKernelGGL(k_ob_fetch<3>, grid, dim3(256), 0, (hipStream_t)stream, images, H, W, uv, N, out);
  else
    hipLaunchKernelGGL(k_ob_fetch<1>, grid, dim3(256), 0, (hipStream_t)stream, images, H, W, uv, N, out);
  return launched("k_ob_fetch");
}

int rb_ob_gather(const int* index, int n_obs, const float* x, long N, const float* cam_loc, const float* pose_inv, const float* K, int M,
                 const float* images, const float* masks, int H, int W, int C, float* uv, float* view_dir, float* rgb, unsigned char* valid,
                 rb_ob_stream_t stream) {
  if (check_points(N) || check_cameras(M) || check_images(H, W, C)) return 1;
  if (n_obs < 1 || n_obs > RB_OB_MAX_OBS) return fail("n_obs = %d outside 1 .. %d", n_obs, RB_OB_MAX_OBS);
  if (N == 0) return 0;
  if (!index || !x || !cam_loc || !pose_inv || !K || !images) return fail("null pointer: index / x / cam_loc / pose_inv / K / images");
  if (!uv || !view_dir || !rgb || !valid) return fail("null pointer: uv / view_dir / rgb / valid");
  const dim3 grid(blocks_of(N), (unsigned)n_obs);
  if (C == 3)
    hipLaunchKernelGGL(k_ob_gather<3>, grid, dim3(256), 0, (hipStream_t)stream, index, x, N, cam_loc, pose_inv, K, M, images, masks, H, W, uv,
                       view_dir, rgb, valid);
  else
    hipLaunchKernelGGL(k_ob_gather<1>, grid, dim3(256), 0, (hipStream_t)stream, index, x, N, cam_loc, pose_inv, K, M, images, masks, H, W, uv,
                       view_dir, rgb, valid);
  return launched("k_ob_gather");
}

int rb_ob_select(const unsigned char* vis, const float* draws, int M, long N, int n_obs, int* index, int* count, rb_ob_stream_t stream) {
  if (check_points(N) || check_cameras(M)) return 1;
  if (n_obs < 1 || n_obs > RB_OB_MAX_OBS) return fail("n_obs = %d outside 1 .. %d", n_obs, RB_OB_MAX_OBS);
  if (N == 0) return 0;
  if (!vis || !draws || !index || !count) return fail("null pointer: vis / draws / index / count");
  hipLaunchKernelGGL(k_ob_select, dim3(blocks_of(N)), dim3(256), 0, (hipStream_t)stream, vis, draws, M, N, n_obs, index, count);
  return launched("k_ob_select");
}

int rb_ob_accumulate(const float* x, const float* normals, long N, const float* cam_loc, const float* pose_inv, const float* K, int M,
                     const float* images, int H, int W, int C, const unsigned char* vis, float* weight, float* mean, float* var,
                     int* count, rb_ob_stream_t stream) {
  if (check_points(N) || check_cameras(M) || check_images(H, W, C)) return 1;
  if (N == 0) return 0;
  if (!x || !normals || !cam_loc || !pose_inv || !K || !images || !vis) return fail("null pointer: x / normals / cam_loc / pose_inv / K / images / vis");
  if (!weight || !mean || !var || !count) return fail("null pointer: weight / mean / var / count");
  if (C == 3)
    hipLaunchKernelGGL(k_ob_accumulate<3>, dim3(blocks_of(N)), dim3(256), 0, (hipStream_t)stream, x, normals, N, cam_loc, pose_inv, K, M, images,
                       H, W, vis, weight, mean, var, count);
  else
    hipLaunchKernelGGL(k_ob_accumulate<1>, dim3(blocks_of(N)), dim3(256), 0, (hipStream_t)stream, x, normals, N, cam_loc, pose_inv, K, M, images,
                       H, W, vis, weight, mean, var, count);
  return launched("k_ob_accumulate");
}

}  // extern "C"
