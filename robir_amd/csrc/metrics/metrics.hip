// librobir_hip_metrics.so: image metrics on the device (include/robir_hip_metrics.h) -- the sums behind MSE / MAE / PSNR / the
// albedo ratio, the angular error of two normal fields and SSIM, V views per launch.  The arithmetic is metrics_math.h; this file holds the
// thread indexing, the LDS staging of the SSIM tiles, the two-stage reductions, the argument checks and the launches.
//
// No atomics: a per-view sum is G block partials in fp64 (plain stores) that a second launch adds in index order.
#include "../../../include/robir_hip_metrics.h"
#include <hip/hip_runtime.h>
#include "metrics_math.h"
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

namespace {

using namespace rb::mt;

static_assert(MAX_GROUPS == RB_MT_MAX_GROUPS && ROWS == RB_MT_ROWS && TILE == RB_MT_SSIM_TILE && MAX_CHANNELS == RB_MT_MAX_CHANNELS,
              "the header names the work shape");
static_assert(TRANSFER_NONE == RB_MT_NONE && TRANSFER_CLIP == RB_MT_CLIP && TRANSFER_GAMMA22 == RB_MT_GAMMA22 &&
                  TRANSFER_GAMMA22_Q8 == RB_MT_GAMMA22_Q8,
              "the header names the transfers");
static_assert(ROWS == 256 && TILE * TILE == 256, "256-thread workgroups: one row per thread and stride, one SSIM window per thread");
constexpr long MAX_ROWS = (1L << 31) - 1;
constexpr int FINISH_CHUNK = 128;                       // partials of one view staged in LDS at a time by k_mt_finish
constexpr int MAX_SLOTS = 1 + 5 * MAX_CHANNELS;         // output values per view of the widest reduction

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

long groups_of(long P) {
  const long g = (P + ROWS - 1) / ROWS;
  return g < MAX_GROUPS ? g : MAX_GROUPS;
}

long tiles_of(long H, long W) { return ((H - HALO + TILE - 1) / TILE) * ((W - HALO + TILE - 1) / TILE); }

// the 256 fp64 registers of a workgroup added by a fixed tree; every thread gets the sum, and red may be written again on return
__device__ __forceinline__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// grid (G, V); thread j of workgroup b of view v: rows 256 b + j + 256 G k, k = 0, 1, ...   part: [V][G][1 + 5 C]
template <int C>
__global__ __launch_bounds__(256) void k_mt_pair(const float* __restrict__ pred, const float* __restrict__ gt, long P,
                                                 const unsigned char* __restrict__ mask, const float* __restrict__ scale, int transfer,
                                                 double* __restrict__ part) {
  __shared__ double red[256];
  constexpr int K = 1 + 5 * C;
  const long base = (long)blockIdx.y * P;
  float sc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) sc[c] = scale ? scale[c] : 1.f;
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  for (long r = (long)blockIdx.x * ROWS + threadIdx.x; r < P; r += (long)gridDim.x * ROWS) {
    if (mask && !mask[base + r]) continue;
    acc[0] += 1.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      double p, g;
      load_pair(pred[(base + r) * C + c], gt[(base + r) * C + c], sc[c], transfer, p, g);
      pair_terms(p, g, acc + 1 + 5 * c);
    }
  }
  double* out = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * K;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double s = block_sum(acc[k], red);
    if (threadIdx.x == 0) out[k] = s;
  }
}

// the same walk over the rows of two [V, P, 3] fields; part: [V][G][2] = {count, sum of angle}
__global__ __launch_bounds__(256) void k_mt_angular(const float* __restrict__ a, const float* __restrict__ b, long P,
                                                    const unsigned char* __restrict__ mask, double* __restrict__ part) {
  __shared__ double red[256];
  const long base = (long)blockIdx.y * P;
  double cnt = 0.0, sum = 0.0;
  for (long r = (long)blockIdx.x * ROWS + threadIdx.x; r < P; r += (long)gridDim.x * ROWS) {
    if (mask && !mask[base + r]) continue;
    double angle;
    if (angle_between(a + 3 * (base + r), b + 3 * (base + r), angle)) {
      cnt += 1.0;
      sum += angle;
    }
  }
  double* out = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
  const double c = block_sum(cnt, red), s = block_sum(sum, red);
  if (threadIdx.x == 0) {
    out[0] = c;
    out[1] = s;
  }
}

// grid (tiles, V), tiles in row-major order over the map; thread t: window (t / 16, t % 16) of the tile.  part: [V][tiles][2]
template <int C>
__global__ __launch_bounds__(256) void k_mt_ssim(const float* __restrict__ pred, const float* __restrict__ gt, long H, long W,
                                                 const unsigned char* __restrict__ mask, const float* __restrict__ scale, int transfer,
                                                 Window win, float* __restrict__ map, double* __restrict__ part) {
  __shared__ double sp[C][PATCH][PATCH], sg[C][PATCH][PATCH];      // the transferred patch of both images, every channel
  __shared__ double hm[5][PATCH][TILE];                            // the horizontal pass of one channel's five moments
  __shared__ double red[256];
  const long v = blockIdx.y, mh = H - HALO, mw = W - HALO;
  const long tiles_x = (mw + TILE - 1) / TILE;
  const long y0 = ((long)blockIdx.x / tiles_x) * TILE, x0 = ((long)blockIdx.x % tiles_x) * TILE;
  float sc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) sc[c] = scale ? scale[c] : 1.f;
  // one pass over tile + halo: PATCH rows of PATCH * C contiguous floats; outside the image: zeros, which feed only windows that are not stored
  for (int idx = threadIdx.x; idx < PATCH * PATCH * C; idx += 256) {
    const int r = idx / (PATCH * C), e = idx % (PATCH * C), col = e / C, c = e % C;
    const long gy = y0 + r, gx = x0 + col;
    double p = 0.0, g = 0.0;
    if (gy < H && gx < W) {
      const long at = ((v * H + gy) * W + gx) * C + c;
      load_pair(pred[at], gt[at], sc[c], transfer, p, g);
    }
    sp[c][r][col] = p;
    sg[c][r][col] = g;
  }
  __syncthreads();
  const int ti = threadIdx.x / TILE, tj = threadIdx.x % TILE;
  const long oi = y0 + ti, oj = x0 + tj;
  const bool inside = oi < mh && oj < mw;
  const bool counted = inside && (!mask || mask[(v * H + oi + RADIUS) * W + oj + RADIUS]);
  double sum = 0.0;
  float vals[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    for (int it = threadIdx.x; it < PATCH * TILE; it += 256) {
      const int r = it / TILE, j = it % TILE;
      double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < TAPS; ++k) {
        double t[5];
        moment_terms(sp[c][r][j + k], sg[c][r][j + k], t);
#pragma unroll
        for (int q = 0; q < 5; ++q) m[q] += win.w[k] * t[q];
      }
#pragma unroll
      for (int q = 0; q < 5; ++q) hm[q][r][j] = m[q];
    }
    __syncthreads();
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < TAPS; ++k) {
#pragma unroll
      for (int q = 0; q < 5; ++q) m[q] += win.w[k] * hm[q][ti + k][tj];
    }
    const double s = counted ? ssim_quotient(m) : 0.0;
    sum += s;
    vals[c] = (float)s;
    __syncthreads();      // hm is written again by the next channel
  }
  if (map && inside) {
    float* o = map + ((v * mh + oi) * mw + oj) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = vals[c];
  }
  double* out = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
  const double n = block_sum(counted ? 1.0 : 0.0, red), s = block_sum(sum, red);
  if (threadIdx.x == 0) {
    out[0] = n;
    out[1] = s;
  }
}

// grid V: view v's G partials [G][K] added in index order, thread k < K the k-th value (its loads come from LDS, FINISH_CHUNK partials at a
// time); out [V][K]
__global__ __launch_bounds__(256) void k_mt_finish(const double* __restrict__ part, long G, int K, double* __restrict__ out) {
  __shared__ double buf[FINISH_CHUNK * MAX_SLOTS];
  const double* src = part + (long)blockIdx.x * G * K;
  double s = 0.0;
  for (long b0 = 0; b0 < G; b0 += FINISH_CHUNK) {
    const int n = (int)((G - b0 < FINISH_CHUNK) ? G - b0 : FINISH_CHUNK);
    for (int i = threadIdx.x; i < n * K; i += 256) buf[i] = src[b0 * K + i];
    __syncthreads();
    if ((int)threadIdx.x < K)
      for (int b = 0; b < n; ++b) s += buf[b * K + threadIdx.x];
    __syncthreads();
  }
  if ((int)threadIdx.x < K) out[(long)blockIdx.x * K + threadIdx.x] = s;
}

int check_views_rows(long V, long P) {
  RB_REQUIRE(V >= 0, "V = %ld is negative", V);
  RB_REQUIRE(P >= 0, "P = %ld is negative", P);
  RB_REQUIRE(V <= RB_MT_MAX_VIEWS, "V = %ld: more than %d views", V, RB_MT_MAX_VIEWS);
  RB_REQUIRE(P <= MAX_ROWS, "P = %ld: 2^31 or more pixels", P);
  return 0;
}

int check_channels(int C) {
  RB_REQUIRE(C >= 1 && C <= MAX_CHANNELS, "C = %d: 1 .. %d channels", C, MAX_CHANNELS);
  return 0;
}

int check_transfer(int transfer) {
  RB_REQUIRE(transfer_known(transfer), "transfer = %d: 0 (none), 1 (clip), 2 (gamma 2.2) or 3 (gamma 2.2, 8 bit)", transfer);
  return 0;
}

int check_image(long V, long H, long W) {
  RB_REQUIRE(V >= 0, "V = %ld is negative", V);
  RB_REQUIRE(H >= 0 && W >= 0, "H = %ld, W = %ld: negative", H, W);
  RB_REQUIRE(V <= RB_MT_MAX_VIEWS, "V = %ld: more than %d views", V, RB_MT_MAX_VIEWS);
  RB_REQUIRE(H >= TAPS && W >= TAPS, "H = %ld, W = %ld: SSIM needs at least one valid 11 x 11 window", H, W);
  RB_REQUIRE(H <= MAX_ROWS / W, "H = %ld, W = %ld: 2^31 or more pixels", H, W);
  return 0;
}

int check_scratch(const void* scratch, long scratch_bytes, long need, const char* query) {
  RB_REQUIRE(scratch, "null pointer: scratch");
  RB_REQUIRE(((uintptr_t)scratch & 7) == 0, "scratch is not 8-byte aligned");
  RB_REQUIRE(scratch_bytes >= need, "scratch_bytes = %ld: %s = %ld", scratch_bytes, query, need);
  return 0;
}

int finish(const double* part, long V, long G, int K, double* stats, hipStream_t stream) {
  hipLaunchKernelGGL(k_mt_finish, dim3((unsigned)V), dim3(256), 0, stream, part, G, K, stats);
  return launched("k_mt_finish");
}

}  // namespace

extern "C" {

int rb_mt_abi_version(void) { return RB_MT_ABI_VERSION; }

const char* rb_mt_last_error(void) { return g_err; }

long rb_mt_groups(long P) { return (P < 0 || P > MAX_ROWS) ? -1 : groups_of(P); }

long rb_mt_ssim_tiles(long H, long W) {
  if (H < 0 || W < 0) return -1;
  if (H == 0 || W == 0) return 0;
  if (H < TAPS || W < TAPS || H > MAX_ROWS / W) return -1;
  return tiles_of(H, W);
}

long rb_mt_pair_scratch_bytes(long V, long P, int C) {
  if (V < 0 || V > RB_MT_MAX_VIEWS || P < 0 || P > MAX_ROWS || C < 1 || C > MAX_CHANNELS) return -1;
  return 8 * V * groups_of(P) * (1 + 5 * C);
}

long rb_mt_angular_scratch_bytes(long V, long P) {
  if (V < 0 || V > RB_MT_MAX_VIEWS || P < 0 || P > MAX_ROWS) return -1;
  return 16 * V * groups_of(P);
}

long rb_mt_ssim_scratch_bytes(long V, long H, long W) {
  const long t = rb_mt_ssim_tiles(H, W);
  if (V < 0 || V > RB_MT_MAX_VIEWS || t < 0) return -1;
  return 16 * V * t;
}

int rb_mt_pair_stats(const float* pred, const float* gt, long V, long P, int C, const unsigned char* mask, const float* scale, int transfer,
                     double* stats, void* scratch, long scratch_bytes, rb_mt_stream_t stream) {
  if (check_views_rows(V, P) || check_channels(C) || check_transfer(transfer)) return 1;
  if (V == 0 || P == 0) return 0;
  RB_REQUIRE(pred && gt, "null pointer: pred / gt");
  RB_REQUIRE(stats, "null pointer: stats");
  const long G = groups_of(P);
  const int K = 1 + 5 * C;
  if (check_scratch(scratch, scratch_bytes, 8 * V * G * K, "rb_mt_pair_scratch_bytes(V, P, C)")) return 1;
  double* part = (double*)scratch;
  auto* kernel = C == 1 ? k_mt_pair<1> : C == 2 ? k_mt_pair<2> : C == 3 ? k_mt_pair<3> : k_mt_pair<4>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)G, (unsigned)V), dim3(256), 0, (hipStream_t)stream, pred, gt, P, mask, scale, transfer, part);
  if (launched("k_mt_pair")) return 1;
  return finish(part, V, G, K, stats, (hipStream_t)stream);
}

int rb_mt_angular_stats(const float* a, const float* b, long V, long P, const unsigned char* mask, double* stats, void* scratch,
                        long scratch_bytes, rb_mt_stream_t stream) {
  if (check_views_rows(V, P)) return 1;
  if (V == 0 || P == 0) return 0;
  RB_REQUIRE(a && b, "null pointer: a / b");
  RB_REQUIRE(stats, "null pointer: stats");
  const long G = groups_of(P);
  if (check_scratch(scratch, scratch_bytes, 16 * V * G, "rb_mt_angular_scratch_bytes(V, P)")) return 1;
  double* part = (double*)scratch;
  hipLaunchKernelGGL(k_mt_angular, dim3((unsigned)G, (unsigned)V), dim3(256), 0, (hipStream_t)stream, a, b, P, mask, part);
  if (launched("k_mt_angular")) return 1;
  return finish(part, V, G, 2, stats, (hipStream_t)stream);
}

int rb_mt_ssim(const float* pred, const float* gt, long V, long H, long W, int C, const unsigned char* mask, const float* scale, int transfer,
               double* stats, float* map, void* scratch, long scratch_bytes, rb_mt_stream_t stream) {
  if (check_image(V, H, W) || check_channels(C) || check_transfer(transfer)) return 1;
  if (V == 0) return 0;
  RB_REQUIRE(pred && gt, "null pointer: pred / gt");
  RB_REQUIRE(stats, "null pointer: stats");
  const long G = tiles_of(H, W);
  if (check_scratch(scratch, scratch_bytes, 16 * V * G, "rb_mt_ssim_scratch_bytes(V, H, W)")) return 1;
  double* part = (double*)scratch;
  const Window win = make_window();
  auto* kernel = C == 1 ? k_mt_ssim<1> : C == 2 ? k_mt_ssim<2> : C == 3 ? k_mt_ssim<3> : k_mt_ssim<4>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)G, (unsigned)V), dim3(256), 0, (hipStream_t)stream, pred, gt, H, W, mask, scale, transfer, win, map,
                     part);
  if (launched("k_mt_ssim")) return 1;
  return finish(part, V, G, 2, stats, (hipStream_t)stream);
}

}  // extern "C"
