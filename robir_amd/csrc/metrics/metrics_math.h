// The per-pixel arithmetic of the image metrics (include/robir_hip_metrics.h): the transfer applied on load, one pixel's share of
// the pair sums, one row's angular error, the SSIM window and the SSIM quotient.  No launch geometry and no memory traffic: the kernels of
// metrics.hip index and reduce around these bodies, and a host compiler builds them as they are (tools/metrics_host.cpp) -- the
// photoloss_math.h pattern.
//
// Arithmetic: everything here is fp64 formed from the fp32 inputs; what is stored as fp32 (the SSIM map) is rounded once, by the caller.
#pragma once
#include <math.h>

#ifndef RB_MT_FN
#ifdef __HIPCC__
#define RB_MT_FN __host__ __device__ __forceinline__
#else
#define RB_MT_FN inline
#endif
#endif

namespace rb {
namespace mt {

constexpr int TRANSFER_NONE = 0, TRANSFER_CLIP = 1, TRANSFER_GAMMA22 = 2, TRANSFER_GAMMA22_Q8 = 3;
constexpr int MAX_CHANNELS = 4;
constexpr int ROWS = 256;            // rows per workgroup and per grid stride of the pair / angular kernels
constexpr int MAX_GROUPS = 1024;     // workgroups per view of the pair / angular kernels
constexpr int TAPS = 11, HALO = TAPS - 1, RADIUS = TAPS / 2;
constexpr int TILE = 16;             // SSIM outputs per workgroup and axis
constexpr int PATCH = TILE + HALO;   // SSIM inputs per workgroup and axis
constexpr double SSIM_C1 = 0.01 * 0.01, SSIM_C2 = 0.03 * 0.03;      // (K1 L)^2, (K2 L)^2 with the data range L = 1
constexpr double SHORT_VECTOR = 1e-6;

RB_MT_FN bool transfer_known(int t) { return t >= TRANSFER_NONE && t <= TRANSFER_GAMMA22_Q8; }

RB_MT_FN double clip01(double x) { return fmin(fmax(x, 0.0), 1.0); }

// T(x): nothing, clip, clip(max(x, 0)^(1 / 2.2)), and the last followed by floor(255 x) / 255 (what an 8-bit PNG of it holds)
RB_MT_FN double transfer(double x, int t) {
  if (t == TRANSFER_NONE) return x;
  if (t == TRANSFER_CLIP) return clip01(x);
  const double y = clip01(pow(fmax(x, 0.0), 1.0 / 2.2));
  return t == TRANSFER_GAMMA22_Q8 ? floor(255.0 * y) / 255.0 : y;
}

// p = T(scale * pred), g = T(gt) of one value; scale is the fp32 factor of the channel (1 where the caller has none)
RB_MT_FN void load_pair(float pred, float gt, float scale, int t, double& p, double& g) {
  p = transfer((double)scale * (double)pred, t);
  g = transfer((double)gt, t);
}

// one value's share of a channel's five sums: acc[0 .. 4] += d^2, |d|, p g, p^2, g^2 with d = p - g
RB_MT_FN void pair_terms(double p, double g, double* acc) {
  const double d = p - g;
  acc[0] += d * d;
  acc[1] += fabs(d);
  acc[2] += p * g;
  acc[3] += p * p;
  acc[4] += g * g;
}

// the angle between two rows in radians; false (and no angle) where either is shorter than SHORT_VECTOR
RB_MT_FN bool angle_between(const float* a, const float* b, double& angle) {
  const double ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2];
  const double la = sqrt(ax * ax + ay * ay + az * az), lb = sqrt(bx * bx + by * by + bz * bz);
  if (!(la >= SHORT_VECTOR) || !(lb >= SHORT_VECTOR)) return false;
  const double dot = (ax / la) * (bx / lb) + (ay / la) * (by / lb) + (az / la) * (bz / lb);
  angle = acos(fmin(fmax(dot, -1.0), 1.0));
  return true;
}

// the 11-tap Gaussian window, sigma = 1.5: exp(-x^2 / 4.5) normalised.  Formed on the host and handed to the kernel by value.
struct Window {
  double w[TAPS];
};

inline Window make_window() {
  Window r;
  double s = 0.0;
  for (int k = 0; k < TAPS; ++k) {
    const double x = (double)(k - RADIUS);
    r.w[k] = exp(-x * x / 4.5);
    s += r.w[k];
  }
  for (int k = 0; k < TAPS; ++k) r.w[k] /= s;
  return r;
}

// the five moments' integrands of one pixel pair: x, y, x^2, y^2, x y
RB_MT_FN void moment_terms(double x, double y, double* m) {
  m[0] = x;
  m[1] = y;
  m[2] = x * x;
  m[3] = y * y;
  m[4] = x * y;
}

// Wang et al.'s quotient from the five window means (population moments).  x == y gives exactly 1: 2 mx my == mx^2 + my^2 and
// 2 sxy == sx + sy bit for bit when the two images' moments are the same numbers (no contraction: -ffp-contract=off).
RB_MT_FN double ssim_quotient(const double* m) {
  const double mx = m[0], my = m[1];
  const double sx = m[2] - mx * mx, sy = m[3] - my * my, sxy = m[4] - mx * my;
  return ((2.0 * mx * my + SSIM_C1) * (2.0 * sxy + SSIM_C2)) / ((mx * mx + my * my + SSIM_C1) * (sx + sy + SSIM_C2));
}

}  // namespace mt
}  // namespace rb
