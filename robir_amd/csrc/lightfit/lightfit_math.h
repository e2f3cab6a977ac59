// The light-SG environment map (model/sg_render.py:26-42), its derivative and the fit's step for ONE (pixel, lobe) pair, ONE lobe and ONE
// parameter element.  No launch geometry and no memory traffic: the kernels of lightfit.hip loop and reduce around these bodies, and a host
// compiler builds them as they are (tools/lightfit_host.cpp) -- the sg_shade_bwd_math.h pattern.
//
// For lobe k with raw row s = lgt[k]:  a = s[0:3] / |s[0:3]| (no epsilon),  lam = |s[3]|,  mu = |s[4:7]|,
//   rgb[p] = sum_k mu_k e_pk,   e = exp(lam (c - 1)),   c = d_p . a.
// With the upstream r[p] (3 values) and q = r . mu a lobe needs seven sums over the pixels (Sums):
//   S0[3] = sum r e,   S1 = sum q e (c - 1),   S2[3] = sum q e lam d_p,
// and the chain to the raw row happens once, after the reduction (lobe_chain):
//   d mu_raw = sign(mu_raw) S0,   d lam_raw = sign(lam_raw) S1,   d l = (S2 - a (a . S2)) / |l|        (sign(0) = 0, as torch.abs).
//
// Arithmetic: every quantity is formed in fp64 from the fp32 inputs and accumulated in fp64; what is stored is rounded to
// fp32 once, by the caller.
#pragma once
#include <math.h>

#ifndef RB_LF_FN
#ifdef __HIPCC__
#define RB_LF_FN __device__ __forceinline__
#else
#define RB_LF_FN inline
#endif
#endif

namespace rb {
namespace lf {

struct Lobe {
  double a[3], len, lam, mu[3];      // unit axis, |l|, |lambda_raw|, |mu_raw|
};

RB_LF_FN Lobe lobe_of(const float* s) {
  Lobe L;
  const double x = (double)s[0], y = (double)s[1], z = (double)s[2];
  L.len = sqrt(x * x + y * y + z * z);
  L.a[0] = x / L.len;
  L.a[1] = y / L.len;
  L.a[2] = z / L.len;
  L.lam = fabs((double)s[3]);
  for (int c = 0; c < 3; ++c) L.mu[c] = fabs((double)s[4 + c]);
  return L;
}

// a lane without a lobe: contributes exact zeros to every sum and never a NaN
RB_LF_FN Lobe no_lobe() {
  Lobe L;
  L.a[0] = L.a[1] = 0.0;
  L.a[2] = L.len = 1.0;
  L.lam = 0.0;
  L.mu[0] = L.mu[1] = L.mu[2] = 0.0;
  return L;
}

// e = exp(lam (c - 1)); cm1 receives c - 1
RB_LF_FN double lobe_e(const Lobe& L, const double* d, double& cm1) {
  cm1 = (d[0] * L.a[0] + d[1] * L.a[1] + d[2] * L.a[2]) - 1.0;
  return exp(L.lam * cm1);
}

// the lobe's share of rgb[p]
RB_LF_FN void lobe_rgb(const Lobe& L, double e, double* rgb) {
  for (int c = 0; c < 3; ++c) rgb[c] += L.mu[c] * e;
}

// S += this pixel's terms; S = [S0[3], S1, S2[3]]
RB_LF_FN void lobe_accum(const Lobe& L, const double* d, double cm1, double e, const double* r, double* S) {
  const double q = r[0] * L.mu[0] + r[1] * L.mu[1] + r[2] * L.mu[2];
  const double qe = q * e;
  for (int c = 0; c < 3; ++c) S[c] += r[c] * e;
  S[3] += qe * cm1;
  const double w = qe * L.lam;
  for (int c = 0; c < 3; ++c) S[4 + c] += w * d[c];
}

RB_LF_FN double sign_of(float x) { return x > 0.f ? 1.0 : (x < 0.f ? -1.0 : 0.0); }

// the seven sums of a lobe -> the gradient of its raw row, in the row's order (axis, sharpness, amplitude)
RB_LF_FN void lobe_chain(const float* s, const Lobe& L, const double* S, double* g) {
  const double t = L.a[0] * S[4] + L.a[1] * S[5] + L.a[2] * S[6];
  for (int c = 0; c < 3; ++c) g[c] = (S[4 + c] - L.a[c] * t) / L.len;
  g[3] = sign_of(s[3]) * S[3];
  for (int c = 0; c < 3; ++c) g[4 + c] = sign_of(s[4 + c]) * S[c];
}

// loss = mean((rgb - target)^2) over the 3 n values: the pixel's upstream r = 2 (rgb - target) / (3 n); -> its squared error, unscaled
RB_LF_FN double mse_upstream(const double* rgb, const float* target, double inv_3n, double* r) {
  double sq = 0.0;
  for (int c = 0; c < 3; ++c) {
    const double diff = rgb[c] - (double)target[c];
    sq += diff * diff;
    r[c] = 2.0 * diff * inv_3n;
  }
  return sq;
}

// One element of torch.optim.Adam's step (no weight decay, no amsgrad): bc1 = 1 - beta1^t, bc2 = 1 - beta2^t with t the step number.  The
// moments are formed in fp64 and rounded once; the parameter moves by what the STORED moments say, as the optimiser's own tensors would.
RB_LF_FN void adam_element(float& p, float& m, float& v, double g, double lr, double beta1, double beta2, double eps, double bc1, double bc2) {
  m = (float)(beta1 * (double)m + (1.0 - beta1) * g);
  v = (float)(beta2 * (double)v + (1.0 - beta2) * g * g);
  const double denom = sqrt((double)v) / sqrt(bc2) + eps;
  p = (float)((double)p - (lr / bc1) * ((double)m / denom));
}

}  // namespace lf
}  // namespace rb
