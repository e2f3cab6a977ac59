// The tone curves of ACESToneMapping (model/color_correction.py:31-73,116-137), the fallback x / (x + 1) of InvLoss.forward
// (model/loss.py:108) and their two partial derivatives for ONE element.  No launch geometry and no memory traffic: the kernels of
// photoloss.hip index and reduce around these bodies, and a host compiler builds them as they are (tools/photoloss_host.cpp) -- the
// lightfit_math.h pattern.
//
// With tc = clamp(t, 1e-4, 1), A = aces, I = aces^-1 and c(t) = I(0.73 t):
//   curve 0 (scale_aces)  hdr2ldr  y = A(x) / tc^0.2                 ldr2hdr  y = I(x tc^0.2)
//   curve 1 (warp_aces)   hdr2ldr  y = A(c x / 0.73) / tc            ldr2hdr  y = 0.73 I(x tc) / c
//   curve 2 (ln_space)    hdr2ldr  u = x (0.5 + tc) / 0.5, y = u / (1 + tc u)      ldr2hdr  u = x / (1 - tc x), y = 0.5 u / (0.5 + tc)
//   curve 3 (identity)    y = x        curve 4 (rational, the loss's fallback; no inverse)  y = x / (x + 1)
//
// Arithmetic: value_f32 is fp32 with the expression order of k_tonemap (csrc/misc.hip) -- the same bits; value_d1 forms the
// value and both partial derivatives in fp64 from the fp32 inputs, with the reference's constants as doubles; what is stored is rounded to
// fp32 once, by the caller.  d y / d t carries torch's clamp rule: the gradient passes on the closed interval [1e-4, 1] and is zero outside.
#pragma once
#include <math.h>

#ifndef RB_PL_FN
#ifdef __HIPCC__
#define RB_PL_FN __host__ __device__ __forceinline__
#else
#define RB_PL_FN inline
#endif
#endif

namespace rb {
namespace pl {

constexpr int CURVE_SCALE_ACES = 0, CURVE_WARP_ACES = 1, CURVE_LN_SPACE = 2, CURVE_IDENTITY = 3, CURVE_RATIONAL = 4;
constexpr int MAX_GROUPS = 1024;      // block partials of a scalar reduction (photoloss.hip: groups_of)

RB_PL_FN bool curve_known(int curve) { return curve >= 0 && curve <= CURVE_RATIONAL; }
RB_PL_FN bool curve_reads_shift(int curve) { return curve >= 0 && curve <= CURVE_LN_SPACE; }

// ---------------------------------------------------------------------------------------------------------------- fp32 forward
RB_PL_FN float aces_f32(float x) { return x * (2.51f * x + 0.03f) / (x * (2.43f * x + 0.59f) + 0.14f); }
RB_PL_FN float aces_inv_f32(float x) {
  const float q = 0.59f * x - 0.03f;
  return (q + sqrtf(q * q + 4.f * (2.51f - 2.43f * x) * 0.14f * x)) / (2.f * (2.51f - 2.43f * x));
}

// k_tonemap's body for op 0 (inverse = false) and op 1 (inverse = true); curve 4 has no counterpart there
RB_PL_FN float value_f32(float v, float t, int curve, bool inverse) {
  t = fminf(fmaxf(t, 1e-4f), 1.f);
  float r;
  if (curve == CURVE_SCALE_ACES) {
    const float tp = powf(t, 0.2f);
    r = inverse ? aces_inv_f32(v * tp) : aces_f32(v) / tp;
  } else if (curve == CURVE_WARP_ACES) {
    r = inverse ? 0.73f * aces_inv_f32(v * t) / aces_inv_f32(0.73f * t) : aces_f32(aces_inv_f32(0.73f * t) / 0.73f * v) / t;
  } else if (curve == CURVE_LN_SPACE) {
    if (inverse) {
      const float u = v / (1.f - t * v);
      r = u * 0.5f / (0.5f + t);
    } else {
      const float u = v * (0.5f + t) / 0.5f;
      r = u / (1.f + t * u);
    }
  } else if (curve == CURVE_RATIONAL) {
    r = v / (v + 1.f);
  } else {
    r = v;
  }
  return r;
}

// ---------------------------------------------------------------------------------------------------------------- fp64 value + derivatives
struct D1 {
  double y, dx, dt;      // value, d y / d x, d y / d t (of the UNCLAMPED t)
};

// A(x) = N / D and A'(x) = (N' D - N D') / D^2
RB_PL_FN void aces_d1(double x, double& a, double& da) {
  const double N = x * (2.51 * x + 0.03), D = x * (2.43 * x + 0.59) + 0.14;
  a = N / D;
  da = ((5.02 * x + 0.03) * D - N * (4.86 * x + 0.59)) / (D * D);
}

// I(x) = (q + s) / (2 B), q = 0.59 x - 0.03, B = 2.51 - 2.43 x, s = sqrt(R), R = q^2 + 0.56 B x;
// I'(x) = (0.59 + R' / (2 s)) / (2 B) + 2.43 I / B,  R' = 1.18 q + 0.56 (2.51 - 4.86 x).     R(0) = 9e-4: s > 0 on the domain x < 2.51 / 2.43
RB_PL_FN void aces_inv_d1(double x, double& f, double& df) {
  const double q = 0.59 * x - 0.03, B = 2.51 - 2.43 * x;
  const double s = sqrt(q * q + 4.0 * B * 0.14 * x);
  f = (q + s) / (2.0 * B);
  const double dR = 1.18 * q + 0.56 * (2.51 - 4.86 * x);
  df = (0.59 + dR / (2.0 * s)) / (2.0 * B) + 2.43 * f / B;
}

RB_PL_FN D1 value_d1(double x, float tf, int curve, bool inverse) {
  const double traw = (double)tf;
  const double t = fmin(fmax(traw, 1e-4), 1.0);
  const double pass = (traw >= 1e-4 && traw <= 1.0) ? 1.0 : 0.0;
  D1 r;
  if (curve == CURVE_SCALE_ACES) {
    const double tp = pow(t, 0.2);
    if (inverse) {
      double f, df;
      aces_inv_d1(x * tp, f, df);
      r.y = f;
      r.dx = df * tp;
      r.dt = df * x * 0.2 * tp / t;
    } else {
      double a, da;
      aces_d1(x, a, da);
      r.y = a / tp;
      r.dx = da / tp;
      r.dt = -0.2 * r.y / t;
    }
  } else if (curve == CURVE_WARP_ACES) {
    double c, dc;
    aces_inv_d1(0.73 * t, c, dc);
    dc *= 0.73;
    if (inverse) {
      double f, df;
      aces_inv_d1(x * t, f, df);
      r.y = 0.73 * f / c;
      r.dx = 0.73 * df * t / c;
      r.dt = 0.73 * (df * x * c - f * dc) / (c * c);
    } else {
      double a, da;
      aces_d1(c / 0.73 * x, a, da);
      r.y = a / t;
      r.dx = da * (c / 0.73) / t;
      r.dt = (da * x * dc / 0.73 * t - a) / (t * t);
    }
  } else if (curve == CURVE_LN_SPACE) {
    if (inverse) {
      const double w = 1.0 - t * x, u = x / w, k = 0.5 / (0.5 + t);
      r.y = u * k;
      r.dx = k / (w * w);
      r.dt = u * u * k - u * 0.5 / ((0.5 + t) * (0.5 + t));
    } else {
      const double u = x * (0.5 + t) / 0.5, w = 1.0 + t * u;
      r.y = u / w;
      r.dx = (0.5 + t) / 0.5 / (w * w);
      r.dt = (x / 0.5 - u * u) / (w * w);
    }
  } else if (curve == CURVE_RATIONAL) {
    r.y = x / (x + 1.0);
    r.dx = 1.0 / ((x + 1.0) * (x + 1.0));
    r.dt = 0.0;
  } else {
    r.y = x;
    r.dx = 1.0;
    r.dt = 0.0;
  }
  r.dt *= pass;
  return r;
}

// ---------------------------------------------------------------------------------------------------------------- one row of the loss
// dist(p, g) and d dist / d p: L1 (|p - g|, sign with sign(0) = 0) or L2 ((p - g)^2, 2 (p - g))
RB_PL_FN void dist_d1(double p, double g, bool l2, double& d, double& dd) {
  const double e = p - g;
  if (l2) {
    d = e * e;
    dd = 2.0 * e;
  } else {
    d = fabs(e);
    dd = e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0);
  }
}

// One masked row: pred = curve(sg + indir) (hdr2ldr), the row's share of sum_c dist and, unscaled by 1 / N, d / d x [3] and d / d t.
// sg, indir (may be null), gt: the row's three values.
RB_PL_FN double loss_row(const float* sg, const float* indir, const float* gt, float t, int curve, bool l2, double* gx, double& gt_sum) {
  double acc = 0.0;
  gt_sum = 0.0;
  for (int c = 0; c < 3; ++c) {
    const double x = indir ? (double)sg[c] + (double)indir[c] : (double)sg[c];
    const D1 v = value_d1(x, t, curve, false);
    double d, dd;
    dist_d1(v.y, (double)gt[c], l2, d, dd);
    acc += d;
    gx[c] = dd * v.dx;
    gt_sum += dd * v.dt;
  }
  return acc;
}

}  // namespace pl
}  // namespace rb
