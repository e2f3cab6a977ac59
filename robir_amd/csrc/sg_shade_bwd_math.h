// Reverse mode of the SG shading formulas for ONE (point, lobe) pair and for the point-only BRDF lobe, hand-derived from
// sg_common.h (= model/sg_render.py:62-108, 414-536).  No launch geometry and no memory traffic here: k_sg_shade_bwd
// (sg_shade_bwd.hip) loops and reduces around these bodies, and a host compiler can build them as they are (RB_SG_FN).
//
// Arithmetic: the derivative is formed in fp64 from the fp32 inputs and rounded once when it is stored.  The forward's
// cancelling differences (tmp - ratio - 1 times a sharpness of thousands, 1 - ea eb, ...) are worse in the derivative
// than in the value, fp64 removes them without reformulating anything, and the target of the backward is float64 autograd,
// not bit parity with an fp32 graph.  What DECIDES A BRANCH is taken from the fp32 forward evaluation: the side of
// min(tmp, ratio + 1) in each lambda_trick (sg_product_clamped) and the sign of each hemisphere cosine.
#pragma once
#include "sg_common.h"

namespace rb {
namespace sgb {

typedef double T;
#define SGB_EPS 1e-6
#define SGB_PI 3.14159265358979323846
#define SGB_MU 32.7080
#define SGB_LC 0.0315
#define SGB_AL 31.7003

struct D3 {
  T x, y, z;
};
RB_SG_FN D3 d3(T x, T y, T z) { return D3{x, y, z}; }
RB_SG_FN D3 d3(V3 a) { return D3{(T)a.x, (T)a.y, (T)a.z}; }
RB_SG_FN T ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
RB_SG_FN D3 dscale(D3 a, T s) { return d3(a.x * s, a.y * s, a.z * s); }
RB_SG_FN D3 dadd(D3 a, D3 b) { return d3(a.x + b.x, a.y + b.y, a.z + b.z); }
RB_SG_FN D3 daxpy(T s, D3 a, D3 b) { return d3(s * a.x + b.x, s * a.y + b.y, s * a.z + b.z); }
RB_SG_FN D3 dunit(D3 a) { return dscale(a, 1.0 / (sqrt(ddot(a, a)) + SGB_EPS)); }
// y = x / (|x| + eps): gradient of x from the gradient of y (0 through the norm at x = 0, like torch.norm)
RB_SG_FN D3 dunit_bwd(D3 x, D3 g) {
  const T nrm = sqrt(ddot(x, x)), m = nrm + SGB_EPS;
  const T c = nrm > 0.0 ? ddot(g, x) / (nrm * m * m) : 0.0;
  return d3(g.x / m - x.x * c, g.y / m - x.y * c, g.z / m - x.z * c);
}

// ---- hemisphere_int: value and both partial derivatives; `pos` = the forward's cos >= 0 mask
struct Hemi {
  T H, d_lam, d_cb;
};
RB_SG_FN Hemi hemi_grad(T lam, T cb, bool pos) {
  const T L = lam + SGB_EPS, il = 1.0 / L, sq = sqrt(L);
  const T a = 1.6988 + 10.8438 * il, den = 1.0 + 6.2201 * il + 10.2415 * il * il;
  const T t = sq * a / den;
  const T da = -10.8438 * il * il, dden = -6.2201 * il * il - 2.0 * 10.2415 * il * il * il;
  const T dt = ((0.5 / sq * a + sq * da) * den - sq * a * dden) / (den * den);
  const T ea = exp(-t);
  T s, ds_dt, ds_dcb;
  if (pos) {
    const T eb = exp(-t * cb), N = 1.0 - ea * eb, D = 1.0 - ea + eb - ea * eb;
    s = N / D;
    const T ds_dea = (-eb * D + N * (1.0 + eb)) / (D * D), ds_deb = (-ea * D - N * (1.0 - ea)) / (D * D);
    ds_dt = ds_dea * (-ea) + ds_deb * (-cb * eb);
    ds_dcb = ds_deb * (-t * eb);
  } else {
    const T b = exp(t * cb), om = 1.0 - ea, N = b - ea, D = om * (b + 1.0);
    s = N / D;
    const T ds_db = (D - N * om) / (D * D), ds_dea = (-D + N * (b + 1.0)) / (D * D);
    ds_dt = ds_db * cb * b + ds_dea * (-ea);
    ds_dcb = ds_db * t * b;
  }
  const T e1 = exp(-L), e2 = exp(-2.0 * L), tp = 2.0 * SGB_PI * il;
  const T Ab = tp * (e1 - e2), Au = tp * (1.0 - e1);
  const T dAb = -Ab * il + tp * (2.0 * e2 - e1), dAu = -Au * il + tp * e1;
  Hemi h;
  h.H = Ab * (1.0 - s) + Au * s;
  h.d_lam = dAb * (1.0 - s) + dAu * s + (Au - Ab) * ds_dt * dt;
  h.d_cb = (Au - Ab) * ds_dcb;
  return h;
}

// ---- lambda_trick: forward record and reverse
struct Prod {
  D3 e1, e2, lobe3;
  T r, d, t, lam3, fac;
  bool clamped;
};
RB_SG_FN Prod prod_fwd(D3 u1, T lam1, D3 u2, T lam2, bool clamped) {
  Prod P;
  P.clamped = clamped;
  P.r = lam1 / lam2;
  P.e1 = dunit(u1);
  P.e2 = dunit(u2);
  P.d = ddot(P.e1, P.e2);
  P.t = clamped ? P.r + 1.0 : sqrt(P.r * P.r + 1.0 + 2.0 * P.r * P.d);
  P.lam3 = lam2 * P.t;
  P.lobe3 = daxpy(P.r / P.t, P.e1, dscale(P.e2, 1.0 / P.t));
  P.fac = exp(lam2 * (P.t - P.r - 1.0));
  return P;
}
struct ProdGrad {
  D3 u1, u2;
  T lam1, lam2;
};
RB_SG_FN ProdGrad prod_bwd(const Prod& P, D3 u1, D3 u2, T lam2, D3 g_lobe3, T g_lam3, T g_fac) {
  const T gff = g_fac * P.fac;
  const T g_t = (g_lam3 + gff) * lam2 - ddot(g_lobe3, P.lobe3) / P.t;
  T g_r = -gff * lam2 + ddot(g_lobe3, P.e1) / P.t;
  T g_lam2 = g_lam3 * P.t + gff * (P.t - P.r - 1.0);
  D3 g_e1 = dscale(g_lobe3, P.r / P.t), g_e2 = dscale(g_lobe3, 1.0 / P.t);
  if (P.clamped) {
    g_r += g_t;
  } else {
    g_r += g_t * (P.r + P.d) / P.t;
    const T g_d = g_t * P.r / P.t;
    g_e1 = daxpy(g_d, P.e2, g_e1);
    g_e2 = daxpy(g_d, P.e1, g_e2);
  }
  ProdGrad G;
  G.lam1 = g_r / lam2;
  G.lam2 = g_lam2 - g_r * P.r / lam2;
  G.u1 = dunit_bwd(u1, g_e1);
  G.u2 = dunit_bwd(u2, g_e2);
  return G;
}

// ---- point-only part: the warped BRDF lobe in fp64 with what its reverse needs
struct PointB {
  D3 n, wl;
  T w_lam, w_mu[3], Fr[3], rough, r4, b_mu, fw, k, d1, d2, D1, D2, G, den, vd;
};
RB_SG_FN PointB point_fwd(V3 nf, V3 vf, float rough, float f0, const float* alb, bool has_met, float met) {
  PointB B;
  const D3 n = d3(nf), v = d3(vf);
  B.n = n;
  B.rough = (T)rough;
  B.r4 = 2.0 / (B.rough * B.rough * B.rough * B.rough);
  B.b_mu = B.r4 / SGB_PI;
  const T vdl = fmax(ddot(n, v), 0.0);
  D3 wl = d3(2.0 * vdl * n.x - v.x, 2.0 * vdl * n.y - v.y, 2.0 * vdl * n.z - v.z);
  wl = dunit(wl);
  B.wl = wl;
  B.vd = 4.0 * vdl + SGB_EPS;
  B.w_lam = B.r4 / B.vd;
  const D3 h = dunit(dadd(wl, v));
  const T vdh = fmax(ddot(v, h), 0.0);
  B.fw = exp2(-(5.55473 * vdh + 6.8316) * vdh);
  B.d1 = fmax(ddot(wl, n), 0.0);
  B.d2 = fmax(ddot(v, n), 0.0);
  B.k = (B.rough + 1.0) * (B.rough + 1.0) / 8.0;
  B.D1 = B.d1 * (1.0 - B.k) + B.k + SGB_EPS;
  B.D2 = B.d2 * (1.0 - B.k) + B.k + SGB_EPS;
  B.G = (B.d1 / B.D1) * (B.d2 / B.D2);
  B.den = 4.0 * B.d1 * B.d2 + SGB_EPS;
  for (int c = 0; c < 3; ++c) {
    T sc = (T)f0;
    if (has_met) sc = (1.0 - (T)met) * (T)f0 + (T)alb[c] * (T)met;
    B.Fr[c] = sc + (1.0 - sc) * B.fw;
    B.w_mu[c] = B.b_mu * (B.Fr[c] * B.G / B.den);
  }
  return B;
}
struct PointGrad {
  T rough, f0, alb[3], met;
};
// gradients of (w_lam, w_mu[3]) summed over the point's lobes -> roughness, f0, and with metallic: albedo, metallic
RB_SG_FN PointGrad point_bwd(const PointB& B, float f0, const float* alb, bool has_met, float met, T g_wlam, const T* g_wmu) {
  PointGrad P;
  const T Q = B.G / B.den;
  T g_r4 = g_wlam / B.vd, g_G = 0.0;
  P.f0 = 0.0;
  P.met = 0.0;
  for (int c = 0; c < 3; ++c) {
    g_r4 += g_wmu[c] * B.Fr[c] * Q / SGB_PI;
    g_G += g_wmu[c] * B.b_mu * B.Fr[c] / B.den;
    const T g_sc = g_wmu[c] * B.b_mu * Q * (1.0 - B.fw);
    P.alb[c] = 0.0;
    if (has_met) {
      P.f0 += g_sc * (1.0 - (T)met);
      P.alb[c] = g_sc * (T)met;
      P.met += g_sc * ((T)alb[c] - (T)f0);
    } else {
      P.f0 += g_sc;
    }
  }
  const T G1 = B.d1 / B.D1, G2 = B.d2 / B.D2;
  const T g_k = g_G * (-B.d1 * (1.0 - B.d1) / (B.D1 * B.D1) * G2 - G1 * B.d2 * (1.0 - B.d2) / (B.D2 * B.D2));
  P.rough = g_k * (B.rough + 1.0) / 4.0 - g_r4 * 4.0 * B.r4 / B.rough;
  return P;
}

// ---- one (point, lobe) pair
struct PointIn {                 // what a lobe needs of its point
  V3 nf;                         // fp32 normal and warped lobe: the forward's branch decisions
  V3 wlf;
  float wlamf;
  T bv, sc[3];                   // specular visibility; diffuse scale albedo / pi (1 with lin_diff)
  T gs[3], gd[3];                // upstream gradients after the output clamps (gd = 0 when indir_integral replaces the term)
  bool any_s, any_d;
};
struct LobeGrad {
  T dl[7];                       // raw light SG row: axis, sharpness, amplitude
  T wlam, wmu[3], bv, sc[3], lv; // partials of the point's quantities and of this pair's light visibility
};
RB_SG_FN LobeGrad lobe_bwd(const PointB& B, const PointIn& I, const float* s, bool has_lv, float lvf) {
  LobeGrad O;
  for (int i = 0; i < 7; ++i) O.dl[i] = 0.0;
  O.wlam = O.bv = O.lv = 0.0;
  for (int c = 0; c < 3; ++c) O.wmu[c] = O.sc[c] = 0.0;
  // fp32 forward up to the branch decisions
  V3 llf = v3(s[0], s[1], s[2]);
  const float lnf = norm3(llf) + RB_TINY;
  llf = v3(llf.x / lnf, llf.y / lnf, llf.z / lnf);
  const float llamf = fabsf(s[3]);
  // fp64 inputs
  const D3 a = d3((T)s[0], (T)s[1], (T)s[2]);
  const D3 ll = dunit(a);
  const T l_lam = fabs((T)s[3]);
  const T mu0[3] = {fabs((T)s[4]), fabs((T)s[5]), fabs((T)s[6])};
  const T lv = has_lv ? (T)lvf : 1.0;
  const D3 n = B.n;
  D3 g_ll = d3(0.0, 0.0, 0.0);
  T g_llam = 0.0, g_mu0[3] = {0.0, 0.0, 0.0};
  if (I.any_s) {
    V3 flf, plf;
    float flamf, ffacf, plamf, pfacf;
    sg_product(llf, llamf, I.wlf, I.wlamf, flf, flamf, ffacf);
    sg_product(I.nf, LAMBDA_COS, flf, flamf, plf, plamf, pfacf);
    const bool cl_f = sg_product_clamped(llf, llamf, I.wlf, I.wlamf), cl_p = sg_product_clamped(I.nf, LAMBDA_COS, flf, flamf);
    const bool pos_p = dot3(plf, I.nf) >= 0.f, pos_f = dot3(flf, I.nf) >= 0.f;
    const Prod F = prod_fwd(ll, l_lam, B.wl, B.w_lam, cl_f);
    const Prod P = prod_fwd(n, SGB_LC, F.lobe3, F.lam3, cl_p);
    const Hemi hp = hemi_grad(P.lam3, ddot(P.lobe3, n), pos_p), hf = hemi_grad(F.lam3, ddot(F.lobe3, n), pos_f);
    const T K = SGB_MU * P.fac * hp.H - SGB_AL * hf.H;
    T S = 0.0;
    for (int c = 0; c < 3; ++c) {
      const T gA = I.gs[c] * F.fac * K;                  // A_c = mu0_c bvis w_mu_c
      g_mu0[c] += gA * I.bv * B.w_mu[c];
      O.bv += gA * mu0[c] * B.w_mu[c];
      O.wmu[c] = gA * mu0[c] * I.bv;
      S += I.gs[c] * mu0[c] * I.bv * B.w_mu[c];
    }
    const T Sf = S * F.fac;
    const ProdGrad gp = prod_bwd(P, n, F.lobe3, F.lam3, dscale(n, Sf * SGB_MU * P.fac * hp.d_cb), Sf * SGB_MU * P.fac * hp.d_lam,
                                 Sf * SGB_MU * hp.H);
    const D3 g_fl = daxpy(-Sf * SGB_AL * hf.d_cb, n, gp.u2);
    const T g_flam = gp.lam2 - Sf * SGB_AL * hf.d_lam;
    const ProdGrad gf = prod_bwd(F, ll, B.wl, B.w_lam, g_fl, g_flam, S * K);
    g_ll = dadd(g_ll, gf.u1);
    g_llam += gf.lam1;
    O.wlam = gf.lam2;
  }
  if (I.any_d) {
    V3 qlf;
    float qlamf, qfacf;
    sg_product(I.nf, LAMBDA_COS, llf, llamf, qlf, qlamf, qfacf);
    const bool cl_q = sg_product_clamped(I.nf, LAMBDA_COS, llf, llamf);
    const bool pos_q = dot3(qlf, I.nf) >= 0.f, pos_l = dot3(llf, I.nf) >= 0.f;
    const Prod Q = prod_fwd(n, SGB_LC, ll, l_lam, cl_q);
    const Hemi hq = hemi_grad(Q.lam3, ddot(Q.lobe3, n), pos_q), hl = hemi_grad(l_lam, ddot(ll, n), pos_l);
    const T Kd = SGB_MU * Q.fac * hq.H - SGB_AL * hl.H;
    T Sd = 0.0;
    for (int c = 0; c < 3; ++c) {
      const T gdm = I.gd[c] * Kd;                        // dmu_c = mu0_c lv sc_c
      g_mu0[c] += gdm * lv * I.sc[c];
      O.lv += gdm * mu0[c] * I.sc[c];
      O.sc[c] = gdm * mu0[c] * lv;
      Sd += I.gd[c] * mu0[c] * lv * I.sc[c];
    }
    const ProdGrad gq = prod_bwd(Q, n, ll, l_lam, dscale(n, Sd * SGB_MU * Q.fac * hq.d_cb), Sd * SGB_MU * Q.fac * hq.d_lam,
                                 Sd * SGB_MU * hq.H);
    g_ll = dadd(g_ll, daxpy(-Sd * SGB_AL * hl.d_cb, n, gq.u2));
    g_llam += gq.lam2 - Sd * SGB_AL * hl.d_lam;
  }
  const D3 g_a = dunit_bwd(a, g_ll);
  O.dl[0] = g_a.x;
  O.dl[1] = g_a.y;
  O.dl[2] = g_a.z;
  O.dl[3] = s[3] > 0.f ? g_llam : (s[3] < 0.f ? -g_llam : 0.0);
  for (int c = 0; c < 3; ++c) O.dl[4 + c] = s[4 + c] > 0.f ? g_mu0[c] : (s[4 + c] < 0.f ? -g_mu0[c] : 0.0);
  return O;
}

}  // namespace sgb
}  // namespace rb
