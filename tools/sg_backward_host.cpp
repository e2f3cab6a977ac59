// Host build of the SG shading backward's per-pair derivative (robir_amd/csrc/sg_shade_bwd_math.h with RB_SG_FN = inline): the loops and sums
// of k_sg_shade_bwd as plain sequential C++, so that the hand derivation can be checked against float64 autograd without a GPU.
// Driven by tools/check_sg_backward_host.py, which compiles this file with the host compiler (-ffp-contract=off).
// -DSGB_NO_ZERO_REEVAL: a stored output of 0 never passes a gradient (the variant DESIGN 4.1 measures the zero re-evaluation against).
#define RB_SG_FN inline
#include <cmath>
using std::sqrt; using std::exp; using std::fabs; using std::fmax; using std::exp2;
#include "sg_shade_bwd_math.h"
using namespace rb; using namespace rb::sgb;
extern "C" int sgb_cpu(const float* normal, const float* view, const float* lgt, int per_point, int M, float f0, const float* rough,
  const float* albedo, const float* metallic, const float* light_vis, const float* bvis, const float* indir, int lin_diff, long n,
  const float* out_spec, const float* out_diff, const float* g_spec, const float* g_diff,
  double* d_rough, double* d_alb, double* d_met, double* d_bvis, double* d_lv, double* d_indir, double* d_lgt, double* d_f0) {
  *d_f0 = 0;
  for (long p = 0; p < n; ++p) {
    V3 nf = v3(normal[3*p], normal[3*p+1], normal[3*p+2]), vf = v3(view[3*p], view[3*p+1], view[3*p+2]);
    const float* alb = albedo + 3*p;
    bool hm = metallic != nullptr; float met = hm ? metallic[p] : 0.f;
    SpecLobe sl = spec_lobe(nf, vf, rough[p], f0, alb, hm ? metallic + p : nullptr);
    PointB B = point_fwd(nf, vf, rough[p], f0, alb, hm, met);
    PointIn I; I.nf = nf; I.wlf = sl.w_lobe; I.wlamf = sl.w_lam; I.bv = bvis[p];
    I.any_s = I.any_d = false;
    for (int c = 0; c < 3; ++c) {
      I.sc[c] = lin_diff ? 1.0 : (double)alb[c] / SGB_PI;
      I.gs[c] = out_spec[3*p+c] > 0.f ? g_spec[3*p+c] : 0.0;
      I.gd[c] = (!indir && out_diff[3*p+c] > 0.f) ? g_diff[3*p+c] : 0.0;
      I.any_s |= I.gs[c] != 0.0; I.any_d |= I.gd[c] != 0.0;
    }
#ifndef SGB_NO_ZERO_REEVAL
    for (int pass = 0; pass < 2; ++pass) {   // stored 0: clamped negative sum, or an exact zero (gradient passes like torch.clamp)?
      bool need = false;
      for (int c = 0; c < 3; ++c) need |= (pass == 0 ? out_spec[3*p+c] : out_diff[3*p+c]) == 0.f && !(pass == 1 && indir);
      if (!need) continue;
      float acc[3] = {0,0,0};
      for (int k = 0; k < M; ++k) {
        const float* s = lgt + (per_point ? p * (long)M * 7 : 0) + k * 7;
        V3 ll = v3(s[0], s[1], s[2]); float ln = norm3(ll) + RB_TINY; ll = v3(ll.x/ln, ll.y/ln, ll.z/ln);
        float l_lam = fabsf(s[3]); float lv = light_vis ? light_vis[p*M+k] : 1.f;
        V3 fl, pl, ql; float flam, ffac, plam, pfac, qlam, qfac;
        sg_product(ll, l_lam, sl.w_lobe, sl.w_lam, fl, flam, ffac); sg_product(nf, LAMBDA_COS, fl, flam, pl, plam, pfac);
        float h_p = hemi_int(plam, dot3(pl, nf)), h_f = hemi_int(flam, dot3(fl, nf));
        sg_product(nf, LAMBDA_COS, ll, l_lam, ql, qlam, qfac);
        float h_q = hemi_int(qlam, dot3(ql, nf)), h_l = hemi_int(l_lam, dot3(ll, nf));
        for (int c = 0; c < 3; ++c) {
          float m0 = fabsf(s[4+c]);
          if (pass == 0) { float f_mu = (m0 * bvis[p]) * sl.w_mu[c] * ffac; float p_mu = MU_COS * f_mu * pfac; acc[c] += p_mu * h_p - f_mu * ALPHA_COS * h_f; }
          else { float dmu = light_vis ? m0 * lv : m0; if (!lin_diff) dmu = dmu * (alb[c] / RB_PI_F); float q_mu = MU_COS * dmu * qfac; acc[c] += q_mu * h_q - dmu * ALPHA_COS * h_l; }
        }
      }
      for (int c = 0; c < 3; ++c) {
        if (pass == 0 && out_spec[3*p+c] == 0.f && acc[c] >= 0.f) { I.gs[c] = g_spec[3*p+c]; I.any_s |= I.gs[c] != 0.0; }
        if (pass == 1 && !indir && out_diff[3*p+c] == 0.f && acc[c] >= 0.f) { I.gd[c] = g_diff[3*p+c]; I.any_d |= I.gd[c] != 0.0; }
      }
    }
#endif
    double wlam = 0, wmu[3] = {0,0,0}, gbv = 0, gsc[3] = {0,0,0};
    for (int k = 0; k < M; ++k) {
      const float* s = lgt + (per_point ? p * (long)M * 7 : 0) + k * 7;
      LobeGrad O = lobe_bwd(B, I, s, light_vis != nullptr, light_vis ? light_vis[p*M+k] : 1.f);
      for (int i = 0; i < 7; ++i) { if (per_point) d_lgt[(p*M+k)*7+i] = O.dl[i]; else d_lgt[k*7+i] += O.dl[i]; }
      wlam += O.wlam; gbv += O.bv; for (int c = 0; c < 3; ++c) { wmu[c] += O.wmu[c]; gsc[c] += O.sc[c]; }
      if (light_vis) d_lv[p*M+k] = O.lv;
    }
    PointGrad G = point_bwd(B, f0, alb, hm, met, wlam, wmu);
    d_rough[p] = G.rough; *d_f0 += G.f0; d_bvis[p] = gbv; if (hm) d_met[p] = G.met;
    for (int c = 0; c < 3; ++c) {
      double a = G.alb[c];
      if (!lin_diff) a += gsc[c] / SGB_PI;
      if (indir) { d_indir[3*p+c] = g_diff[3*p+c] * I.sc[c]; if (!lin_diff) a += g_diff[3*p+c] * (double)indir[3*p+c] / SGB_PI; }
      d_alb[3*p+c] = a;
    }
  }
  return 0;
}
