// Device helpers of the spherical-Gaussian shading kernels, shared by the forward (sg_shade.hip) and its reverse mode
// (sg_shade_bwd.hip): constants of the clamped-cosine fit, 3-vectors, hemisphere_int / lambda_trick / the warped BRDF lobe
// (model/sg_render.py:62-108, 414-458) in plain fp32.  The forward's rounding is defined by these bodies (compiled with
// -ffp-contract=off): change nothing here without the golden and determinism tests.
// RB_SG_FN may be predefined (e.g. `inline`) to compile the helpers for the host; wave_sum exists on the device only.
#pragma once
#include <math.h>

#ifndef RB_SG_FN
#define RB_SG_FN __device__ __forceinline__
#endif

namespace rb {

#define RB_TINY 1e-6f
#define RB_PI_F ((float)3.14159265358979323846)
#define MU_COS 32.7080f
#define LAMBDA_COS 0.0315f
#define ALPHA_COS 31.7003f

struct V3 {
  float x, y, z;
};
RB_SG_FN V3 v3(float x, float y, float z) { return V3{x, y, z}; }
RB_SG_FN float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
RB_SG_FN float norm3(V3 a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
RB_SG_FN V3 unit_eps3(V3 a) {  // norm_axis (sg_render.py:107-108)
  float n = norm3(a) + RB_TINY;
  return v3(a.x / n, a.y / n, a.z / n);
}
RB_SG_FN V3 cross3(V3 a, V3 b) {
  return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

// hemisphere_int (sg_render.py:62-81); both branches evaluated and blended like the reference
RB_SG_FN float hemi_int(float lam, float cb) {
  lam = lam + RB_TINY;
  const float il = 1.f / lam;
  const float t = sqrtf(lam) * (1.6988f + 10.8438f * il) / (1.f + 6.2201f * il + 10.2415f * il * il);
  const float ea = expf(-t);
  const float mask = cb >= 0.f ? 1.f : 0.f;
  const float eb = expf(-t * fmaxf(cb, 0.f));
  const float s1 = (1.f - ea * eb) / (1.f - ea + eb - ea * eb);
  const float b = expf(t * fminf(cb, 0.f));
  const float s2 = (b - ea) / ((1.f - ea) * (b + 1.f));
  const float s = mask * s1 + (1.f - mask) * s2;
  const float two_pi = 2.f * RB_PI_F;
  const float a_b = two_pi / lam * (expf(-lam) - expf(-2.f * lam));
  const float a_u = two_pi / lam * (1.f - expf(-lam));
  return a_b * (1.f - s) + a_u * s;
}

// lambda_trick (sg_render.py:84-104): SG1 (lam1 << lam2) x SG2; mu handled by the caller (factor returned)
RB_SG_FN void sg_product(V3 lobe1, float lam1, V3 lobe2, float lam2, V3& lobe3, float& lam3, float& mu_factor) {
  const float ratio = lam1 / lam2;
  lobe1 = unit_eps3(lobe1);
  lobe2 = unit_eps3(lobe2);
  const float d = dot3(lobe1, lobe2);
  float tmp = sqrtf(ratio * ratio + 1.f + 2.f * ratio * d);
  tmp = fminf(tmp, ratio + 1.f);
  lam3 = lam2 * tmp;
  const float a = ratio / tmp, b = 1.f / tmp;
  lobe3 = v3(a * lobe1.x + b * lobe2.x, a * lobe1.y + b * lobe2.y, a * lobe1.z + b * lobe2.z);
  mu_factor = expf(lam2 * (tmp - ratio - 1.f));
}

// Which side of sg_product's `min(tmp, ratio + 1)` the fp32 evaluation above takes: true = the bound ratio + 1 (the
// square root rounded above it); a tie counts as the square root.  Same operations in the same order as sg_product.
RB_SG_FN bool sg_product_clamped(V3 lobe1, float lam1, V3 lobe2, float lam2) {
  const float ratio = lam1 / lam2;
  lobe1 = unit_eps3(lobe1);
  lobe2 = unit_eps3(lobe2);
  const float d = dot3(lobe1, lobe2);
  return sqrtf(ratio * ratio + 1.f + 2.f * ratio * d) > ratio + 1.f;
}

#ifdef __HIPCC__
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
#endif

// Point-only part of the specular BRDF SG (sg_render.py:414-458): warped lobe/lambda and the 3-channel amplitude.
struct SpecLobe {
  V3 w_lobe;
  float w_lam;
  float w_mu[3];
};
RB_SG_FN SpecLobe spec_lobe(V3 n, V3 v, float rough, float f0, const float* albedo, const float* metallic) {
  SpecLobe s;
  const float r4 = 2.f / (rough * rough * rough * rough);
  const float b_mu = r4 / RB_PI_F;
  const float vdl = fmaxf(dot3(n, v), 0.f);
  V3 wl = v3(2.f * vdl * n.x - v.x, 2.f * vdl * n.y - v.y, 2.f * vdl * n.z - v.z);
  const float wn = norm3(wl) + RB_TINY;
  wl = v3(wl.x / wn, wl.y / wn, wl.z / wn);
  s.w_lobe = wl;
  s.w_lam = r4 / (4.f * vdl + RB_TINY);
  V3 h = v3(wl.x + v.x, wl.y + v.y, wl.z + v.z);
  const float hn = norm3(h) + RB_TINY;
  h = v3(h.x / hn, h.y / hn, h.z / hn);
  const float vdh = fmaxf(dot3(v, h), 0.f);
  const float fw = exp2f(-(5.55473f * vdh + 6.8316f) * vdh);
  const float d1 = fmaxf(dot3(wl, n), 0.f);
  const float d2 = fmaxf(dot3(v, n), 0.f);
  const float k = (rough + 1.f) * (rough + 1.f) / 8.f;
  const float G = (d1 / (d1 * (1.f - k) + k + RB_TINY)) * (d2 / (d2 * (1.f - k) + k + RB_TINY));
  const float den = 4.f * d1 * d2 + RB_TINY;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float sc = f0;
    if (metallic) sc = (1.f - metallic[0]) * f0 + albedo[c] * metallic[0];
    const float Fr = sc + (1.f - sc) * fw;
    s.w_mu[c] = b_mu * (Fr * G / den);
  }
  return s;
}

}  // namespace rb
