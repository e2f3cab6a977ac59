// Reverse mode of k_sg_shade (sg_shade.hip): gradients of <g_spec, spec> + <g_diff, diff> with respect to the light SGs, the
// scalar Fresnel F0, roughness, albedo, metallic, both visibilities and the indirect integral.  Same work shape as the forward:
// one wavefront per surface point, lanes over light lobes, everything recomputed from the inputs (the forward saves nothing but
// its outputs).  The per-pair derivative is sg_shade_bwd_math.h: fp64, branch decisions from the fp32 forward.
//
// Launch geometry (rb_sg_shade_bwd_groups): a persistent grid of G = min(ceil(n / 4), 512) workgroups of four waves; wave w of
// workgroup b takes the points 4 b + w, 4 b + w + 4 G, ...
//
// Cross-point sums (the shared light's [M,7] gradient and d_f0) use no atomics, so that they are bit-reproducible: every lane
// keeps the fp64 partial rows of the two lobes it owns (lobe tile of 128 = blockIdx.y; M <= 128 is one tile, further tiles are
// further workgroups that evaluate only their own lobes) in registers across its points, the four waves of a workgroup are
// added through LDS in wave order, each workgroup stores one slab [M*7 + 1] of doubles into the caller's scratch with plain
// vector stores, and k_sg_bwd_slab_sum adds the G slabs in index order and rounds to fp32 once.
#include "../../include/robir_hip.h"
#include "common.h"
#include "sg_shade_bwd_math.h"
#include <stdint.h>

namespace rb {

#define SGB_WAVES 4
#define SGB_MAX_GROUPS 512
#define SGB_TILE 128            // lobes whose shared-light partials one workgroup keeps: two per lane

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct SgBwdArgs {
  const float *normal, *view, *lgt, *f0, *rough, *albedo, *metallic, *light_vis, *bvis, *indir_integral;
  const float *out_spec, *out_diff, *g_spec, *g_diff;
  float *d_rough, *d_albedo, *d_metallic, *d_bvis, *d_light_vis, *d_indir_integral, *d_lgt;
  double* slab;                 // [G][stride] or null (neither the shared light's gradient nor d_f0 wanted)
  long n, stride;
  int per_point_lgt, M, lin_diff, want_spec;
};

// The forward's lobe sums BEFORE the clamp at zero, evaluated exactly as k_sg_shade does (same helpers, same lane assignment,
// same wave_sum): a stored output of 0 is either a negative sum that was clamped (no gradient) or an exact zero -- zero
// visibility, zero amplitudes -- through which torch.clamp(min=0) passes the gradient.  Only points with a stored zero come here.
__device__ __noinline__ void forward_sums(const SgBwdArgs& A, long p, int lane, V3 nn, const SpecLobe& sl, const float* alb, float bv,
                                          float* spec, float* diff) {
  const float* L = A.lgt + (A.per_point_lgt ? p * (long)A.M * 7 : 0L);
  spec[0] = spec[1] = spec[2] = diff[0] = diff[1] = diff[2] = 0.f;
  for (int k = lane; k < A.M; k += 64) {
    const float* s = L + k * 7;
    V3 ll = v3(s[0], s[1], s[2]);
    const float ln = norm3(ll) + RB_TINY;
    ll = v3(ll.x / ln, ll.y / ln, ll.z / ln);
    const float l_lam = fabsf(s[3]);
    const float lv = A.light_vis ? A.light_vis[p * A.M + k] : 1.f;
    V3 f_lobe, p_lobe, q_lobe;
    float f_lam, f_fac, p_lam, p_fac, q_lam, q_fac;
    sg_product(ll, l_lam, sl.w_lobe, sl.w_lam, f_lobe, f_lam, f_fac);
    sg_product(nn, LAMBDA_COS, f_lobe, f_lam, p_lobe, p_lam, p_fac);
    const float h_p = hemi_int(p_lam, dot3(p_lobe, nn));
    const float h_f = hemi_int(f_lam, dot3(f_lobe, nn));
    sg_product(nn, LAMBDA_COS, ll, l_lam, q_lobe, q_lam, q_fac);
    const float h_q = hemi_int(q_lam, dot3(q_lobe, nn));
    const float h_l = hemi_int(l_lam, dot3(ll, nn));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float mu0 = fabsf(s[4 + c]);
      const float f_mu = (mu0 * bv) * sl.w_mu[c] * f_fac;
      const float p_mu = MU_COS * f_mu * p_fac;
      spec[c] += p_mu * h_p - f_mu * ALPHA_COS * h_f;
      float dmu = A.light_vis ? mu0 * lv : mu0;
      if (!A.lin_diff) dmu = dmu * (alb[c] / RB_PI_F);
      const float q_mu = MU_COS * dmu * q_fac;
      diff[c] += q_mu * h_q - dmu * ALPHA_COS * h_l;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    spec[c] = wave_sum(spec[c]);
    diff[c] = wave_sum(diff[c]);
  }
}

template <bool SHARED>
__global__ __launch_bounds__(256) void k_sg_shade_bwd(const SgBwdArgs A) {
  using namespace sgb;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int tile = blockIdx.y;
  const bool point_out = tile == 0;          // the per-point gradients and d_f0 come from the workgroups of the first lobe tile
  const int M = A.M;
  T acc[2][7];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 7; ++i) acc[j][i] = 0.0;
  T f0_acc = 0.0;
  const float f0 = A.f0[0];
  for (long p = blockIdx.x * (long)SGB_WAVES + w; p < A.n; p += (long)gridDim.x * SGB_WAVES) {
    const V3 nn = v3(A.normal[3 * p], A.normal[3 * p + 1], A.normal[3 * p + 2]);
    const V3 vv = v3(A.view[3 * p], A.view[3 * p + 1], A.view[3 * p + 2]);
    const float alb[3] = {A.albedo[3 * p], A.albedo[3 * p + 1], A.albedo[3 * p + 2]};
    const bool has_met = A.metallic != nullptr;
    const float met = has_met ? A.metallic[p] : 0.f;
    const float rough = A.rough[p], bv = A.bvis[p];
    const SpecLobe sl = spec_lobe(nn, vv, rough, f0, alb, has_met ? A.metallic + p : nullptr);
    // upstream gradients behind the forward's clamps
    float os[3], od[3], gsf[3], gdf[3];
    bool zero = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      os[c] = A.out_spec[3 * p + c];
      od[c] = A.out_diff[3 * p + c];
      gsf[c] = A.g_spec[3 * p + c];
      gdf[c] = A.g_diff[3 * p + c];
      zero |= os[c] == 0.f || (!A.indir_integral && od[c] == 0.f);
    }
    bool pass_s[3], pass_d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      pass_s[c] = os[c] > 0.f;
      pass_d[c] = od[c] > 0.f;
    }
    if (zero) {                              // wave-uniform
      float fs[3], fd[3];
      forward_sums(A, p, lane, nn, sl, alb, bv, fs, fd);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        pass_s[c] = fs[c] >= 0.f;
        pass_d[c] = fd[c] >= 0.f;
      }
    }
    PointIn I;
    I.nf = nn;
    I.wlf = sl.w_lobe;
    I.wlamf = sl.w_lam;
    I.bv = (T)bv;
    I.any_s = I.any_d = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      I.sc[c] = A.lin_diff ? 1.0 : (T)alb[c] / SGB_PI;
      I.gs[c] = pass_s[c] ? (T)gsf[c] : 0.0;
      I.gd[c] = (!A.indir_integral && pass_d[c]) ? (T)gdf[c] : 0.0;
      I.any_s |= I.gs[c] != 0.0;
      I.any_d |= I.gd[c] != 0.0;
    }
    I.any_s = I.any_s && A.want_spec;
    const PointB B = point_fwd(nn, vv, rough, f0, alb, has_met, met);
    const float* L = A.lgt + (A.per_point_lgt ? p * (long)M * 7 : 0L);
    T s_wlam = 0.0, s_bv = 0.0, s_wmu[3] = {0.0, 0.0, 0.0}, s_sc[3] = {0.0, 0.0, 0.0};
    for (int j0 = 0; j0 * 64 < M; j0 += 2) {
      const bool mine = SHARED && j0 == 2 * tile;
      if (!mine && !point_out) continue;
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int k = (j0 + jj) * 64 + lane;
        if (k >= M) continue;
        const LobeGrad O = lobe_bwd(B, I, L + k * 7, A.light_vis != nullptr, A.light_vis ? A.light_vis[p * M + k] : 1.f);
        if (SHARED) {
          if (mine) {
#pragma unroll
            for (int i = 0; i < 7; ++i) acc[jj][i] += O.dl[i];
          }
        } else if (A.d_lgt) {
          float* o = A.d_lgt + (p * (long)M + k) * 7;
#pragma unroll
          for (int i = 0; i < 7; ++i) o[i] = (float)O.dl[i];
        }
        if (point_out) {
          s_wlam += O.wlam;
          s_bv += O.bv;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            s_wmu[c] += O.wmu[c];
            s_sc[c] += O.sc[c];
          }
          if (A.d_light_vis) A.d_light_vis[p * M + k] = (float)O.lv;
        }
      }
    }
    if (point_out) {
      s_wlam = wave_sum_d(s_wlam);
      s_bv = wave_sum_d(s_bv);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        s_wmu[c] = wave_sum_d(s_wmu[c]);
        s_sc[c] = wave_sum_d(s_sc[c]);
      }
      const PointGrad G = point_bwd(B, f0, alb, has_met, met, s_wlam, s_wmu);
      f0_acc += G.f0;
      if (lane == 0) {
        if (A.d_rough) A.d_rough[p] = (float)G.rough;
        if (A.d_bvis) A.d_bvis[p] = (float)s_bv;
        if (A.d_metallic) A.d_metallic[p] = (float)G.met;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          T a = G.alb[c];
          if (!A.lin_diff) a += s_sc[c] / SGB_PI;
          if (A.indir_integral) {
            if (!A.lin_diff) a += (T)gdf[c] * (T)A.indir_integral[3 * p + c] / SGB_PI;
            if (A.d_indir_integral) A.d_indir_integral[3 * p + c] = (float)((T)gdf[c] * I.sc[c]);
          }
          if (A.d_albedo) A.d_albedo[3 * p + c] = (float)a;
        }
      }
    }
  }
  if (!A.slab) return;                       // kernel-uniform
  // ---- the four waves of the workgroup, in wave order, then one slab per workgroup
  __shared__ double lds[SGB_WAVES][SGB_TILE * 7];
  __shared__ double lds_f0[SGB_WAVES];
  if (SHARED) {
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
      for (int i = 0; i < 7; ++i) lds[w][(jj * 64 + lane) * 7 + i] = acc[jj][i];
  }
  if (lane == 0) lds_f0[w] = f0_acc;
  __syncthreads();
  double* slab = A.slab + blockIdx.x * A.stride;
  if (SHARED) {
    for (int e = threadIdx.x; e < SGB_TILE * 7; e += 256) {
      const long g = (long)tile * SGB_TILE * 7 + e;
      if (g < (long)M * 7) slab[g] = ((lds[0][e] + lds[1][e]) + lds[2][e]) + lds[3][e];
    }
  }
  if (point_out && threadIdx.x == 0) slab[A.stride - 1] = ((lds_f0[0] + lds_f0[1]) + lds_f0[2]) + lds_f0[3];
}

// d_lgt[e] / d_f0 = the G slabs added in index order in fp64, rounded once
__global__ void k_sg_bwd_slab_sum(const double* __restrict__ slab, int G, long stride, float* __restrict__ d_lgt,
                                  float* __restrict__ d_f0) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e >= stride) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += slab[g * stride + e];
  if (e < stride - 1) {
    if (d_lgt) d_lgt[e] = (float)s;
  } else if (d_f0) {
    d_f0[0] = (float)s;
  }
}

}  // namespace rb

using namespace rb;

extern "C" {

int rb_sg_shade_bwd_groups(long n) {
  if (n <= 0) return 0;
  const long g = (n + SGB_WAVES - 1) / SGB_WAVES;
  return (int)(g < SGB_MAX_GROUPS ? g : SGB_MAX_GROUPS);
}

long rb_sg_shade_bwd_scratch_floats(int M) {
  if (M < 1) return 0;
  return 2L * SGB_MAX_GROUPS * ((long)M * 7 + 1);
}

int rb_sg_shade_bwd(const float* normal, const float* view, const float* lgt, int per_point_lgt, int M, const float* f0,
                    const float* rough, const float* albedo, const float* metallic, const float* light_vis, const float* bvis,
                    const float* indir_integral, int lin_diff, long n, const float* out_spec, const float* out_diff,
                    const float* g_spec, const float* g_diff, float* d_rough, float* d_albedo, float* d_metallic, float* d_bvis,
                    float* d_light_vis, float* d_indir_integral, float* d_lgt, float* d_f0, float* scratch, long scratch_floats,
                    rb_stream_t stream) {
  if (n <= 0) return 0;
  RB_REQUIRE(normal && view && lgt && f0 && rough && albedo && bvis && out_spec && out_diff && g_spec && g_diff, "null pointer");
  RB_REQUIRE(M >= 1, "need at least one lobe");
  RB_REQUIRE(!d_metallic || metallic, "d_metallic without metallic");
  RB_REQUIRE(!d_light_vis || light_vis, "d_light_vis without light_vis");
  RB_REQUIRE(!d_indir_integral || indir_integral, "d_indir_integral without indir_integral");
  const bool shared = !per_point_lgt && d_lgt;
  const bool slabs = shared || d_f0;
  if (slabs) {
    RB_REQUIRE(scratch, "null pointer (scratch: the shared light's gradient and d_f0 are summed through it)");
    RB_REQUIRE(scratch_floats >= rb_sg_shade_bwd_scratch_floats(M), "scratch smaller than rb_sg_shade_bwd_scratch_floats(M)");
    RB_REQUIRE(((uintptr_t)scratch & 7) == 0, "scratch must be 8-byte aligned");
  }
  SgBwdArgs A;
  A.normal = normal, A.view = view, A.lgt = lgt, A.f0 = f0, A.rough = rough, A.albedo = albedo, A.metallic = metallic;
  A.light_vis = light_vis, A.bvis = bvis, A.indir_integral = indir_integral, A.out_spec = out_spec, A.out_diff = out_diff;
  A.g_spec = g_spec, A.g_diff = g_diff, A.d_rough = d_rough, A.d_albedo = d_albedo, A.d_metallic = d_metallic, A.d_bvis = d_bvis;
  A.d_light_vis = d_light_vis, A.d_indir_integral = d_indir_integral, A.d_lgt = d_lgt;
  A.slab = slabs ? (double*)scratch : nullptr;
  A.n = n, A.stride = (shared ? (long)M * 7 : 0L) + 1;
  A.per_point_lgt = per_point_lgt ? 1 : 0, A.M = M, A.lin_diff = lin_diff ? 1 : 0;
  // the specular chain feeds every gradient but the light visibility's, the indirect integral's and (without metallic) albedo's
  A.want_spec = (d_rough || d_bvis || d_lgt || d_f0 || d_metallic || (d_albedo && metallic)) ? 1 : 0;
  const int G = rb_sg_shade_bwd_groups(n);
  hipStream_t s = (hipStream_t)stream;
  if (shared)
    hipLaunchKernelGGL(k_sg_shade_bwd<true>, dim3(G, (M + SGB_TILE - 1) / SGB_TILE), dim3(256), 0, s, A);
  else
    hipLaunchKernelGGL(k_sg_shade_bwd<false>, dim3(G, 1), dim3(256), 0, s, A);
  int rc = check_launch("k_sg_shade_bwd");
  if (rc != 0 || !slabs) return rc;
  hipLaunchKernelGGL(k_sg_bwd_slab_sum, grid1d(A.stride, 256), dim3(256), 0, s, (const double*)scratch, G, A.stride,
                     shared ? d_lgt : nullptr, d_f0);
  return check_launch("k_sg_bwd_slab_sum");
}

}  // extern "C"
