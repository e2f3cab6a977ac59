// Light-SG ("diffuse") visibility: get_diffuse_visibility, model/sg_render.py:111-195 -- 90 % of the reference's
// PBR forward time.  Per surface point: L*nsamp (128*32 = 4096) cone-sampled directions shared by all points of a
// chunk, cull n.d <= 1e-6, visibility MLP on the survivors, softmax[...,1], SG-weighted mean per lobe.
//
// MI355X design: the [n,4096,*] tensors of the reference are never materialised.
//   * the first MLP layer is split:  relu(W0p.PE(p) + b0  +  W0d.PE(d))  -> a per-point row A[n,256] and a
//     per-direction table B[C*4096,256] (both produced by rb_linear_64_256), so layer 0 costs two loads + add;
//   * one workgroup per point: cull + wave-ballot compaction of the surviving directions into LDS, then rounds of
//     128 survivors (4 waves x 2 tiles x 16) through the three 256x256 hidden layers on the fp32 MFMA engine
//     (mlp_engine.h; activations stay in registers), VALU 256->2 head, softmax, result scattered to an LDS
//     visibility table; finally the SG-weighted mean per lobe (deterministic order).
#include "dvis_fused.h"

namespace rb {

__device__ __forceinline__ void unit_eps(float v[3]) {  // norm_axis (sg_render.py:107-108)
  float n = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) + RB_TINY;
  v[0] /= n;
  v[1] /= n;
  v[2] /= n;
}

// Directions in a cone around `axis` (sg_render.py:123-146 / 213-240): z-cross tangent frame, theta = 2*pi*u1,
// phi = u2 * phi_range.
__device__ __forceinline__ void cone_dir(const float axis[3], float u_theta, float u_phi, float phi_range, float d[3]) {
  float U[3] = {0.f * axis[2] - 1.f * axis[1], 1.f * axis[0] - 0.f * axis[2], 0.f * axis[1] - 0.f * axis[0]};
  unit_eps(U);
  float V[3] = {axis[1] * U[2] - axis[2] * U[1], axis[2] * U[0] - axis[0] * U[2], axis[0] * U[1] - axis[1] * U[0]};
  unit_eps(V);
  const float pi = (float)3.14159265358979323846;
  float th = u_theta * 2.f * pi;
  float ph = u_phi * phi_range;
  float ct = cosf(th), st = sinf(th), cp = cosf(ph), sp = sinf(ph);
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = U[c] * ct * sp + V[c] * st * sp + axis[c] * cp;
}

// One thread per (chunk, lobe): sample directions, SG weights and their per-lobe sum.
// lgt[L,7] raw light SGs (first row's light is used for every point: sg_render.py:388-390).
// direct = 0: lgt are RAW light SGs as render_with_sg receives them (it normalises the lobe and takes |lambda| before the
// call, sg_render.py:364-366, and get_diffuse_visibility normalises again, :126);  direct = 1: lgt[:, :3] / lgt[:, 3] are
// the lgtSGLobes / lgtSGLambdas arguments of a direct get_diffuse_visibility call (one normalisation, lambda as given).
__global__ void k_dvis_dirs(const float* __restrict__ lgt, int L, int nsamp, int C, int direct,
                            const float* __restrict__ u_theta,
                            const float* __restrict__ u_phi, float thr, float* __restrict__ dirs,
                            float* __restrict__ wdir, float* __restrict__ wsum) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C * L) return;
  const int l = i % L;
  // batch-global minimum sharpness over the lobes (sg_render.py:131-133)
  float mn = 3.0e38f;
  for (int k = 0; k < L; ++k) mn = fminf(mn, fmaxf(direct ? lgt[k * 7 + 3] : fabsf(lgt[k * 7 + 3]), 1e-4f));
  const float rng = fminf(mn, thr);
  float a[3] = {lgt[l * 7], lgt[l * 7 + 1], lgt[l * 7 + 2]};
  if (!direct) unit_eps(a);  // render_with_sg normalisation (sg_render.py:364)
  unit_eps(a);               // norm_axis inside get_diffuse_visibility (sg_render.py:126)
  const float lam = direct ? lgt[l * 7 + 3] : fabsf(lgt[l * 7 + 3]);
  const float sharp = fmaxf(lam, 1e-4f);
  const float phi_range = acosf((-0.95f * rng) / sharp + 1.f);
  float s = 0.f;
  for (int k = 0; k < nsamp; ++k) {
    const long j = (long)i * nsamp + k;
    float d[3];
    cone_dir(a, u_theta[j], u_phi[j], phi_range, d);
    dirs[3 * j] = d[0];
    dirs[3 * j + 1] = d[1];
    dirs[3 * j + 2] = d[2];
    const float w = expf(lam * ((d[0] * a[0] + d[1] * a[1] + d[2] * a[2]) - 1.f));
    wdir[j] = w;
    s += w;
  }
  wsum[i] = s + RB_TINY;
}

}  // namespace rb

using namespace rb;

extern "C" {

int rb_dvis_dirs(const float* lgt, int L, int nsamp, int C, int direct, const float* u_theta, const float* u_phi, float thr,
                 float* dirs, float* wdir, float* wsum, rb_stream_t stream) {
  RB_REQUIRE(lgt && u_theta && u_phi && dirs && wdir && wsum, "null pointer");
  RB_REQUIRE(L > 0 && nsamp > 0 && C > 0, "bad sizes");
  hipLaunchKernelGGL(k_dvis_dirs, grid1d((long)C * L, 64), dim3(64), 0, (hipStream_t)stream, lgt, L, nsamp, C, direct, u_theta,
                     u_phi, thr, dirs, wdir, wsum);
  return check_launch("k_dvis_dirs");
}

int rb_dvis_fused(const float* normals, const int* chunk_id, long n, const float* A, const float* Bd, const float* dirs,
                  const float* wdir, const float* wsum, const float* Whid, const float* wlast, const float* blast, int L,
                  int nsamp, int argmax_vis, int precision, int scale_log2, float* vis_out,
                  unsigned long long* eval_count, rb_stream_t stream) {
  if (n <= 0) return 0;
  RB_REQUIRE(precision == 0 || precision == 5, "precision: 0 = fp32 MFMA; 5 = f16x3 split (first-generation kernel)");
  RB_REQUIRE(normals && A && Bd && dirs && wdir && wsum && Whid && wlast && blast && vis_out, "null pointer");
  RB_REQUIRE(n <= RB_MAX_BLOCKS, "too many points for one launch (one workgroup each)");
  RB_REQUIRE(L > 0 && L <= 256 && nsamp > 0 && (long)L * nsamp <= DVIS_MAX_DIRS, "need L <= 256 and L*nsamp <= 4096");
  if (precision == 5)   // the kernel in the legacy library, a refusal in the default one: whichever this library links
    return dvis_fused_h3(normals, chunk_id, n, A, Bd, dirs, wdir, wsum, Whid, wlast, blast, L, nsamp, argmax_vis, scale_log2, vis_out,
                         eval_count, stream);
  hipLaunchKernelGGL((k_dvis_fused<false, 1, 2>), dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, normals, chunk_id, n, A,
                     Bd, dirs, wdir, wsum, (const f4*)Whid, wlast, blast, L, nsamp, argmax_vis, 1.0f, vis_out, eval_count,
                     (unsigned*)nullptr);
  return check_launch("k_dvis_fused");
}

}  // extern "C"
