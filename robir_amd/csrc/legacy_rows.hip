// Legacy library only: the feature-row forms of the f32-input MFMA networks (the <false> instances of mlp_f32.h) with the kernels
// that assemble their rows, and the f16x3 weight packer of the first split-precision generation (mlp_kernels_h3.hip).
#include "../../include/robir_hip_legacy.h"
#include "common.h"
#include "mlp_f32.h"
#include "pe.h"

namespace rb {

// f16x3 packing (mlp_engine.h, H3Ring): chunk jb = [bias*2^s (16 floats)] ++ [kb][hi|lo][lane][8 halves],
// half slot (lane, j) = W[16jb + (lane&15)][32kb + (j<4 ? 4g+j : 16+4g+j-4)] * 2^s, g = lane>>4.
__global__ void k_pack_layer_h3(const float* __restrict__ W, const float* __restrict__ b, int n_out, int k_in,
                                int n_pad, int k_pad, const int* __restrict__ perm, float scale, float* __restrict__ out) {
  const long chunk = 16 + (long)k_pad * 16;        // in floats (one float = two halves)
  const long total = (long)(n_pad / 16) * chunk;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int jb = (int)(i / chunk);
    const long o = i - (long)jb * chunk;
    if (o < 16) {
      const int j = jb * 16 + (int)o;
      out[i] = (b != nullptr && j < n_out) ? b[j] * scale : 0.f;
      continue;
    }
    // float index q inside the half area: [kb][hilo][lane][4 floats = 8 halves]
    const long q = o - 16;
    const int pair = (int)(q & 3), lane = (int)((q >> 2) & 63), hilo = (int)((q >> 8) & 1), kb = (int)(q >> 9);
    const int row = jb * 16 + (lane & 15), g = lane >> 4;
    _Float16 hv[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int j = pair * 2 + e;
      const int k = 32 * kb + (j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4));
      float v = 0.f;
      const int kin = perm ? perm[k] : k;          // packed slot k <- input column kin (-1: zero padding)
      if (row < n_out && kin >= 0 && kin < k_in) v = W[(long)row * k_in + kin] * scale;
      const _Float16 h = (_Float16)v;
      hv[e] = hilo == 0 ? h : (_Float16)(v - (float)h);
    }
    union {
      _Float16 h[2];
      float f;
    } u;
    u.h[0] = hv[0];
    u.h[1] = hv[1];
    out[i] = u.f;
  }
}

// X[M,128] = [PE10(p) | PE10(d) | 0 0]   (VisNetwork input, implicit_differentiable_renderer.py:250-256); 32 threads per row
__global__ void k_feat_vis(const float* __restrict__ p, const float* __restrict__ d, long M, int rep,
                           float* __restrict__ X) {
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < M * 32; t += (long)gridDim.x * blockDim.x) {
    const long i = t >> 5;
    const int q = (int)(t & 31);
    const long ip = i / rep;  // each point is paired with `rep` consecutive directions
    const float a[3] = {p[3 * ip], p[3 * ip + 1], p[3 * ip + 2]};
    const float b[3] = {d[3 * i], d[3 * i + 1], d[3 * i + 2]};
    f4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int f = 4 * q + e;
      v[e] = f < 63 ? pe10_feature(a, f, -1, 0.f) : (f < 126 ? pe10_feature(b, f - 63, -1, 0.f) : 0.f);
    }
    reinterpret_cast<f4*>(X + i * 128)[q] = v;
  }
}

// X[M,304] = [feat*feat_scale (256) | x*x_scale (3) | PE4(view) (27) | normal (3) | 0 x15]
// (RenderingNetwork input, model/neus_model.py:535-545; the packed first layer is column-permuted to match)
__global__ void k_feat_color(const float* __restrict__ x, float x_scale, const float* __restrict__ view,
                             const float* __restrict__ normal, const float* __restrict__ feat, long feat_stride,
                             float feat_scale, long M, float* __restrict__ X) {
  const int t = threadIdx.x;  // 256 threads: one feature each; rows by grid stride (M * 256 may exceed 2^32 work-items)
  for (long i = blockIdx.x; i < M; i += gridDim.x) {
    float* row = X + i * 304;
    row[t] = feat[i * feat_stride + t] * feat_scale;
    if (t == 0) {
      float v[3] = {view[3 * i], view[3 * i + 1], view[3 * i + 2]};
      row[256] = x[3 * i] * x_scale;
      row[257] = x[3 * i + 1] * x_scale;
      row[258] = x[3 * i + 2] * x_scale;
      write_pe<4>(v, row + 259);
      row[286] = normal[3 * i];
      row[287] = normal[3 * i + 1];
      row[288] = normal[3 * i + 2];
#pragma unroll
      for (int k = 289; k < 304; ++k) row[k] = 0.f;
    }
  }
}

// T[M,48] = columns 256..303 of the row above: [x*x_scale (3) | PE4(view) (27) | normal (3) | 0 x15] (rb_color_mlp_h3_two)
__global__ void k_feat_color_tail(const float* __restrict__ x, float x_scale, const float* __restrict__ view,
                                  const float* __restrict__ normal, long M, float* __restrict__ T) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= M) return;
  float row[48];
  float v[3] = {view[3 * i], view[3 * i + 1], view[3 * i + 2]};
  row[0] = x[3 * i] * x_scale;
  row[1] = x[3 * i + 1] * x_scale;
  row[2] = x[3 * i + 2] * x_scale;
  write_pe<4>(v, row + 3);
  row[30] = normal[3 * i];
  row[31] = normal[3 * i + 1];
  row[32] = normal[3 * i + 2];
#pragma unroll
  for (int k = 33; k < 48; ++k) row[k] = 0.f;
  f4* dst = reinterpret_cast<f4*>(T + i * 48);
#pragma unroll
  for (int k = 0; k < 12; ++k) dst[k] = f4{row[4 * k], row[4 * k + 1], row[4 * k + 2], row[4 * k + 3]};
}

}  // namespace rb

using namespace rb;

extern "C" {

int rb_pack_layer_h3(const float* W, const float* b, int n_out, int k_in, int n_pad, int k_pad, const int* perm,
                     int scale_log2, float* out, rb_stream_t stream) {
  RB_REQUIRE(W && out, "null pointer");
  RB_REQUIRE(n_pad % 16 == 0 && k_pad % 32 == 0 && n_pad >= n_out && (perm || k_pad >= k_in), "bad padding");
  RB_REQUIRE(scale_log2 >= -14 && scale_log2 <= 14, "scale_log2 out of range");
  long total = rb_packed_layer_floats(n_pad, k_pad);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_pack_layer_h3, dim3(blocks), dim3(256), 0, (hipStream_t)stream, W, b, n_out, k_in, n_pad, k_pad,
                     perm, ldexpf(1.0f, scale_log2), out);
  return check_launch("k_pack_layer_h3");
}

int rb_feat_vis(const float* p, const float* d, long M, int rep, float* X, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(p && d && X, "null pointer");
  RB_REQUIRE(rep >= 1, "rep must be >= 1");
  const long vblocks = (M * 32 + 255) / 256;
  hipLaunchKernelGGL(k_feat_vis, dim3((unsigned)(vblocks < RB_MAX_BLOCKS ? vblocks : RB_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream, p, d, M,
                     rep, X);
  return check_launch("k_feat_vis");
}

int rb_feat_color(const float* x, float x_scale, const float* view, const float* normal, const float* feat,
                  long feat_stride, float feat_scale, long M, float* X, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(x && view && normal && feat && X, "null pointer");
  hipLaunchKernelGGL(k_feat_color, dim3((unsigned)(M < RB_MAX_BLOCKS ? M : RB_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream, x, x_scale, view, normal, feat,
                     feat_stride, feat_scale, M, X);
  return check_launch("k_feat_color");
}

int rb_feat_color_tail(const float* x, float x_scale, const float* view, const float* normal, long M, float* T, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(x && view && normal && T, "null pointer");
  hipLaunchKernelGGL(k_feat_color_tail, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, x_scale, view, normal, M, T);
  return check_launch("k_feat_color_tail");
}

int rb_vis_mlp(const float* X, long M, const float* Wp, float* logits, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(X && Wp && logits, "null pointer");
  hipLaunchKernelGGL(k_vis_mlp<false>, grid1d(M, 128), dim3(256), 0, (hipStream_t)stream, X, M, (const f4*)Wp, logits, nullptr, 1);
  return check_launch("k_vis_mlp");
}

int rb_linear_64_256(const float* X, long M, const float* Wp, float* Y, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(X && Wp && Y, "null pointer");
  hipLaunchKernelGGL(k_linear_64_256<false>, grid1d(M, 128), dim3(256), 0, (hipStream_t)stream, X, M, (const f4*)Wp, Y);
  return check_launch("k_linear_64_256");
}

int rb_sdf_mlp(const float* X, long M, const float* Wp, int mode, float out_scale, float grad_scale, float* out0,
               float* grad, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(X && Wp && out0, "null pointer");
  RB_REQUIRE((mode >= 0 && mode <= 3) || mode == 4 || mode == 6, "mode must be 0..3, or 4 / 6 (= 0 / 2 with library-grade activations)");
  RB_REQUIRE((mode & 3) < 2 || grad, "jvp modes need a gradient output");
  const long MR = (mode & 3) >= 2 ? 4 * M : M;
  dim3 grid = grid1d(MR, 128), block(256);
  hipStream_t s = (hipStream_t)stream;
  const f4* W = (const f4*)Wp;
  switch (mode) {
    case 0: hipLaunchKernelGGL(k_sdf_mlp<0>, grid, block, 0, s, X, MR, W, out_scale, grad_scale, out0, grad, 1.0f); break;
    case 1: hipLaunchKernelGGL(k_sdf_mlp<1>, grid, block, 0, s, X, MR, W, out_scale, grad_scale, out0, grad, 1.0f); break;
    case 2: hipLaunchKernelGGL(k_sdf_mlp<2>, grid, block, 0, s, X, MR, W, out_scale, grad_scale, out0, grad, 1.0f); break;
    case 3: hipLaunchKernelGGL(k_sdf_mlp<3>, grid, block, 0, s, X, MR, W, out_scale, grad_scale, out0, grad, 1.0f); break;
    case 4: hipLaunchKernelGGL((k_sdf_mlp<0, true>), grid, block, 0, s, X, MR, W, out_scale, grad_scale, out0, grad, 1.0f); break;
    default: hipLaunchKernelGGL((k_sdf_mlp<2, true>), grid, block, 0, s, X, MR, W, out_scale, grad_scale, out0, grad, 1.0f); break;
  }
  return check_launch("k_sdf_mlp");
}

int rb_color_mlp(const float* X, long M, const float* Wp, float* rgb, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(X && Wp && rgb, "null pointer");
  hipLaunchKernelGGL(k_color_mlp<false>, grid1d(M, 128), dim3(256), 0, (hipStream_t)stream, X, M, (const f4*)Wp, rgb, nullptr, 0L, 1.0f,
                     nullptr, 1.0f, nullptr, nullptr);
  return check_launch("k_color_mlp");
}

int rb_illum_mlp(const float* X, long M, const float* Wp, float* raw, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(X && Wp && raw, "null pointer");
  hipLaunchKernelGGL(k_wide_mlp<false>, grid1d(M, 64), dim3(256), 0, (hipStream_t)stream, X, M, (const f4*)Wp, raw);
  return check_launch("k_wide_mlp<illum>");
}

}  // extern "C"
