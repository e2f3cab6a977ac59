// Entry points of the f32-input MFMA networks (the fp32 override and the exact policy's reference precision): the kernels of
// mlp_f32.h on points, the reverse-mode SDF gradient pass, the auto-encoder decoder and the small element-wise kernels around them.
// All pointers are device pointers; nothing allocates.
#include "../../include/robir_hip.h"
#include "common.h"
#include "mlp_f32.h"

namespace rb {

// ---- d sdf / d (encoded input) by reverse mode on the f32-input MFMA (the exact policy's counterpart of sdf_back.hip): the sigmoid
// tiles of k_sdf_mlp<5> in, two 64-wide gradient rows per point out (layer 0's and the skip connection's share: k_pe_grad_points
// contracts them with the encoding's Jacobian).  One pass over the transposed layers instead of the three tangent rows per point of
// the forward-mode kernels (modes 2 / 3): 2 x the value pass's MACs instead of 4 x.
// Wt (packing.pack_sdf_back): W7^T, W6^T, W5^T, [W4^T: 193 -> 208 rows | 63 -> 64 skip rows] (N = 272), W3^T (K = 208), W2^T, W1^T,
// W0^T (N = 64), no biases; w8row = row 0 of layer 8 (d sdf / d h7).
__global__ __launch_bounds__(256, 1) void k_sdf_back_f32(const f4* __restrict__ sig, long M, const f4* __restrict__ Wt,
                                                          const float* __restrict__ w8row, float* __restrict__ gfeat) {
  __shared__ f4 lds[2 * chunk_f4(272)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  WStream<272> ws;
  ws.init(lds, tid);
  constexpr long LF = layer_f4<256, 256>();
  const f4* b7 = Wt;
  const f4* b4 = b7 + 3 * LF;
  const f4* b3 = b4 + layer_f4<256, 272>();
  const f4* b2 = b3 + layer_f4<208, 256>();
  const f4* b0 = b2 + 2 * LF;
  const long row0 = ((long)blockIdx.x * 4 + wave) * 32 + (lane & 15);
  const f4* sig_tile = sig + (((long)blockIdx.x * 4 + wave) * 2) * (8L * 16 * 64) + lane;
  const float inv_sqrt2 = 0.70710678118654752440f;
  float dh[2][64], dz[2][64];
  // dz = dh (.) sigmoid(100 z) of `layer`, NB k-blocks
  auto gate = [&](auto nb_tag, const auto& hh, auto& zz, int layer) {
    constexpr int NB = decltype(nb_tag)::value;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int kb = 0; kb < NB; ++kb) {
        const f4 sg = sig_tile[((long)t * 8 + layer) * (16 * 64) + kb * 64];
#pragma unroll
        for (int r = 0; r < 4; ++r) zz[t][kb * 4 + r] = hh[t][kb * 4 + r] * sg[r];
      }
  };
  using I13 = std::integral_constant<int, 13>;
  using I16 = std::integral_constant<int, 16>;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int kb = 0; kb < 16; ++kb) {
      const f4 v = *reinterpret_cast<const f4*>(w8row + kb * 16 + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) dh[t][kb * 4 + r] = v[r];
    }
  ws.prime<chunk_f4(256)>(b7);
#pragma unroll 1
  for (int l = 0; l < 3; ++l) {                 // layers 7, 6, 5
    gate(I16{}, dh, dz, 7 - l);
    dense_layer<256, 256, 2, 256>(ws, b7 + l * LF, l < 2 ? b7 + (l + 1) * LF : b4, dz, dh, lane, false);
  }
  gate(I16{}, dh, dz, 4);
  float skip[2][16];
  {
    float dhs[2][68];
    dense_layer<256, 272, 2, 208>(ws, b4, b3, dz, dhs, lane, false);
    float dz3[2][52];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int i = 0; i < 52; ++i) dh[t][i] = dhs[t][i] * inv_sqrt2;
#pragma unroll
      for (int i = 0; i < 16; ++i) skip[t][i] = dhs[t][52 + i] * inv_sqrt2;
    }
    gate(I13{}, dh, dz3, 3);
    dense_layer<208, 256, 2, 256>(ws, b3, b2, dz3, dh, lane, false);
  }
  gate(I16{}, dh, dz, 2);
  dense_layer<256, 256, 2, 256>(ws, b2, b2 + LF, dz, dh, lane, false);
  gate(I16{}, dh, dz, 1);
  dense_layer<256, 256, 2, 256>(ws, b2 + LF, b0, dz, dh, lane, false);
  gate(I16{}, dh, dz, 0);
  float dx[2][16];
  dense_layer<256, 64, 2, 0>(ws, b0, nullptr, dz, dx, lane, false);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const long row = row0 + 16 * t;
    if (row >= M) continue;
    f4* dst = reinterpret_cast<f4*>(gfeat + row * 128) + g;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      dst[kb * 4] = f4{dx[t][kb * 4], dx[t][kb * 4 + 1], dx[t][kb * 4 + 2], dx[t][kb * 4 + 3]};
      dst[16 + kb * 4] = f4{skip[t][kb * 4], skip[t][kb * 4 + 1], skip[t][kb * 4 + 2], skip[t][kb * 4 + 3]};
    }
  }
}

// host-side launchers for sdf_value_grad.hip (rb_sdf_value_grad_f32_points)
int launch_sdf_f32_store(const float* xyz, long M, float in_scale, const float* Wp, float out_scale, float* out0, float* sig,
                         hipStream_t s) {
  hipLaunchKernelGGL((k_sdf_mlp<5, false, true>), grid1d(M, 128), dim3(256), 0, s, xyz, M, (const f4*)Wp, out_scale, 1.0f, out0, sig, in_scale);
  return check_launch("k_sdf_mlp<5>");
}
int launch_sdf_back_f32(const float* sig, long M, const float* Wt, const float* w8row, float* gfeat, hipStream_t s) {
  hipLaunchKernelGGL(k_sdf_back_f32, grid1d(M, 128), dim3(256), 0, s, (const f4*)sig, M, (const f4*)Wt, w8row, gfeat);
  return check_launch("k_sdf_back_f32");
}

// ---- SparseAE decoder (sg_envmap_material.py:61-68): 32 -> 128 -> 128 LeakyReLU(0.2) -> n_out(16)
__global__ __launch_bounds__(256, 1) void k_ae_decode(const float* __restrict__ L, long M, const f4* __restrict__ Wp,
                                                       int n_out, int sigmoid_out, float* __restrict__ Y) {
  __shared__ f4 lds[2 * chunk_f4(128)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  WStream<128> ws;
  ws.init(lds, tid);
  const f4* w0 = Wp;
  const f4* w1 = w0 + layer_f4<32, 128>();
  const f4* w2 = w1 + layer_f4<128, 128>();
  const long row0 = ((long)blockIdx.x * 4 + wave) * 32 + (lane & 15);
  float in0[2][8], h[2][32], z[2][32];
  load_features<32>(L, row0, M, lane, in0[0]);
  load_features<32>(L, row0 + 16, M, lane, in0[1]);
  ws.prime<chunk_f4(32)>(w0);
  dense_layer<32, 128, 2, 128>(ws, w0, w1, in0, z, lane, true);
  activate<128, 2, ACT_LEAKY02>(z, h);
  dense_layer<128, 128, 2, 128>(ws, w1, w2, h, z, lane, true);
  activate<128, 2, ACT_LEAKY02>(z, h);
  float o[2][4];
  dense_layer<128, 16, 2, 0>(ws, w2, nullptr, h, o, lane, true);
  const int g = lane >> 4;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const long row = row0 + 16 * t;
    if (row < M) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 4 * g + r;
        if (j < n_out) {
          float v = o[t][r];
          Y[row * n_out + j] = sigmoid_out ? 1.0f / (1.0f + expf(-v)) : v;
        }
      }
    }
  }
}

// ---- small element-wise pieces of the auto-encoders / indirect-illumination head
// latent = act(raw * (1 - var));  act: 0 sigmoid, 1 softplus(beta=1, threshold 20)   (sg_envmap_material.py:74-99)
// writes lat[M,32]; if lat2 != null also lat2 = lat + noise*noise_scale (smooth_on_latent branch)
__global__ void k_ae_latent(const float* __restrict__ raw, long M, const float* __restrict__ var, int act,
                            const float* __restrict__ noise, float noise_scale, float* __restrict__ lat,
                            float* __restrict__ lat2) {
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= M * 32) return;
  float v = raw[i];
  if (var) v = v * (1.0f - var[i & 31]);
  float a;
  if (act == 0) {
    a = 1.0f / (1.0f + expf(-v));
  } else if (act == 1) {
    a = v > 20.0f ? v : log1pf(expf(v));
  } else {
    a = v;                      // SparseAE.encode: the pre-activation latent
  }
  lat[i] = a;
  if (lat2) lat2[i] = a + noise[i] * noise_scale;
}

// y = a + s*b over n floats
__global__ void k_axpy(const float* __restrict__ a, const float* __restrict__ b, float s, long n, float* __restrict__ y) {
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i < n) y[i] = a[i] + s * b[i];
}

// IndirctIllumNetwork head (implicit_differentiable_renderer.py:206-218): raw[M,24,6] -> sgs[M,24,7]
__global__ void k_illum_decode(const float* __restrict__ raw, long n_lobes, float* __restrict__ sgs) {
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n_lobes) return;
  const float* r = raw + i * 6;
  const float two_pi = (float)(2.0 * 3.14159265358979323846), pi = (float)3.14159265358979323846;
  float a = 1.0f / (1.0f + expf(-r[0])), b = 1.0f / (1.0f + expf(-r[1]));
  float theta = a * 2.0f * pi, phi = b * pi;
  (void)two_pi;
  float* o = sgs + i * 7;
  o[0] = cosf(theta) * sinf(phi);
  o[1] = sinf(theta) * sinf(phi);
  o[2] = cosf(phi);
  o[3] = (1.0f / (1.0f + expf(-r[2]))) * 30.0f + 0.1f;
  o[4] = fmaxf(r[3], 0.f);
  o[5] = fmaxf(r[4], 0.f);
  o[6] = fmaxf(r[5], 0.f);
}

}  // namespace rb

using namespace rb;

extern "C" {

int rb_vis_mlp_points(const float* p, const float* d, long M, int rep, const float* Wp, float* logits, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(p && d && Wp && logits, "null pointer");
  RB_REQUIRE(rep >= 1, "rep must be >= 1");
  hipLaunchKernelGGL(k_vis_mlp<true>, grid1d(M, 128), dim3(256), 0, (hipStream_t)stream, p, M, (const f4*)Wp, logits, d, rep);
  return check_launch("k_vis_mlp<points>");
}

int rb_linear_pe10_256(const float* x, long M, const float* Wp, float* Y, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(x && Wp && Y, "null pointer");
  hipLaunchKernelGGL(k_linear_64_256<true>, grid1d(M, 128), dim3(256), 0, (hipStream_t)stream, x, M, (const f4*)Wp, Y);
  return check_launch("k_linear_64_256<points>");
}

int rb_sdf_mlp_points(const float* x, long M, float in_scale, const float* Wp, int mode, float out_scale, float grad_scale,
                      float* out0, float* grad, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(x && Wp && out0, "null pointer");
  RB_REQUIRE((mode >= 0 && mode <= 3) || mode == 4 || mode == 6, "mode must be 0..3, or 4 / 6 (= 0 / 2 with library-grade activations)");
  RB_REQUIRE((mode & 3) < 2 || grad, "jvp modes need a gradient output");
  const long MR = (mode & 3) >= 2 ? 4 * M : M;
  dim3 grid = grid1d(MR, 128), block(256);
  hipStream_t s = (hipStream_t)stream;
  const f4* W = (const f4*)Wp;
  switch (mode) {
    case 0: hipLaunchKernelGGL((k_sdf_mlp<0, false, true>), grid, block, 0, s, x, MR, W, out_scale, grad_scale, out0, grad, in_scale); break;
    case 1: hipLaunchKernelGGL((k_sdf_mlp<1, false, true>), grid, block, 0, s, x, MR, W, out_scale, grad_scale, out0, grad, in_scale); break;
    case 2: hipLaunchKernelGGL((k_sdf_mlp<2, false, true>), grid, block, 0, s, x, MR, W, out_scale, grad_scale, out0, grad, in_scale); break;
    case 3: hipLaunchKernelGGL((k_sdf_mlp<3, false, true>), grid, block, 0, s, x, MR, W, out_scale, grad_scale, out0, grad, in_scale); break;
    case 4: hipLaunchKernelGGL((k_sdf_mlp<0, true, true>), grid, block, 0, s, x, MR, W, out_scale, grad_scale, out0, grad, in_scale); break;
    default: hipLaunchKernelGGL((k_sdf_mlp<2, true, true>), grid, block, 0, s, x, MR, W, out_scale, grad_scale, out0, grad, in_scale); break;
  }
  return check_launch("k_sdf_mlp<points>");
}

int rb_color_mlp_points(const float* feat, long feat_stride, float feat_scale, const float* x, float x_scale, const float* view,
                        const float* normal, long M, const float* Wp, float* rgb, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(feat && x && view && normal && Wp && rgb, "null pointer");
  hipLaunchKernelGGL(k_color_mlp<true>, grid1d(M, 128), dim3(256), 0, (hipStream_t)stream, nullptr, M, (const f4*)Wp, rgb, feat, feat_stride,
                     feat_scale, x, x_scale, view, normal);
  return check_launch("k_color_mlp<points>");
}

int rb_wide_mlp_points(const float* x, const float* extra, long M, const float* Wp, int encoder, float* Y, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(x && Wp && Y, "null pointer");
  if (encoder) {
    hipLaunchKernelGGL((k_wide_mlp<true, true>), grid1d(M, 64), dim3(256), 0, (hipStream_t)stream, x, M, (const f4*)Wp, Y, extra);
  } else {
    hipLaunchKernelGGL((k_wide_mlp<false, true>), grid1d(M, 64), dim3(256), 0, (hipStream_t)stream, x, M, (const f4*)Wp, Y, extra);
  }
  return check_launch("k_wide_mlp<points>");
}

int rb_cesr_net_points(const float* x, long M, int kind, int n_label, const float* Wp, float* Y, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(x && Wp && Y, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  dim3 grid = grid1d(M, 64), block(256);
  const f4* W = (const f4*)Wp;
  switch (kind) {
    case 0: hipLaunchKernelGGL((k_softplus512<64, 464, false, true>), grid, block, 0, s, x, M, 1, W, 3, Y); break;
    case 2:
      RB_REQUIRE(n_label >= 1 && n_label <= 128, "n_label must be 1..128");
      hipLaunchKernelGGL((k_softplus512<192, 336, true, true>), grid, block, 0, s, x, M, n_label, W, 2, Y);
      break;
    default: return rb::fail("rb_cesr_net_points", "kind: 0 normal_net on PE10(x), 2 shadow_net on (point, one-hot label) rows");
  }
  return check_launch("k_softplus512<points>");
}

int rb_cesr_net(const float* X, long M, int kind, int n_label, const float* Wp, float* Y, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(X && Wp && Y, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  dim3 grid = grid1d(M, 64), block(256);
  const f4* W = (const f4*)Wp;
  switch (kind) {
    case 0: hipLaunchKernelGGL((k_softplus512<64, 464, false>), grid, block, 0, s, X, M, 1, W, 3, Y); break;
    case 1: hipLaunchKernelGGL((k_softplus512<192, 336, false>), grid, block, 0, s, X, M, 1, W, 2, Y); break;
    case 2:
      RB_REQUIRE(n_label >= 1 && n_label <= 128, "n_label must be 1..128");
      hipLaunchKernelGGL((k_softplus512<192, 336, true>), grid, block, 0, s, X, M, n_label, W, 2, Y);
      break;
    default: return rb::fail("rb_cesr_net", "kind: 0 normal_net, 1 shadow_net (dense rows), 2 shadow_net (point x one-hot label)");
  }
  return check_launch("k_softplus512");
}

int rb_ae_encode(const float* X, long M, const float* Wp, float* raw_latent, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(X && Wp && raw_latent, "null pointer");
  hipLaunchKernelGGL(k_wide_mlp<true>, grid1d(M, 64), dim3(256), 0, (hipStream_t)stream, X, M, (const f4*)Wp,
                     raw_latent);
  return check_launch("k_wide_mlp<enc>");
}

int rb_ae_latent(const float* raw, long M, const float* var, int act, const float* noise, float noise_scale, float* lat,
                 float* lat2, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(raw && lat, "null pointer");
  RB_REQUIRE(!lat2 || noise, "lat2 needs noise");
  RB_REQUIRE(act >= 0 && act <= 2, "act: 0 sigmoid, 1 softplus, 2 none");
  hipLaunchKernelGGL(k_ae_latent, grid1d(M * 32, 256), dim3(256), 0, (hipStream_t)stream, raw, M, var, act, noise,
                     noise_scale, lat, lat2);
  return check_launch("k_ae_latent");
}

int rb_ae_decode(const float* lat, long M, const float* Wp, int n_out, int sigmoid_out, float* Y, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(lat && Wp && Y, "null pointer");
  RB_REQUIRE(n_out >= 1 && n_out <= 16, "n_out must be 1..16");
  hipLaunchKernelGGL(k_ae_decode, grid1d(M, 128), dim3(256), 0, (hipStream_t)stream, lat, M, (const f4*)Wp, n_out,
                     sigmoid_out, Y);
  return check_launch("k_ae_decode");
}

int rb_axpy(const float* a, const float* b, float s, long n, float* y, rb_stream_t stream) {
  if (n <= 0) return 0;
  RB_REQUIRE(a && b && y, "null pointer");
  hipLaunchKernelGGL(k_axpy, grid1d(n, 256), dim3(256), 0, (hipStream_t)stream, a, b, s, n, y);
  return check_launch("k_axpy");
}

int rb_illum_decode(const float* raw, long M, float* sgs, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(raw && sgs, "null pointer");
  hipLaunchKernelGGL(k_illum_decode, grid1d(M * 24, 256), dim3(256), 0, (hipStream_t)stream, raw, M * 24, sgs);
  return check_launch("k_illum_decode");
}

}  // extern "C"
