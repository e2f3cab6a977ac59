// The first-generation network kernels on the f32-input MFMA (execution scheme: mlp_engine.h), as templates: mlp_f32.hip
// instantiates the forms that encode their input themselves (and the dense-row CESR / encoder forms the default header declares),
// legacy_rows.hip the feature-row forms of the legacy library.
#pragma once
#include "mlp_engine.h"
#include <type_traits>

namespace rb {

// =====================================================================================================
// Kernels.  All: 256 threads (4 waves), 1 wave per SIMD, rows_per_block = 64*NT.
// =====================================================================================================

// ---- visibility MLP: X[M,128] -> logits[M,2]   126(128) -> 256 x4 ReLU -> 2(16)
// FUSED: X = points p, Xd = directions d (rep directions per point): [PE10(p) | PE10(d)] encoded in the kernel (load_features_vis).
template <bool FUSED>
__global__ __launch_bounds__(256, 1) void k_vis_mlp(const float* __restrict__ X, long M, const f4* __restrict__ Wp,
                                                     float* __restrict__ Y, const float* __restrict__ Xd, int rep) {
  __shared__ f4 lds[2 * chunk_f4(256)];
  __shared__ float pe_scratch[FUSED ? 4 * 2 * 16 * 128 : 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  WStream<256> ws;
  ws.init(lds, tid);
  const f4* wl0 = Wp;
  const f4* wl1 = wl0 + layer_f4<128, 256>();
  const f4* wl4 = wl1 + 3 * layer_f4<256, 256>();
  const long row0 = ((long)blockIdx.x * 4 + wave) * 32 + (lane & 15);
  float h[2][64], z[2][64];
  {
    float in0[2][32];
    if constexpr (FUSED) {
      load_features_vis(X, Xd, rep, row0, M, lane, pe_scratch + (wave * 2 + 0) * 2048, in0[0]);
      load_features_vis(X, Xd, rep, row0 + 16, M, lane, pe_scratch + (wave * 2 + 1) * 2048, in0[1]);
    } else {
      load_features<128>(X, row0, M, lane, in0[0]);
      load_features<128>(X, row0 + 16, M, lane, in0[1]);
    }
    ws.prime<chunk_f4(128)>(wl0);
    dense_layer<128, 256, 2, 256>(ws, wl0, wl1, in0, z, lane, true);
  }
  activate<256, 2, ACT_RELU>(z, h);
#pragma unroll 1
  for (int l = 0; l < 3; ++l) {
    const f4* wl = wl1 + l * layer_f4<256, 256>();
    dense_layer<256, 256, 2, 256>(ws, wl, wl + layer_f4<256, 256>(), h, z, lane, true);
    activate<256, 2, ACT_RELU>(z, h);
  }
  float o[2][4];
  dense_layer<256, 16, 2, 0>(ws, wl4, nullptr, h, o, lane, true);
  if ((lane >> 4) == 0) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      long row = row0 + 16 * t;
      if (row < M) {
        Y[row * 2] = o[t][0];
        Y[row * 2 + 1] = o[t][1];
      }
    }
  }
}

// ---- single linear layer X[M,64] -> Y[M,256] (no activation); used to split the visibility net's first layer
//      into a per-point and a per-direction half for the fused diffuse-visibility kernel.
// FUSED: X = points / directions [M,3], encoded in the kernel.
template <bool FUSED>
__global__ __launch_bounds__(256, 1) void k_linear_64_256(const float* __restrict__ X, long M,
                                                           const f4* __restrict__ Wp, float* __restrict__ Y) {
  __shared__ f4 lds[2 * chunk_f4(64)];
  __shared__ float pe_scratch[FUSED ? 4 * 2 * 16 * 64 : 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  WStream<64> ws;
  ws.init(lds, tid);
  const long row0 = ((long)blockIdx.x * 4 + wave) * 32 + (lane & 15);
  float in0[2][16], z[2][64];
  if constexpr (FUSED) {
    load_features_pe10x(X, nullptr, row0, M, lane, pe_scratch + (wave * 2 + 0) * 1024, in0[0]);
    load_features_pe10x(X, nullptr, row0 + 16, M, lane, pe_scratch + (wave * 2 + 1) * 1024, in0[1]);
  } else {
    load_features<64>(X, row0, M, lane, in0[0]);
    load_features<64>(X, row0 + 16, M, lane, in0[1]);
  }
  ws.prime<chunk_f4(64)>(Wp);
  dense_layer<64, 256, 2, 0>(ws, Wp, nullptr, in0, z, lane, true);
  const int g = lane >> 4;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    long row = row0 + 16 * t;
    if (row < M) {
      f4* dst = reinterpret_cast<f4*>(Y + row * 256) + g;
#pragma unroll
      for (int jb = 0; jb < 16; ++jb) dst[jb * 4] = f4{z[t][jb * 4], z[t][jb * 4 + 1], z[t][jb * 4 + 2], z[t][jb * 4 + 3]};
    }
  }
}

// ---- NeuS SDF network (model/neus_model.py:385-417): PE10 (64) -> 256,256,256,193(208) -> skip cat /sqrt2 (272)
//      -> 256 x4 -> 257(272) | 1(16);  Softplus(beta=100, threshold 20).
// MODE 0: sdf only -> out0[M]          MODE 1: sdf+feat -> out0[M,257]
// MODE 2: forward-mode jvp, sdf only: X[4M,64] (value row + 3 tangent rows per point); out0[M], grad[M,3]
// MODE 3: forward-mode jvp, full:     X[4M,64]; out0[M,257], grad[M,3]
// FUSED: the rows are not read but encoded in the kernel from the points (mlp_engine.h: load_features_pe10).
template <int MODE, bool PRECISE = false, bool FUSED = false>
__global__ __launch_bounds__(256, 1) void k_sdf_mlp(const float* __restrict__ X, long MR, const f4* __restrict__ Wp,
                                                     float out_scale, float grad_scale, float* __restrict__ out0,
                                                     float* __restrict__ grad, float in_scale) {
  // MODE 5 (value rows, all 257 outputs): also stores sigmoid(100 z) of every hidden pre-activation for the reverse-mode gradient
  // pass k_sdf_back_f32 (mlp_f32.hip) through `grad` -- [tile][layer 8][k-block 16][lane 64] float4, in the register order of this engine.
  constexpr bool JVP = MODE == 2 || MODE == 3;
  constexpr bool FULL = (MODE == 1 || MODE == 3 || MODE == 5);
  constexpr bool STORE = MODE == 5;
  constexpr int NL = FULL ? 272 : 16;
  __shared__ f4 lds[2 * chunk_f4(272)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  WStream<272> ws;
  ws.init(lds, tid);
  constexpr long LF = layer_f4<256, 256>();
  const f4* w0 = Wp;
  const f4* w1 = w0 + layer_f4<64, 256>();
  const f4* w3 = w1 + 2 * LF;
  const f4* w4 = w3 + layer_f4<256, 208>();
  const f4* w5 = w4 + layer_f4<272, 256>();
  const f4* w8 = w5 + 3 * LF;
  const long row0 = ((long)blockIdx.x * 4 + wave) * 32 + (lane & 15);  // row of X (a jvp column when JVP)
  const bool bias_on = JVP ? ((lane & 3) == 0) : true;
  const float inv_sqrt2 = 0.70710678118654752440f;
  float x0[2][16], ha[2][64], z[2][64];
  if constexpr (FUSED) {                               // X = the points xyz[M,3]
    __shared__ float pe_scratch[4 * 2 * 16 * 64];      // 32 KB: one encoded tile per wave and tile
    load_features_pe10<JVP>(X, in_scale, row0, MR, lane, pe_scratch + (wave * 2 + 0) * 1024, x0[0]);
    load_features_pe10<JVP>(X, in_scale, row0 + 16, MR, lane, pe_scratch + (wave * 2 + 1) * 1024, x0[1]);
  } else {
    load_features<64>(X, row0, MR, lane, x0[0]);
    load_features<64>(X, row0 + 16, MR, lane, x0[1]);
  }
  // activation of one hidden layer (softplus_into), in MODE 5 with the sigmoid store
  f4* sig_tile = nullptr;
  if constexpr (STORE) sig_tile = reinterpret_cast<f4*>(grad) + (((long)blockIdx.x * 4 + wave) * 2) * (8L * 16 * 64) + lane;
  auto act = [&](auto nreg_tag, auto hreg_tag, const auto& zz, auto& hh, float scale, int layer) {
    constexpr int NREG = decltype(nreg_tag)::value, HREG = decltype(hreg_tag)::value;
    if constexpr (STORE) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kb = 0; kb < NREG / 4; ++kb) {
          f4 sg;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float s1;
            hh[t][kb * 4 + r] = softplus100<PRECISE>(zz[t][kb * 4 + r], &s1) * scale;
            sg[r] = s1;
          }
          sig_tile[((long)t * 8 + layer) * (16 * 64) + kb * 64] = sg;
        }
    } else {
      softplus_into<NREG, HREG, JVP, PRECISE>(zz, hh, lane, scale);
    }
  };
  using I52 = std::integral_constant<int, 52>;
  using I64 = std::integral_constant<int, 64>;
  using I68 = std::integral_constant<int, 68>;
  ws.prime<chunk_f4(64)>(w0);
  dense_layer<64, 256, 2, 256>(ws, w0, w1, x0, z, lane, bias_on);
  act(I64{}, I64{}, z, ha, 1.0f, 0);
#pragma unroll 1
  for (int l = 0; l < 2; ++l) {
    dense_layer<256, 256, 2, 256>(ws, w1 + l * LF, w1 + (l + 1) * LF, ha, z, lane, bias_on);
    act(I64{}, I64{}, z, ha, 1.0f, 1 + l);
  }
  {
    float hs[2][68];
    {
      float z3[2][52];
      dense_layer<256, 208, 2, 272>(ws, w3, w4, ha, z3, lane, bias_on);
      act(I52{}, I68{}, z3, hs, inv_sqrt2, 3);   // neurons 193..207 are padding: zero weights downstream
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) hs[t][52 + i] = x0[t][i] * inv_sqrt2;
    dense_layer<272, 256, 2, 256>(ws, w4, w5, hs, z, lane, bias_on);
  }
  act(I64{}, I64{}, z, ha, 1.0f, 4);
#pragma unroll 1
  for (int l = 0; l < 3; ++l) {
    dense_layer<256, 256, 2, 256>(ws, w5 + l * LF, w5 + (l + 1) * LF, ha, z, lane, bias_on);
    act(I64{}, I64{}, z, ha, 1.0f, 5 + l);
  }
  float zo[2][NL / 4];
  dense_layer<256, NL, 2, 0>(ws, w8, nullptr, ha, zo, lane, bias_on);

  const int g = lane >> 4;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const long row = row0 + 16 * t;
    if (row >= MR) continue;
    if constexpr (!JVP) {
      if constexpr (FULL) {
#pragma unroll
        for (int jb = 0; jb < NL / 16; ++jb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = jb * 16 + 4 * g + r;
            if (j < 257) out0[row * 257 + j] = zo[t][jb * 4 + r] * out_scale;
          }
      } else {
        if (g == 0) out0[row] = zo[t][0] * out_scale;
      }
    } else {
      const long m = row >> 2;
      const int c = (int)(row & 3);
      if (c == 0) {
        if constexpr (FULL) {
#pragma unroll
          for (int jb = 0; jb < NL / 16; ++jb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int j = jb * 16 + 4 * g + r;
              if (j < 257) out0[m * 257 + j] = zo[t][jb * 4 + r] * out_scale;
            }
        } else {
          if (g == 0) out0[m] = zo[t][0] * out_scale;
        }
      } else if (g == 0) {
        grad[m * 3 + (c - 1)] = zo[t][0] * grad_scale;
      }
    }
  }
}

// ---- NeuS colour network (model/neus_model.py:535-560): 289(304) -> 256 x4 ReLU -> 3(16) -> sigmoid
// FUSED: no assembled rows: the 256 feature columns are read in place from the SDF net's output rows and lane (n, g) ENCODES its
// twelve tail columns [x * x_scale | PE4(view) | normal | 0 x15] itself (embedview_fn, model/neus_model.py:535-545; the sincosf
// calls of write_pe<4>: bit-identical operands).
__device__ __forceinline__ float color_tail_feature(const float* __restrict__ px, float x_scale, const float* __restrict__ pv,
                                                    const float* __restrict__ pn, long i, int f) {
  if (f < 3) return px[3 * i + f] * x_scale;
  if (f < 6) return pv[3 * i + f - 3];
  if (f >= 30) return f < 33 ? pn[3 * i + f - 30] : 0.f;
  const int k = (f - 6) / 6, r = (f - 6) - 6 * k, c = r >= 3 ? r - 3 : r;
  float sn, cs;
  sincosf(pv[3 * i + c] * (float)(1 << k), &sn, &cs);
  return r >= 3 ? cs : sn;
}
template <bool FUSED>
__global__ __launch_bounds__(256, 1) void k_color_mlp(const float* __restrict__ X, long M, const f4* __restrict__ Wp,
                                                       float* __restrict__ rgb, const float* __restrict__ feat, long feat_stride,
                                                       float feat_scale, const float* __restrict__ px, float x_scale,
                                                       const float* __restrict__ pv, const float* __restrict__ pn) {
  __shared__ f4 lds[2 * chunk_f4(304)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  WStream<304> ws;
  ws.init(lds, tid);
  constexpr long LF = layer_f4<256, 256>();
  const f4* w0 = Wp;
  const f4* w1 = w0 + layer_f4<304, 256>();
  const f4* w4 = w1 + 3 * LF;
  const long row0 = ((long)blockIdx.x * 4 + wave) * 32 + (lane & 15);
  float h[2][64], z[2][64];
  {
    float in0[2][76];
    if constexpr (FUSED) {
      const int g = lane >> 4;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const long row = row0 + 16 * t;
        const bool ok = row < M;
        const long rr = ok ? row : 0;
        const float* pf = feat + rr * feat_stride + g * 4;
#pragma unroll
        for (int kb = 0; kb < 16; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r) in0[t][kb * 4 + r] = ok ? pf[kb * 16 + r] * feat_scale : 0.f;
#pragma unroll 1
        for (int kb = 0; kb < 3; ++kb) {
          float v[4];
#pragma unroll 1
          for (int r = 0; r < 4; ++r) v[r] = color_tail_feature(px, x_scale, pv, pn, rr, 16 * kb + 4 * g + r);
#pragma unroll
          for (int r = 0; r < 4; ++r) in0[t][64 + kb * 4 + r] = ok ? v[r] : 0.f;
        }
      }
    } else {
      load_features<304>(X, row0, M, lane, in0[0]);
      load_features<304>(X, row0 + 16, M, lane, in0[1]);
    }
    ws.prime<chunk_f4(304)>(w0);
    dense_layer<304, 256, 2, 256>(ws, w0, w1, in0, z, lane, true);
  }
  activate<256, 2, ACT_RELU>(z, h);
#pragma unroll 1
  for (int l = 0; l < 3; ++l) {
    dense_layer<256, 256, 2, 256>(ws, w1 + l * LF, w1 + (l + 1) * LF, h, z, lane, true);
    activate<256, 2, ACT_RELU>(z, h);
  }
  float o[2][4];
  dense_layer<256, 16, 2, 0>(ws, w4, nullptr, h, o, lane, true);
  if ((lane >> 4) == 0) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const long row = row0 + 16 * t;
      if (row < M) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[row * 3 + c] = 1.0f / (1.0f + expf(-o[t][c]));
      }
    }
  }
}

// ---- 512-wide nets, one 16-sample tile per wave.
// ENC = false: IndirctIllumNetwork.lobe_layer  64 -> 512 x4 ReLU -> 144            (raw outputs [M,144])
// ENC = true : SparseAE encoder                64 -> 512 x4 LeakyReLU(0.2) -> 32   (raw latent  [M,32])
// FUSED: X = points [M,3], extra [M] or NULL = column 63 (hdr_shift of the indirect-illumination net): [PE10(x) | extra] encoded here.
template <bool ENC, bool FUSED = false>
__global__ __launch_bounds__(256, 1) void k_wide_mlp(const float* __restrict__ X, long M, const f4* __restrict__ Wp,
                                                      float* __restrict__ Y, const float* __restrict__ extra = nullptr) {
  constexpr int NO = ENC ? 32 : 144;
  constexpr int ACT = ENC ? ACT_LEAKY02 : ACT_RELU;
  __shared__ f4 lds[2 * chunk_f4(512)];
  __shared__ float pe_scratch[FUSED ? 4 * 16 * 64 : 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  WStream<512> ws;
  ws.init(lds, tid);
  constexpr long LF = layer_f4<512, 512>();
  const f4* w0 = Wp;
  const f4* w1 = w0 + layer_f4<64, 512>();
  const f4* w4 = w1 + 3 * LF;
  const long row = ((long)blockIdx.x * 4 + wave) * 16 + (lane & 15);
  float h[1][128], z[1][128];
  {
    float in0[1][16];
    if constexpr (FUSED) {
      load_features_pe10x(X, extra, row, M, lane, pe_scratch + wave * 1024, in0[0]);
    } else {
      load_features<64>(X, row, M, lane, in0[0]);
    }
    ws.prime<chunk_f4(64)>(w0);
    dense_layer<64, 512, 1, 512>(ws, w0, w1, in0, z, lane, true);
  }
  activate<512, 1, ACT>(z, h);
#pragma unroll 1
  for (int l = 0; l < 3; ++l) {
    dense_layer<512, 512, 1, 512>(ws, w1 + l * LF, w1 + (l + 1) * LF, h, z, lane, true);
    activate<512, 1, ACT>(z, h);
  }
  float o[1][NO / 4];
  dense_layer<512, NO, 1, 0>(ws, w4, nullptr, h, o, lane, true);
  if (row < M) {
    const int g = lane >> 4;
#pragma unroll
    for (int jb = 0; jb < NO / 16; ++jb) {
      f4* dst = reinterpret_cast<f4*>(Y + row * NO + jb * 16) + g;
      *dst = f4{o[0][jb * 4], o[0][jb * 4 + 1], o[0][jb * 4 + 2], o[0][jb * 4 + 3]};
    }
  }
}

// ---- 512-wide SDFNetwork-style nets of the CESR stage (training/train_cesr.py:106-110):
//   shadow_net = SDFNetwork(63+128 -> 2, 512 x 8, skip [4], multires 0)   input [PE10(x) | one-hot light-lobe label]
//   normal_net = SDFNetwork(63 -> 3,     512 x 8, skip [4], multires 0)   input PE10(x)
// (model/neus_model.py:312-417 with multires = 0: no internal encoding).  Softplus(beta=100), skip concat /sqrt(2).
// K0P = padded input width (192 / 64), N3P = padded width of lin3 (336 / 464), K4 = N3P + K0P = 528 for both.
// ONEHOT: rows are (point, label) pairs, label = row % n_label; the kernel reads PE features of point row / n_label
// from Xp[n,64] and synthesises the one-hot part in registers (never materialised: it would be 98 KB per point).
// FUSED: X = the points [.,3]: the 63 encoded columns (model/embedder.py:17-38) are computed in the kernel (mlp_engine.h).
template <int K0P, int N3P, bool ONEHOT, bool FUSED = false>
__global__ __launch_bounds__(256, 1) void k_softplus512(const float* __restrict__ X, long M, int n_label,
                                                         const f4* __restrict__ Wp, int n_out, float* __restrict__ Y) {
  constexpr int K4 = N3P + K0P;
  static_assert(K4 == 528, "both CESR nets give a 528-wide skip layer");
  __shared__ f4 lds[2 * chunk_f4(528)];
  __shared__ float pe_scratch[FUSED ? 4 * 16 * 64 : 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  WStream<528> ws;
  ws.init(lds, tid);
  constexpr long LF = layer_f4<512, 512>();
  const f4* w0 = Wp;
  const f4* w1 = w0 + layer_f4<K0P, 512>();
  const f4* w3 = w1 + 2 * LF;
  const f4* w4 = w3 + layer_f4<512, N3P>();
  const f4* w5 = w4 + layer_f4<K4, 512>();
  const f4* w8 = w5 + 3 * LF;
  const long row = ((long)blockIdx.x * 4 + wave) * 16 + (lane & 15);
  const float inv_sqrt2 = 0.70710678118654752440f;
  float x0[1][K0P / 4], h[1][128], z[1][128];
  if constexpr (ONEHOT) {
    const bool ok = row < M;
    const long pt = ok ? row / n_label : 0;
    const int label = ok ? (int)(row % n_label) : -1;
    float enc[16];
    if constexpr (FUSED) load_features_pe10x(X, nullptr, row, M, lane, pe_scratch + wave * 1024, enc, n_label);
    const f4* p = reinterpret_cast<const f4*>(X + (FUSED ? 0 : pt * 64)) + g;
#pragma unroll
    for (int kb = 0; kb < K0P / 16; ++kb) {
      f4 v = f4{0.f, 0.f, 0.f, 0.f};
      if constexpr (FUSED) {
        if (kb < 4) v = f4{enc[kb * 4], enc[kb * 4 + 1], enc[kb * 4 + 2], enc[kb * 4 + 3]};
      } else {
        if (kb < 4 && ok) v = p[kb * 4];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = kb * 16 + 4 * g + r;
        float e = v[r];
        if (k == 63) e = 0.f;                       // column 63 of Xp is padding; the one-hot block starts here
        if (k >= 63 && k - 63 == label) e = 1.f;
        x0[0][kb * 4 + r] = e;
      }
    }
  } else if constexpr (FUSED && K0P == 64) {
    load_features_pe10x(X, nullptr, row, M, lane, pe_scratch + wave * 1024, x0[0]);
  } else {
    load_features<K0P>(X, row, M, lane, x0[0]);
  }
  ws.prime<chunk_f4(K0P)>(w0);
  dense_layer<K0P, 512, 1, 512>(ws, w0, w1, x0, z, lane, true);
  activate<512, 1, ACT_SOFTPLUS100>(z, h);
#pragma unroll 1
  for (int l = 0; l < 2; ++l) {
    dense_layer<512, 512, 1, 512>(ws, w1 + l * LF, w1 + (l + 1) * LF, h, z, lane, true);
    activate<512, 1, ACT_SOFTPLUS100>(z, h);
  }
  {
    float hs[1][K4 / 4];
    {
      float z3[1][N3P / 4];
      dense_layer<512, N3P, 1, K4>(ws, w3, w4, h, z3, lane, true);
#pragma unroll
      for (int i = 0; i < N3P / 4; ++i) hs[0][i] = act_fn<ACT_SOFTPLUS100>(z3[0][i]) * inv_sqrt2;
    }
#pragma unroll
    for (int i = 0; i < K0P / 4; ++i) hs[0][N3P / 4 + i] = x0[0][i] * inv_sqrt2;
    dense_layer<K4, 512, 1, 512>(ws, w4, w5, hs, z, lane, true);
  }
  activate<512, 1, ACT_SOFTPLUS100>(z, h);
#pragma unroll 1
  for (int l = 0; l < 3; ++l) {
    dense_layer<512, 512, 1, 512>(ws, w5 + l * LF, w5 + (l + 1) * LF, h, z, lane, true);
    activate<512, 1, ACT_SOFTPLUS100>(z, h);
  }
  float o[1][4];
  dense_layer<512, 16, 1, 0>(ws, w8, nullptr, h, o, lane, true);
  if (row < M && g == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < n_out) Y[row * n_out + r] = o[0][r];
  }
}

}  // namespace rb
