// Visibility MLP (VisNetwork.forward, model/implicit_differentiable_renderer.py:241-258: [PE10(p) | PE10(d)] -> 256 x4 ReLU -> 2
// logits) with EXACT fp32 operands on the f16 matrix pipe ("f16x6") -- the default precision policy's kernel for the stand-alone
// visibility evaluations (specular visibility, trace_radiance), round 3.  The one-tile machine of x6_ring.h (sx_layer), the net as one cyclic
// stream of 65 chunks (K = 128 for the first layer, 256 after: x6_layout.h), both encodings computed in the kernel
// (load_features_vis: row i takes point i / rep).  Replaces k_vis_mlp (f32-input MFMA).  Weights: packing.pack_vis_x6.
#include "../../include/robir_hip.h"
#include "common.h"
#include "mlp_engine.h"
#include "x6_layout.h"
#include <type_traits>

namespace rb {

constexpr int VX_SLOT_B = 24 * 1024 + 512;

__global__ __launch_bounds__(256, 1) void k_vis_x6(const float* __restrict__ P, const float* __restrict__ Dr, int rep, long M,
                                                    const f4* __restrict__ Wp, float* __restrict__ logits,
                                                    unsigned* __restrict__ range_word) {
  using Net = SxVisNet;
  using Stream = SxStream<Net>;
  __shared__ f4 ring[4 * VX_SLOT_B / 16];              // 98 KB
  __shared__ f4 bias_ring[4 * 16];
  __shared__ float pe_scratch[4 * 16 * 128];           // 32 KB: the encoder's exchange rows (mlp_engine.h)
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long nrounds = (M + 63) >> 6;
  if ((long)blockIdx.x >= nrounds) return;

  const float negk = -2048.0f;
  SxRing rg = sx_ring<VX_SLOT_B>(ring, bias_ring, lane, wave);
  unsigned sat = 0u;
  u4 xh[8], xm[8], xl[8];              // operands of the current layer (K <= 256): three pieces, one tile
  u4 yh[8], ym[8], yl[8];              // ... of the next layer
  long rrow = 0;

  auto put_pair = [&](float v0, float v1, u4& dh, u4& dm, u4& dl, int q) {
    unsigned h, m, l;
    sx_split_pair(v0, v1, negk, h, m, l);
    dh[q] = h;
    dm[q] = m;
    dl[q] = l;
    sat = sat_acc(sat, h);
  };
  // this round's rows -> operands of layer 0: both encodings by the four lane groups of a row
  auto load_layer0 = [&]() {
    float in0[32];
    load_features_vis(P, Dr, rep, rrow, M, lane, pe_scratch + wave * 2048, in0);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = (2 * kb + (q >> 1)) * 4 + (q & 1) * 2;
        put_pair(in0[i], in0[i + 1], xh[kb], xm[kb], xl[kb], q);
      }
  };

  auto run_layer = [&](auto LI_tag, int cb) {
    constexpr int LI = decltype(LI_tag)::value;
    constexpr int K = Net::K(LI), KB = K / 32, NCH = Net::nch(LI), NP = sx_np(K), CB = 16 * LI;
    constexpr bool OUT = LI == 4;
    SxAcc accs[2];
    const f4* wl = Wp + Stream::coff(cb);
    const f4* wnext[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) wnext[i] = Wp + Stream::coff(cb + NCH + i);
    asm volatile("" : "+s"(wl));
    auto hidden_pair = [&](const SxAcc& a, int pj, int q) {
      put_pair(fmaxf(sx_combine(a, 2 * q), 0.f), fmaxf(sx_combine(a, 2 * q + 1), 0.f), yh[pj >> 1], ym[pj >> 1], yl[pj >> 1], (pj & 1) * 2 + q);
    };
    sx_layer<KB, NCH, (KB >= 8 ? 2 : 1), (KB >= 8 ? 1 : 2), SxKs<128, 256>>(
        rg, accs, xh, xm, xl,
        [&](int jb) {      // chunk jb+1 must have landed: this wave's copies of chunk jb+2 may still be in flight
          const int allowed = jb + 2 < NCH ? NP : sx_np(Net::K(Stream::layer_of(CB + jb + 2)));
          if (allowed >= 7) sx_wait<7>();
          else sx_wait<4>();
        },
        [&](int j3) {
          return SxSrc{j3 < NCH ? wl + (long)j3 * sx_cf4(K) : wnext[j3 - NCH < 3 ? j3 - NCH : 0], j3 < NCH ? K : Net::K(Stream::layer_of(CB + j3))};
        },
        [&](int jb, int kb) {      // relu + three-way split of chunk jb-1
          if (jb > 0 && !OUT) {
            if (kb == 0) hidden_pair(accs[(jb - 1) & 1], jb - 1, 0);
            if (kb == 3) hidden_pair(accs[(jb - 1) & 1], jb - 1, 1);
          }
        });
    const SxAcc& last = accs[(NCH - 1) & 1];
    if constexpr (OUT) {
      if (g == 0 && rrow < M) {
        logits[rrow * 2] = sx_combine(last, 0);
        logits[rrow * 2 + 1] = sx_combine(last, 1);
      }
    } else {
      hidden_pair(last, NCH - 1, 0);
      hidden_pair(last, NCH - 1, 1);
#pragma unroll
      for (int kb = 0; kb < 8; ++kb) {
        xh[kb] = yh[kb];
        xm[kb] = ym[kb];
        xl[kb] = yl[kb];
      }
    }
  };

  // ---- prologue: chunks 0, 1, 2 of the stream (layer 0: K = 128)
  sx_prologue<128>(rg, [&](int c) { return Wp + Stream::coff(c); });

  for (long round = blockIdx.x; round < nrounds; round += gridDim.x) {
    rrow = round * 64 + wave * 16 + (lane & 15);
    load_layer0();
    // layer 0 (K = 128) | 1, 2 (one instance) | 3 (followed by the output chunk and the next round's first chunks) | 4
#pragma unroll 1
    for (int l = 0; l < 5; ++l) {
      if (l == 0) run_layer(std::integral_constant<int, 0>{}, 0);
      else if (l == 3) run_layer(std::integral_constant<int, 3>{}, 48);
      else if (l == 4) run_layer(std::integral_constant<int, 4>{}, 64);
      else run_layer(std::integral_constant<int, 1>{}, 16 * l);
    }
  }
  range_report(sat, range_word);
  sx_wait<0>();
  __syncthreads();
}

}  // namespace rb

using namespace rb;

extern "C" int rb_vis_x6_points(const float* p, const float* d, long M, int rep, const float* Wp, float* logits, int n_workgroups,
                               rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(p && d && Wp && logits, "null pointer");
  RB_REQUIRE(rep >= 1, "rep must be >= 1");
  const int pg = persistent_grid((M + 63) / 64, n_workgroups);
  if (pg <= 0) return rb::fail(__func__, "device query failed");
  const unsigned grid = (unsigned)pg;
  hipLaunchKernelGGL(k_vis_x6, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, d, rep, M, (const f4*)Wp, logits,
                     range_flags() ? range_flags() + RB_RANGE_VIS : nullptr);
  return check_launch("k_vis_x6");
}
