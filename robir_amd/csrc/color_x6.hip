// NeuS colour network (RenderingNetwork.forward, model/neus_model.py:535-560) with EXACT fp32 operands on the f16 matrix pipe
// ("f16x6") -- the default precision policy's colour kernel, round 3.  The one-tile machine of x6_ring.h (sx_layer; the net as one cyclic stream of 65
// chunks -- K = 320 for the first layer, 256 after: x6_layout.h -- through a 4-slot LDS ring of 30 KB slots) with k_color_ring8's inputs: the 256
// feature columns read where the SDF network wrote them, [x | PE4(view) | normal] encoded in the kernel.  Replaces k_color_mlp
// (f32-input MFMA: 134 ms of BASELINE config 2's 584 at the reference's precision).  Weights: packing.pack_color_x6.
#include "../../include/robir_hip.h"
#include "common.h"
#include "mlp_engine.h"
#include "x6_layout.h"
#include <type_traits>

namespace rb {

constexpr int CX_SLOT_B = 30 * 1024 + 512;
typedef float f4u8x __attribute__((ext_vector_type(4), aligned(4)));

__global__ __launch_bounds__(256, 1) void k_color_x6(const float* __restrict__ feat, long feat_stride, float feat_scale,
                                                      const float* __restrict__ pxyz, float x_scale, const float* __restrict__ pview,
                                                      const float* __restrict__ pnormal, long M, const f4* __restrict__ Wp,
                                                      float* __restrict__ rgb, unsigned* __restrict__ range_word) {
  using Net = SxColorNet;
  using Stream = SxStream<Net>;
  __shared__ f4 ring[4 * CX_SLOT_B / 16];              // 122 KB
  __shared__ f4 bias_ring[4 * 16];
  __shared__ float tail_lds[4 * 16 * 48];              // 12 KB: the encoded tail of the round's rows
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long nrounds = (M + 63) >> 6;
  if ((long)blockIdx.x >= nrounds) return;

  const float negk = -2048.0f;
  SxRing rg = sx_ring<CX_SLOT_B>(ring, bias_ring, lane, wave);
  unsigned sat = 0u;
  u4 xh[10], xm[10], xl[10];           // operands of the current layer (K <= 320): three pieces, one tile
  u4 yh[8], ym[8], yl[8];              // ... of the next layer
  long rrow = 0;

  // range sentinel: `sat` in the domain of sat_acc_nonneg (hidden activations are >= 0: one instruction per pair); the signed inputs
  // of a round go through sat_acc into `sat_in`, folded into `sat` behind them
  unsigned sat_in = 0u;
  auto put_pair = [&](float v0, float v1, u4& dh, u4& dm, u4& dl, int q, auto nonneg) {
    unsigned h, m, l;
    sx_split_pair(v0, v1, negk, h, m, l);
    dh[q] = h;
    dm[q] = m;
    dl[q] = l;
    if constexpr (decltype(nonneg)::value) sat = sat_acc_nonneg(sat, h);
    else sat_in = sat_acc(sat_in, h);
  };
  auto fold_sat_in = [&]() {
    if ((short)(sat_in & 0xffffu) >= 0x7ffe || (short)(sat_in >> 16) >= 0x7ffe) sat = 0x7c007c00u;
    sat_in = 0u;
  };
  // this round's rows -> operands of layer 0: features in place (x feat_scale), tail encoded by the four lane groups of a row
  auto load_layer0 = [&]() {
    const bool ok = rrow < M;
    const long rr = ok ? rrow : 0;
    float in0[80];
    const float* pf = feat + rr * feat_stride + g * 4;
#pragma unroll
    for (int kb = 0; kb < 16; ++kb) {
      const f4u8x v = *reinterpret_cast<const f4u8x*>(pf + kb * 16);
#pragma unroll
      for (int r = 0; r < 4; ++r) in0[kb * 4 + r] = ok ? v[r] * feat_scale : 0.f;
    }
    float pv[3], px[3], pn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      pv[c] = pview[3 * rr + c];
      px[c] = pxyz[3 * rr + c];
      pn[c] = pnormal[3 * rr + c];
    }
    float* trow = tail_lds + (wave * 16 + (lane & 15)) * 48;
    if (g == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        trow[c] = px[c] * x_scale;
        trow[3 + c] = pv[c];
        trow[30 + c] = pn[c];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 5; ++i) trow[33 + (g - 1) * 5 + i] = 0.f;
    }
#pragma unroll 1
    for (int j = g; j < 12; j += 4) {         // write_pe<4>: frequency k = j / 3, axis c = j % 3
      const int k = j / 3, c = j - 3 * k;
      float sn, cs;
      sincosf((c == 0 ? pv[0] : (c == 1 ? pv[1] : pv[2])) * (float)(1 << k), &sn, &cs);
      trow[6 + 6 * k + c] = sn;
      trow[6 + 6 * k + 3 + c] = cs;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // same wave, in-order LDS: all four lane groups have written
    const f4* pt = reinterpret_cast<const f4*>(trow) + g;
#pragma unroll
    for (int kb = 0; kb < 3; ++kb) {
      const f4 v = ok ? pt[kb * 4] : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r) in0[64 + kb * 4 + r] = v[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) in0[76 + r] = 0.f;
#pragma unroll
    for (int kb = 0; kb < 10; ++kb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = (2 * kb + (q >> 1)) * 4 + (q & 1) * 2;
        put_pair(in0[i], in0[i + 1], xh[kb], xm[kb], xl[kb], q, std::false_type{});
      }
    fold_sat_in();
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
      put_pair(fmaxf(sx_combine(a, 2 * q), 0.f), fmaxf(sx_combine(a, 2 * q + 1), 0.f), yh[pj >> 1], ym[pj >> 1], yl[pj >> 1], (pj & 1) * 2 + q, std::true_type{});
    };
    sx_layer<KB, NCH, 2, 1, SxKs<320, 256>>(
        rg, accs, xh, xm, xl,
        [&](int jb) {      // chunk jb+1 must have landed: this wave's copies of chunk jb+2 may still be in flight
          const int allowed = jb + 2 < NCH ? NP : sx_np(Net::K(Stream::layer_of(CB + jb + 2)));
          if (allowed >= 9) sx_wait<9>();
          else sx_wait<7>();
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
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[rrow * 3 + c] = 1.0f / (1.0f + expf(-sx_combine(last, c)));
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

  // ---- prologue: chunks 0, 1, 2 of the stream (layer 0: K = 320)
  sx_prologue<320>(rg, [&](int c) { return Wp + Stream::coff(c); });

  for (long round = blockIdx.x; round < nrounds; round += gridDim.x) {
    rrow = round * 64 + wave * 16 + (lane & 15);
    load_layer0();
    // layer 0 (K = 320) | 1, 2 (one instance) | 3 (followed by the output chunk and the next round's first chunks) | 4
#pragma unroll 1
    for (int l = 0; l < 5; ++l) {
      if (l == 0) run_layer(std::integral_constant<int, 0>{}, 0);
      else if (l == 3) run_layer(std::integral_constant<int, 3>{}, 48);
      else if (l == 4) run_layer(std::integral_constant<int, 4>{}, 64);
      else run_layer(std::integral_constant<int, 1>{}, 16 * l);
    }
  }
  range_report<true>(sat, range_word);
  sx_wait<0>();
  __syncthreads();
}

}  // namespace rb

using namespace rb;

extern "C" int rb_color_x6_points(const float* feat, long feat_stride, float feat_scale, const float* x, float x_scale, const float* view,
                                  const float* normal, long M, const float* Wp, float* rgb, int two_tile, int n_workgroups,
                                  rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(feat && x && view && normal && Wp && rgb, "null pointer");
  if (two_tile)      // two 16-row tiles per wave, rounds of 128 rows (color_x6t.hip): the form for launches that fill the grid
    return rb::launch_color_x6t(feat, feat_stride, feat_scale, x, x_scale, view, normal, M, Wp, rgb, n_workgroups, (hipStream_t)stream);
  const int pg = persistent_grid((M + 63) / 64, n_workgroups);
  if (pg <= 0) return rb::fail(__func__, "device query failed");
  const unsigned grid = (unsigned)pg;
  hipLaunchKernelGGL(k_color_x6, dim3(grid), dim3(256), 0, (hipStream_t)stream, feat, feat_stride, feat_scale, x, x_scale, view, normal, M,
                     (const f4*)Wp, rgb, range_flags() ? range_flags() + RB_RANGE_COLOR : nullptr);
  return check_launch("k_color_x6");
}
