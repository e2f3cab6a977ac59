// d sdf / d (encoded input) by reverse mode with EXACT fp32 operands on the f16 matrix pipe ("f16x6") -- the default precision
// policy's gradient pass, round 3: k_sdf_back_f32 (mlp_f32.hip, f32-input MFMA) on the one-tile machine of x6_ring.h (sx_layer).
//
// In: the sigmoid tiles the value pass stored (k_sdf_x6<5> / k_sdf_mlp<5>: [tile = row / 16][layer 8][chunk 16][lane 64] float4).
// Out: two 64-wide gradient rows per point (layer 0's and the skip connection's share; k_pe_grad_points contracts them with the
// encoding's Jacobian).  The net, back to front, as one cyclic stream of 117 chunks (16 output rows x K x 3 pieces):
//   stream layer   0     1     2     3             4            5     6     7
//   matrix         W7^T  W6^T  W5^T  [W4^T]        W3^T         W2^T  W1^T  W0^T
//   K              256   256   256   256           224          256   256   256
//   chunks         16    16    16    13 + 4 skip   16           16    16    4
//   gate (sigmoid) l6    l5    l4    l3 (x 1/sqrt2; skip rows: x 1/sqrt2, out)   l2  l1  l0   -- (out)
// A layer's operands are dz = dh (.) sigmoid(100 z): the gate of a chunk's sixteen rows is one float4 per lane, loaded at the top of the
// layer (sixteen plain loads, credited in the counted waits of the layer's first two chunks) and multiplied in where the forward
// kernels apply the softplus.  Weights: packing.pack_sdf_back_x6.
#include "../../include/robir_hip.h"
#include "common.h"
#include "mlp_engine.h"
#include "x6_layout.h"
#include <cstdlib>
#include <type_traits>

namespace rb {

constexpr int BX_SLOT_B = 24 * 1024 + 512;
static_assert(sx_np(224) == 7 && sx_np(256) == 7 && sx_units(224) == 3 && sx_units(256) == 3, "every chunk of this stream is seven copies in three blocks per wave");

__global__ __launch_bounds__(256, 1) void k_sdf_back_x6(const f4* __restrict__ sig, long M, const f4* __restrict__ Wt,
                                                         const float* __restrict__ w8row, float* __restrict__ gfeat,
                                                         unsigned* __restrict__ range_word) {
  using Net = SxSdfBackNet<224>;
  using Stream = SxStream<Net>;
  __shared__ f4 ring[4 * BX_SLOT_B / 16];              // 98 KB
  __shared__ f4 bias_ring[4 * 16];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long nrounds = (M + 63) >> 6;
  if ((long)blockIdx.x >= nrounds) return;

  const float negk = -2048.0f, inv_sqrt2 = 0.70710678118654752440f;
  SxRing rg = sx_ring<BX_SLOT_B>(ring, bias_ring, lane, wave);
  unsigned sat = 0u;
  u4 xh[8], xm[8], xl[8];              // operands of the current layer: three pieces, one tile
  u4 yh[8], ym[8], yl[8];              // ... of the next layer
  long rrow = 0;
  const f4* sig_tile = sig;            // this wave's tile of the round: + (layer * 16 + chunk) * 64

  auto put_pair = [&](float v0, float v1, u4& dh, u4& dm, u4& dl, int q) {
    unsigned h, m, l;
    sx_split_pair(v0, v1, negk, h, m, l);
    dh[q] = h;
    dm[q] = m;
    dl[q] = l;
    sat = sat_acc(sat, h);
  };
  // operands of stream layer 0: d sdf / d h7 (row 0 of layer 8) gated by layer 7's sigmoid
  auto load_layer0 = [&]() {
    float p[64];
#pragma unroll
    for (int blk = 0; blk < 16; ++blk) {
      const f4 w = *reinterpret_cast<const f4*>(w8row + blk * 16 + 4 * g);
      const f4 s = sig_tile[(7 * 16 + blk) * 64];
#pragma unroll
      for (int r = 0; r < 4; ++r) p[blk * 4 + r] = w[r] * s[r];
    }
#pragma unroll
    for (int kb = 0; kb < 8; ++kb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = (2 * kb + (q >> 1)) * 4 + (q & 1) * 2;
        put_pair(p[i], p[i + 1], xh[kb], xm[kb], xl[kb], q);
      }
  };

  // GATE: sigmoid layer that gates this stream layer's outputs (-1: none, stream layer 7)
  auto run_layer = [&](auto LI_tag, int cb, int gate) {
    constexpr int LI = decltype(LI_tag)::value;
    constexpr int K = Net::K(LI), KB = K / 32, NCH = Net::nch(LI), CB = Stream::cbase(LI);
    constexpr bool OUT = LI == 7, SKIPL = LI == 3;
    constexpr int NSIG = OUT ? 0 : (SKIPL ? 13 : 16);
    SxAcc accs[2];
    const f4* wl = Wt + Stream::coff(cb);
    const f4* wnext[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) wnext[i] = Wt + Stream::coff(cb + NCH + i);
    asm volatile("" : "+s"(wl));
    // the gates of this layer's output chunks (plain loads: in flight over the first chunks)
    f4 sg[NSIG > 0 ? NSIG : 1];
    if constexpr (NSIG > 0) {
#pragma unroll
      for (int i = 0; i < NSIG; ++i) sg[i] = sig_tile[((long)gate * 16 + i) * 64];
    }
    auto hidden_pair = [&](const SxAcc& a, int pj, int q) {
      float v0 = sx_combine(a, 2 * q), v1 = sx_combine(a, 2 * q + 1);
      if (SKIPL) {
        v0 *= inv_sqrt2;
        v1 *= inv_sqrt2;
      }
      const f4 s = sg[pj < NSIG ? pj : 0];
      put_pair(v0 * s[2 * q], v1 * s[2 * q + 1], yh[pj >> 1], ym[pj >> 1], yl[pj >> 1], (pj & 1) * 2 + q);
    };
    auto output_chunk = [&](const SxAcc& a, int col0, float scale) {      // sixteen gradient columns of this lane's row
      if (rrow < M) *(reinterpret_cast<f4*>(gfeat + rrow * 128 + col0) + g) = f4{sx_combine(a, 0) * scale, sx_combine(a, 1) * scale, sx_combine(a, 2) * scale, sx_combine(a, 3) * scale};
    };
    auto epilogue = [&](const SxAcc& a, int pj, int q) {      // q = 0, 1: halves of a hidden chunk; outputs go out at q = 0
      if (OUT) {
        if (q == 0) output_chunk(a, pj * 16, 1.0f);
      } else if (SKIPL && pj >= 13) {
        if (q == 0) output_chunk(a, 64 + (pj - 13) * 16, inv_sqrt2);
      } else {
        hidden_pair(a, pj, q);
      }
    };
    sx_layer<KB, NCH, (KB % 2 == 0 ? 2 : 1), (KB % 2 == 0 ? 1 : 2), SxKs<224, 256>>(
        rg, accs, xh, xm, xl,
        [&](int jb) {      // chunk jb+1 must have landed: the copies of chunk jb+2 (7) -- and, in the layer's first two chunks, the
                           // younger gate loads -- may still be in flight
          if (jb < 2 && NSIG == 16) sx_wait<7 + 16>();
          else if (jb < 2 && NSIG == 13) sx_wait<7 + 13>();
          else sx_wait<7>();
        },
        [&](int j3) {
          return SxSrc{j3 < NCH ? wl + (long)j3 * sx_cf4(K) : wnext[j3 - NCH < 3 ? j3 - NCH : 0], j3 < NCH ? K : Net::K(Stream::layer_of(CB + j3))};
        },
        [&](int jb, int kb) {
          if (jb > 0) {
            if (kb == 0) epilogue(accs[(jb - 1) & 1], jb - 1, 0);
            if (kb == 3) epilogue(accs[(jb - 1) & 1], jb - 1, 1);
          }
        });
    const SxAcc& last = accs[(NCH - 1) & 1];
    epilogue(last, NCH - 1, 0);
    epilogue(last, NCH - 1, 1);
    if constexpr (!OUT) {
      constexpr int KBN = Net::K(LI + 1) / 32;
#pragma unroll
      for (int kb = 0; kb < KBN; ++kb) {
        xh[kb] = yh[kb];
        xm[kb] = ym[kb];
        xl[kb] = yl[kb];
      }
      if constexpr (SKIPL) {      // W3^T takes 224 = 208 + 16 zero slots: the second half of k-block 6 is padding
#pragma unroll
        for (int q = 2; q < 4; ++q) {
          xh[6][q] = 0u;
          xm[6][q] = 0u;
          xl[6][q] = 0u;
        }
      }
    }
  };

  // ---- prologue: chunks 0, 1, 2 of the stream
  sx_prologue<256>(rg, [&](int c) { return Wt + Stream::coff(c); });

  for (long round = blockIdx.x; round < nrounds; round += gridDim.x) {
    rrow = round * 64 + wave * 16 + (lane & 15);
    sig_tile = sig + ((round * 4 + wave) * 8) * (16L * 64) + lane;
    load_layer0();
    // stream layers 0, 1, 2, 5, 6 (one instance) | 3 (W4^T: gate + skip rows) | 4 (W3^T, K = 224) | 7 (W0^T: outputs)
#pragma unroll 1
    for (int l = 0; l < 8; ++l) {
      const int cb = l < 4 ? 16 * l : (l == 4 ? 65 : 81 + 16 * (l - 5));
      if (l == 3) run_layer(std::integral_constant<int, 3>{}, cb, 3);
      else if (l == 4) run_layer(std::integral_constant<int, 4>{}, cb, 2);
      else if (l == 7) run_layer(std::integral_constant<int, 7>{}, cb, -1);
      else run_layer(std::integral_constant<int, 0>{}, cb, 6 - l);
    }
  }
  range_report(sat, range_word);
  sx_wait<0>();
  __syncthreads();
}

// host-side launcher for sdf_value_grad.hip (rb_sdf_value_grad_x6_points)
int launch_sdf_back_x6(const float* sig, long M, const float* Wt, const float* w8row, float* gfeat, hipStream_t s) {
  const int pg = persistent_grid((M + 63) / 64, 0);
  if (pg <= 0) return rb::fail(__func__, "device query failed");
  const unsigned grid = (unsigned)pg;
  hipLaunchKernelGGL(k_sdf_back_x6, dim3(grid), dim3(256), 0, s, (const f4*)sig, M, (const f4*)Wt, w8row, gfeat,
                     range_flags() ? range_flags() + RB_RANGE_SDF : nullptr);
  return check_launch("k_sdf_back_x6");
}

}  // namespace rb
