// The one-tile exact-operand ("f16x6") chunk-stream machine: sdf_x6.hip, color_x6.hip, vis_x6.hip, sdf_back_x6.hip (the two-tile form is
// x6t_engine.h).  Four waves, one 16-row tile each; every operand as three f16 pieces, the six partial products of weight >= 2^-22 in
// three fp32 accumulators by weight class (vis_diffuse_x6.hip has the arithmetic); the net as one cyclic stream of UNITS (x6_layout.h)
// through a 4-slot LDS ring that LDS-DMA fills three units ahead of the MFMAs.  The two K = 512 kernels (a chunk is two units) stand
// apart: wide_x6.hip runs a unit loop of its own on the pieces here (everything but sx_layer: under sx_layer its encoder instances
// spill); cesr_x6.hip (one MFMA per filler slot, spread copies) uses only the copies, the split and SxAcc -- with the ring state and the
// helpers below its register allocation moves (AGPR 225 -> 241, scratch 304 -> 344 bytes).  profiles/x6_engine_refactor.md has both.
//   * the copy of a packed unit (rb_pack_layer_x6: 16 bias floats, then [k-block][piece h | m | l][lane] float4), counted waits, the exact
//     three-way split of an fp32 value, the accumulators (SxAcc) and the ring's state (SxRing);
//   * sx_prologue: the first three units of the stream;
//   * sx_layer: one layer -- NU units (chunks of 16 output neurons) of KB k-blocks.  Per unit: fragments read BS
//     k-blocks at a time, D = BS DB k-blocks ahead of the MFMAs and across the unit's end; in the unit's middle a counted wait, ONE
//     s_barrier (the next unit has landed in every wave's view) and the next unit's bias; six MFMA runs per BS k-blocks, one per product,
//     a weight class per accumulator; the copies of the unit three ahead spread over the unit's second half; at the layer's end the slot
//     table is rotated so that slot 0 is the next layer's first unit.  A kernel passes three callables: its counted wait, the source of
//     the unit three ahead, and a filler called behind the MFMAs of every k-block (where it puts the previous chunk's epilogue).
// Timing ablations (wrong results; tools/build_variant.sh): -DSX_ABL_NOBAR no barrier, -DSX_ABL_NOREAD no fragment reads, -DSX_ABL_NODMA no
// copies behind the prologue's.
#pragma once
#include "common.h"
#include "mlp_engine.h"
#include <type_traits>

namespace rb {

__host__ __device__ constexpr long sx_cf4(int K) { return 4 + 6L * K; }                    // float4s of a packed chunk (bias first)
// copies of a chunk by one wave: the bias head (one 256-byte instruction), then its span of the chunk's NS = 3 K / 32 fragment slices
// of 1 KB: NSW = ceil(NS / 4) consecutive slices from min(v NSW, NS - NSW) (the last wave's span is shifted back into the chunk: a few
// slices are copied twice), in blocks of <= 4 instructions that share one M0 write.
__host__ __device__ constexpr int sx_ns(int K) { return 3 * K / 32; }
__host__ __device__ constexpr int sx_nsw(int K) { return (sx_ns(K) + 3) / 4; }
__host__ __device__ constexpr int sx_np(int K) { return 1 + sx_nsw(K); }                   // instructions per wave and chunk
__host__ __device__ constexpr int sx_units(int K) { return 1 + (sx_nsw(K) + 3) / 4; }

__device__ __forceinline__ void sx_dma4(const f4* gbase_uniform, unsigned lane_byte_off, unsigned lds_byte_uniform) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2" ::"s"(lds_byte_uniform), "v"(lane_byte_off), "s"(gbase_uniform) : "memory");
}
template <int NPC>
__device__ __forceinline__ void sx_dma_block(const f4* g, unsigned v, unsigned l) {
  static_assert(NPC >= 1 && NPC <= 4, "");
  if constexpr (NPC == 1) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(l), "v"(v), "s"(g) : "memory");
  else if constexpr (NPC == 2) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024" ::"s"(l), "v"(v), "s"(g) : "memory");
  else if constexpr (NPC == 3) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024\n\tglobal_load_lds_dwordx4 %1, %2 offset:2048" ::"s"(l), "v"(v), "s"(g) : "memory");
  else asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024\n\tglobal_load_lds_dwordx4 %1, %2 offset:2048\n\tglobal_load_lds_dwordx4 %1, %2 offset:3072" ::"s"(l), "v"(v), "s"(g) : "memory");
}
template <int K>
__device__ __forceinline__ void sx_copy_unit(int u, const f4* src_chunk, unsigned lane4, unsigned lane16, unsigned bias_dst,
                                             unsigned slot_dst, int wave) {
  constexpr int NS = sx_ns(K), NSW = sx_nsw(K);
  if (u == 0) {
    sx_dma4(src_chunk, lane4, bias_dst);
  } else {
    const int first = wave * NSW < NS - NSW ? wave * NSW : NS - NSW;
    const unsigned sb = (unsigned)(first + 4 * (u - 1)) * 1024u;
    const f4* src = src_chunk + 4 + sb / 16;
    if (NSW - 4 * (u - 1) >= 4) sx_dma_block<4>(src, lane16, slot_dst + sb);
    else if (NSW - 4 * (u - 1) == 3) sx_dma_block<3>(src, lane16, slot_dst + sb);
    else if (NSW - 4 * (u - 1) == 2) sx_dma_block<2>(src, lane16, slot_dst + sb);
    else sx_dma_block<1>(src, lane16, slot_dst + sb);
  }
}
template <int N>
__device__ __forceinline__ void sx_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// exact three-way split of two fp32 values (vis_diffuse_x6.hip): v = h + m 2^-11 + l 2^-22 (the two scalings as v_pk_mul_f32 gave no gain
// and were removed: profiles/r03_sdf_x6_ablation.md)
__device__ __forceinline__ void sx_split_pair(float v0, float v1, float negk, unsigned& h, unsigned& m, unsigned& l) {
  const unsigned hu = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(v0, v1));
  const float s0 = v0 * 2048.0f, s1 = v1 * 2048.0f;
  float d0, d1;
  asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(d0) : "v"(hu), "s"(negk), "v"(s0));
  asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d1) : "v"(hu), "s"(negk), "v"(s1));
  const unsigned mu = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(d0, d1));
  const float e0 = d0 * 2048.0f, e1 = d1 * 2048.0f;
  unsigned lu;
  asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(lu) : "v"(mu), "s"(negk), "v"(e0));
  asm("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lu) : "v"(mu), "s"(negk), "v"(e1));
  h = hu;
  m = mu;
  l = lu;
}
struct SxAcc {
  f4 c0, c1, c2;   // classes 2^0, 2^-11, 2^-22
};
__device__ __forceinline__ void sx_zero_acc(SxAcc& a, const f4& bias) {
  a.c0 = bias;
  a.c1 = f4{0.f, 0.f, 0.f, 0.f};
  a.c2 = f4{0.f, 0.f, 0.f, 0.f};
}
constexpr float SX_C11 = 1.0f / 2048.0f;
__device__ __forceinline__ float sx_combine(const SxAcc& a, int r) { return __builtin_fmaf(__builtin_fmaf(a.c2[r], SX_C11, a.c1[r]), SX_C11, a.c0[r]); }
__device__ __forceinline__ void sx_mfma(f4& acc, const u4& w, const u4& x) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, w), __builtin_bit_cast(h8, x), acc, 0, 0, 0);
}

// The ring: four slots of SLOT_B bytes for the fragments of a unit, four of 256 bytes for its bias.  Slot i of the tables holds unit
// u = i (mod 4) of the CURRENT layer (sx_rotate at the layer's end).
struct SxRing {
  const f4 *ring, *bias_ring;              // the two LDS arrays
  unsigned ring_b, bias_b;                 // ... as LDS byte addresses (the copies' destinations)
  unsigned slot_b[4], bslot_b[4];          // byte offsets of the slots
  unsigned lane16, lane4;
  int lane, g, wave;
};
template <int SLOT_B>
__device__ __forceinline__ SxRing sx_ring(const f4* ring, const f4* bias_ring, int lane, int wave) {
  SxRing rg;
  rg.ring = ring;
  rg.bias_ring = bias_ring;
  rg.ring_b = (unsigned)(unsigned long)((__attribute__((address_space(3))) char*)ring);
  rg.bias_b = (unsigned)(unsigned long)((__attribute__((address_space(3))) char*)bias_ring);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    rg.slot_b[i] = (unsigned)i * SLOT_B;
    rg.bslot_b[i] = (unsigned)i * 256u;
  }
  rg.lane16 = (unsigned)lane * 16u;
  rg.lane4 = (unsigned)lane * 4u;
  rg.lane = lane;
  rg.g = lane >> 4;
  rg.wave = wave;
  return rg;
}
__device__ __forceinline__ const u4* sx_frag_of(const SxRing& rg, int u) {      // this lane's fragments of unit u of the layer
  return reinterpret_cast<const u4*>(reinterpret_cast<const char*>(rg.ring) + rg.slot_b[u & 3]) + rg.lane;
}
__device__ __forceinline__ f4 sx_bias_of(const SxRing& rg, int u) {
  return *(reinterpret_cast<const f4*>(reinterpret_cast<const char*>(rg.bias_ring) + rg.bslot_b[u & 3]) + rg.g);
}
template <int R>
__device__ __forceinline__ void sx_rotate(SxRing& rg) {      // slot 0 = the slot of unit R
  unsigned a[4], b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[i] = rg.slot_b[(i + R) & 3];
    b[i] = rg.bslot_b[(i + R) & 3];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    rg.slot_b[i] = a[i];
    rg.bslot_b[i] = b[i];
  }
}
// units 0, 1, 2 of the stream (all of the first layer: K0) into slots 0, 1, 2; src_of(c) = the unit's chunk head in the blob
template <int K0, class SrcOf>
__device__ __forceinline__ void sx_prologue(const SxRing& rg, SrcOf&& src_of) {
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int un = 0; un < sx_units(K0); ++un)
      sx_copy_unit<K0>(un, src_of(c), rg.lane4, rg.lane16, rg.bias_b + rg.bslot_b[c], rg.ring_b + rg.slot_b[c], rg.wave);
  sx_wait<0>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

struct SxSrc {
  const f4* chunk;
  int K;
};
template <int... K>
struct SxKs {};
template <int K0, int... Kn, class F>
__device__ __forceinline__ void sx_for_k(SxKs<K0, Kn...>, int K, F&& f) {      // f(integral_constant<int, K>) for the K of the list (the last: any other)
  if constexpr (sizeof...(Kn) == 0) f(std::integral_constant<int, K0>{});
  else if (K == K0) f(std::integral_constant<int, K0>{});
  else sx_for_k(SxKs<Kn...>{}, K, f);
}

// One layer (see the head of this file).  accs: the units' accumulators, alternating (the caller finishes the layer's last unit from
// accs[(NU - 1) & 1]); xh / xm / xl: the layer's operands by k-block.
//   wait(u)        in the middle of unit u, before the barrier: unit u + 1 must have landed -- this wave's younger loads (the copies of
//                  unit u + 2, whatever else the kernel issued) may stay in flight;
//   next(u3)       unit u3 = u + 3 of the layer (>= NU: the units behind it in the stream): its chunk head in the blob and its K, one of
//                  the stream's unit sizes Ks = SxKs<...>; the engine places the unit's sx_units(K) copy blocks over the k-blocks of the
//                  unit's second half;
//   filler(u, kb)  behind the MFMAs of k-block kb of unit u.
template <int KB, int NU, int BS, int DB, class Ks, int NX, class Wait, class Next, class Filler>
__device__ __forceinline__ void sx_layer(SxRing& rg, SxAcc (&accs)[2], const u4 (&xh)[NX], const u4 (&xm)[NX], const u4 (&xl)[NX],
                                         Wait&& wait, Next&& next, Filler&& filler) {
  constexpr int D = BS * DB, NB = BS * (DB + 1), HB = KB / 2, NSTEP = NU * KB;
  static_assert(D + BS - 1 <= KB - HB, "reads of the next unit start after the barrier");
  static_assert(KB <= NX, "");
  f4 bnext = f4{0.f, 0.f, 0.f, 0.f};
  u4 wfh[NB], wfm[NB], wfl[NB];
  sx_zero_acc(accs[0], sx_bias_of(rg, 0));
#pragma unroll
#ifdef SX_ABL_NOREAD
  for (int i = 0; i < NB; ++i)
#else
  for (int i = 0; i < D; ++i)
#endif
    if (i < NSTEP) {
      const u4* f = sx_frag_of(rg, i / KB) + (3 * (i % KB)) * 64;
      wfh[i % NB] = f[0];
      wfm[i % NB] = f[64];
      wfl[i % NB] = f[128];
    }
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    SxAcc& acc = accs[u & 1];
    if (u > 0) sx_zero_acc(acc, bnext);
    const SxSrc nx3 = next(u + 3);
    const int sl3 = (u + 3) & 3;
    const unsigned dst3 = rg.ring_b + rg.slot_b[sl3], bdst3 = rg.bias_b + rg.bslot_b[sl3];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const int st = u * KB + kb;
      if (kb == HB) {
        wait(u);
#ifndef SX_ABL_NOBAR
        __builtin_amdgcn_s_barrier();
#endif
        asm volatile("" ::: "memory");
        bnext = sx_bias_of(rg, u + 1);
      }
      if (st % BS == 0) {
#pragma unroll
        for (int i = BS - 1; i >= 0; --i) {
          const int s2 = st + D + i;
#ifdef SX_ABL_NOREAD                  // the registers are redefined behind the compiler's back (no instruction)
          if (s2 < NSTEP) asm volatile("" : "+v"(wfl[s2 % NB]), "+v"(wfm[s2 % NB]), "+v"(wfh[s2 % NB]));
#else
          if (s2 < NSTEP) {
            const u4* f = sx_frag_of(rg, s2 / KB) + (3 * (s2 % KB)) * 64;
            wfl[s2 % NB] = f[128];
            wfm[s2 % NB] = f[64];
            wfh[s2 % NB] = f[0];
          }
#endif
        }
      }
      // the six products of BS k-blocks, a run per product: class 2 (wl.xh, wm.xm, wh.xl), class 1 (wm.xh, wh.xm), class 0 (wh.xh)
      if (st % BS == BS - 1 || kb == KB - 1) {
        const int k0 = (st % BS == BS - 1) ? (kb - (BS - 1) > 0 ? kb - (BS - 1) : 0) : kb - (st % BS);
#pragma unroll
        for (int k = k0; k <= kb; ++k) sx_mfma(acc.c2, wfl[(u * KB + k) % NB], xh[k]);
#pragma unroll
        for (int k = k0; k <= kb; ++k) sx_mfma(acc.c2, wfm[(u * KB + k) % NB], xm[k]);
#pragma unroll
        for (int k = k0; k <= kb; ++k) sx_mfma(acc.c2, wfh[(u * KB + k) % NB], xl[k]);
#pragma unroll
        for (int k = k0; k <= kb; ++k) sx_mfma(acc.c1, wfm[(u * KB + k) % NB], xh[k]);
#pragma unroll
        for (int k = k0; k <= kb; ++k) sx_mfma(acc.c1, wfh[(u * KB + k) % NB], xm[k]);
#pragma unroll
        for (int k = k0; k <= kb; ++k) sx_mfma(acc.c0, wfh[(u * KB + k) % NB], xh[k]);
      }
      filler(u, kb);
#ifndef SX_ABL_NODMA
      if (kb >= HB)
        sx_for_k(Ks{}, nx3.K, [&](auto K3_tag) {
          constexpr int K3 = decltype(K3_tag)::value, nu3 = sx_units(K3);
#pragma unroll
          for (int un = 0; un < nu3; ++un)
            if ((un * (KB - HB)) / nu3 == kb - HB) sx_copy_unit<K3>(un, nx3.chunk, rg.lane4, rg.lane16, bdst3, dst3, rg.wave);
        });
#endif
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  sx_rotate<NU & 3>(rg);
}

}  // namespace rb
