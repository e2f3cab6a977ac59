// The chunk machine of the plain-f16 light-visibility kernels (the labelled throughput mode: vis_diffuse_f16t.hip has its arithmetic and
// what it is narrower than), written once for the tile-list form's second generation k_dvis_f16t2 (vis_diffuse_f16t.hip) and the
// point-block form k_dvis_f16p (vis_diffuse_f16p.hip).  What differs stays in their sources: where a round's rows come from, the layer-0
// conversion and where the pair values go.
//
// A wave holds the one-piece f16 operands of FOUR 16-sample tiles for the current and the next layer (2 x 4 x 32 registers).  The weights
// are a blob of their own (packing.pack_vis_f16_head: 49 x 16 biases, then the h fragments of the 49 chunks, 8 KB each, contiguous): a
// chunk = 16 output neurons x 256 = [k-block 8][lane 64] x 16 B.  The 48 hidden chunks stream cyclically through an eight-slot LDS ring
// (slot = chunk % 8) by LDS-DMA, a wave copying the 2 KB of k-blocks 2 w, 2 w + 1 (one M0 setting, two copies); chunk 48, the 256 -> 2
// head, is resident in the LDS.
//   * STEPS of two chunks: one counted wait + workgroup barrier per 64 MFMAs; the copies of step s + F16_DIST are issued at the top of
//     step s, in front of its wait (their slots belong to step s - 2, which every wave has left: it passed barrier s - 1);
//   * the three hidden layers straight-line with the operand sets changing roles (no hand-over moves), two fragment sets and two
//     accumulator sets alternating by chunk parity (no accumulator moves: a chain starts from the bias registers);
//   * k-block outermost, the four tiles inside: consecutive MFMAs never share an accumulator (a vector instruction between two MFMAs of
//     ONE accumulator chain costs ~43 cycles, between different chains ~6), and each k-step carries its share of the other work: one
//     fragment read of the next chunk, relu + truncation of one value pair of the previous chunk;
//   * relu AFTER the truncation, on pairs (v_cvt_pkrtz + v_pk_max_f16: max(rtz(x), 0) = rtz(max(x, 0)));
//   * odd chunks walk their k-blocks downwards: the summation order of the first generation, k_dvis_f16t -- the three kernels give the
//     same bits per pair (tests/test_sg_gpu.py).
// Timing switches (wrong results or extra output; tools/build_variant.sh): -DF16_ABL=<bits> 1 no copies / barriers, 2 no fragment reads,
// 4 no epilogue of the hidden chunks, 8 (alone) no layer-0 conversion in k_dvis_f16t2; -DF16_TIMING s_memtime phase stamps; -DF16_NS=<slots>.
#pragma once
#include "dvis_tiles.h"
#include "mlp_engine.h"
#include "x6_ring.h"
#include "x6t_engine.h"

namespace rb {

constexpr int F16_WF4 = 512;                   // h fragments of a chunk: [kb 8][lane 64] x 16 B = 8 KB
constexpr int F16_TILES = 4;
constexpr int F16_BIAS_F4 = 49 * 4;            // the blob's bias head, in float4
#ifndef F16_NS
#define F16_NS 8
#endif
#ifndef F16_ABL
#define F16_ABL 0
#endif
constexpr int F16_SLOTS = F16_NS;              // ring slots (8 KB each): 48 % F16_SLOTS == 0
constexpr int F16_DIST = F16_SLOTS / 2 - 2;    // the copies of step s + F16_DIST are issued at the top of step s
static_assert(48 % F16_SLOTS == 0 && F16_SLOTS % 2 == 0 && F16_DIST >= 1, "ring");

// phase stamps: F16_T_BEGIN in front of the round loop, F16_T_ROUND at the top of a round, F16_T(i) behind phase i, F16_T_REPORT at the end
#ifdef F16_TIMING
#define F16_T_BEGIN                                                                              \
  unsigned long long tacc[6] = {0, 0, 0, 0, 0, 0}, tlast = __builtin_amdgcn_s_memtime(); \
  int trounds = 0;
#define F16_T_ROUND ++trounds;
#define F16_T(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); tacc[i] += t_ - tlast; tlast = t_; }
#define F16_T_REPORT(NAME, HEAD)                                                                                                                  \
  if ((blockIdx.x == 0 || blockIdx.x == 100) && threadIdx.x == 0)                                                                                 \
    printf(NAME " wg %d rounds %d cycles/round: conv %llu L1 %llu L2 %llu L3 %llu " HEAD " %llu lookup %llu\n", (int)blockIdx.x, trounds,       \
           tacc[0] / trounds, tacc[1] / trounds, tacc[2] / trounds, tacc[3] / trounds, tacc[4] / trounds, tacc[5] / trounds);
#else
#define F16_T_BEGIN
#define F16_T_ROUND
#define F16_T(i)
#define F16_T_REPORT(NAME, HEAD)
#endif

typedef _Float16 f16_h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned f16_relu_pack(float a, float b) {      // relu after the truncation, on the pair
  const f16_h2 h = __builtin_bit_cast(f16_h2, __builtin_amdgcn_cvt_pkrtz(a, b));
  const f16_h2 z = f16_h2{(_Float16)0.0f, (_Float16)0.0f};
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(h, z));
}

#define F16_MFMA(ACC, WREG, XREG) \
  ACC = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, WREG), __builtin_bit_cast(h8, XREG), ACC, 0, 0, 0)

typedef u4 F16Ops[F16_TILES][8];              // the B operands of a layer: four tiles x eight k-blocks, one 128-bit tuple each

struct F16Ring {
  const f4* Wf;                   // the blob's fragments: chunk c at Wf + c F16_WF4
  const f4* bias_tab;             // LDS: [49][4]
  unsigned ring_b, ring_lane;     // the ring's LDS address (+ lane 16)
  int wave, g;
  u4 wh[2][8];                    // the fragments of the current chunk and of the next one, by chunk parity
  f4 bias;                        // the bias of the chunk to come
};

// the bias table and the head chunk -> the LDS
__device__ __forceinline__ void f16_load_tables(f4* bias_tab, f4* headw, const f4* W, int tid) {
  for (int i = tid; i < 49 * 4; i += 256) bias_tab[i] = W[i];
  for (int i = tid; i < F16_WF4; i += 256) headw[i] = W[F16_BIAS_F4 + 48L * F16_WF4 + i];
  __syncthreads();
}
// this wave's 2 KB (k-blocks 2 w, 2 w + 1) of chunk c -> slot c % F16_SLOTS: one M0 setting, two copies
__device__ __forceinline__ void f16_copy_chunk(const F16Ring& r, int c, unsigned lv) {
  const f4* src = r.Wf + (long)c * F16_WF4 + (2 * r.wave) * 64;
  xt_dma16_imm<0>(src, lv, r.ring_b + (unsigned)(c % F16_SLOTS) * 8192u + (unsigned)(2 * r.wave) * 1024u);
  xt_dma16_keep<1024>(src, lv);
}
// The ring's prologue: f16_ring_init, the copies of steps 0 .. F16_DIST - 1 (F16_RING_PRIME), then -- behind whatever else the kernel
// requests first -- f16_ring_start: the wait that leaves at most WAIT copies in flight, the barrier and the fragments of chunk 0.
// (The prologue's copies are a macro: as a function, the same four statements moved k_dvis_f16t2's register allocation,
// profiles/dvis_f16_engine_refactor.md.)
__device__ __forceinline__ void f16_ring_init(F16Ring& r, f4* ring, const f4* W, const f4* bias_tab, int wave, int lane) {
  r.Wf = W + F16_BIAS_F4, r.bias_tab = bias_tab, r.wave = wave, r.g = lane >> 4;
  r.ring_b = (unsigned)(unsigned long)((__attribute__((address_space(3))) char*)ring);
  r.ring_lane = r.ring_b + (unsigned)lane * 16u;
  asm volatile("" : "+v"(r.ring_lane));
}
#define F16_RING_PRIME(R)                                                                               \
  {                                                                                                     \
    const unsigned lv_ = xt_lane16<0>();                                                                \
    _Pragma("unroll") for (int c_ = 0; c_ < 2 * F16_DIST; ++c_) f16_copy_chunk(R, c_, lv_);             \
  }
template <int WAIT>
__device__ __forceinline__ void f16_ring_start(F16Ring& r) {
  sx_wait<WAIT>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
#pragma unroll
  for (int k = 0; k < 8; ++k) r.wh[0][k] = ((xt_lds_u4p)r.ring_lane)[k * 64];
#if F16_ABL & 2
#pragma unroll
  for (int k = 0; k < 8; ++k) r.wh[1][k] = ((xt_lds_u4p)r.ring_lane)[k * 64 + 512];
#endif
  r.bias = r.bias_tab[r.g];
}

// One hidden layer: operands X -> outputs Y (the next layer's operands); cb = the layer's first chunk (0, 16, 32).  hook(sb) is called
// behind the barrier of step sb = 0 .. 7 and returns the number of memory operations it issued: they are YOUNGER than the ring copies
// the wait of step sb + 1 is for, which therefore leaves that many more in flight, and older than those of step sb + 2, whose wait
// covers them.
template <class Hook>
__device__ __forceinline__ void f16_layer(F16Ring& r, const F16Ops& X, F16Ops& Y, int cb, Hook&& hook) {
  f4 acc[2][F16_TILES];
  int younger = 0;
#pragma unroll
  for (int sb = 0; sb < 8; ++sb) {
#if !(F16_ABL & 1)
    {   // the copies of step sb + F16_DIST (cyclic over the 48 chunks), then: step sb + 1 has landed once only these are in flight
      const int n4 = (cb + 2 * sb + 2 * F16_DIST) % 48;
      const unsigned lv = xt_lane16<0>();
      f16_copy_chunk(r, n4, lv);
      f16_copy_chunk(r, n4 + 1, lv);
    }
    xt_wait(4 * (F16_DIST - 1) + younger);
    __builtin_amdgcn_s_barrier();
#endif
    asm volatile("" ::: "memory");
    younger = hook(sb);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int jb = 2 * sb + h;
      const xt_lds_u4p nfrag = (xt_lds_u4p)(r.ring_lane + (unsigned)((cb + jb + 1) % F16_SLOTS) * 8192u);
      const f4 nbias = r.bias_tab[(cb + jb + 1) * 4 + r.g];
      // the next chunk's fragments go to the OTHER register set: requested a whole chunk before their first use (step s + 1 has landed
      // by barrier s: the wait above leaves only step s + 2 in flight), no wait on the LDS in front of a chunk
      const u4 (&wc)[8] = r.wh[jb & 1];
      u4 (&wn)[8] = r.wh[(jb & 1) ^ 1];
      f4 (&ac)[F16_TILES] = acc[jb & 1];
      const f4 (&pv)[F16_TILES] = acc[(jb & 1) ^ 1];
#pragma unroll
      for (int k_ = 0; k_ < 8; ++k_) {
        const int k = (jb & 1) ? 7 - k_ : k_;       // k_dvis_f16t's summation order (odd chunks downwards): the same bits per pair
#pragma unroll
        for (int t = 0; t < F16_TILES; ++t) {
          if (k_ == 0) ac[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, wc[k]), __builtin_bit_cast(h8, X[t][k]), r.bias, 0, 0, 0);
          else F16_MFMA(ac[t], wc[k], X[t][k]);
        }
        // the other work of a k-step behind its four MFMAs (one instruction behind EACH MFMA instead: measured the same, 74.1 against 74.4 ms)
#if !(F16_ABL & 2)
        wn[k_] = nfrag[k_ * 64];
#endif
#if F16_ABL & 4
        if (jb > 0) asm volatile("" ::"v"(pv[k_ >> 1]));     // the accumulators stay "used": the MFMAs survive
#endif
        if (jb > 0 && !(F16_ABL & 4)) {
          const int t = k_ >> 1, pj = jb - 1;
          Y[t][pj >> 1][(pj & 1) * 2 + (k_ & 1)] = f16_relu_pack(pv[t][(k_ & 1) * 2], pv[t][(k_ & 1) * 2 + 1]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      r.bias = nbias;
    }
  }
#pragma unroll
  for (int t = 0; t < F16_TILES; ++t) {
    Y[t][7][2] = f16_relu_pack(acc[1][t][0], acc[1][t][1]);
    Y[t][7][3] = f16_relu_pack(acc[1][t][2], acc[1][t][3]);
  }
}

// The head: chunk 48 from its resident LDS copy against operands X; the two logits of this lane's pair of tile t (lanes 0 .. 15 hold
// them) -> l0[t], l1[t].  The ring's bias register is set for the next round's chunk 0.
__device__ __forceinline__ void f16_head(F16Ring& r, const f4* headw, int lane, const F16Ops& X, float (&l0)[F16_TILES], float (&l1)[F16_TILES]) {
  const xt_lds_u4p hw = (xt_lds_u4p)((unsigned)(unsigned long)((__attribute__((address_space(3))) char*)headw) + (unsigned)lane * 16u);
  f4 acc[F16_TILES];
#pragma unroll
  for (int t = 0; t < F16_TILES; ++t) acc[t] = r.bias;
#pragma unroll
  for (int kb = 0; kb < 8; ++kb) {
    const u4 fh = hw[kb * 64];
#pragma unroll
    for (int t = 0; t < F16_TILES; ++t) F16_MFMA(acc[t], fh, X[t][kb]);
  }
  r.bias = r.bias_tab[r.g];
#pragma unroll
  for (int t = 0; t < F16_TILES; ++t) l0[t] = acc[t][0], l1[t] = acc[t][1];
}

// ---- the tile-list form's rows (k_dvis_f16t, k_dvis_f16t2): rounds of sixteen tiles of the global list, four per wave.  Declared in the
// kernel, with a (pair_j, tile_info), A, Bd, arow_b (the LDS address of a_rows), total_rounds, total_tiles, wave, lane and g in scope:
// tile_lookup(round) reads the records and direction indices of the wave's tiles in `round`; fetch_rows(parity) then requests their
// rows: the A rows by LDS-DMA into a_rows[parity][tile of the round][256 floats], the Bd rows into `raw`.  jjn = this lane's direction
// index per tile, -1: padding.  (A macro that declares lambdas, not functions: as functions -- members of a struct that holds the
// state, or free ones that get it by reference, inlined by force or not -- the same statements compiled to another register allocation
// in both kernels, profiles/dvis_f16_engine_refactor.md.)
#define F16_TILE_LIST_ROWS                                                                                                                       \
  f4 raw[F16_TILES][16];                                                                                                                         \
  int jjn[F16_TILES];                                                                                                                            \
  int tpn[F16_TILES], tbn[F16_TILES], jn2[F16_TILES];                                                                                            \
  auto tile_lookup = [&](long round) {                                                                                                           \
    _Pragma("unroll") for (int t = 0; t < F16_TILES; ++t) {                                                                                      \
      const long T = round * 16 + wave * F16_TILES + t;                                                                                          \
      DvisTile rec{-1, 0};                                                                                                                       \
      int j = 0xFFFF;                                                                                                                            \
      if (round < total_rounds && T < total_tiles) {                                                                                             \
        rec = a.tile_info[T];                                                                                                                    \
        j = (int)a.pair_j[T * 16 + (lane & 15)];                                                                                                 \
      }                                                                                                                                          \
      tpn[t] = __builtin_amdgcn_readfirstlane(rec.point);                                                                                        \
      tbn[t] = __builtin_amdgcn_readfirstlane(rec.dir_base);                                                                                     \
      jn2[t] = j;                                                                                                                                \
    }                                                                                                                                            \
  };                                                                                                                                             \
  auto fetch_rows = [&](int parity_next) {                                                                                                       \
    _Pragma("unroll") for (int t = 0; t < F16_TILES; ++t) {                                                                                      \
      const long prow = tpn[t] < 0 ? 0L : (long)tpn[t];                                                                                          \
      xt_dma16_imm<0>(reinterpret_cast<const f4*>(A + prow * 256), xt_lane16<0>(),                                                               \
                      arow_b + (unsigned)(parity_next * 16 + wave * F16_TILES + t) * 1024u);                                                     \
    }                                                                                                                                            \
    _Pragma("unroll") for (int t = 0; t < F16_TILES; ++t) {                                                                                      \
      jjn[t] = (tpn[t] < 0 || jn2[t] == 0xFFFF) ? -1 : jn2[t];                                                                                   \
      const long row = (long)tbn[t] + (jjn[t] < 0 ? 0 : jjn[t]);                                                                                 \
      const f4* brow = reinterpret_cast<const f4*>(Bd + row * 256) + g;                                                                          \
      _Pragma("unroll") for (int kb = 0; kb < 16; ++kb) raw[t][kb] = brow[kb * 4];                                                               \
    }                                                                                                                                            \
  };

}  // namespace rb
