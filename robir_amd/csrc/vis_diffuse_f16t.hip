// Light-SG visibility in PLAIN f16 -- one f16 MFMA product per multiply-add, fp32 accumulation: the labelled THROUGHPUT mode
// `BASELINE.json configs[4]` names ("fp16 MLP weights on MFMA"), round 4.  NARROWER than the reference's fp32 and never the default:
// weights are the round-to-nearest f16 of the fp32 weights (the h pieces of the exact-operand blob, rb_pack_layer_x6), activations are
// truncated to f16 between the layers (v_cvt_pkrtz), sums are fp32.  robir_amd/precision.py selects it with ROBIR_PRECISION=f16 only;
// DESIGN.md has its measured error against the oracle.  (get_diffuse_visibility, model/sg_render.py:111-195; VisNetwork,
// model/implicit_differentiable_renderer.py:241-258.)
//
// Machine: the persistent tile-list form of k_dvis_x6t (vis_diffuse_x6t.hip; k_dvis3_cull / k_dvis3_reduce of dvis_tiles.hip around it)
// with FOUR 16-sample tiles per wave -- one-piece operands of four tiles and two layers are 256 registers -- rounds of sixteen tiles, the h
// fragments of a chunk (8 KB) through a four-slot LDS ring, a chunk = four runs of eight MFMAs (one accumulator each), the fragments
// refilled behind the last run, relu + truncation of the previous chunk (four instructions per value pair) between the runs.
#include "dvis_f16_engine.h"

namespace rb {

constexpr int FT_CF4 = 4 + 1536;         // a packed chunk of the exact-operand blob in global memory (bias, then [kb][piece][lane])

struct FtArgs {
  const float *A, *Bd;
  const f4* W49;
  int argmax_vis;
  const unsigned short* pair_j;
  const DvisTile* tile_info;
  const unsigned long long* counters;
  float* pair_vis;
};

__global__ __launch_bounds__(256, 1) void k_dvis_f16t(const FtArgs a) {
  __shared__ f4 ring[4 * F16_WF4];          // 32 KB
  __shared__ f4 headw[F16_WF4];             // 8 KB: chunk 48 (256 -> 2 head)
  __shared__ f4 bias_tab[49 * 4];
  __shared__ f4 a_rows[2 * 16 * 64];        // 32 KB: [round parity][tile of the round][256 floats]
  const float* __restrict__ A = a.A;
  const float* __restrict__ Bd = a.Bd;
  const f4* __restrict__ W49 = a.W49;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = gridDim.x;
  const long total_tiles = (long)a.counters[0];
  const long total_rounds = (total_tiles + 15) >> 4;
  for (int i = tid; i < 49 * 4; i += 256) bias_tab[i] = W49[(long)(i >> 2) * FT_CF4 + (i & 3)];
  for (int i = tid; i < F16_WF4; i += 256) headw[i] = W49[48L * FT_CF4 + 4 + ((i >> 6) * 3) * 64 + (i & 63)];
  __syncthreads();
  if ((long)blockIdx.x >= total_rounds) return;           // workgroup-uniform

  const unsigned ring_b = (unsigned)(unsigned long)((__attribute__((address_space(3))) char*)ring);
  const unsigned arow_b = (unsigned)(unsigned long)((__attribute__((address_space(3))) char*)a_rows);
  unsigned ring_lane = ring_b + (unsigned)lane * 16u;
  asm volatile("" : "+v"(ring_lane));
  // a wave copies the h fragments of k-blocks 2 w, 2 w + 1 of a chunk: 1 KB each, 3 KB apart in the blob, adjacent in the ring
  auto copy_chunk_piece = [&](int i, const f4* chunk_frag0, int slot) {
    xt_dma16_imm<0>(chunk_frag0 + ((2 * wave + i) * 3) * 64, xt_lane16<0>(), ring_b + (unsigned)slot * 8192u + (unsigned)(2 * wave + i) * 1024u);
  };
  u4 wh[8];
  f4 bias;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < 2; ++i) copy_chunk_piece(i, W49 + (long)c * FT_CF4 + 4, c);
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // chunk 0 landed; chunks 1, 2 stay in flight
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
#pragma unroll
  for (int k = 0; k < 8; ++k) wh[k] = ((xt_lds_u4p)ring_lane)[k * 64];
  bias = bias_tab[g];

  F16Ops P, Q;                         // one-piece B operands of the current / next layer, four tiles
  f4 prev[F16_TILES];
  auto ep_tile = [&](int t, int pj) {      // relu + truncation of tile t's sixteen outputs of chunk pj -> the next layer's operands
#pragma unroll
    for (int q = 0; q < 2; ++q)
      Q[t][pj >> 1][(pj & 1) * 2 + q] =
          __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(fmaxf(prev[t][2 * q], 0.f), fmaxf(prev[t][2 * q + 1], 0.f)));
  };

  int jj[F16_TILES];
  F16_TILE_LIST_ROWS
  long rd = blockIdx.x;
  int parity = 0;
  tile_lookup(rd);
  fetch_rows(0);
  for (; rd < total_rounds; rd += G) {
    tile_lookup(rd + G);
    // ---- layer 0: relu(A[point] + Bd[dir]) truncated to f16, straight into the operand registers
#pragma unroll
    for (int t = 0; t < F16_TILES; ++t) {
      jj[t] = jjn[t];
      const f4* arow = a_rows + (parity * 16 + wave * F16_TILES + t) * 64;
#pragma unroll
      for (int kb = 0; kb < 16; ++kb) {
        const f4 bv = raw[t][kb];
        const f4 av = arow[kb * 4 + g];
#pragma unroll
        for (int q = 0; q < 2; ++q)
          P[t][kb / 2][(kb & 1) * 2 + q] = __builtin_bit_cast(
              unsigned, __builtin_amdgcn_cvt_pkrtz(fmaxf(av[2 * q] + bv[2 * q], 0.f), fmaxf(av[2 * q + 1] + bv[2 * q + 1], 0.f)));
      }
    }
#pragma unroll 1
    for (int l = 0; l < 3; ++l) {
      const f4* Wl = W49 + (long)l * 16 * FT_CF4 + 4;
      const f4* Wn = W49 + (long)(l == 2 ? 0 : l + 1) * 16 * FT_CF4 + 4;
#pragma unroll
      for (int jb = 0; jb < 16; ++jb) {
        f4 acc[F16_TILES];
        // chunk jb+1 has landed once at most this wave's two copies of chunk jb+2 are in flight; past the barrier every wave has finished
        // with chunk jb-1, whose slot the copies of chunk jb+3 reuse
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const int nx3 = jb + 3;
        const f4* dsrc = nx3 < 16 ? Wl + (long)nx3 * FT_CF4 : Wn + (long)(nx3 - 16) * FT_CF4;
        const xt_lds_u4p nfrag = (xt_lds_u4p)(ring_lane + (unsigned)((jb + 1) & 3) * 8192u);
        const f4 nbias = bias_tab[(l * 16 + jb + 1) * 4 + g];
        const bool down = (jb & 1) != 0;        // alternate the walking direction: a chunk starts with the fragment requested last
#pragma unroll
        for (int t = 0; t < F16_TILES; ++t) {
          acc[t] = bias;
#pragma unroll
          for (int k_ = 0; k_ < 8; ++k_) {
            const int k = down ? 7 - k_ : k_;
            F16_MFMA(acc[t], wh[k], P[t][k]);
            if (t == F16_TILES - 1) wh[k] = nfrag[k * 64];
          }
          if (t < 2) copy_chunk_piece(t, dsrc, nx3 & 3);
          if (jb > 0) ep_tile(t, jb - 1);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int t = 0; t < F16_TILES; ++t) prev[t] = acc[t];
        bias = nbias;
      }
#pragma unroll
      for (int t = 0; t < F16_TILES; ++t) ep_tile(t, 15);
#pragma unroll
      for (int t = 0; t < F16_TILES; ++t)
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) P[t][kb] = Q[t][kb];
    }
    // ---- head: chunk 48 from its resident LDS copy; next round's rows are requested first
    fetch_rows(parity ^ 1);
    {
      const xt_lds_u4p hw = (xt_lds_u4p)((unsigned)(unsigned long)((__attribute__((address_space(3))) char*)headw) + (unsigned)lane * 16u);
      f4 acc[F16_TILES];
#pragma unroll
      for (int t = 0; t < F16_TILES; ++t) acc[t] = bias;
#pragma unroll
      for (int kb = 0; kb < 8; ++kb) {
        const u4 fh = hw[kb * 64];
#pragma unroll
        for (int t = 0; t < F16_TILES; ++t) F16_MFMA(acc[t], fh, P[t][kb]);
      }
      bias = bias_tab[g];
#pragma unroll
      for (int t = 0; t < F16_TILES; ++t)
        if (g == 0 && jj[t] >= 0) a.pair_vis[(rd * 16 + wave * F16_TILES + t) * 16 + (lane & 15)] = dvis_value(acc[t][0], acc[t][1], a.argmax_vis);
    }
    parity ^= 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Second generation (round 5).  The first kernel above runs at 0.41 of the f16 pipe WITHOUT reaching the package cap (1212 W of 1400):
// with 32 MFMAs per chunk and wave, what surrounds them decides -- a counted wait + workgroup barrier per chunk, two LDS-DMA copies of
// six issue slots each (the h fragments of a chunk are 3 KB apart in the exact-operand blob: no shared M0), sixteen accumulator moves,
// five vector instructions per value pair of the epilogue, and 128 moves per tile set and layer for the operand hand-over.  The chunk
// machine of dvis_f16_engine.h removes them (steps of two chunks on an eight-slot ring, a weight blob of its own, straight-line layers
// with alternating operand and accumulator sets, relu on pairs); this kernel puts the tile list's rows around it.
// The same products summed in the same order: bit-identical to the first kernel (tests/test_sg_gpu.py).
__global__ __launch_bounds__(256, 1) void k_dvis_f16t2(const FtArgs a) {
  __shared__ f4 ring[F16_SLOTS * F16_WF4];  // slot = chunk % F16_SLOTS
  __shared__ f4 headw[F16_WF4];             // 8 KB: chunk 48 (256 -> 2 head)
  __shared__ f4 bias_tab[49 * 4];
  __shared__ f4 a_rows[2 * 16 * 64];        // 32 KB: [round parity][tile of the round][256 floats]
  const float* __restrict__ A = a.A;
  const float* __restrict__ Bd = a.Bd;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = gridDim.x;
  const long total_tiles = (long)a.counters[0];
  const long total_rounds = (total_tiles + 15) >> 4;
  f16_load_tables(bias_tab, headw, a.W49, tid);           // a.W49: [49][4] biases | [49][8][64] h fragments
  if ((long)blockIdx.x >= total_rounds) return;           // workgroup-uniform

  const unsigned arow_b = (unsigned)(unsigned long)((__attribute__((address_space(3))) char*)a_rows);
  F16Ring ring_s;
  f16_ring_init(ring_s, ring, a.W49, bias_tab, wave, lane);
  F16_RING_PRIME(ring_s)
  f16_ring_start<4 * (F16_DIST - 1)>(ring_s);             // step 0 landed

  F16Ops P, Q;
  int jj[F16_TILES];
  F16_TILE_LIST_ROWS
  long rd = blockIdx.x;
  int parity = 0;
  tile_lookup(rd);
  fetch_rows(0);
  auto no_hook = [](int) { return 0; };
  F16_T_BEGIN
  for (; rd < total_rounds; rd += G) {
    tile_lookup(rd + G);
    F16_T_ROUND
    F16_T(5)
    // ---- layer 0: relu(A[point] + Bd[dir]) truncated to f16, straight into the operand registers
#pragma unroll
    for (int t = 0; t < F16_TILES; ++t) {
      jj[t] = jjn[t];
      const f4* arow = a_rows + (parity * 16 + wave * F16_TILES + t) * 64;
#pragma unroll
      for (int kb = 0; kb < (F16_ABL == 8 ? 1 : 16); ++kb) {
        const f4 bv = raw[t][kb];
        const f4 av = arow[kb * 4 + g];
        P[t][kb / 2][(kb & 1) * 2] = f16_relu_pack(av[0] + bv[0], av[1] + bv[1]);
        P[t][kb / 2][(kb & 1) * 2 + 1] = f16_relu_pack(av[2] + bv[2], av[3] + bv[3]);
      }
#if F16_ABL == 8
#pragma unroll
      for (int kb = 1; kb < 16; ++kb) {
        P[t][kb / 2][(kb & 1) * 2] = __builtin_bit_cast(unsigned, raw[t][kb][0]);
        P[t][kb / 2][(kb & 1) * 2 + 1] = __builtin_bit_cast(unsigned, raw[t][kb][2]);
      }
#endif
    }
    F16_T(0)
    f16_layer(ring_s, P, Q, 0, no_hook);
    F16_T(1)
    f16_layer(ring_s, Q, P, 16, no_hook);
    F16_T(2)
    f16_layer(ring_s, P, Q, 32, no_hook);
    F16_T(3)
    // ---- head, operands in Q; next round's rows are requested first
    fetch_rows(parity ^ 1);
    float l0[F16_TILES], l1[F16_TILES];
    f16_head(ring_s, headw, lane, Q, l0, l1);
#pragma unroll
    for (int t = 0; t < F16_TILES; ++t)
      if (g == 0 && jj[t] >= 0) a.pair_vis[(rd * 16 + wave * F16_TILES + t) * 16 + (lane & 15)] = dvis_value(l0[t], l1[t], a.argmax_vis);
    parity ^= 1;
    F16_T(4)
  }
  F16_T_REPORT("f16t2", "head+fetch")
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

}  // namespace rb

using namespace rb;

extern "C" int rb_dvis_stream_f16(const float* normals, const int* chunk_id, long n, const float* A, const float* Bd,
                                  const float* dirs, const float* wdir, const float* wsum, const float* W49, int L, int nsamp,
                                  int argmax_vis, int scale_log2, unsigned short* pair_j, float* pair_vis, int* tile_info,
                                  int* point_info, unsigned long long* counters, int n_workgroups, float* vis_out,
                                  unsigned long long* eval_count, rb_stream_t stream) {
  // scale_log2 carries the blob format: 0 = the exact-operand blob of rb_dvis_stream_x6 (first kernel: reads its h pieces in place),
  // 1 = the f16 blob (49 x 16 biases, then the h fragments chunk by chunk: packing.pack_vis_f16_head) -> the second-generation kernel
  const char* const format_error =
      scale_log2 == 0 || scale_log2 == 1 ? nullptr
                                         : "scale_log2: 0 = exact-operand blob (first-generation kernel), 1 = f16 blob (second generation)";
  return dvis_tile_list_launch(__func__, format_error, "k_dvis_f16t", normals, chunk_id, n, A, Bd, dirs, wdir, wsum, W49, L, nsamp, pair_j,
                               pair_vis, tile_info, point_info, counters, n_workgroups, vis_out, eval_count, stream,
                               [&](const DvisTile* tiles, dim3 grid, hipStream_t s) {
                                 FtArgs a{};
                                 a.A = A, a.Bd = Bd, a.W49 = (const f4*)W49, a.argmax_vis = argmax_vis;
                                 a.pair_j = pair_j, a.tile_info = tiles, a.counters = counters, a.pair_vis = pair_vis;
                                 hipLaunchKernelGGL(scale_log2 == 1 ? k_dvis_f16t2 : k_dvis_f16t, grid, dim3(256), 0, s, a);
                               });
}
