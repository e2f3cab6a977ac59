// The first-generation light-visibility kernel (see vis_diffuse.hip for the scheme): H3 = false, the fp32-MFMA form rb_dvis_fused
// launches for precision 0 (vis_diffuse.hip); H3 = true, the f16x3 split-precision form of precision 5 (vis_diffuse_h3.hip).
#pragma once
#include "dvis_tiles.h"
#include "mlp_engine.h"

namespace rb {

// rb_dvis_fused with precision 5, after its argument checks.  The legacy library launches the kernel (vis_diffuse_h3.hip); the
// default library links a refusal in its place (vis_diffuse_h3_stub.hip).
int dvis_fused_h3(const float* normals, const int* chunk_id, long n, const float* A, const float* Bd, const float* dirs,
                  const float* wdir, const float* wsum, const float* Whid, const float* wlast, const float* blast, int L, int nsamp,
                  int argmax_vis, int scale_log2, float* vis_out, unsigned long long* eval_count, rb_stream_t stream);

template <bool H3, int CH, int NT, bool DMA = false>
__global__ __launch_bounds__(256, NT == 1 ? 2 : 1) void k_dvis_fused(
    const float* __restrict__ normals, const int* __restrict__ cid, long n, const float* __restrict__ A,
    const float* __restrict__ Bd, const float* __restrict__ dirs, const float* __restrict__ wdir,
    const float* __restrict__ wsum, const f4* __restrict__ Whid, const float* __restrict__ wlast,
    const float* __restrict__ blast, int L, int nsamp, int argmax_vis, float w_unscale, float* __restrict__ vis_out,
    unsigned long long* __restrict__ eval_count, unsigned* __restrict__ range_word) {
  unsigned sat = 0u;   // range sentinel of the split-precision path (operands are ReLU outputs: >= 0)
  __shared__ f4 lds_w[(H3 ? 3 : 2) * chunk_f4(256)];
  __shared__ float vis_tab[DVIS_MAX_DIRS];
  __shared__ unsigned short idx_list[DVIS_MAX_DIRS];
  __shared__ f4 a_row[64];
  __shared__ f4 w_last[128];  // [2][256]
  __shared__ int s_count;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const long p = blockIdx.x;
  const int LS = L * nsamp;
  const long dbase = (cid ? (long)cid[p] : 0L) * LS;
  if (tid == 0) s_count = 0;
  if (tid < 64) a_row[tid] = reinterpret_cast<const f4*>(A + p * 256)[tid];
  if (tid < 128) w_last[tid] = reinterpret_cast<const f4*>(wlast)[tid];
  for (int j = tid; j < LS; j += 256) vis_tab[j] = 0.f;
  __syncthreads();
  // ---- cull + compaction (order inside the list is irrelevant: results are scattered by direction index)
  const float nx = normals[3 * p], ny = normals[3 * p + 1], nz = normals[3 * p + 2];
  for (int j0 = 0; j0 < LS; j0 += 256) {
    const int j = j0 + tid;
    bool front = false;
    if (j < LS) {
      const float* d = dirs + 3 * (dbase + j);
      const float c = nx * d[0] + ny * d[1] + nz * d[2];  // sum(n*d): separate mul/add (-ffp-contract=off)
      front = c > RB_TINY;
    }
    const unsigned long long m = __ballot(front);
    int base = 0;
    if (lane == 0 && m) base = atomicAdd(&s_count, __popcll(m));
    base = __shfl(base, 0);
    if (front) idx_list[base + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)j;
  }
  __syncthreads();
  const int S = s_count;
  if (tid == 0 && eval_count) atomicAdd(eval_count, (unsigned long long)S);

  WStream<256> ws;
  H3Ring<NT, 48, DMA> ring;
  constexpr long LF = (long)16 * chunk_f4(256);
  const float b0 = blast[0], b1 = blast[1];
  constexpr int RS = 64 * NT;   // samples per workgroup round
  const int rounds = (S + RS - 1) / RS;
  if constexpr (H3) {
    if (rounds > 0) ring.start(lds_w, Whid, tid);
  } else {
    ws.init(lds_w, tid);
    if (rounds > 0) ws.prime<chunk_f4(256)>(Whid);
  }
  for (int rd = 0; rd < rounds; ++rd) {
    float z[NT][64];    // pre-activation of the last hidden layer (fp32 path: every layer)
    int jj[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int si = rd * RS + wave * (16 * NT) + t * 16 + (lane & 15);
      jj[t] = si < S ? (int)idx_list[si] : -1;
    }
    if constexpr (!H3) {
      float h[NT][64];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int j = jj[t] < 0 ? 0 : jj[t];
        const f4* brow = reinterpret_cast<const f4*>(Bd + (dbase + j) * 256) + g;
#pragma unroll
        for (int kb = 0; kb < 16; ++kb) {
          const f4 bv = brow[kb * 4];
          const f4 av = a_row[kb * 4 + g];
#pragma unroll
          for (int r = 0; r < 4; ++r) h[t][kb * 4 + r] = fmaxf(av[r] + bv[r], 0.f);
        }
      }
#pragma unroll 1
      for (int l = 0; l < 3; ++l) {
        const f4* wl = Whid + l * LF;
        const f4* wn = (l < 2) ? wl + LF : Whid;  // wrap: the next round starts again at hidden layer 0
        dense_layer<256, 256, NT, 256>(ws, wl, wn, h, z, lane, true);
        if (l < 2) activate<256, NT, ACT_RELU>(z, h);
      }
    } else {
      // split-precision hidden stack: activations travel as packed hi/lo halves, accumulators are fp32
      unsigned xh[NT][8][4], xl[NT][8][4];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int j = jj[t] < 0 ? 0 : jj[t];
        const f4* brow = reinterpret_cast<const f4*>(Bd + (dbase + j) * 256) + g;
#pragma unroll
        for (int kb = 0; kb < 16; ++kb) {
          const f4 bv = brow[kb * 4];
          const f4 av = a_row[kb * 4 + g];
#pragma unroll
          for (int q = 0; q < 2; ++q)
            split_pair(fmaxf(av[2 * q] + bv[2 * q], 0.f), fmaxf(av[2 * q + 1] + bv[2 * q + 1], 0.f),
                       xh[t][kb / 2][(kb & 1) * 2 + q], xl[t][kb / 2][(kb & 1) * 2 + q]);
        }
      }
#pragma unroll 1
      for (int l = 0; l < 3; ++l) {
        if (l > 0) relu_split<256, NT>(z, w_unscale, xh, xl);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int kb = 0; kb < 8; ++kb)
#pragma unroll
            for (int q = 0; q < 4; ++q) sat = sat_acc_nonneg(sat, xh[t][kb][q]);
#pragma unroll
        for (int jb = 0; jb < 16; ++jb) {
          f4 res[NT];
          ring.template chunk<CH>(xh, xl, res);
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) z[t][jb * 4 + r] = res[t][r];
        }
      }
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 64; ++i) z[t][i] = z[t][i] * w_unscale;
    }
    // 256 -> 2 head on the VALU: each lane owns 64 of the 256 activations of its sample
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      float l0 = 0.f, l1 = 0.f;
#pragma unroll
      for (int kb = 0; kb < 16; ++kb) {
        const f4 wa = w_last[kb * 4 + g];
        const f4 wb = w_last[64 + kb * 4 + g];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float hv = fmaxf(z[t][kb * 4 + r], 0.f);
          l0 += hv * wa[r];
          l1 += hv * wb[r];
        }
      }
      l0 += __shfl_xor(l0, 16);
      l0 += __shfl_xor(l0, 32);
      l1 += __shfl_xor(l1, 16);
      l1 += __shfl_xor(l1, 32);
      l0 += b0;
      l1 += b1;
      if (g == 0 && jj[t] >= 0) vis_tab[jj[t]] = dvis_value(l0, l1, argmax_vis);
    }
  }
  if constexpr (H3) range_report<true>(sat, range_word);
  // drain the weight ring (the LDS-DMA variant still has chunks in flight that target this workgroup's LDS)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid < L) {
    const float* w = wdir + dbase + (long)tid * nsamp;
    float acc = 0.f;
    for (int k = 0; k < nsamp; ++k) acc += vis_tab[tid * nsamp + k] * w[k];
    vis_out[p * L + tid] = acc / wsum[(cid ? cid[p] : 0) * L + tid];
  }
}

}  // namespace rb
