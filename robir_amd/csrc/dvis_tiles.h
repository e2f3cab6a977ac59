// What the light-visibility kernels share (get_diffuse_visibility, model/sg_render.py:111-195): the visibility of a pair from its two
// logits, and the persistent tile-list ("stream") form's plumbing -- the tile record, the two passes around the persistent kernel
// (dvis_tiles.hip) and the host side of a launch.  k_dvis_x6t<stream> (vis_diffuse_x6t.hip), k_dvis_f16t / k_dvis_f16t2
// (vis_diffuse_f16t.hip) and the legacy k_dvis3_stream (vis_diffuse_v3.hip) are the persistent kernels.
#pragma once
#include "../../include/robir_hip.h"
#include "common.h"

namespace rb {

#define RB_TINY 1e-6f
constexpr int DVIS_MAX_DIRS = 4096;     // directions of a point (L * nsamp): the per-point tables in the LDS, 16-bit direction indices

// record of a 16-sample tile of the global list
struct DvisTile {
  int point;       // -1: no such tile
  int dir_base;    // first row of the point's chunk in dirs / Bd (chunk id * L * nsamp)
};

// k_dvis3_cull: counters[0] = tiles allocated so far (atomic), counters[1] = surviving pairs (statistics)
__global__ void k_dvis3_cull(const float* __restrict__ normals, const int* __restrict__ cid, long n, const float* __restrict__ dirs, int LS,
                             unsigned short* __restrict__ pair_j, DvisTile* __restrict__ tile_info, int2* __restrict__ point_info,
                             unsigned long long* __restrict__ counters, unsigned long long* __restrict__ eval_count);
__global__ void k_dvis3_reduce(const int* __restrict__ cid, long n, const float* __restrict__ wdir, const float* __restrict__ wsum,
                               const unsigned short* __restrict__ pair_j, const float* __restrict__ pair_vis,
                               const int2* __restrict__ point_info, int L, int nsamp, float* __restrict__ vis_out);

// visibility of a (point, direction) pair from the two logits of the network's head: softmax(l)[1], or its argmax
__device__ __forceinline__ float dvis_value(float l0, float l1, int argmax_vis) {
  if (argmax_vis) return l1 > l0 ? 1.f : 0.f;
  const float mx = fmaxf(l0, l1);
  const float e0 = expf(l0 - mx), e1 = expf(l1 - mx);
  return e1 / (e0 + e1);
}

// Host side of a tile-list launch: the checks, zeroed counters, cull | the persistent kernel (launch(tiles, workgroups, stream), named
// `kernel` in a launch error) | reduce.  fn = the entry point (it heads the error text); format_error: what is wrong with the weight
// blob's format word, nullptr if nothing.  n_workgroups <= 0: one workgroup per compute unit.
template <class Launch>
int dvis_tile_list_launch(const char* fn, const char* format_error, const char* kernel, const float* normals, const int* chunk_id, long n,
                          const float* A, const float* Bd, const float* dirs, const float* wdir, const float* wsum, const float* W49, int L,
                          int nsamp, unsigned short* pair_j, float* pair_vis, int* tile_info, int* point_info, unsigned long long* counters,
                          int n_workgroups, float* vis_out, unsigned long long* eval_count, rb_stream_t stream, Launch&& launch) {
#define DVIS_REQUIRE(cond, msg) \
  if (!(cond)) return rb::fail(fn, msg)
  if (n <= 0) return 0;
  DVIS_REQUIRE(normals && A && Bd && dirs && wdir && wsum && W49 && vis_out, "null pointer");
  DVIS_REQUIRE(pair_j && pair_vis && tile_info && point_info && counters, "null scratch pointer");
  DVIS_REQUIRE(n <= RB_MAX_BLOCKS, "too many points for one launch (one workgroup each in the cull / reduce passes)");
  DVIS_REQUIRE(L > 0 && L <= 256 && nsamp > 0 && (long)L * nsamp <= DVIS_MAX_DIRS && (L * nsamp) % 16 == 0,
               "need L <= 256, L*nsamp <= 4096 and a multiple of 16");
  DVIS_REQUIRE((long)n * (L * nsamp / 16) < (1L << 31), "tile index would overflow 31 bits");
  DVIS_REQUIRE(!format_error, format_error);
  hipStream_t s = (hipStream_t)stream;
  if (n_workgroups <= 0) n_workgroups = device_cus();
  DVIS_REQUIRE(n_workgroups > 0, "device query failed");
#undef DVIS_REQUIRE
  if (hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), s) != hipSuccess) return rb::fail(fn, "memset failed");
  DvisTile* const tiles = reinterpret_cast<DvisTile*>(tile_info);
  hipLaunchKernelGGL(k_dvis3_cull, dim3((unsigned)n), dim3(256), 0, s, normals, chunk_id, n, dirs, L * nsamp, pair_j, tiles,
                     reinterpret_cast<int2*>(point_info), counters, eval_count);
  if (int rc = check_launch("k_dvis3_cull")) return rc;
  launch(static_cast<const DvisTile*>(tiles), dim3((unsigned)n_workgroups), s);
  if (int rc = check_launch(kernel)) return rc;
  hipLaunchKernelGGL(k_dvis3_reduce, dim3((unsigned)n), dim3(256), 0, s, chunk_id, n, wdir, wsum, pair_j, pair_vis,
                     reinterpret_cast<const int2*>(point_info), L, nsamp, vis_out);
  return check_launch("k_dvis3_reduce");
}

}  // namespace rb
