// Legacy library only: rb_dvis_fused's precision 5, the f16x3 split-precision form of k_dvis_fused -- one tile per wave, two
// workgroups per CU, weights staged by LDS-DMA (global_load_lds).
#include "../../include/robir_hip_legacy.h"
#include "dvis_fused.h"

namespace rb {

int dvis_fused_h3(const float* normals, const int* chunk_id, long n, const float* A, const float* Bd, const float* dirs,
                  const float* wdir, const float* wsum, const float* Whid, const float* wlast, const float* blast, int L, int nsamp,
                  int argmax_vis, int scale_log2, float* vis_out, unsigned long long* eval_count, rb_stream_t stream) {
  hipLaunchKernelGGL((k_dvis_fused<true, 2, 1, true>), dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, normals, chunk_id,
                     n, A, Bd, dirs, wdir, wsum, (const f4*)Whid, wlast, blast, L, nsamp, argmax_vis,
                     ldexpf(1.0f, -scale_log2), vis_out, eval_count,
                     range_flags() ? range_flags() + RB_RANGE_DVIS : nullptr);
  return check_launch("k_dvis_fused");
}

}  // namespace rb
