// Feature rows for the kernels that do not encode their input themselves: PE10 (value and forward-mode tangent rows) and the
// integrated PE.  All pointers are device pointers; nothing allocates.
#include "../../include/robir_hip.h"
#include "common.h"
#include "mlp_engine.h"
#include "pe.h"

namespace rb {

// X[M,64] = [PE10(x*scale) | extra]  (extra = 0, or hdr_shift for the indirect-illumination net)
// jvp != 0: X[4M,64], row 4m = PE, rows 4m+1..3 = dPE/dx, dPE/dy, dPE/dz  (forward-mode SDF gradient)
__global__ void k_feat_pe10(const float* __restrict__ x, long M, float scale, const float* __restrict__ extra, int jvp,
                            float* __restrict__ X) {
  const long rows = jvp ? 4 * M : M;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < rows * 16; t += (long)gridDim.x * blockDim.x) {
    const long row = t >> 4;
    const int q = (int)(t & 15);
    const long i = jvp ? row >> 2 : row;
    const int tangent_of = jvp ? (int)(row & 3) - 1 : -1;
    const float a[3] = {x[3 * i] * scale, x[3 * i + 1] * scale, x[3 * i + 2] * scale};
    const float last = (!jvp && extra) ? extra[i] : 0.f;
    f4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = pe10_feature(a, 4 * q + e, tangent_of, last);
    reinterpret_cast<f4*>(X + row * 64)[q] = v;
  }
}

// Integrated PE, isotropic covariance var*I, full-covariance code path of the reference
// (model/neus_model.py:14-57): [exp(-v_k/2) sin(2^k x_c) (k-major, 30) | exp(-v_k/2) sin(2^k x_c + pi/2) (30)],
// arguments wrapped mod 100*pi when |arg| >= 100*pi.  X[M,64], columns 60..63 zero.
__device__ __forceinline__ float py_mod(float a, float m) {  // torch.remainder: sign of the divisor
  float r = fmodf(a, m);
  if (r != 0.f && ((r < 0.f) != (m < 0.f))) r += m;
  return r;
}
__global__ void k_feat_ipe(const float* __restrict__ x, long M, float var, const float* __restrict__ noise,
                           float noise_scale, float* __restrict__ X) {
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= M) return;
  const float big = (float)(100.0 * 3.14159265358979323846);
  const float half_pi = (float)(0.5 * 3.14159265358979323846);
  float* row = X + i * 64;
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    const float f = (float)(1 << k);
    const float damp = expf(-0.5f * (var * (f * f)));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float y = x[3 * i + c] * f;
      float y2 = y + half_pi;
      float a1 = fabsf(y) < big ? y : py_mod(y, big);
      float a2 = fabsf(y2) < big ? y2 : py_mod(y2, big);
      float e1 = damp * sinf(a1), e2 = damp * sinf(a2);
      if (noise) {
        e1 += noise[i * 60 + 3 * k + c] * noise_scale;
        e2 += noise[i * 60 + 30 + 3 * k + c] * noise_scale;
      }
      row[3 * k + c] = e1;
      row[30 + 3 * k + c] = e2;
    }
  }
  row[60] = row[61] = row[62] = row[63] = 0.f;
}

}  // namespace rb

using namespace rb;

extern "C" {

int rb_feat_pe10(const float* x, long M, float scale, const float* extra, int jvp, float* X, rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(x && X, "null pointer");
  RB_REQUIRE(!(jvp && extra), "extra column not supported with jvp rows");
  const long blocks = ((jvp ? 4 * M : M) * 16 + 255) / 256;
  hipLaunchKernelGGL(k_feat_pe10, dim3((unsigned)(blocks < RB_MAX_BLOCKS ? blocks : RB_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream, x, M,
                     scale, extra, jvp, X);
  return check_launch("k_feat_pe10");
}

int rb_feat_ipe(const float* x, long M, float var, const float* noise, float noise_scale, float* X,
                rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(x && X, "null pointer");
  hipLaunchKernelGGL(k_feat_ipe, grid1d(M, 128), dim3(128), 0, (hipStream_t)stream, x, M, var, noise, noise_scale, X);
  return check_launch("k_feat_ipe");
}

}  // extern "C"
