// Device-side positional-encoding helpers of the feature-row kernels (feat.hip, legacy_rows.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace rb {

// =====================================================================================================
// Feature construction (positional encodings).  Accurate sinf/cosf: arguments reach 2^9*|x|.
// PE layout (model/embedder.py:17-38): [x(3) | sin(2^0 x)(3) | cos(2^0 x)(3) | sin(2^1 x)(3) | ...].
// =====================================================================================================
template <int L>
__device__ __forceinline__ void write_pe(const float x[3], float* __restrict__ dst) {
  dst[0] = x[0];
  dst[1] = x[1];
  dst[2] = x[2];
#pragma unroll
  for (int k = 0; k < L; ++k) {
    const float f = (float)(1 << k);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = x[c] * f;
      float sn, cs;
      sincosf(a, &sn, &cs);                  // one argument reduction for both (same values as sinf / cosf)
      dst[3 + 6 * k + c] = sn;
      dst[3 + 6 * k + 3 + c] = cs;
    }
  }
}
// d(PE)/dx_c : only the components of coordinate c are non-zero.
template <int L>
__device__ __forceinline__ void write_pe_tangent(const float x[3], int c, float* __restrict__ dst) {
#pragma unroll
  for (int i = 0; i < 3 + 6 * L; ++i) dst[i] = 0.f;
  dst[c] = 1.f;
#pragma unroll
  for (int k = 0; k < L; ++k) {
    const float f = (float)(1 << k);
    const float a = x[c] * f;
    float sn, cs;
    sincosf(a, &sn, &cs);
    dst[3 + 6 * k + c] = f * cs;
    dst[3 + 6 * k + 3 + c] = -f * sn;
  }
}

// Sixteen threads per row, one float4 of the row each: the stores of a wave are 4 x 256 contiguous bytes (a thread per row wrote
// 64 floats 256 B apart from its neighbours': 0.29 ms per 2^20 rows, neither compute- nor bandwidth-bound).  Every feature is the
// same sincosf of the same argument as before: identical rows.
__device__ __forceinline__ float pe10_feature(const float a[3], int f, int tangent_of /* -1: value row */, float last) {
  if (f == 63) return tangent_of < 0 ? last : 0.f;
  if (f < 3) return tangent_of < 0 ? a[f] : (f == tangent_of ? 1.f : 0.f);
  const int k = (f - 3) / 6, r = (f - 3) - 6 * k, c = r >= 3 ? r - 3 : r;
  if (tangent_of >= 0 && c != tangent_of) return 0.f;
  const float fr = (float)(1 << k);
  float sn, cs;
  sincosf((c == 0 ? a[0] : (c == 1 ? a[1] : a[2])) * fr, &sn, &cs);
  if (tangent_of < 0) return r >= 3 ? cs : sn;
  return r >= 3 ? -fr * sn : fr * cs;
}

}  // namespace rb
