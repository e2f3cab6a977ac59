// SDF value + gradient by reverse mode, the default library's two precisions: a value pass that stores sigmoid(100 z) of every
// hidden pre-activation, one gradient row per point back through the transposed layers (the scheme: sdf_back.hip's header), and the
// contraction with the Jacobian of the positional encoding, k_pe_grad_points below.
#include "../../include/robir_hip.h"
#include "common.h"

namespace rb {

// grad[m, c] = grad_scale * sum_f (gfeat[m,0,f] + gfeat[m,1,f]) * dPE_f/dx_c (model/embedder.py:17-38: [x | sin(2^k x) | cos(2^k x)],
// k = 0..9: d sin(2^k x_c) = 2^k cos(2^k x_c), d cos = -2^k sin), the encoding recomputed from the points: the same sincosf of
// the same argument as the features the value pass used.
__global__ void k_pe_grad_points(const float* __restrict__ gfeat, const float* __restrict__ xyz, float in_scale, long M,
                                 float grad_scale, float* __restrict__ grad) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= 3 * M) return;
  const long m = i / 3;
  const int c = (int)(i - 3 * m);
  const float* gf = gfeat + m * 128;
  const float a = xyz[i] * in_scale;
  float acc = gf[c] + gf[64 + c];
#pragma unroll 1
  for (int k = 0; k < 10; ++k) {
    const float f = (float)(1 << k);
    float sn, cs;
    sincosf(a * f, &sn, &cs);
    const int is = 3 + 6 * k + c, ic = is + 3;
    acc += f * ((gf[is] + gf[64 + is]) * cs - (gf[ic] + gf[64 + ic]) * sn);
  }
  grad[i] = acc * grad_scale;
}

void launch_pe_grad_points(const float* gfeat, const float* xyz, float in_scale, long M, float grad_scale, float* grad, hipStream_t s) {
  const long n = 3 * M;
  hipLaunchKernelGGL(k_pe_grad_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, gfeat, xyz, in_scale, M, grad_scale, grad);
}

}  // namespace rb

using namespace rb;

// The same op at the reference's precision (exact policy): k_sdf_mlp<5> (f32-input MFMA, sigmoid tiles out), k_sdf_back_f32,
// k_pe_grad_points.  scratch: rb_sdf_value_grad_f32_scratch_floats(M) floats.
extern "C" long rb_sdf_value_grad_f32_scratch_floats(long M) {
  const long tiles = (M + 127) / 128 * 8;
  return tiles * (8L * 16 * 64 * 4) + ((M + 127) / 128 * 128) * 128L;
}
extern "C" int rb_sdf_value_grad_f32_points(const float* x, long M, float in_scale, const float* Wp, const float* Wt, const float* w8row,
                                            float out_scale, float grad_scale, float* out0, float* grad, float* scratch,
                                            rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(x && Wp && Wt && w8row && out0 && grad && scratch, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const long tiles = (M + 127) / 128 * 8;
  float* sig = scratch;
  float* gfeat = scratch + tiles * (8L * 16 * 64 * 4);
  int rc = launch_sdf_f32_store(x, M, in_scale, Wp, out_scale, out0, sig, s);
  if (rc) return rc;
  rc = launch_sdf_back_f32(sig, M, Wt, w8row, gfeat, s);
  if (rc) return rc;
  launch_pe_grad_points(gfeat, x, in_scale, M, grad_scale, grad, s);
  return check_launch("k_pe_grad_points");
}

// ... with both passes on exact three-piece operands: same scratch.  two_tile = 0: k_sdf_x6<5> (csrc/sdf_x6.hip, Wp = packing.pack_sdf_x6)
// + k_sdf_back_x6 (csrc/sdf_back_x6.hip, Wt = packing.pack_sdf_back_x6), one 16-row tile per wave; two_tile = 1: k_sdf_x6t<5> +
// k_sdf_back_x6t (csrc/sdf_x6t.hip, sdf_back_x6t.hip; Wt = packing.pack_sdf_back_x6(two_tile=True): W3^T's K padded to 256).
extern "C" int rb_sdf_value_grad_x6_points(const float* x, long M, float in_scale, const float* Wp, const float* Wt, const float* w8row,
                                           float out_scale, float grad_scale, float* out0, float* grad, float* scratch, int two_tile,
                                           rb_stream_t stream) {
  if (M <= 0) return 0;
  RB_REQUIRE(x && Wp && Wt && w8row && out0 && grad && scratch, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const long tiles = (M + 127) / 128 * 8;
  float* sig = scratch;
  float* gfeat = scratch + tiles * (8L * 16 * 64 * 4);
  int rc = two_tile ? launch_sdf_x6t(x, M, in_scale, Wp, 5, out_scale, out0, sig, 0, s) : launch_sdf_x6_store(x, M, in_scale, Wp, out_scale, out0, sig, s);
  if (rc) return rc;
  rc = two_tile ? launch_sdf_back_x6t(sig, M, Wt, w8row, gfeat, s) : launch_sdf_back_x6(sig, M, Wt, w8row, gfeat, s);
  if (rc) return rc;
  launch_pe_grad_points(gfeat, x, in_scale, M, grad_scale, grad, s);
  return check_launch("k_pe_grad_points");
}
