// The atlas fit's arithmetic for ONE row (taps, fetch), ONE segment (the gather that transposes the fetch) and ONE (texel, channel) element
// (lazy Adam).  No launch geometry and no LDS: the kernels of texfit.hip loop around these bodies, and a host compiler builds them as they
// are (tools/texfit_host.cpp) -- the raster_math.h pattern.  tests/texfit_restatement.py states the same operations in numpy.
//
// Conventions (include/robir_hip_texfit.h): an atlas [R,R,Cs], row 0 at the top, texel = row R + column; a fetch at (u, v):
//   x = u R - 0.5, y = (1 - v) R - 0.5, x0 = floor x, y0 = floor y, wx1 = x - x0, wx0 = (x0 + 1) - x (likewise y),
//   taps nw, ne, sw, se with weights wx0 wy0, wx1 wy0, wx0 wy1, wx1 wy1; value = ((a nw + b ne) + c sw) + d se; zero padding.
// These are the numbers the mesh view's plane fetch forms (raster/raster_math.h: fetch_bilinear / fetch_nearest), so that the forward of the
// fit is the view's forward and its reverse mode is the transpose of exactly that linear map.
// Arithmetic: taps and fetch plain fp32, one rounding per operation (-ffp-contract=off); the gather and Adam in fp64 from the fp32 inputs,
// every stored value rounded once.
#pragma once
#include <math.h>

#ifndef RB_TF_FN
#ifdef __HIPCC__
#define RB_TF_FN __host__ __device__ __forceinline__
#else
#define RB_TF_FN inline
#endif
#endif

namespace rb {
namespace tf {

constexpr int MAX_CHANNELS = 16;

// the four taps of the fetch at (u, v): texel [4] (-1: outside the image), weight [4] (+0 there)
RB_TF_FN void taps_row(float u, float v, int R, int filter, int* texel, float* weight) {
  const float fr = (float)R;
  if (filter == 0) {        // the containing texel, clamped (NaN -> 0)
    const float lim = (float)(R - 1);
    const int c = (int)fminf(fmaxf(floorf(u * fr), 0.0f), lim), r = (int)fminf(fmaxf(floorf((1.0f - v) * fr), 0.0f), lim);
    texel[0] = r * R + c;
    weight[0] = 1.0f;
    for (int k = 1; k < 4; ++k) {
      texel[k] = -1;
      weight[k] = 0.0f;
    }
    return;
  }
  const float x = u * fr - 0.5f, y = (1.0f - v) * fr - 0.5f;
  const float x0 = floorf(x), y0 = floorf(y);
  const float wx1 = x - x0, wx0 = (x0 + 1.0f) - x, wy1 = y - y0, wy0 = (y0 + 1.0f) - y;
  const float w[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
  // x0, y0 beyond the image by more than a texel name no texel: clamp before the conversion so that it cannot overflow (NaN -> -2)
  const int c0 = (int)fminf(fmaxf(x0, -2.0f), fr + 1.0f), r0 = (int)fminf(fmaxf(y0, -2.0f), fr + 1.0f);
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + (k & 1), r = r0 + (k >> 1);
    const bool in = c >= 0 && c < R && r >= 0 && r < R;
    texel[k] = in ? r * R + c : -1;
    weight[k] = in ? w[k] : 0.0f;
  }
}

// out [C] = ((a w0 + b w1) + c w2) + d w3 over the first C of the Cs channels; an absent tap's value is +0 and its product is formed
RB_TF_FN void fetch_row(const float* planes, int R, int Cs, const int* texel, const float* weight, int C, float* out) {
  const long texels = (long)R * R;
  for (int ch = 0; ch < C; ++ch) {
    float val[4];
    for (int k = 0; k < 4; ++k) val[k] = texel[k] >= 0 && texel[k] < texels ? planes[(long)texel[k] * Cs + ch] : 0.0f;
    out[ch] = ((val[0] * weight[0] + val[1] * weight[1]) + val[2] * weight[2]) + val[3] * weight[3];
  }
}

// out [C] = sum over the pairs p0 <= p < p1, in ascending p, of (double) weight (double) g_tex[row]; a row outside [0, n) is passed over
RB_TF_FN void gather_segment(const int* pair_row, const float* pair_weight, long p0, long p1, const float* g_tex, long n, int C, float* out) {
  double acc[MAX_CHANNELS];
  for (int ch = 0; ch < MAX_CHANNELS; ++ch) acc[ch] = 0.0;
  for (long p = p0; p < p1; ++p) {
    const long row = pair_row[p];
    if (row < 0 || row >= n) continue;
    const double w = (double)pair_weight[p];
    for (int ch = 0; ch < C; ++ch) acc[ch] += w * (double)g_tex[row * C + ch];
  }
  for (int ch = 0; ch < C; ++ch) out[ch] = (float)acc[ch];
}

// One element of a lazy Adam step with a clamp: bc1 = 1 - beta1^t, bc2 = 1 - beta2^t.  The moments are formed in fp64 and rounded once; the
// parameter moves by what the STORED moments say, as the optimiser's own tensors would.
RB_TF_FN void adam_element(float& p, float& m, float& v, double g, double lr, double lo, double hi, double beta1, double beta2, double eps,
                           double bc1, double bc2) {
  m = (float)(beta1 * (double)m + (1.0 - beta1) * g);
  v = (float)(beta2 * (double)v + (1.0 - beta2) * (g * g));
  const double step = lr * ((double)m / bc1) / (sqrt((double)v / bc2) + eps);
  p = (float)fmin(fmax((double)p - step, lo), hi);
}

}  // namespace tf
}  // namespace rb
