// The multi-view observation arithmetic for ONE (camera, point) pair and ONE point: the inverse projection of the reference's
// inv_camera_params (model/focus_sampler.py:17-30), grid_sample's bilinear fetch with align_corners=True and zero padding, the choice of the
// n_obs largest keys and the weighted colour statistics.  No launch geometry: the kernels of observe.hip call these bodies once per thread,
// and a host compiler builds them as they are (tools/observe_host.cpp) -- the texbake_math.h pattern.  tests/observe_restatement.py states
// the same operations in numpy fp32.
//
// Conventions (include/robir_hip_observe.h):
//   a camera is 24 numbers: its centre c [3], the first three rows of its inverse pose [3][4] (pose_inv is passed as [4][4], the last row is
//     never read) and K [3][3];
//   u runs along the image's W columns, v along its H rows: images are [M, H, W, C] with row 0 first;
//   every sum is associated from the left; plain fp32, one rounding per operation (-ffp-contract=off), IEEE division and square root.
#pragma once
#include <math.h>

#ifndef RB_OB_FN
#ifdef __HIPCC__
#define RB_OB_FN __host__ __device__ __forceinline__
#else
#define RB_OB_FN inline
#endif
#endif

namespace rb {
namespace ob {

constexpr int MAX_OBS = 8;      // candidates one thread of the selection keeps in registers

// view_dir [3], uv [2] and the depth z (positive in front of the camera) of point x seen from the camera (c, pinv, K)
RB_OB_FN void project(const float* x, const float* c, const float* pinv, const float* K, float* dir, float* uv, float& z) {
  const float d0 = x[0] - c[0], d1 = x[1] - c[1], d2 = x[2] - c[2];
  const float len = fmaxf(sqrtf((d0 * d0 + d1 * d1) + d2 * d2), 1e-12f);
  dir[0] = d0 / len;
  dir[1] = d1 / len;
  dir[2] = d2 / len;
  const float p0 = dir[0] + c[0], p1 = dir[1] + c[1], p2 = dir[2] + c[2];
  float row[3];
  for (int i = 0; i < 3; ++i) row[i] = ((pinv[4 * i] * p0 + pinv[4 * i + 1] * p1) + pinv[4 * i + 2] * p2) + pinv[4 * i + 3];
  z = -row[2];
  const float zz = z != 0.0f ? z : 1e-5f;
  const float q0 = row[0] / zz, q1 = -(row[1] / zz), q2 = -(row[2] / zz);
  uv[0] = (K[0] * q0 + K[1] * q1) + K[2] * q2;
  uv[1] = (K[3] * q0 + K[4] * q1) + K[5] * q2;
}

// grid_sample(bilinear, zeros padding, align_corners=True) of an [H, W, C] image at the pixel position (u, v): the coordinate goes through
// grid_sample's normalised form and back in fp32, texels out of the image count as +0 and every product is formed
template <int C>
RB_OB_FN void fetch(const float* img, int H, int W, float u, float v, float* o) {
  const float gx = u / (float)W * 2.0f - 1.0f, gy = v / (float)H * 2.0f - 1.0f;
  const float x = ((gx + 1.0f) / 2.0f) * (float)(W - 1), y = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
  const float x0 = floorf(x), y0 = floorf(y);
  const float wx1 = x - x0, wx0 = (x0 + 1.0f) - x, wy1 = y - y0, wy0 = (y0 + 1.0f) - y;
  const float nw = wx0 * wy0, ne = wx1 * wy0, sw = wx0 * wy1, se = wx1 * wy1;
  // x0, y0 beyond the image by more than a texel contribute nothing: clamp before the conversion so that it cannot overflow (NaN -> -2)
  const int c0 = (int)fminf(fmaxf(x0, -2.0f), (float)W + 1.0f), r0 = (int)fminf(fmaxf(y0, -2.0f), (float)H + 1.0f);
  const bool cin0 = c0 >= 0 && c0 < W, cin1 = c0 + 1 >= 0 && c0 + 1 < W, rin0 = r0 >= 0 && r0 < H, rin1 = r0 + 1 >= 0 && r0 + 1 < H;
  for (int ch = 0; ch < C; ++ch) {
    const float a = rin0 && cin0 ? img[((long)r0 * W + c0) * C + ch] : 0.0f;
    const float b = rin0 && cin1 ? img[((long)r0 * W + c0 + 1) * C + ch] : 0.0f;
    const float c = rin1 && cin0 ? img[((long)(r0 + 1) * W + c0) * C + ch] : 0.0f;
    const float d = rin1 && cin1 ? img[((long)(r0 + 1) * W + c0 + 1) * C + ch] : 0.0f;
    o[ch] = ((a * nw + b * ne) + c * sw) + d * se;
  }
}

// the pair (camera m, point n), written to element e of the outputs: x [N][3]; cam_loc [M][3], pose_inv [M][4][4], K [M][3][3];
// images [M][H][W][C], masks [M][H][W] or null; uv [.][2], view_dir [.][3], rgb [.][C], valid [.]
template <int C>
RB_OB_FN void scatter_pair(int m, long n, long e, const float* x, const float* cam_loc, const float* pose_inv, const float* K,
                           const float* images, const float* masks, int H, int W, float* uv, float* view_dir, float* rgb,
                           unsigned char* valid) {
  float dir[3], p[2], z, col[C];
  project(x + 3 * n, cam_loc + 3 * m, pose_inv + 16 * m, K + 9 * m, dir, p, z);
  const long plane = (long)H * W;
  fetch<C>(images + (long)m * plane * C, H, W, p[0], p[1], col);
  bool ok = p[0] >= 0.0f && p[0] < (float)W && p[1] >= 0.0f && p[1] < (float)H && z > 0.0f;
  if (masks) {
    float mk[1];
    fetch<1>(masks + (long)m * plane, H, W, p[0], p[1], mk);
    ok = ok && mk[0] > 0.5f;
  }
  uv[2 * e] = p[0];
  uv[2 * e + 1] = p[1];
  for (int k = 0; k < 3; ++k) view_dir[3 * e + k] = dir[k];
  for (int ch = 0; ch < C; ++ch) rgb[C * e + ch] = col[ch];
  valid[e] = ok ? 1 : 0;
}

// row k of point n of the gathered form: the pair (index[k][n], n) written to element k N + n; zeros where the index names no camera
template <int C>
RB_OB_FN void gather_pair(int k, long n, long N, int M, const int* index, const float* x, const float* cam_loc, const float* pose_inv,
                          const float* K, const float* images, const float* masks, int H, int W, float* uv, float* view_dir, float* rgb,
                          unsigned char* valid) {
  const long e = (long)k * N + n;
  const int m = index[e];
  if (m >= 0 && m < M) {
    scatter_pair<C>(m, n, e, x, cam_loc, pose_inv, K, images, masks, H, W, uv, view_dir, rgb, valid);
    return;
  }
  uv[2 * e] = uv[2 * e + 1] = 0.0f;
  for (int j = 0; j < 3; ++j) view_dir[3 * e + j] = 0.0f;
  for (int ch = 0; ch < C; ++ch) rgb[C * e + ch] = 0.0f;
  valid[e] = 0;
}

// point n: the cameras of the n_obs largest keys (vis != 0) + 0.01 draws, largest first, ties to the lower camera; -1 where M < n_obs.
// A NaN key is never chosen.  vis, draws [M][N]; index [n_obs][N]; count [N] = the number of cameras with vis != 0
RB_OB_FN void select_point(long n, long N, int M, int n_obs, const unsigned char* vis, const float* draws, int* index, int* count) {
  float keys[MAX_OBS];
  int ids[MAX_OBS];
  for (int k = 0; k < MAX_OBS; ++k) {
    keys[k] = -INFINITY;
    ids[k] = -1;
  }
  int seen = 0;
  for (int m = 0; m < M; ++m) {
    const long e = (long)m * N + n;
    const bool v = vis[e] != 0;
    seen += v ? 1 : 0;
    float ck = (v ? 1.0f : 0.0f) + 0.01f * draws[e];
    int ci = m;
    bool ins = false;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int k = 0; k < MAX_OBS; ++k) {
      if (k < n_obs) {
        ins = ins || ck > keys[k];      // strictly larger: an equal key stays behind the earlier camera
        if (ins) {
          const float tk = keys[k];
          const int ti = ids[k];
          keys[k] = ck;
          ids[k] = ci;
          ck = tk;
          ci = ti;
        }
      }
    }
  }
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int k = 0; k < MAX_OBS; ++k)
    if (k < n_obs) index[(long)k * N + n] = ids[k];
  count[n] = seen;
}

// point n: over the cameras with vis != 0 in ascending order, w = max(-(normal . view_dir), 0) and the colour fetched at the projection:
//   weight = sum w;  mean = (sum w rgb) / weight;  var = max((sum (w rgb) rgb) / weight - mean mean, 0);  count = the cameras with w > 0;
// all zero where weight == 0
template <int C>
RB_OB_FN void accumulate_point(long n, long N, int M, const float* x, const float* normals, const float* cam_loc, const float* pose_inv,
                               const float* K, const float* images, int H, int W, const unsigned char* vis, float* weight, float* mean,
                               float* var, int* count) {
  float sw = 0.0f, s1[C], s2[C];
  for (int ch = 0; ch < C; ++ch) s1[ch] = s2[ch] = 0.0f;
  int cnt = 0;
  const long plane = (long)H * W;
  const float n0 = normals[3 * n], n1 = normals[3 * n + 1], n2 = normals[3 * n + 2];
  for (int m = 0; m < M; ++m) {
    if (!vis[(long)m * N + n]) continue;
    float dir[3], p[2], z, col[C];
    project(x + 3 * n, cam_loc + 3 * m, pose_inv + 16 * m, K + 9 * m, dir, p, z);
    const float w = fmaxf(-((n0 * dir[0] + n1 * dir[1]) + n2 * dir[2]), 0.0f);
    if (!(w > 0.0f)) continue;
    fetch<C>(images + (long)m * plane * C, H, W, p[0], p[1], col);
    sw = sw + w;
    for (int ch = 0; ch < C; ++ch) {
      const float wc = w * col[ch];
      s1[ch] = s1[ch] + wc;
      s2[ch] = s2[ch] + wc * col[ch];
    }
    ++cnt;
  }
  const bool any = sw > 0.0f;
  weight[n] = any ? sw : 0.0f;
  count[n] = any ? cnt : 0;
  for (int ch = 0; ch < C; ++ch) {
    const float mu = any ? s1[ch] / sw : 0.0f;
    mean[C * n + ch] = mu;
    var[C * n + ch] = any ? fmaxf(s2[ch] / sw - mu * mu, 0.0f) : 0.0f;
  }
}

}  // namespace ob
}  // namespace rb
