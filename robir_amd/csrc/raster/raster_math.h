// The camera-space rasteriser's arithmetic for ONE vertex, ONE face, ONE (face, pixel) pair and ONE G-buffer row.  No launch geometry and no
// LDS: the kernels of raster.hip loop around these bodies, and a host compiler builds them as they are (tools/raster_host.cpp) -- the
// texbake_math.h pattern.  tests/meshrender_restatement.py states the same operations in numpy fp32.
//
// Conventions (include/robir_hip_raster.h):
//   camera: looks along -z, y up; P = the inverse of the camera-to-world pose, K the intrinsics:
//     row_i = ((P[i][0] x0 + P[i][1] x1) + P[i][2] x2) + P[i][3];  zc = -row_2;  qx = row_0 / zc;  qy = -row_1 / zc;
//     u = (K00 qx + K01 qy) + K02;  v = (K10 qx + K11 qy) + K12;  w = 1 / zc;
//   the sample point of pixel (row r, column c) is (u, v) = (c, r);
//   edge function of the directed edge p -> q at (x, y):  (qx - px)(y - py) - (qy - py)(x - px), ALWAYS evaluated from the endpoint that
//     sorts first by (x, then y) and negated when the face names the edge the other way round (texbake_math.h's rule: the two faces of a
//     shared edge compute the same number with opposite meaning, so no rounding leaves a hole on the edge or lets both faces miss it);
//   a face covers a sample point when the three edge functions, multiplied by the sign of the face's area, are all >= 0 (inclusive) and the
//     pixel lies in the face's pixel box; a face with a corner at zc <= near, a non-finite screen coordinate or a zero / non-finite area
//     covers nothing -- no clipping;
//   depth: l_k = e_k / area (l2 = (1 - l0) - l1), d = (l0 w0 + l1 w1) + l2 w2 = 1 / zc at the pixel; the largest d > 0 wins.
// Arithmetic: plain fp32, one rounding per operation (-ffp-contract=off), IEEE division and square root, sums associated as written.
#pragma once
#include <math.h>

#ifndef RB_RS_FN
#ifdef __HIPCC__
#define RB_RS_FN __host__ __device__ __forceinline__
#else
#define RB_RS_FN inline
#endif
#endif

namespace rb {
namespace rs {

constexpr int TILE = 8;       // pixels per tile edge: one wave per tile
constexpr int BATCH = 64;     // faces one wave sets up at a time
constexpr int MAX_CHANNELS = 16;

// x [3] -> s [4] = (u, v, w, zc);  P [4][4] (rows 0 .. 2 are read), K [3][3]
RB_RS_FN void project(const float* x, const float* P, const float* K, float* s) {
  float row[3];
  for (int i = 0; i < 3; ++i) row[i] = ((P[4 * i] * x[0] + P[4 * i + 1] * x[1]) + P[4 * i + 2] * x[2]) + P[4 * i + 3];
  const float zc = -row[2];
  const float qx = row[0] / zc, qy = -row[1] / zc;
  s[0] = (K[0] * qx + K[1] * qy) + K[2];
  s[1] = (K[3] * qx + K[4] * qy) + K[5];
  s[2] = 1.0f / zc;
  s[3] = zc;
}

// a face ready for its pixels, 24 words: edge k runs from corner k + 1 to corner k + 2 (mod 3), opposite corner k
struct Face {
  float px[3], py[3], qx[3], qy[3];      // the edge's endpoints, the one that sorts first by (x, then y) in p
  float sg[3];                           // -1 where the face names the edge from q to p, else 1
  float area;                            // edge 2 (corner 0 -> 1) at corner 2: twice the signed screen area
  float w[3];                            // 1 / zc of the corners
  int c0, c1, r0, r1;                    // pixel box, inclusive; empty (c0 > c1) for a skipped face
  int id;                                // the face's index (raster.hip keeps it beside the record)
};

RB_RS_FN float min3(float a, float b, float c) { return fminf(fminf(a, b), c); }
RB_RS_FN float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
RB_RS_FN bool finite_f(float a) { return fabsf(a) <= 3.402823466e38f; }      // false for NaN

RB_RS_FN float edge_at(const Face& f, int k, float x, float y) {
  return f.sg[k] * ((f.qx[k] - f.px[k]) * (y - f.py[k]) - (f.qy[k] - f.py[k]) * (x - f.px[k]));
}

// s0, s1, s2: the corners' (u, v, w, zc)
RB_RS_FN Face face_of(const float* s0, const float* s1, const float* s2, int H, int W, float near, int cull) {
  Face f;
  const float* s[3] = {s0, s1, s2};
  for (int k = 0; k < 3; ++k) {
    const float* a = s[(k + 1) % 3];
    const float* b = s[(k + 2) % 3];
    const bool swap = b[0] < a[0] || (b[0] == a[0] && b[1] < a[1]);
    f.px[k] = swap ? b[0] : a[0];
    f.py[k] = swap ? b[1] : a[1];
    f.qx[k] = swap ? a[0] : b[0];
    f.qy[k] = swap ? a[1] : b[1];
    f.sg[k] = swap ? -1.0f : 1.0f;
    f.w[k] = s[k][2];
  }
  f.area = edge_at(f, 2, s2[0], s2[1]);
  f.c0 = f.r0 = 0;
  f.c1 = f.r1 = -1;
  f.id = -1;
  for (int k = 0; k < 3; ++k) {
    if (!(s[k][3] > near)) return f;                                                  // behind the near plane, or NaN
    if (!finite_f(s[k][0]) || !finite_f(s[k][1]) || !finite_f(s[k][2])) return f;
  }
  if (!(f.area != 0.0f) || !finite_f(f.area)) return f;
  if ((cull == 1 && f.area < 0.0f) || (cull == 2 && f.area > 0.0f)) return f;
  // sample points c inside [min, max]: ceil / floor of the coordinates themselves
  const float c0 = fmaxf(ceilf(min3(s0[0], s1[0], s2[0])), 0.0f), c1 = fminf(floorf(max3(s0[0], s1[0], s2[0])), (float)(W - 1));
  const float r0 = fmaxf(ceilf(min3(s0[1], s1[1], s2[1])), 0.0f), r1 = fminf(floorf(max3(s0[1], s1[1], s2[1])), (float)(H - 1));
  if (!(c0 <= c1) || !(r0 <= r1)) return f;
  f.c0 = (int)c0;
  f.c1 = (int)c1;
  f.r0 = (int)r0;
  f.r1 = (int)r1;
  return f;
}

// tiles of TILE x TILE pixels the face's pixel box touches: columns tx0 .. , rows ty0 .. , tw columns wide; returns their number (0: skipped)
RB_RS_FN long face_tiles(const Face& f, int& tx0, int& ty0, int& tw) {
  if (f.c0 > f.c1) {
    tx0 = ty0 = tw = 0;
    return 0;
  }
  tx0 = f.c0 / TILE;
  ty0 = f.r0 / TILE;
  tw = f.c1 / TILE - tx0 + 1;
  return (long)tw * (f.r1 / TILE - ty0 + 1);
}

// does the face cover the sample point of pixel (r, c)?  d = 1 / zc there, b01 = the perspective-correct weights of corners 0 and 1
RB_RS_FN bool sample(const Face& f, int r, int c, float& d, float* b01) {
  if (c < f.c0 || c > f.c1 || r < f.r0 || r > f.r1) return false;
  const float x = (float)c, y = (float)r;
  const float e0 = edge_at(f, 0, x, y), e1 = edge_at(f, 1, x, y), e2 = edge_at(f, 2, x, y);
  const float s = f.area > 0.0f ? 1.0f : -1.0f;
  if (!(s * e0 >= 0.0f && s * e1 >= 0.0f && s * e2 >= 0.0f)) return false;
  const float l0 = e0 / f.area, l1 = e1 / f.area, l2 = (1.0f - l0) - l1;
  const float t0 = l0 * f.w[0], t1 = l1 * f.w[1];
  d = (t0 + t1) + l2 * f.w[2];
  b01[0] = t0 / d;
  b01[1] = t1 / d;
  return true;
}

// ---------------------------------------------------------------------------------------------------------------- the G-buffer
// (b0 a + b1 b) + b2 c for n components
RB_RS_FN void interp(const float* a, const float* b, const float* c, float b0, float b1, float b2, int n, float* o) {
  for (int k = 0; k < n; ++k) o[k] = (b0 * a[k] + b1 * b[k]) + b2 * c[k];
}

RB_RS_FN void unit(const float* v, float* o) {
  const float len = fmaxf(sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]), 1e-12f);
  o[0] = v[0] / len;
  o[1] = v[1] / len;
  o[2] = v[2] / len;
}

// the texel that contains (u, v) of an [R, R, C] image, row 0 at the top: column floor(u R), row floor((1 - v) R), clamped (NaN -> 0)
RB_RS_FN void fetch_nearest(const float* img, int R, int C, float u, float v, float* o) {
  const float fr = (float)R, lim = (float)(R - 1);
  const int c = (int)fminf(fmaxf(floorf(u * fr), 0.0f), lim), r = (int)fminf(fmaxf(floorf((1.0f - v) * fr), 0.0f), lim);
  for (int ch = 0; ch < C; ++ch) o[ch] = img[((long)r * R + c) * C + ch];
}

// rb_tb_sample's bilinear fetch: texel coordinates x = u R - 0.5, y = (1 - v) R - 0.5, texels out of the image count as +0 and every product
// is formed, so the association is the same at the border
RB_RS_FN void fetch_bilinear(const float* img, int R, int C, float u, float v, float* o) {
  const float fr = (float)R;
  const float x = u * fr - 0.5f, y = (1.0f - v) * fr - 0.5f;
  const float x0 = floorf(x), y0 = floorf(y);
  const float wx1 = x - x0, wx0 = (x0 + 1.0f) - x, wy1 = y - y0, wy0 = (y0 + 1.0f) - y;
  const float nw = wx0 * wy0, ne = wx1 * wy0, sw = wx0 * wy1, se = wx1 * wy1;
  // x0, y0 beyond the image by more than a texel contribute nothing: clamp before the conversion so that it cannot overflow (NaN -> -2)
  const int c0 = (int)fminf(fmaxf(x0, -2.0f), fr + 1.0f), r0 = (int)fminf(fmaxf(y0, -2.0f), fr + 1.0f);
  const bool cin0 = c0 >= 0 && c0 < R, cin1 = c0 + 1 >= 0 && c0 + 1 < R, rin0 = r0 >= 0 && r0 < R, rin1 = r0 + 1 >= 0 && r0 + 1 < R;
  for (int ch = 0; ch < C; ++ch) {
    const float a = rin0 && cin0 ? img[((long)r0 * R + c0) * C + ch] : 0.0f;
    const float b = rin0 && cin1 ? img[((long)r0 * R + c0 + 1) * C + ch] : 0.0f;
    const float c = rin1 && cin0 ? img[((long)(r0 + 1) * R + c0) * C + ch] : 0.0f;
    const float d = rin1 && cin1 ? img[((long)(r0 + 1) * R + c0 + 1) * C + ch] : 0.0f;
    o[ch] = ((a * nw + b * ne) + c * sw) + d * se;
  }
}

// G-buffer row i of pixel t.  Every output pointer names row i already; tex / normal may be null (with planes / vnormals)
RB_RS_FN void gbuffer_row(long t, long n_pixels, const int* face_id, const float* bary, const int* faces, long F, const float* vertices,
                          long V, const float* uv, const float* vnormals, const float* cam, const float* planes, int R, int C, int filter,
                          float* position, float* uv_out, float* view_dir, float* tex, float* normal) {
  float p[3] = {0.0f, 0.0f, 0.0f}, q[2] = {0.0f, 0.0f}, vd[3] = {0.0f, 0.0f, 0.0f}, nr[3] = {0.0f, 0.0f, 0.0f}, tx[MAX_CHANNELS];
  for (int ch = 0; ch < MAX_CHANNELS; ++ch) tx[ch] = 0.0f;
  if (t >= 0 && t < n_pixels) {
    const int f = face_id[t];
    if (f >= 0 && f < F) {
      const long v0 = faces[3 * (long)f], v1 = faces[3 * (long)f + 1], v2 = faces[3 * (long)f + 2];
      if (v0 >= 0 && v0 < V && v1 >= 0 && v1 < V && v2 >= 0 && v2 < V) {
        const float b0 = bary[2 * t], b1 = bary[2 * t + 1], b2 = (1.0f - b0) - b1;
        interp(vertices + 3 * v0, vertices + 3 * v1, vertices + 3 * v2, b0, b1, b2, 3, p);
        interp(uv + 6 * (long)f, uv + 6 * (long)f + 2, uv + 6 * (long)f + 4, b0, b1, b2, 2, q);
        const float dc[3] = {cam[0] - p[0], cam[1] - p[1], cam[2] - p[2]};
        unit(dc, vd);
        if (planes) {
          if (filter == 0) fetch_nearest(planes, R, C, q[0], q[1], tx);
          else fetch_bilinear(planes, R, C, q[0], q[1], tx);
        }
        if (vnormals) {
          float m[3];
          interp(vnormals + 3 * v0, vnormals + 3 * v1, vnormals + 3 * v2, b0, b1, b2, 3, m);
          unit(m, nr);
        }
      }
    }
  }
  for (int k = 0; k < 3; ++k) {
    position[k] = p[k];
    view_dir[k] = vd[k];
    if (normal) normal[k] = nr[k];
  }
  uv_out[0] = q[0];
  uv_out[1] = q[1];
  if (tex)
    for (int ch = 0; ch < C; ++ch) tex[ch] = tx[ch];
}

}  // namespace rs
}  // namespace rb
