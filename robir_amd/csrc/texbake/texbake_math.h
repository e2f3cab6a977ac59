// The texture-space rasteriser's arithmetic for ONE face and ONE texel, and the per-triangle atlas for ONE face corner.  No launch geometry
// and no memory traffic: the kernels of texbake.hip loop around these bodies, and a host compiler builds them as they are
// (tools/texbake_host.cpp) -- the lightfit_math.h pattern.  tests/texbake_restatement.py states the same operations in numpy fp32.
//
// Conventions (include/robir_hip_texbake.h):
//   texel space: x = u R, y = (1 - v) R (row 0 is the image's top, v points up as in OBJ); the centre of texel (r, c) is (c + 0.5, r + 0.5);
//   edge function of the directed edge p -> q at (x, y):  (qx - px)(y - py) - (qy - py)(x - px), ALWAYS evaluated from the endpoint that
//     sorts first by (x, then y) and negated when the face names the edge the other way round: the two faces of a shared edge compute the
//     same number with opposite meaning, so no rounding can leave a hole on the edge or let both faces miss it;
//   a face covers a texel centre when the three edge functions, multiplied by the sign of the face's area, are all >= 0 (inclusive) and the
//     texel lies in the face's texel box (the centres inside its bounding box, clipped to the texture);
//   faces with zero or non-finite area cover nothing.
// Arithmetic: plain fp32, one rounding per operation (-ffp-contract=off), IEEE division.
#pragma once
#include <math.h>

#ifndef RB_TB_FN
#ifdef __HIPCC__
#define RB_TB_FN __host__ __device__ __forceinline__
#else
#define RB_TB_FN inline
#endif
#endif

namespace rb {
namespace tb {

constexpr int TILE = 8;      // texels per tile edge: one wave per tile

struct Face {
  float x[3], y[3];          // the corners in texel space
  float area;                // edge function of corner 0 -> 1 at corner 2 (twice the signed area)
  int c0, c1, r0, r1;        // texel box, inclusive; empty (c0 > c1) for a skipped face
};

RB_TB_FN float edge_fn(float ax, float ay, float bx, float by, float x, float y) {
  const bool swap = bx < ax || (bx == ax && by < ay);
  const float px = swap ? bx : ax, py = swap ? by : ay, qx = swap ? ax : bx, qy = swap ? ay : by;
  const float e = (qx - px) * (y - py) - (qy - py) * (x - px);
  return swap ? -e : e;
}

RB_TB_FN float min3(float a, float b, float c) { return fminf(fminf(a, b), c); }
RB_TB_FN float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// uv: the face's three (u, v) pairs
RB_TB_FN Face face_of(const float* uv, int R) {
  Face f;
  const float fr = (float)R;
  for (int k = 0; k < 3; ++k) {
    f.x[k] = uv[2 * k] * fr;
    f.y[k] = (1.0f - uv[2 * k + 1]) * fr;
  }
  f.area = edge_fn(f.x[0], f.y[0], f.x[1], f.y[1], f.x[2], f.y[2]);
  f.c0 = f.r0 = 0;
  f.c1 = f.r1 = -1;
  if (!(f.area != 0.0f) || !(fabsf(f.area) <= 3.402823466e38f)) return f;      // zero, NaN or infinite
  // centres c + 0.5 inside [min, max]: ceil / floor of a rounded difference are never tighter than the exact ones
  const float lim = (float)(R - 1);
  const float c0 = fmaxf(ceilf(min3(f.x[0], f.x[1], f.x[2]) - 0.5f), 0.0f), c1 = fminf(floorf(max3(f.x[0], f.x[1], f.x[2]) - 0.5f), lim);
  const float r0 = fmaxf(ceilf(min3(f.y[0], f.y[1], f.y[2]) - 0.5f), 0.0f), r1 = fminf(floorf(max3(f.y[0], f.y[1], f.y[2]) - 0.5f), lim);
  if (!(c0 <= c1) || !(r0 <= r1)) return f;
  f.c0 = (int)c0;
  f.c1 = (int)c1;
  f.r0 = (int)r0;
  f.r1 = (int)r1;
  return f;
}

// tiles of TILE x TILE texels the face's texel box touches: columns tx0 .. tx1, rows ty0 .. ty1; returns their number (0: skipped face)
RB_TB_FN long face_tiles(const Face& f, int& tx0, int& ty0, int& tw) {
  if (f.c0 > f.c1) {
    tx0 = ty0 = tw = 0;
    return 0;
  }
  tx0 = f.c0 / TILE;
  ty0 = f.r0 / TILE;
  tw = f.c1 / TILE - tx0 + 1;
  return (long)tw * (f.r1 / TILE - ty0 + 1);
}

// does the face cover the centre of texel (r, c)?  b01 = the barycentric weights of corners 0 and 1 (that of corner 2 is 1 - b0 - b1)
RB_TB_FN bool covers(const Face& f, int r, int c, float* b01) {
  if (c < f.c0 || c > f.c1 || r < f.r0 || r > f.r1) return false;
  const float x = (float)c + 0.5f, y = (float)r + 0.5f;
  const float e0 = edge_fn(f.x[1], f.y[1], f.x[2], f.y[2], x, y);
  const float e1 = edge_fn(f.x[2], f.y[2], f.x[0], f.y[0], x, y);
  const float e2 = edge_fn(f.x[0], f.y[0], f.x[1], f.y[1], x, y);
  const float s = f.area > 0.0f ? 1.0f : -1.0f;
  if (!(s * e0 >= 0.0f && s * e1 >= 0.0f && s * e2 >= 0.0f)) return false;
  b01[0] = e0 / f.area;
  b01[1] = e1 / f.area;
  return true;
}

// ---------------------------------------------------------------------------------------------------------------- the atlas
// One right triangle per face: face f sits in cell f >> 1 (row-major in a grid of ncols columns of S x S texels), half f & 1.  In
// cell-local texel units the lower triangle is (1, 1), (S - 3.5, 1), (1, S - 3.5), the upper one (S - 1, S - 1), (3.5, S - 1),
// (S - 1, 3.5): a pad of one texel and hypotenuses at x + y = S -+ 2.5.
RB_TB_FN long atlas_ncols(long F) {
  const long cells = (F + 1) / 2;
  long n = (long)sqrt((double)cells);
  while (n * n < cells) ++n;
  while (n > 1 && (n - 1) * (n - 1) >= cells) --n;
  return n < 1 ? 1 : n;
}

RB_TB_FN void atlas_corner(long f, int k, long ncols, int S, int R, float* uv) {
  const long cell = f >> 1;
  const float s = (float)S, x0 = (float)((cell % ncols) * S), y0 = (float)((cell / ncols) * S);
  float lx, ly;
  if (f & 1) {
    lx = k == 1 ? 3.5f : s - 1.0f;
    ly = k == 2 ? 3.5f : s - 1.0f;
  } else {
    lx = k == 1 ? s - 3.5f : 1.0f;
    ly = k == 2 ? s - 3.5f : 1.0f;
  }
  const float fr = (float)R;
  uv[0] = (x0 + lx) / fr;
  uv[1] = 1.0f - (y0 + ly) / fr;
}

}  // namespace tb
}  // namespace rb
