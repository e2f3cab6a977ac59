// robir_amd/csrc/photoloss/photoloss_math.h built for the host: a stand-alone program with plain loops over the rows around the same
// bodies the kernels of photoloss.hip call, for tools/check_photoloss_host.py (the photometric loss's arithmetic checked without a GPU).
//
//   photoloss_host IN OUT
//   IN:  int32 kind, n, curve, flag, shift_stride, has_indir
//        kind 0 (a curve; flag = inverse):  float32 x[n][3], shift[shift_stride ? n : 1]
//        kind 1 (the loss; flag = l2):      float32 sg[n][3], indir[n][3] (if has_indir), gt[n][3], uint8 m1[n], m2[n],
//                                           float32 shift[shift_stride ? n : 1]
//   OUT: kind 0: float32 y[n][3] (value_f32); float64 y[n][3], dx[n][3], dt[n][3] (value_d1)
//        kind 1: float64 loss (the rows added in index order, / n), gx[n][3], gshift[n] (both / n, zeros outside the mask)
#include "photoloss/photoloss_math.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

using namespace rb::pl;

template <class T>
static bool get(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <class T>
static void put(std::vector<char>& out, const std::vector<T>& v) {
  if (v.empty()) return;
  const char* p = reinterpret_cast<const char*>(v.data());
  out.insert(out.end(), p, p + v.size() * sizeof(T));
}

static int write_out(const char* path, const std::vector<char>& bytes) {
  FILE* o = fopen(path, "wb");
  if (!o) return 1;
  const size_t w = bytes.empty() ? 0 : fwrite(bytes.data(), 1, bytes.size(), o);      // n = 0: an empty file
  return fclose(o) != 0 || w != bytes.size();
}

static int run_curve(FILE* f, const int* hdr, const char* out_path) {
  const size_t n = (size_t)hdr[1];
  const int curve = hdr[2], inverse = hdr[3], stride = hdr[4];
  std::vector<float> x, shift;
  if (!get(f, x, 3 * n) || !get(f, shift, stride ? n : 1)) return 1;
  std::vector<float> y(3 * n);
  std::vector<double> y64(3 * n), dx(3 * n), dt(3 * n);
  for (size_t i = 0; i < 3 * n; ++i) {
    const float t = shift[(i / 3) * (size_t)stride];
    y[i] = value_f32(x[i], t, curve, inverse != 0);
    const D1 v = value_d1((double)x[i], t, curve, inverse != 0);
    y64[i] = v.y;
    dx[i] = v.dx;
    dt[i] = v.dt;
  }
  std::vector<char> bytes;
  put(bytes, y), put(bytes, y64), put(bytes, dx), put(bytes, dt);
  return write_out(out_path, bytes);
}

static int run_loss(FILE* f, const int* hdr, const char* out_path) {
  const size_t n = (size_t)hdr[1];
  const int curve = hdr[2], l2 = hdr[3], stride = hdr[4], has_indir = hdr[5];
  std::vector<float> sg, indir, gt, shift;
  std::vector<unsigned char> m1, m2;
  if (!get(f, sg, 3 * n) || (has_indir && !get(f, indir, 3 * n)) || !get(f, gt, 3 * n) || !get(f, m1, n) || !get(f, m2, n) ||
      !get(f, shift, stride ? n : 1))
    return 1;
  std::vector<double> loss(1, 0.0), gx(3 * n, 0.0), gs(n, 0.0);
  const double inv_n = n ? 1.0 / (double)n : 0.0;
  for (size_t r = 0; r < n; ++r) {
    if (!(m1[r] && m2[r])) continue;
    double g[3], s;
    loss[0] += loss_row(sg.data() + 3 * r, has_indir ? indir.data() + 3 * r : nullptr, gt.data() + 3 * r, shift[r * (size_t)stride], curve,
                        l2 != 0, g, s);
    for (int c = 0; c < 3; ++c) gx[3 * r + c] = g[c] * inv_n;
    gs[r] = s * inv_n;
  }
  loss[0] *= inv_n;
  std::vector<char> bytes;
  put(bytes, loss), put(bytes, gx), put(bytes, gs);
  return write_out(out_path, bytes);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: photoloss_host IN OUT\n");
    return 64;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  int hdr[6];
  int rc = 1;
  if (fread(hdr, sizeof(int), 6, f) == 6 && (hdr[0] == 0 || hdr[0] == 1) && hdr[1] >= 0 && hdr[1] <= (1 << 24) && curve_known(hdr[2]) &&
      (hdr[3] == 0 || hdr[3] == 1) && (hdr[4] == 0 || hdr[4] == 1) && (hdr[5] == 0 || hdr[5] == 1))
    rc = hdr[0] == 0 ? run_curve(f, hdr, argv[2]) : run_loss(f, hdr, argv[2]);
  fclose(f);
  return rc;
}
