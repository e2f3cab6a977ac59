// robir_amd/csrc/metrics/metrics_math.h built for the host: a stand-alone program with plain loops around the same bodies the kernels of
// metrics.hip call, for tools/check_metrics_host.py (the metrics' arithmetic checked without a GPU).  One view per run.
//
//   metrics_host IN OUT
//   IN:  int32 kind, n0, n1, C, transfer, has_mask, has_scale
//        kind 0 (pair sums; P = n0):      float32 pred[P][C], gt[P][C], uint8 mask[P] (if has_mask), float32 scale[C] (if has_scale)
//        kind 1 (angular; P = n0, C = 3): float32 a[P][3], b[P][3], uint8 mask[P] (if has_mask)
//        kind 2 (SSIM; H = n0, W = n1):   float32 pred[H][W][C], gt[H][W][C], uint8 mask[H][W] (if has_mask), float32 scale[C] (if has_scale)
//   OUT: kind 0: float64 count, sums[C][5] (the rows added in index order)
//        kind 1: float64 count, sum of angles
//        kind 2: float64 count, sum, map[H-10][W-10][C] (zeros at the windows that are not counted; horizontal pass, then vertical, as the kernel)
#include "metrics/metrics_math.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

using namespace rb::mt;

template <class T>
static bool get(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int write_out(const char* path, const std::vector<double>& v) {
  FILE* o = fopen(path, "wb");
  if (!o) return 1;
  const size_t w = v.empty() ? 0 : fwrite(v.data(), sizeof(double), v.size(), o);
  return fclose(o) != 0 || w != v.size();
}

static int run_pair(FILE* f, const int* hdr, const char* out_path) {
  const size_t P = (size_t)hdr[1], C = (size_t)hdr[3];
  const int t = hdr[4];
  std::vector<float> pred, gt, scale;
  std::vector<unsigned char> mask;
  if (!get(f, pred, P * C) || !get(f, gt, P * C) || (hdr[5] && !get(f, mask, P)) || (hdr[6] && !get(f, scale, C))) return 1;
  std::vector<double> out(1 + 5 * C, 0.0);
  for (size_t r = 0; r < P; ++r) {
    if (hdr[5] && !mask[r]) continue;
    out[0] += 1.0;
    for (size_t c = 0; c < C; ++c) {
      double p, g;
      load_pair(pred[r * C + c], gt[r * C + c], hdr[6] ? scale[c] : 1.f, t, p, g);
      pair_terms(p, g, out.data() + 1 + 5 * c);
    }
  }
  return write_out(out_path, out);
}

static int run_angular(FILE* f, const int* hdr, const char* out_path) {
  const size_t P = (size_t)hdr[1];
  std::vector<float> a, b;
  std::vector<unsigned char> mask;
  if (!get(f, a, 3 * P) || !get(f, b, 3 * P) || (hdr[5] && !get(f, mask, P))) return 1;
  std::vector<double> out(2, 0.0);
  for (size_t r = 0; r < P; ++r) {
    double angle;
    if (hdr[5] && !mask[r]) continue;
    if (!angle_between(a.data() + 3 * r, b.data() + 3 * r, angle)) continue;
    out[0] += 1.0;
    out[1] += angle;
  }
  return write_out(out_path, out);
}

static int run_ssim(FILE* f, const int* hdr, const char* out_path) {
  const size_t H = (size_t)hdr[1], W = (size_t)hdr[2], C = (size_t)hdr[3];
  const int t = hdr[4];
  if (H < (size_t)TAPS || W < (size_t)TAPS) return 1;
  std::vector<float> pred, gt, scale;
  std::vector<unsigned char> mask;
  if (!get(f, pred, H * W * C) || !get(f, gt, H * W * C) || (hdr[5] && !get(f, mask, H * W)) || (hdr[6] && !get(f, scale, C))) return 1;
  const Window win = make_window();
  const size_t mh = H - HALO, mw = W - HALO;
  std::vector<double> out(2 + mh * mw * C, 0.0), hm(5 * H * mw);
  for (size_t c = 0; c < C; ++c) {
    for (size_t r = 0; r < H; ++r)
      for (size_t j = 0; j < mw; ++j) {
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < TAPS; ++k) {
          double p, g, q[5];
          load_pair(pred[(r * W + j + k) * C + c], gt[(r * W + j + k) * C + c], hdr[6] ? scale[c] : 1.f, t, p, g);
          moment_terms(p, g, q);
          for (int s = 0; s < 5; ++s) m[s] += win.w[k] * q[s];
        }
        for (int s = 0; s < 5; ++s) hm[(s * H + r) * mw + j] = m[s];
      }
    for (size_t i = 0; i < mh; ++i)
      for (size_t j = 0; j < mw; ++j) {
        if (hdr[5] && !mask[(i + RADIUS) * W + j + RADIUS]) continue;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < TAPS; ++k)
          for (int s = 0; s < 5; ++s) m[s] += win.w[k] * hm[(s * H + i + k) * mw + j];
        const double v = ssim_quotient(m);
        out[2 + (i * mw + j) * C + c] = v;
        out[1] += v;
        if (c == 0) out[0] += 1.0;
      }
  }
  return write_out(out_path, out);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: metrics_host IN OUT\n");
    return 64;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  int hdr[7];
  int rc = 1;
  if (fread(hdr, sizeof(int), 7, f) == 7 && hdr[0] >= 0 && hdr[0] <= 2 && hdr[1] >= 0 && hdr[1] <= (1 << 24) && hdr[2] >= 0 &&
      hdr[2] <= (1 << 12) && (hdr[0] != 2 || hdr[1] <= (1 << 12)) && hdr[3] >= 1 && hdr[3] <= MAX_CHANNELS && transfer_known(hdr[4]) &&
      (hdr[5] == 0 || hdr[5] == 1) && (hdr[6] == 0 || hdr[6] == 1))
    rc = hdr[0] == 0 ? run_pair(f, hdr, argv[2]) : hdr[0] == 1 ? run_angular(f, hdr, argv[2]) : run_ssim(f, hdr, argv[2]);
  fclose(f);
  return rc;
}
