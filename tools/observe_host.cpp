// robir_amd/csrc/observe/observe_math.h built for the host: a stand-alone program with plain loops over cameras and points around the same
// bodies the kernels of observe.hip call, for tools/check_observe_host.py (the observation arithmetic's check without a GPU).
//
//   observe_host IN OUT
//   IN:  int32 M, N, H, W, C, has_masks, n_obs; float32 x[N][3], normals[N][3], cam_loc[M][3], pose_inv[M][4][4], K[M][3][3],
//        images[M][H][W][C], masks[M][H][W] (if has_masks), uint8 vis[M][N], float32 draws[M][N]
//   OUT: scatter: float32 uv[M][N][2], view_dir[M][N][3], rgb[M][N][C], uint8 valid[M][N];
//        select:  int32 index[n_obs][N], count[N];
//        gather (of that index): float32 uv[n_obs][N][2], view_dir[n_obs][N][3], rgb[n_obs][N][C], uint8 valid[n_obs][N];
//        accumulate: float32 weight[N], mean[N][C], var[N][C], int32 count[N]
#include "observe/observe_math.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace rb::ob;

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

template <int C>
static int run(FILE* f, const int* hdr, const char* out_path) {
  const int M = hdr[0], H = hdr[2], W = hdr[3], has_masks = hdr[5], n_obs = hdr[6];
  const long N = hdr[1];
  const size_t MN = (size_t)M * N, plane = (size_t)H * W;
  std::vector<float> x, normals, cam_loc, pose_inv, K, images, masks, draws;
  std::vector<unsigned char> vis;
  bool ok = get(f, x, 3 * N) && get(f, normals, 3 * N) && get(f, cam_loc, 3 * (size_t)M) && get(f, pose_inv, 16 * (size_t)M) &&
            get(f, K, 9 * (size_t)M) && get(f, images, M * plane * C) && (!has_masks || get(f, masks, M * plane)) && get(f, vis, MN) &&
            get(f, draws, MN);
  if (!ok) return 1;
  const float* mk = has_masks ? masks.data() : nullptr;

  std::vector<float> uv(2 * MN), dir(3 * MN), rgb(C * MN);
  std::vector<unsigned char> valid(MN);
  for (int m = 0; m < M; ++m)
    for (long n = 0; n < N; ++n)
      scatter_pair<C>(m, n, (long)m * N + n, x.data(), cam_loc.data(), pose_inv.data(), K.data(), images.data(), mk, H, W, uv.data(), dir.data(),
                      rgb.data(), valid.data());

  std::vector<int> index((size_t)n_obs * N), seen(N);
  for (long n = 0; n < N; ++n) select_point(n, N, M, n_obs, vis.data(), draws.data(), index.data(), seen.data());

  const size_t KN = (size_t)n_obs * N;
  std::vector<float> guv(2 * KN), gdir(3 * KN), grgb(C * KN);
  std::vector<unsigned char> gvalid(KN);
  for (int k = 0; k < n_obs; ++k)
    for (long n = 0; n < N; ++n)
      gather_pair<C>(k, n, N, M, index.data(), x.data(), cam_loc.data(), pose_inv.data(), K.data(), images.data(), mk, H, W, guv.data(),
                     gdir.data(), grgb.data(), gvalid.data());

  std::vector<float> weight(N), mean((size_t)C * N), var((size_t)C * N);
  std::vector<int> count(N);
  for (long n = 0; n < N; ++n)
    accumulate_point<C>(n, N, M, x.data(), normals.data(), cam_loc.data(), pose_inv.data(), K.data(), images.data(), H, W, vis.data(),
                        weight.data(), mean.data(), var.data(), count.data());

  std::vector<char> bytes;
  put(bytes, uv), put(bytes, dir), put(bytes, rgb), put(bytes, valid);
  put(bytes, index), put(bytes, seen);
  put(bytes, guv), put(bytes, gdir), put(bytes, grgb), put(bytes, gvalid);
  put(bytes, weight), put(bytes, mean), put(bytes, var), put(bytes, count);
  FILE* o = fopen(out_path, "wb");
  if (!o) return 1;
  const size_t w = bytes.empty() ? 0 : fwrite(bytes.data(), 1, bytes.size(), o);      // N = 0: an empty file
  return fclose(o) != 0 || w != bytes.size();
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: observe_host IN OUT\n");
    return 64;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  int hdr[7];
  int rc = 1;
  if (fread(hdr, sizeof(int), 7, f) == 7 && hdr[0] >= 1 && hdr[0] <= 4096 && hdr[1] >= 0 && hdr[1] <= (1 << 24) && hdr[2] >= 2 &&
      hdr[2] <= 16384 && hdr[3] >= 2 && hdr[3] <= 16384 && (hdr[4] == 1 || hdr[4] == 3) && hdr[6] >= 1 && hdr[6] <= MAX_OBS)
    rc = hdr[4] == 3 ? run<3>(f, hdr, argv[2]) : run<1>(f, hdr, argv[2]);
  fclose(f);
  return rc;
}
