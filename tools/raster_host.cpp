// robir_amd/csrc/raster/raster_math.h built for the host: a stand-alone program with plain loops over vertices, faces, pixels and G-buffer
// rows around the same bodies the kernels of raster.hip loop around, for tools/check_raster_host.py (the rasteriser's check without a GPU).
//
//   raster_host project IN OUT    IN:  int32 V, float32 pose_inv[16], K[9], vertices[V][3]
//                                 OUT: float32 screen[V][4]
//   raster_host raster IN OUT     IN:  int32 H, W, V, F, cull, float32 near, float32 screen[V][4], int32 faces[F][3]
//                                 OUT: int32 counts[F], int32 face_id[H][W], float32 bary[H][W][2], float32 depth[H][W]
//   raster_host gbuffer IN OUT    IN:  int32 H, W, V, F, R, C, filter, has_vn, n (-1: the image form), int32 face_id[H][W], float32 bary[H][W][2],
//                                      int32 faces[F][3], float32 vertices[V][3], uv[F][3][2], vn[V][3] (has_vn), cam[3], planes[R][R][C]
//                                      (R > 0), int64 index[n] (n >= 0)
//                                 OUT: float32 position[n][3], uv[n][2], view_dir[n][3], tex[n][C] (R > 0), normal[n][3] (has_vn)
#include "raster/raster_math.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace rb::rs;

static int write_all(const char* path, const std::vector<char>& bytes) {
  FILE* f = fopen(path, "wb");
  if (!f) return 1;
  const size_t n = fwrite(bytes.data(), 1, bytes.size(), f);
  return fclose(f) != 0 || n != bytes.size();
}

template <class T>
static void put(std::vector<char>& out, const std::vector<T>& v) {
  const char* p = reinterpret_cast<const char*>(v.data());
  out.insert(out.end(), p, p + v.size() * sizeof(T));
}

template <class T>
static bool get(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}

static int project_main(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return 1;
  int V;
  std::vector<float> P, K, x;
  if (fread(&V, sizeof(int), 1, f) != 1 || V < 0 || !get(f, P, 16) || !get(f, K, 9) || !get(f, x, (size_t)V * 3)) return fclose(f), 1;
  fclose(f);
  std::vector<float> screen((size_t)V * 4);
  for (long i = 0; i < V; ++i) project(x.data() + 3 * i, P.data(), K.data(), screen.data() + 4 * i);
  std::vector<char> bytes;
  put(bytes, screen);
  return write_all(out, bytes);
}

static Face load_face(const std::vector<float>& screen, long V, const int* idx, int H, int W, float near, int cull) {
  float s[3][4];
  const bool ok = idx[0] >= 0 && idx[0] < V && idx[1] >= 0 && idx[1] < V && idx[2] >= 0 && idx[2] < V;
  for (int j = 0; j < 3; ++j)
    for (int k = 0; k < 4; ++k) s[j][k] = ok ? screen[4 * (size_t)idx[j] + k] : NAN;
  return face_of(s[0], s[1], s[2], H, W, near, cull);
}

static int raster_main(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return 1;
  int hdr[5];
  float near;
  if (fread(hdr, sizeof(int), 5, f) != 5 || fread(&near, sizeof(float), 1, f) != 1) return fclose(f), 1;
  const int H = hdr[0], W = hdr[1], cull = hdr[4];
  const long V = hdr[2], F = hdr[3];
  if (H < 1 || W < 1 || H > 16384 || W > 16384 || V < 0 || F < 0) return fclose(f), 1;
  std::vector<float> screen;
  std::vector<int> faces;
  if (!get(f, screen, (size_t)V * 4) || !get(f, faces, (size_t)F * 3)) return fclose(f), 1;
  fclose(f);
  std::vector<int> counts(F), face_id((size_t)H * W, -1);
  std::vector<float> bary((size_t)H * W * 2, 0.0f), best((size_t)H * W, 0.0f), depth((size_t)H * W, 0.0f);
  for (long i = 0; i < F; ++i) {                      // ascending faces: a strictly larger d replaces the owner
    const Face face = load_face(screen, V, faces.data() + 3 * i, H, W, near, cull);
    int tx0, ty0, tw;
    counts[i] = (int)face_tiles(face, tx0, ty0, tw);
    for (int r = face.r0; r <= face.r1; ++r)
      for (int c = face.c0; c <= face.c1; ++c) {
        const size_t t = (size_t)r * W + c;
        float d, w[2];
        if (sample(face, r, c, d, w) && d > best[t]) {
          best[t] = d;
          face_id[t] = (int)i;
          bary[2 * t] = w[0];
          bary[2 * t + 1] = w[1];
        }
      }
  }
  for (size_t t = 0; t < depth.size(); ++t) depth[t] = face_id[t] < 0 ? 0.0f : 1.0f / best[t];
  std::vector<char> bytes;
  put(bytes, counts);
  put(bytes, face_id);
  put(bytes, bary);
  put(bytes, depth);
  return write_all(out, bytes);
}

static int gbuffer_main(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return 1;
  int h[9];
  if (fread(h, sizeof(int), 9, f) != 9) return fclose(f), 1;
  const int H = h[0], W = h[1], R = h[4], C = h[5], filter = h[6], has_vn = h[7];
  const long V = h[2], F = h[3], n_index = h[8], n_pixels = (long)H * W;
  if (H < 1 || W < 1 || V < 0 || F < 0 || R < 0 || C < 0 || C > MAX_CHANNELS) return fclose(f), 1;
  std::vector<int> face_id, faces;
  std::vector<float> bary, vertices, uv, vn, cam, planes;
  std::vector<long> index;
  bool ok = get(f, face_id, (size_t)n_pixels) && get(f, bary, (size_t)n_pixels * 2) && get(f, faces, (size_t)F * 3) &&
            get(f, vertices, (size_t)V * 3) && get(f, uv, (size_t)F * 6) && (!has_vn || get(f, vn, (size_t)V * 3)) && get(f, cam, 3) &&
            (R == 0 || get(f, planes, (size_t)R * R * C)) && (n_index < 0 || get(f, index, (size_t)n_index));
  fclose(f);
  if (!ok) return 1;
  const long n = n_index < 0 ? n_pixels : n_index;
  std::vector<float> position((size_t)n * 3), uv_out((size_t)n * 2), view_dir((size_t)n * 3), tex(R ? (size_t)n * C : 0),
      normal(has_vn ? (size_t)n * 3 : 0);
  for (long i = 0; i < n; ++i)
    gbuffer_row(n_index < 0 ? i : index[i], n_pixels, face_id.data(), bary.data(), faces.data(), F, vertices.data(), V, uv.data(),
                has_vn ? vn.data() : nullptr, cam.data(), R ? planes.data() : nullptr, R, C, filter, position.data() + 3 * i,
                uv_out.data() + 2 * i, view_dir.data() + 3 * i, R ? tex.data() + (size_t)C * i : nullptr,
                has_vn ? normal.data() + 3 * i : nullptr);
  std::vector<char> bytes;
  put(bytes, position);
  put(bytes, uv_out);
  put(bytes, view_dir);
  put(bytes, tex);
  put(bytes, normal);
  return write_all(out, bytes);
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "project")) return project_main(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "raster")) return raster_main(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "gbuffer")) return gbuffer_main(argv[2], argv[3]);
  fprintf(stderr, "usage: raster_host project|raster|gbuffer IN OUT\n");
  return 64;
}
