// robir_amd/csrc/texbake/texbake_math.h built for the host: a stand-alone program with plain loops over faces and texels around the same
// bodies the kernels of texbake.hip loop around, for tools/check_texbake_host.py (the rasteriser's and the atlas' check without a GPU).
//
//   texbake_host raster IN OUT    IN:  int32 R, int32 F, float32 uv[F][3][2]
//                                 OUT: int32 counts[F], int32 face_id[R][R], float32 bary[R][R][2]
//   texbake_host atlas F R OUT    OUT: float32 uv[F][3][2]   (exit status 2 when the cell is smaller than 6 texels)
#include "texbake/texbake_math.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace rb::tb;

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

static int raster(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return 1;
  int hdr[2];
  if (fread(hdr, sizeof(int), 2, f) != 2 || hdr[0] < 1 || hdr[0] > 16384 || hdr[1] < 0) return fclose(f), 1;
  const int R = hdr[0];
  const long F = hdr[1];
  std::vector<float> uv((size_t)F * 6);
  if (fread(uv.data(), sizeof(float), uv.size(), f) != uv.size()) return fclose(f), 1;
  fclose(f);
  std::vector<int> counts(F), face_id((size_t)R * R, -1);
  std::vector<float> bary((size_t)R * R * 2, 0.0f);
  for (long i = 0; i < F; ++i) {                      // ascending faces: the first that covers a texel centre owns it
    const Face face = face_of(uv.data() + 6 * i, R);
    int tx0, ty0, tw;
    counts[i] = (int)face_tiles(face, tx0, ty0, tw);
    for (int r = face.r0; r <= face.r1; ++r)
      for (int c = face.c0; c <= face.c1; ++c) {
        const size_t t = (size_t)r * R + c;
        float w[2];
        if (face_id[t] < 0 && covers(face, r, c, w)) {
          face_id[t] = (int)i;
          bary[2 * t] = w[0];
          bary[2 * t + 1] = w[1];
        }
      }
  }
  std::vector<char> bytes;
  put(bytes, counts);
  put(bytes, face_id);
  put(bytes, bary);
  return write_all(out, bytes);
}

static int atlas(long F, int R, const char* out) {
  if (F < 1 || R < 1) return 1;
  const long ncols = atlas_ncols(F), S = R / ncols;
  if (S < 6) return 2;
  std::vector<float> uv((size_t)F * 6);
  for (long f = 0; f < F; ++f)
    for (int k = 0; k < 3; ++k) atlas_corner(f, k, ncols, (int)S, R, uv.data() + 6 * f + 2 * k);
  std::vector<char> bytes;
  put(bytes, uv);
  return write_all(out, bytes);
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "raster")) return raster(argv[2], argv[3]);
  if (argc == 5 && !strcmp(argv[1], "atlas")) return atlas(atol(argv[2]), atoi(argv[3]), argv[4]);
  fprintf(stderr, "usage: texbake_host raster IN OUT | atlas F R OUT\n");
  return 64;
}
