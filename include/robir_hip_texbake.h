/* robir_hip_texbake.h -- C ABI of librobir_hip_texbake.so: baking into texture space on the device (gfx950 / MI355X).  A deterministic
 * per-triangle UV atlas, a UV-space rasteriser (the counterpart of the reference's OpenGL pass, model/rasterizor.py), attribute
 * interpolation, border dilation (model/texture_model.py: erode_map) and the surface sampler's arithmetic (TexSampler.sample).  A library
 * of its own next to the two renderer libraries, the four training libraries and the light-fitting library, whose export lists and ABI
 * versions stay as they are.
 *
 * Conventions, as in the other auxiliary libraries' headers:
 *   - every pointer is a DEVICE pointer; tensors are dense row-major, fp32 / int32 unless stated;
 *   - the library never allocates, never synchronises and keeps no state; kernels are enqueued on the given stream (rb_tb_stream_t ==
 *     hipStream_t, 0 = default stream);
 *   - every entry point returns 0 on success, non-zero on error (text via rb_tb_last_error(), thread local), never throws, and validates
 *     its arguments BEFORE any launch -- the library loads and answers argument errors on a machine without a GPU;
 *   - gather kernels, one thread per output element, no atomics, plain fp32 with one rounding per operation and IEEE division / square
 *     root: the same inputs give the same bytes on every run, and tests/texbake_restatement.py reproduces every kernel bit for bit;
 *   - plain HIP runtime dependency; no name of this header exists in the other seven.
 *
 * Texture space (robir_amd/csrc/texbake/texbake_math.h).  A texture has R x R texels, R <= 16384; images are [R, R, C] with
 * row 0 at the TOP.  A UV pair maps to texel space as x = u R, y = (1 - v) R (v points up, as in OBJ); the centre of texel (r, c) is
 * (c + 0.5, r + 0.5).  UVs are given per face corner, uv [F, 3, 2]; F < 2^31.
 */
#ifndef ROBIR_HIP_TEXBAKE_H
#define ROBIR_HIP_TEXBAKE_H

#ifdef __cplusplus
extern "C" {
#endif

#define RB_TB_ABI_VERSION 1
#define RB_TB_TILE 8          /* texels per tile edge: one wave per tile */
#define RB_TB_MAX_RESOLUTION 16384

typedef void* rb_tb_stream_t; /* hipStream_t */

int rb_tb_abi_version(void);
const char* rb_tb_last_error(void);

/* Cell size S = R / ncols (integer division) of the per-triangle atlas of F faces, ncols = ceil(sqrt(ceil(F / 2))); -1 on an argument
 * error (F < 1, F >= 2^31, R < 1, R > 16384) and when S < 6, the smallest cell in which every face owns a texel centre: the error text
 * names the smallest resolution that works, 6 ncols. */
long rb_tb_atlas_cell(long F, int R);

/* uv [F, 3, 2] of the per-triangle atlas: face f goes to cell f >> 1 (row-major in ncols columns of S x S texels), half f & 1; in cell-local
 * texel units (x right, y down) the lower triangle is (1, 1), (S - 3.5, 1), (1, S - 3.5) and the upper one (S - 1, S - 1), (3.5, S - 1),
 * (S - 1, 3.5), corners in that order; u = X / R, v = 1 - Y / R.  No uncovered texel is 8-adjacent to covered texels of two faces. */
int rb_tb_atlas_uv(long F, int R, float* uv, rb_tb_stream_t stream);

/* counts [F] int32: the number of tiles of 8 x 8 texels that the face's texel box (the texel centres inside its UV bounding box, clipped to
 * the texture) touches; 0 for a face with zero or non-finite area and for one whose box holds no centre.  F == 0 returns 0 without a launch. */
int rb_tb_bin_count(const float* uv, long F, int R, int* counts, rb_tb_stream_t stream);

/* The (tile, face) pairs in face order, a face's tiles in row-major order: pair p belongs to the last face f with base[f] <= p, base [F]
 * int64 being the exclusive prefix of counts and P its total, 0 <= P < 2^31 (more pairs are refused, nothing wraps).  tile = ty ntiles + tx,
 * ntiles = ceil(R / 8).  pair_tile, pair_face [P] int32.  A pair that base assigns beyond its face's count gets tile = face = -1. */
int rb_tb_bin_emit(const float* uv, long F, int R, const long* base, long P, int* pair_tile, int* pair_face, rb_tb_stream_t stream);

/* One workgroup per tile, one thread per texel.  tile_start [ntiles^2 + 1] int32: pair_face[tile_start[t] .. tile_start[t + 1]) are the
 * faces of tile t in ASCENDING index (the pairs sorted by tile with a stable sort).  The first face that covers the texel centre wins: the
 * three edge functions (qx - px)(y - py) - (qy - py)(x - px), each evaluated from the endpoint that sorts first by (x, then y) and negated
 * when the face names the edge the other way round, times the sign of the area, all >= 0.
 *   face_id [R, R] int32, -1 where no face covers;  bary [R, R, 2]: the weights of corners 0 and 1 (that of corner 2 is 1 - b0 - b1), 0 where
 *   empty.  F == 0 or P == 0 (pair_face may then be null) gives all -1. */
int rb_tb_raster(const float* uv, long F, int R, const int* tile_start, const int* pair_face, long P, int* face_id, float* bary,
                 rb_tb_stream_t stream);

/* out[i] = (b0 attr[faces[f][0]] + b1 attr[faces[f][1]]) + b2 attr[faces[f][2]], b2 = (1 - b0) - b1, f = face_id[t], (b0, b1) = bary[t]:
 * the reference's render_texture(uvs, faces, vertex_colors).  index == null: t = i over all n_texels texels (the image form, n must equal
 * n_texels); otherwise t = index[i], index [n] int64 (the list form of the chunked bake).  faces [F, 3] int32, attr [V, C], out [n, C],
 * 1 <= C <= 64.  Zeros where face_id is negative; a texel, face or vertex index out of range also gives zeros, never a read out of bounds. */
int rb_tb_interp(const int* face_id, const float* bary, long n_texels, const long* index, long n, const int* faces, long F,
                 const float* attr, long V, int C, float* out, rb_tb_stream_t stream);

/* One ring of the reference's erode_map.  image [H, W, C], mask [H, W] uint8 (non-zero = covered).  An uncovered texel with at least one
 * covered 8-neighbour becomes the mean of its covered neighbours -- summed in row-major neighbour order from 0, divided by the count -- and
 * its byte in mask_out is 1; every other texel and mask byte is copied.  dst / mask_out must not alias image / mask (ping-pong).
 * The reference's get_vert_norm_mask_maps is two rings on position and normal and one ring on the mask. */
int rb_tb_dilate(const float* image, const unsigned char* mask, int H, int W, int C, float* dst, unsigned char* mask_out,
                 rb_tb_stream_t stream);

/* TexSampler.sample's arithmetic for n UV pairs (mesh / OBJ convention), one thread per sample.  position, normal [R, R, 3], mask [R, R]
 * fp32.  Bilinear fetches with zero padding and align_corners=False: x = u R - 0.5, y = (1 - v) R - 0.5, the four products
 * value x weight added in the order nw, ne, sw, se (torch.nn.functional.grid_sample's).  p = position at uv:
 *   x [n, 3] = p scale;  normal [n, 3] = the fetched normal / max(|.|, 1e-4);  object_mask [n] uint8 = the fetched mask > 0.1;
 *   tangent_u [n, 3] = (position at uv + (0, 0.001)) - p, tangent_v [n, 3] = (position at uv + (0.001, 0)) - p, both / max(|.|, 1e-4)
 *   (the reference's assignment: tangent_u is the v-difference). */
int rb_tb_sample(const float* position, const float* normal, const float* mask, int R, const float* uv, long n, float scale, float* x,
                 float* normal_out, unsigned char* object_mask, float* tangent_u, float* tangent_v, rb_tb_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROBIR_HIP_TEXBAKE_H */
