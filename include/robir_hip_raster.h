/* robir_hip_raster.h -- C ABI of librobir_hip_raster.so: drawing a triangle mesh into a camera's image on the device (gfx950 / MI355X).
 * The projection of the vertices, tile binning, a camera-space rasteriser with a depth test and perspective-correct weights, and the
 * G-buffer (position, uv, view direction, a fetch of the baked planes) that robir_amd/meshrender.py shades.  The counterpart in camera
 * space of librobir_hip_texbake.so's UV-space rasteriser; a library of its own next to the eleven others, whose export lists and ABI
 * versions stay as they are.
 *
 * Conventions, as in the other auxiliary libraries' headers:
 *   - every pointer is a DEVICE pointer; tensors are dense row-major, fp32 / int32 unless stated;
 *   - the library never allocates, never synchronises and keeps no state; kernels are enqueued on the given stream (rb_rs_stream_t ==
 *     hipStream_t, 0 = default stream);
 *   - every entry point returns 0 on success, non-zero on error (text via rb_rs_last_error(), thread local), never throws, and validates
 *     its arguments BEFORE any launch -- the library loads and answers argument errors on a machine without a GPU;
 *   - gather kernels, no atomics, plain fp32 with one rounding per operation and IEEE division / square root, sums associated as written:
 *     the same inputs give the same bytes on every run, and tests/meshrender_restatement.py reproduces every kernel bit for bit;
 *   - plain HIP runtime dependency; no name of this header exists in the other eleven.
 *
 * Camera (robir_amd/csrc/raster/raster_math.h): the renderer's and rb_ob_scatter's, looking along -z with y up.  pose_inv
 * [4,4] is the inverse of the camera-to-world pose (its last row is never read), K [3,3] the intrinsics.  For a vertex x:
 *     row_i = ((P[i][0] x0 + P[i][1] x1) + P[i][2] x2) + P[i][3];   zc = -row_2;   qx = row_0 / zc;   qy = -row_1 / zc;
 *     u = (K00 qx + K01 qy) + K02;   v = (K10 qx + K11 qy) + K12;   w = 1 / zc.
 * The sample point of pixel (row r, column c) is (u, v) = (c, r): the integer pixel grid of the renderer's uv input, no half-pixel offset.
 * Images are [H, W, .] with row 0 first, 1 <= H, W <= 16384; F < 2^31; fewer than 2^31 (tile, face) pairs.
 *
 * A face is SKIPPED WHOLE -- nothing is clipped -- when a corner has zc <= near (or NaN), when one of its screen coordinates (u, v, w) is not
 * finite, when its screen area is zero or not finite, when a vertex index is outside [0, V), or when `cull` drops it: 0 keeps both
 * windings, 1 drops faces of negative screen area, 2 drops faces of positive screen area (area = the edge function of corner 0 -> 1 at
 * corner 2, in (u, v) with v pointing down the rows).  A camera inside the object is out of scope.
 *
 * Coverage is texbake's rule: the edge function (qx - px)(y - py) - (qy - py)(x - px) of every edge is evaluated from the endpoint that
 * sorts first by (x, then y) and negated when the face names the edge the other way round, so the two faces of a shared edge compute the
 * same number with opposite meaning; the three values times the sign of the area must all be >= 0 (inclusive), and the pixel must lie in
 * the face's pixel box (the sample points inside its bounding box, clipped to the image).
 *
 * Depth: with the screen weights l0 = e0 / area, l1 = e1 / area, l2 = (1 - l0) - l1 (e_k: the edge opposite corner k),
 *     d = (l0 w0 + l1 w1) + l2 w2;  the largest d > 0 wins, equal d goes to the lowest face index.
 */
#ifndef ROBIR_HIP_RASTER_H
#define ROBIR_HIP_RASTER_H

#ifdef __cplusplus
extern "C" {
#endif

#define RB_RS_ABI_VERSION 1
#define RB_RS_TILE 8          /* pixels per tile edge: one wave per tile */
#define RB_RS_BATCH 64        /* faces of a tile set up at a time */
#define RB_RS_MAX_RESOLUTION 16384
#define RB_RS_MAX_CHANNELS 16

typedef void* rb_rs_stream_t; /* hipStream_t */

int rb_rs_abi_version(void);
const char* rb_rs_last_error(void);

/* vertices [V,3] -> screen [V,4] = (u, v, w, zc), one thread per vertex.  pose_inv [4,4], K [3,3].  V == 0 returns 0 without a launch. */
int rb_rs_project(const float* vertices, long V, const float* pose_inv, const float* K, float* screen, rb_rs_stream_t stream);

/* counts [F] int32: the number of tiles of 8 x 8 pixels that the face's pixel box touches; 0 for a skipped face and for one whose box holds
 * no sample point.  screen [V,4], faces [F,3] int32.  near > 0.  F == 0 returns 0 without a launch. */
int rb_rs_bin_count(const float* screen, long V, const int* faces, long F, int H, int W, float near, int cull, int* counts,
                    rb_rs_stream_t stream);

/* The (tile, face) pairs in face order, a face's tiles in row-major order: pair p belongs to the last face f with base[f] <= p, base [F]
 * int64 being the exclusive prefix of counts and P its total, 0 <= P < 2^31 (more pairs are refused, nothing wraps).  tile = ty ntx + tx,
 * ntx = ceil(W / 8).  pair_tile, pair_face [P] int32.  A pair that base assigns beyond its face's count gets tile = face = -1.
 * P == 0 returns 0 without a launch. */
int rb_rs_bin_emit(const float* screen, long V, const int* faces, long F, int H, int W, float near, int cull, const long* base, long P,
                   int* pair_tile, int* pair_face, rb_rs_stream_t stream);

/* One wave per tile, one lane per pixel.  tile_start [ntx nty + 1] int32: pair_face[tile_start[t] .. tile_start[t + 1]) are the faces of
 * tile t in ASCENDING index (the pairs sorted by tile with a stable sort).  They are taken in batches of 64: lane j sets up face j of the
 * batch into LDS, then every lane walks the batch, the pixel box first.
 *   face_id [H,W] int32, -1 where empty;  bary [H,W,2] = (l0 w0 / d, l1 w1 / d), the perspective-correct weights of corners 0 and 1 (that
 *   of corner 2 is 1 - b0 - b1), 0 where empty;  depth [H,W] = 1 / d, the winner's zc at the pixel, 0 where empty.
 * F == 0 or P == 0 (screen, faces, pair_face may then be null) gives an empty image. */
int rb_rs_raster(const float* screen, long V, const int* faces, long F, int H, int W, float near, int cull, const int* tile_start,
                 const int* pair_face, long P, int* face_id, float* bary, float* depth, rb_rs_stream_t stream);

/* The G-buffer, one thread per output row.  index == null: row i is pixel i of the H W pixels (the image form, n must equal H W);
 * otherwise row i is pixel index[i], index [n] int64 (the list form: the hit rows only).  With f = face_id[t], (b0, b1) = bary[t],
 * b2 = (1 - b0) - b1 and the face's corners a, b, c:
 *   position [n,3] = (b0 x_a + b1 x_b) + b2 x_c from vertices [V,3];   uv_out [n,2] likewise from uv [F,3,2] (per face corner, OBJ: v up);
 *   view_dir [n,3] = (cam - position) / max(|cam - position|, 1e-12): unit, from the point to the camera cam_loc [3];
 *   tex [n,C] (planes != null): the plane stack planes [R,R,C], row 0 at the top, 1 <= C <= 16, 1 <= R <= 16384, at uv_out.
 *     filter 0: the texel that contains the uv, column floor(u R), row floor((1 - v) R), clamped to the image;
 *     filter 1: rb_tb_sample's bilinear: x = u R - 0.5, y = (1 - v) R - 0.5, zero padding, the products added in the order nw, ne, sw, se;
 *   normal [n,3] (vnormals != null, [V,3]): (b0 n_a + b1 n_b) + b2 n_c over max(|.|, 1e-12).
 * Zeros where face_id is negative; a pixel, face or vertex index out of range also gives zeros, never a read out of bounds. */
int rb_rs_gbuffer(const int* face_id, const float* bary, int H, int W, const long* index, long n, const int* faces, long F,
                  const float* vertices, long V, const float* uv, const float* vnormals, const float* cam_loc, const float* planes, int R,
                  int C, int filter, float* position, float* uv_out, float* view_dir, float* tex, float* normal, rb_rs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROBIR_HIP_RASTER_H */
