/* robir_hip_observe.h -- C ABI of librobir_hip_observe.so: multi-view observations of surface points on the device (gfx950 / MI355X).
 * Which training views see a surface point, along which direction and with what pixel colour: the per-pair arithmetic of the reference's
 * inv_camera_params and FocusSampler.scatter_sample (model/focus_sampler.py), the choice of n_obs views per point that
 * TexSpaceSampler.sample_observations_sorted makes with a full sort (training/tex_module.py), and a fused weighted mean / variance of the
 * observed colour for baking.  A library of its own next to the two renderer libraries, the four training libraries, the light-fitting
 * and the texture-baking library, whose export lists and ABI versions stay as they are.
 *
 * Conventions, as in the other auxiliary libraries' headers:
 *   - every pointer is a DEVICE pointer; tensors are dense row-major, fp32 / int32 / uint8 as stated;
 *   - the library never allocates, never synchronises and keeps no state; kernels are enqueued on the given stream (rb_ob_stream_t ==
 *     hipStream_t, 0 = default stream);
 *   - every entry point returns 0 on success, non-zero on error (text via rb_ob_last_error(), thread local), never throws, and validates
 *     its arguments BEFORE any launch -- the library loads and answers argument errors on a machine without a GPU;
 *   - gather kernels, no atomics, plain fp32 with one rounding per operation, sums associated from the left, IEEE division and square
 *     root: the same inputs give the same bytes on every run, and tests/observe_restatement.py reproduces every kernel bit for bit;
 *   - plain HIP runtime dependency; no name of this header exists in the other eight.
 *
 * Cameras and images (robir_amd/csrc/observe/observe_math.h).  M cameras, 1 <= M <= 4096: cam_loc [M, 3] (pose[:3, 3]),
 * pose_inv [M, 4, 4] (the inverse of the camera-to-world pose; the last row is never read), K [M, 3, 3].  images [M, H, W, C], C = 1 or 3,
 * masks [M, H, W] fp32, H, W >= 2, row 0 first.  A pixel position is (u, v), u along the W columns and v along the H rows.
 *
 * The projection of point x by camera m:
 *   view_dir = (x - c) / max(|x - c|, 1e-12);   row_i = sum_j pose_inv[i][j] (view_dir + c, 1)_j, i = 0..2;   z = -row_2;
 *   q = (row_0, -row_1, -row_2) / (z, or 1e-5 where z == 0);   (u, v) = the first two components of K q.
 * The bilinear fetch at (u, v) is torch.nn.functional.grid_sample's with align_corners=True and zero padding, including its round trip
 * through normalised coordinates in fp32: g = u / W 2 - 1, ix = ((g + 1) / 2) (W - 1) (and v with H); the four products value x weight
 * are added in the order nw, ne, sw, se.
 *
 * Two departures from the reference, both deliberate:
 *   - u is divided by and compared with W and v with H; the reference uses (H, W) in that order for (u, v), which is the same only for
 *     square images;
 *   - a pair whose point lies behind the camera (z <= 0) is not valid; the reference projects it mirrored into the image.
 */
#ifndef ROBIR_HIP_OBSERVE_H
#define ROBIR_HIP_OBSERVE_H

#ifdef __cplusplus
extern "C" {
#endif

#define RB_OB_ABI_VERSION 1
#define RB_OB_MAX_CAMERAS 4096
#define RB_OB_MAX_OBS 8

typedef void* rb_ob_stream_t; /* hipStream_t */

int rb_ob_abi_version(void);
const char* rb_ob_last_error(void);

/* One thread per (camera, point) pair, grid (ceil(N / 256), M).  x [N, 3].
 *   uv [M, N, 2], view_dir [M, N, 3], rgb [M, N, C] = images[m] fetched at uv;
 *   valid [M, N] uint8 = 0 <= u < W and 0 <= v < H and z > 0 and (masks[m] fetched at uv) > 0.5.  masks == null leaves the mask term out
 *   (the reference's masks.numel() == 0).  A NaN uv compares false: valid = 0.
 * N == 0 returns 0 without a launch.  0 <= N < 2^31. */
int rb_ob_scatter(const float* x, long N, const float* cam_loc, const float* pose_inv, const float* K, int M, const float* images,
                  const float* masks, int H, int W, int C, float* uv, float* view_dir, float* rgb, unsigned char* valid,
                  rb_ob_stream_t stream);

/* out [M, N, C] = images[m] fetched at uv [M, N, 2] (FocusSampler.sample_images; with C = 1 on the masks, the value that sample_masks
 * compares with 0.5).  One thread per (camera, position) pair.  N == 0 returns 0 without a launch. */
int rb_ob_fetch(const float* images, int M, int H, int W, int C, const float* uv, long N, float* out, rb_ob_stream_t stream);

/* rb_ob_scatter for the pairs (index[k][n], n) only, index [n_obs, N] int32 as rb_ob_select writes it: uv [n_obs, N, 2], view_dir
 * [n_obs, N, 3], rgb [n_obs, N, C], valid [n_obs, N], the same bytes as the rows of rb_ob_scatter's outputs; zeros where the index is
 * negative or >= M.  One thread per (row, point) pair.  N == 0 returns 0 without a launch. */
int rb_ob_gather(const int* index, int n_obs, const float* x, long N, const float* cam_loc, const float* pose_inv, const float* K, int M,
                 const float* images, const float* masks, int H, int W, int C, float* uv, float* view_dir, float* rgb, unsigned char* valid,
                 rb_ob_stream_t stream);

/* One thread per point.  vis [M, N] uint8, draws [M, N] fp32.  index [n_obs, N] int32: the cameras of the n_obs largest keys
 * (vis != 0 ? 1 : 0) + 0.01 draws, the largest first, ties to the lower camera index (torch.sort(descending)[:n_obs] of the reference with
 * a stable order); -1 in the rows beyond M.  A NaN key is never chosen.  count [N] int32: the number of cameras with vis != 0.
 * 1 <= n_obs <= 8: the candidates stay in registers.  N == 0 returns 0 without a launch. */
int rb_ob_select(const unsigned char* vis, const float* draws, int M, long N, int n_obs, int* index, int* count, rb_ob_stream_t stream);

/* One thread per point, the cameras in ascending order; only pairs with vis[m][n] != 0 are projected and fetched.  normals [N, 3].
 *   w_m = max(-(normal . view_dir_m), 0);  cameras with w_m == 0 do not contribute;
 *   weight [N] = sum_m w_m;
 *   mean [N, C] = (sum_m w_m rgb_m) / weight;
 *   var [N, C]  = max((sum_m (w_m rgb_m) rgb_m) / weight - mean mean, 0), each sum in fp32 in camera order;
 *   count [N] int32 = the number of contributing cameras;
 * weight, mean, var and count are 0 where weight == 0.  Nothing of size M N is written.  N == 0 returns 0 without a launch. */
int rb_ob_accumulate(const float* x, const float* normals, long N, const float* cam_loc, const float* pose_inv, const float* K, int M,
                     const float* images, int H, int W, int C, const unsigned char* vis, float* weight, float* mean, float* var,
                     int* count, rb_ob_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROBIR_HIP_OBSERVE_H */
