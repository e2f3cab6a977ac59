/* robir_hip_lightfit.h -- C ABI of librobir_hip_lightfit.so: fitting the light SGs to an environment map on the device (gfx950 / MI355X).
 * The reverse mode of the SG environment map, the fused steps of the fit (forward, MSE, gradient, Adam) and the area down-sample that
 * prepares the target.  A library of its own next to the two renderer libraries and the four training libraries, whose export lists and ABI
 * versions stay as they are.
 *
 * Conventions, as in the training libraries' headers:
 *   - every pointer is a DEVICE pointer; tensors are dense row-major fp32 unless stated;
 *   - the library never allocates, never synchronises and keeps no state: scratch memory is the caller's (a size query says how
 *     much), kernels are enqueued on the given stream (rb_lf_stream_t == hipStream_t, 0 = default stream);
 *   - every entry point returns 0 on success, non-zero on error (text via rb_lf_last_error(), thread local), never throws, and
 *     validates its arguments BEFORE any launch -- the library loads and answers argument errors on a machine without a GPU;
 *   - plain HIP runtime dependency; no name of this header exists in the other six.
 */
#ifndef ROBIR_HIP_LIGHTFIT_H
#define ROBIR_HIP_LIGHTFIT_H

#ifdef __cplusplus
extern "C" {
#endif

#define RB_LF_ABI_VERSION 1

typedef void* rb_lf_stream_t; /* hipStream_t */

int rb_lf_abi_version(void);
const char* rb_lf_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * The function (model/sg_render.py:26-42; robir_amd/csrc/lightfit/lightfit_math.h).  For lobe k with raw row s = lgt[k]:
 *   a = s[0:3] / |s[0:3]| (no epsilon),  lam = |s[3]|,  mu = |s[4:7]|,  rgb[p] = sum_k mu_k exp(lam_k (dirs[p] . a_k - 1)).
 * Arithmetic: every quantity is formed in fp64 from the fp32 inputs and accumulated in fp64; each stored value is rounded to fp32 once
 *   (loss_hist stays fp64).
 * Work shape: G = rb_lf_groups(n) = min(ceil(n / 4), 512) workgroups of four waves in a persistent grid; wave w of workgroup b takes the
 *   pixels 4 b + w, 4 b + w + 4 G, ...; a lane owns lobes k and k + 64 of a 128-lobe tile and keeps their seven partial sums in fp64
 *   registers over all its pixels; ceil(M / 128) tiles are as many rows of workgroups.  The four waves are added through LDS in wave order,
 *   each workgroup stores one slab of 7 M + 1 doubles (the loss partial rides along) with plain stores, and one finishing kernel adds the G
 *   slabs in index order, applies the chain to the raw rows and -- rb_lf_fit_steps -- the Adam update.  With M <= 128 the three colour sums
 *   of a pixel are one wave reduction inside the step; with more lobes rb_lf_fit_steps runs a first pass that stores rgb [n, 3] in fp64.
 *   Two launches per call or step, three with a second lobe tile.  No atomics, no cooperative launch, no graph capture: the order of every
 *   sum is a function of (n, M) alone and the same inputs give the same bytes on every run.
 * Scratch: rb_lf_scratch_bytes(n, M) = 8 (rb_lf_groups(n) (7 M + 1) + (M > 128 ? 3 n : 0)) bytes, 8-byte aligned; contents undefined
 *   before and after a call.  Both queries return -1 on an argument error (n < 0, M < 1) and 0 for n == 0.
 * Any M >= 1 (up to 128 x 65535); 0 <= n <= 2^36.
 * ------------------------------------------------------------------------------------------------------------ */
long rb_lf_groups(long n);
long rb_lf_scratch_bytes(long n, int M);

/* Reverse mode of rb_envmap_sg for an arbitrary upstream gradient: d_lgt [M, 7] = d <g_rgb, rgb> / d lgt, g_rgb [n, 3].
 * n == 0 returns 0 without a launch and leaves d_lgt untouched. */
int rb_lf_envmap_sg_bwd(const float* lgt, int M, const float* dirs, long n, const float* g_rgb, float* d_lgt, void* scratch,
                        long scratch_bytes, rb_lf_stream_t stream);

/* n_steps steps of the fit, enqueued without a host round trip.  Step i: rgb from the current lgt; loss = mean((rgb - target)^2) over the
 * 3 n values; its gradient; one torch.optim.Adam update (no weight decay, no amsgrad) with the bias corrections 1 - beta^t of the step
 * number t = first_step + i + 1, formed on the host in double.
 *   lgt, adam_m, adam_v [M, 7]   fp32, updated in place: the parameters and both moments as the optimiser holds them.  An element's update
 *                                is computed in fp64 and rounded once per stored value; the parameter moves by the stored moments.
 *   target [n, 3]; loss_hist [n_steps] fp64: loss_hist[i] is the loss BEFORE step i's update.
 *   first_step >= 0, n_steps >= 0, 0 <= beta1, beta2 < 1, eps >= 0.
 * n == 0 or n_steps == 0 returns 0 without a launch. */
int rb_lf_fit_steps(float* lgt, float* adam_m, float* adam_v, int M, const float* dirs, const float* target, long n, long first_step,
                    long n_steps, double lr, double beta1, double beta2, double eps, double* loss_hist, void* scratch, long scratch_bytes,
                    rb_lf_stream_t stream);

/* Exact area-weighted down-sample: dst[y, x] is the coverage-weighted mean of the source pixels that the footprint
 * [y H0 / H, (y + 1) H0 / H) x [x W0 / W, (x + 1) W0 / W) overlaps -- the plain box mean for integer ratios, the identity (bit for bit) for
 * equal sizes.  The overlaps are integers in units of 1 / (H W) of a source pixel, the sum is fp64, the result is rounded to fp32 once.
 * src [H0, W0, 3], dst [H, W, 3]; 1 <= H <= H0, 1 <= W <= W0, H0 W0 <= 2^31: up-sampling is refused. */
int rb_lf_area_resize(const float* src, int H0, int W0, float* dst, int H, int W, rb_lf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROBIR_HIP_LIGHTFIT_H */
