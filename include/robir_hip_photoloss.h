/* robir_hip_photoloss.h -- C ABI of librobir_hip_photoloss.so: the photometric loss of stages 3 and 4 on the device (gfx950 / MI355X).
 * The reverse mode of the tone curves of ACESToneMapping (model/color_correction.py:31-73,116-137) and the fused image loss of
 * InvLoss.forward (model/loss.py:31-42,97-110): tone map, masked L1 / L2 distance, its sum and its gradient in one pass over the rows.
 * A library of its own next to the two renderer libraries and the seven other auxiliary libraries, whose export lists and ABI versions stay
 * as they are.
 *
 * Conventions, as in the training libraries' headers:
 *   - every pointer is a DEVICE pointer; tensors are dense row-major fp32 unless stated;
 *   - the library never allocates, never synchronises and keeps no state: scratch memory is the caller's (a size query says how
 *     much), kernels are enqueued on the given stream (rb_pl_stream_t == hipStream_t, 0 = default stream);
 *   - every entry point returns 0 on success, non-zero on error (text via rb_pl_last_error(), thread local), never throws, and
 *     validates its arguments BEFORE any launch -- the library loads and answers argument errors on a machine without a GPU;
 *   - plain HIP runtime dependency; no name of this header exists in the other nine.
 */
#ifndef ROBIR_HIP_PHOTOLOSS_H
#define ROBIR_HIP_PHOTOLOSS_H

#ifdef __cplusplus
extern "C" {
#endif

#define RB_PL_ABI_VERSION 1

/* curve: ACESToneMapping's hdr_mode 0 / 1 / 2, 3 for every other hdr_mode (identity), 4 for InvLoss.forward's fallback x / (x + 1) */
#define RB_PL_CURVE_SCALE_ACES 0
#define RB_PL_CURVE_WARP_ACES 1
#define RB_PL_CURVE_LN_SPACE 2
#define RB_PL_CURVE_IDENTITY 3
#define RB_PL_CURVE_RATIONAL 4
#define RB_PL_MAX_GROUPS 1024

typedef void* rb_pl_stream_t; /* hipStream_t */

int rb_pl_abi_version(void);
const char* rb_pl_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * The curves (robir_amd/csrc/photoloss/photoloss_math.h).  x [n, 3]; shift: [n] per row (shift_stride 1) or a single value
 *   (shift_stride 0), clamped to [1e-4, 1] as make_shift does; curves 3 and 4 do not read it (shift may be NULL there).
 *   inverse 0: hdr2ldr, 1: ldr2hdr (curve 4 has no inverse).  rb_tonemap's op 2 (ldr2hdr(x^2.2), used under no_grad only) has no
 *   counterpart here: inverse = 2 is refused.
 * Arithmetic: forward values are fp32 with rb_tonemap's expression order (the same bits).  Derivatives are formed in fp64 from the fp32
 *   inputs and rounded to fp32 once on store.  The clamp passes the shift's gradient on the closed interval [1e-4, 1] and zeroes it outside.
 * Work shape: wave64, 256-thread workgroups, one thread per row (rb_pl_tonemap: per element).  A SCALAR sum (the single-value shift's
 *   gradient, the loss) is reduced in two stages: G = rb_pl_groups(n) = min(ceil(n / 256), 1024) workgroups; thread j of workgroup b takes
 *   the rows 256 b + j, 256 (b + G) + j, ... in that order into an fp64 register, the 256 registers are added by a fixed tree in LDS, the
 *   workgroup stores its partial with a plain store, and a second launch adds the G partials in index order.  No atomics: the order of
 *   every sum is a function of n alone and the same inputs give the same bytes on every run.
 * Scratch: rb_pl_scratch_bytes(n) = 16 rb_pl_groups(n) bytes, 8-byte aligned; contents undefined before and after a call.  Both queries
 *   return -1 for n < 0 and 0 for n == 0.  0 <= n < 2^31.
 * ------------------------------------------------------------------------------------------------------------ */
long rb_pl_groups(long n);
long rb_pl_scratch_bytes(long n);

/* y [n, 3] = curve(x, shift): the bits of rb_tonemap for curves 0 .. 3.  n == 0 returns 0 without a launch. */
int rb_pl_tonemap(const float* x, long n, const float* shift, int shift_stride, int curve, int inverse, float* y, rb_pl_stream_t stream);

/* Reverse mode of the curve for an upstream gradient gy [n, 3]:
 *   gx [n, 3]  = gy * d y / d x                                    (NULL: skipped)
 *   gshift     = sum over a row's three channels of gy * d y / d t  [n] with shift_stride 1; with shift_stride 0 ONE value, the sum over all
 *                rows by the two-stage reduction above (needs scratch)                      (NULL: skipped)
 * Curves 3 and 4 write zeros to gshift.  n == 0 returns 0 without a launch and leaves the outputs untouched. */
int rb_pl_tonemap_bwd(const float* x, long n, const float* shift, int shift_stride, int curve, int inverse, const float* gy, float* gx,
                      float* gshift, void* scratch, long scratch_bytes, rb_pl_stream_t stream);

/* The fused image loss.  With m = net_mask & obj_mask (bytes, non-zero = true), x = sg_rgb + indir_rgb (indir_rgb NULL: absent),
 * pred = hdr2ldr curve(x, shift) and dist = |pred - gt| (l2 == 0) or (pred - gt)^2 (l2 == 1):
 *   loss [1]     = sum_{rows in m} sum_c dist / N          accumulated in fp64 by the two-stage reduction, stored as fp32
 *   g_rgb [N, 3] = d loss / d sg_rgb = d loss / d indir_rgb (NULL: skipped); exact zeros outside m; L1 uses sign(0) = 0
 *   g_shift      = d loss / d shift: [N] (shift_stride 1) or one value (shift_stride 0)      (NULL: skipped)
 * x, pred and every derivative are formed in fp64 from the fp32 inputs.  An empty m gives loss 0 and zero gradients.  Two launches.
 * N == 0 returns 0 without a launch and leaves the outputs untouched. */
int rb_pl_image_loss(const float* sg_rgb, const float* indir_rgb, const float* gt, const unsigned char* net_mask,
                     const unsigned char* obj_mask, long N, const float* shift, int shift_stride, int curve, int l2, float* loss,
                     float* g_rgb, float* g_shift, void* scratch, long scratch_bytes, rb_pl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROBIR_HIP_PHOTOLOSS_H */
