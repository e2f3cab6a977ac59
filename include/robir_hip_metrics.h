/* robir_hip_metrics.h -- C ABI of librobir_hip_metrics.so: image metrics on the device (gfx950 / MI355X).
 * The sums behind MSE, MAE, PSNR and the albedo ratio, the angular error of two normal fields and Wang et al.'s SSIM, for V views at once,
 * with the transfer (clip, gamma 2.2, 8-bit quantisation) applied on load -- the evaluation protocol of the relighting tool chain
 * (scripts/relight.py:19-20 tone maps and clips what it writes).  A library of its own next to the two renderer libraries and the eight
 * other auxiliary libraries, whose export lists and ABI versions stay as they are.
 *
 * Conventions, as in the training libraries' headers:
 *   - every pointer is a DEVICE pointer; images are dense row-major fp32, channels last; masks are bytes (non-zero = true);
 *   - the library never allocates, never synchronises and keeps no state: scratch memory is the caller's (a size query says how
 *     much), kernels are enqueued on the given stream (rb_mt_stream_t == hipStream_t, 0 = default stream);
 *   - every entry point returns 0 on success, non-zero on error (text via rb_mt_last_error(), thread local), never throws, and
 *     validates its arguments BEFORE any launch -- the library loads and answers argument errors on a machine without a GPU;
 *   - plain HIP runtime dependency; no name of this header exists in the other ten.
 */
#ifndef ROBIR_HIP_METRICS_H
#define ROBIR_HIP_METRICS_H

#ifdef __cplusplus
extern "C" {
#endif

#define RB_MT_ABI_VERSION 1

/* T, applied on load to both images: p = T(scale_c * pred), g = T(gt); scale [C] is a per-channel fp32 factor on the prediction (NULL: 1).
 * T is formed in fp64 from the fp32 inputs: nothing | min(max(x, 0), 1) | clip(max(x, 0)^(1 / 2.2)) | the last followed by
 * floor(255 x) / 255 (the value an 8-bit PNG of the tone-mapped image holds). */
#define RB_MT_NONE 0
#define RB_MT_CLIP 1
#define RB_MT_GAMMA22 2
#define RB_MT_GAMMA22_Q8 3

#define RB_MT_MAX_CHANNELS 4
#define RB_MT_MAX_VIEWS 65535
#define RB_MT_ROWS 256        /* rows per workgroup of the pair / angular kernels */
#define RB_MT_MAX_GROUPS 1024 /* workgroups per view of the pair / angular kernels */
#define RB_MT_SSIM_TILE 16    /* SSIM outputs per workgroup and axis */

typedef void* rb_mt_stream_t; /* hipStream_t */

int rb_mt_abi_version(void);
const char* rb_mt_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * Reductions.  Every per-view sum is fp64 and is taken in two stages, without atomics: a first launch of
 * G x V workgroups (wave64, 256 threads) leaves G partial sums per view with plain stores, a second launch of V workgroups adds each view's
 * partials in index order, one thread per output value.  The order of every sum is a function of the sizes alone: the same inputs give the
 * same bytes on every run.  One launch pair serves all V views.
 *   pair / angular: G = rb_mt_groups(P) = min(ceil(P / 256), 1024); thread j of workgroup b takes the rows 256 b + j, 256 (b + G) + j, ...
 *     of its view in that order into fp64 registers; the 256 registers are added by a fixed tree in LDS.
 *   SSIM: G = rb_mt_ssim_tiles(H, W) = ceil((H - 10) / 16) ceil((W - 10) / 16), one workgroup per 16 x 16 tile of the map, tiles in
 *     row-major order; the 256 windows of a tile are added by the same tree.
 * Scratch: 8 G V K bytes, K = 1 + 5 C (pair), 2 (angular, SSIM); 8-byte aligned; contents undefined before and after a call.
 * Every query returns -1 on a negative (or otherwise refused) size and 0 on an empty one.  0 <= V <= 65535, 0 <= P < 2^31, H W < 2^31.
 * ------------------------------------------------------------------------------------------------------------ */
long rb_mt_groups(long P);
long rb_mt_ssim_tiles(long H, long W);
long rb_mt_pair_scratch_bytes(long V, long P, int C);
long rb_mt_angular_scratch_bytes(long V, long P);
long rb_mt_ssim_scratch_bytes(long V, long H, long W);

/* pred, gt [V, P, C], 1 <= C <= 4; mask [V, P] or NULL (every pixel).  stats [V][1 + 5 C] fp64, per view:
 *   stats[0]                 the number of masked pixels
 *   stats[1 + 5 c + 0 .. 4]  over the masked pixels, of channel c:  sum d^2, sum |d|, sum p g, sum p^2, sum g^2     (d = p - g)
 * Every product and sum is fp64.  An empty mask gives zeros.  V == 0 or P == 0 returns 0 without a launch and leaves stats untouched. */
int rb_mt_pair_stats(const float* pred, const float* gt, long V, long P, int C, const unsigned char* mask, const float* scale, int transfer,
                     double* stats, void* scratch, long scratch_bytes, rb_mt_stream_t stream);

/* a, b [V, P, 3]; mask [V, P] or NULL.  stats [V][2] fp64, per view: {count, sum of angle}, angle = acos(clamp(a^ . b^, -1, 1)) in radians,
 * the unit vectors formed in fp64.  A row where either vector is shorter than 1e-6 (the masked rows of a render hold zeros) is left out of
 * both.  V == 0 or P == 0 returns 0 without a launch and leaves stats untouched. */
int rb_mt_angular_stats(const float* a, const float* b, long V, long P, const unsigned char* mask, double* stats, void* scratch,
                        long scratch_bytes, rb_mt_stream_t stream);

/* SSIM (Wang et al. 2004) of pred, gt [V, H, W, C], 1 <= C <= 4: an 11-tap Gaussian window, sigma = 1.5, weights exp(-x^2 / 4.5) normalised
 * in fp64; K1 = 0.01, K2 = 0.03, data range 1; population moments (var = E[x^2] - mu^2); VALID windows only: the map has
 * (H - 10) x (W - 10) entries per channel, H < 11 or W < 11 is an argument error.  mask [V, H, W] or NULL: a window counts when its CENTRE
 * pixel (row i + 5, column j + 5 of the image for entry i, j of the map) is in the mask.
 *   stats [V][2] fp64, per view: {the number of counted windows, the sum of SSIM over the channels and the counted windows}
 *   map [V, H - 10, W - 10, C] fp32 or NULL: the SSIM of every counted window, exact zeros at the others
 * The five moments (x, y, x^2, y^2, x y) and the quotient are fp64; a map entry is rounded to fp32 once; the per-view sum is taken from
 * the fp64 values, not from the rounded map.  Separable: a workgroup loads its 16 x 16 tile plus the 10-pixel halo of both images (all
 * channels, transferred) into LDS once, runs the horizontal pass into LDS and the vertical pass into registers.
 * V == 0 returns 0 without a launch and leaves the outputs untouched. */
int rb_mt_ssim(const float* pred, const float* gt, long V, long H, long W, int C, const unsigned char* mask, const float* scale, int transfer,
               double* stats, float* map, void* scratch, long scratch_bytes, rb_mt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROBIR_HIP_METRICS_H */
