/* robir_hip_texfit.h -- C ABI of librobir_hip_texfit.so: fitting the texels of a baked atlas through the mesh view on the device (gfx950 /
 * MI355X).  The linearisation of the G-buffer's plane fetch (taps), the fetch formed from it, its transpose as a gather over (row, tap)
 * pairs sorted by texel, and a lazy Adam step on the touched texels; robir_amd/texfit.py builds the loop around them.  A
 * library of its own next to the twelve others, whose export lists and ABI versions stay as they are.
 *
 * Conventions, as in the other auxiliary libraries' headers:
 *   - every pointer is a DEVICE pointer unless stated; tensors are dense row-major, fp32 / int32 unless stated;
 *   - the library never allocates, never synchronises and keeps no state; kernels are enqueued on the given stream (rb_tf_stream_t ==
 *     hipStream_t, 0 = default stream);
 *   - every entry point returns 0 on success, non-zero on error (text via rb_tf_last_error(), thread local), never throws, and validates
 *     its arguments BEFORE any launch -- the library loads and answers argument errors on a machine without a GPU;
 *   - gather kernels, no atomics; the order of every sum is a function of the inputs' layout alone, so the same inputs give the same bytes
 *     on every run, and tests/texfit_restatement.py reproduces every kernel bit for bit;
 *   - plain HIP runtime dependency; this header names no other library.
 *
 * The atlas is a plane stack planes [R,R,Cs], row 0 at the top, 1 <= R <= 16384; a call works on its first C channels, 1 <= C <= Cs <= 16.
 * texel = row R + column.  n < 2^29 rows, so that the 4 n (row, tap) pairs fit int32.
 *
 * The fetch at (u, v) (v up, as in an OBJ) is the bilinear one with zero padding:
 *     x = u R - 0.5,  y = (1 - v) R - 0.5,  x0 = floor x,  y0 = floor y,
 *     wx1 = x - x0,  wx0 = (x0 + 1) - x,  wy1 = y - y0,  wy0 = (y0 + 1) - y,
 *     taps nw, ne, sw, se = texels (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1) with weights wx0 wy0, wx1 wy0, wx0 wy1, wx1 wy1,
 *     value = ((a nw + b ne) + c sw) + d se,
 * plain fp32 with one rounding per operation.  filter 0 is the texel that contains the uv: column floor(u R), row floor((1 - v) R), clamped
 * to the image (NaN -> 0), one tap of weight 1.
 */
#ifndef ROBIR_HIP_TEXFIT_H
#define ROBIR_HIP_TEXFIT_H

#ifdef __cplusplus
extern "C" {
#endif

#define RB_TF_ABI_VERSION 1
#define RB_TF_MAX_RESOLUTION 16384
#define RB_TF_MAX_CHANNELS 16
#define RB_TF_MAX_ROWS ((1L << 29) - 1)

typedef void* rb_tf_stream_t; /* hipStream_t */

int rb_tf_abi_version(void);
const char* rb_tf_last_error(void);

/* uv [n,2] -> tap_texel [n,4] int32, tap_weight [n,4]: the four taps of the fetch above in the order nw, ne, sw, se, one thread per row.
 * A tap outside the image gets texel -1 and weight +0 (a uv that is not finite: four such taps).  filter 0: tap 0 is the containing texel
 * with weight 1, the three others are -1 / +0.  n == 0 returns 0 without a launch. */
int rb_tf_taps(const float* uv, long n, int R, int filter, int* tap_texel, float* tap_weight, rb_tf_stream_t stream);

/* tex [n,C] = ((a w0 + b w1) + c w2) + d w3 over the first C channels of planes [R,R,Cs], a .. d the texels of the row's four taps; an absent
 * tap (texel outside [0, R R)) contributes the product 0 w.  One thread per row.  For a finite uv these are the bits of the view's own
 * plane fetch.  n == 0 returns 0 without a launch. */
int rb_tf_fetch(const float* planes, int R, int Cs, const int* tap_texel, const float* tap_weight, long n, int C, float* tex,
                rb_tf_stream_t stream);

/* The transpose of the fetch as a gather.  The caller has sorted the P (row, tap) pairs by texel with a STABLE sort (pairs of one texel
 * stay in ascending 4 row + tap order; absent taps sort to the tail, beyond seg_start[T]): pair_row [P] int32, pair_weight [P]; segment s
 * is the pair range [seg_start[s], seg_start[s + 1]) of one touched texel, seg_start [T + 1] int32.  One thread per segment:
 *     grad[s][c] = sum_p (double) pair_weight[p] (double) g_tex[pair_row[p]][c],   g_tex [n,C], grad [T,C],
 * added in ascending p into an fp64 register and rounded to fp32 once.  A segment's bounds are clipped to [0, P]; a row index outside
 * [0, n) contributes nothing and is never read.  T == 0 or P == 0 returns 0 without a launch. */
int rb_tf_scatter(const int* pair_row, const float* pair_weight, long P, const int* seg_start, long T, const float* g_tex, long n, int C,
                  float* grad, rb_tf_stream_t stream);

/* Lazy Adam on the touched texels, one thread per (segment, channel): texel seg_texel[s], channel c < C of planes [R,R,Cs] with the moments
 * adam_m, adam_v [R,R,C] and the gradient grad [T,C].  A texel that no segment names is neither read nor written: its moments do not
 * decay.  lr, lo, hi: HOST arrays of C doubles (step size and clamp per channel); bc1 = 1 - beta1^t, bc2 = 1 - beta2^t are formed by the
 * caller in double.  In fp64 from the fp32 inputs, each stored value rounded once:
 *     m' = beta1 m + (1 - beta1) g;   v' = beta2 v + (1 - beta2) (g g);   both stored as fp32;
 *     p' = min(max(p - lr_c (m' / bc1) / (sqrt(v' / bc2) + eps), lo_c), hi_c) with the STORED m', v'.
 * A texel index outside [0, R R) is skipped.  seg_texel must not name a texel twice (two threads would write one element): the segments
 * built from a sorted pair list never do.  T == 0 returns 0 without a launch. */
int rb_tf_adam(float* planes, float* adam_m, float* adam_v, const int* seg_texel, const float* grad, long T, int R, int Cs, int C,
               const double* lr, const double* lo, const double* hi, double beta1, double beta2, double eps, double bc1, double bc2,
               rb_tf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROBIR_HIP_TEXFIT_H */
