/* robir_hip_illumtrain.h -- C ABI of librobir_hip_illumtrain.so: the training side of the indirect-illumination network (gfx950 / MI355X):
 * the reverse mode of its lobe net and the fused spherical-Gaussian query with its reverse.  A library of its own next to robir_hip.h /
 * robir_hip_legacy.h (ABI version 8), robir_hip_train.h and robir_hip_vistrain.h (ABI version 1 each), whose export lists stay as they are.
 *
 * Conventions, as in robir_hip_vistrain.h:
 *   - every pointer is a DEVICE pointer unless marked HOST; tensors are dense row-major fp32 unless stated;
 *   - the library never allocates, never synchronises and keeps no state: scratch memory is the caller's (a size query says how
 *     much), kernels are enqueued on the given stream (rb_it_stream_t == hipStream_t, 0 = default stream);
 *   - every entry point returns 0 on success, non-zero on error (text via rb_it_last_error(), thread local), never throws, and
 *     validates its arguments BEFORE any launch -- the library loads and answers argument errors on a machine without a GPU;
 *   - plain HIP runtime dependency; no name of this header exists in the other four.
 */
#ifndef ROBIR_HIP_ILLUMTRAIN_H
#define ROBIR_HIP_ILLUMTRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

#define RB_IT_ABI_VERSION 1

typedef void* rb_it_stream_t; /* hipStream_t */

int rb_it_abi_version(void);
const char* rb_it_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * Reverse mode of IndirctIllumNetwork's lobe net (robir_amd/csrc/illumtrain/illum_bwd.hip).
 * Replaces: torch autograd through model/implicit_differentiable_renderer.py:199-218 as the "Illum" stage's radiance_loss
 *           (training/train_visibility.py:297-313, model/loss.py:156-171) differentiates it.
 * The function differentiated, per row i < n:
 *   x        = [PE10(points[i]) | hdr[i]]          64 columns, rb_feat_pe10's layout (hdr in column 63); 63 columns when hdr == NULL
 *   raw      = W4 relu(W3 relu(W2 relu(W1 relu(W0 x + b0) + b1) + b2) + b3) + b4                    64 -> 512 -> 512 -> 512 -> 512 -> 144
 *   lobe j   = raw[6 j .. 6 j + 5] = (a, b, c, m0, m1, m2):  theta = 2 pi sigmoid(a), phi = pi sigmoid(b),
 *   lgt_sgs[i, j, :] = (cos theta sin phi, sin theta sin phi, cos phi, 30 sigmoid(c) + 0.1, relu(m0), relu(m1), relu(m2))
 *   loss     = <g_sgs, lgt_sgs>
 *   params     HOST array of 10 device pointers: W0, b0, ..., W4, b4 -- the nn.Linear tensors themselves, weight row-major [out, in]
 *              (W0 [512,64], or [512,63] when hdr == NULL: the no_hdr net; W4 [144,512]); packed blobs are not read
 *   g_sgs [n,24,7]
 *   grads      HOST array of 10 device pointers in the order of params, each in its parameter's own shape; any may be NULL: that
 *              gradient is not formed.  The data path stops at the lowest layer that wants one.  No gradient with respect to points or hdr.
 * Arithmetic: the encoding is evaluated in fp64 from the fp32 coordinates (x 2^k is exact; sin / cos in double), the four hidden
 *   activations and the raw output are recomputed in fp64 from the fp32 parameters, a ReLU gate is `pre-activation > 0` of that
 *   evaluation, the head's derivative is written out in fp64 from the raw output, and the three product families -- activations,
 *   dZ_{l-1} = (dZ_l W_l) . gate, dW_l = dZ_l^T A_{l-1} with db_l = sum dZ_l as one more column -- are formed in fp64 on
 *   v_mfma_f64_16x16x4_f64; each stored gradient is rounded to fp32 once.
 * Rows and reduction: rows are processed in slabs of slab_rows (the last one shorter).  Inside a slab the row range of a weight gradient
 *   is cut into contiguous partitions of part_rows rows (the last one shorter); one workgroup owns one (64 x 64 output tile, partition),
 *   sums the partition's rows in row order and stores an fp64 partial; a second kernel adds a slab's partials in partition order into the
 *   layer's fp64 accumulator, slabs add in slab order, a last kernel rounds.  No atomics.  The association is a function of
 *   (n, slab_rows, part_rows) alone -- never of the number of compute units or of occupancy: the same arguments give the same bytes on every
 *   run; other slab_rows / part_rows change the fp64 association only.  part_rows == slab_rows is the unsplit form.
 * Scratch: rb_it_lobe_bwd_scratch_bytes(n, slab_rows, part_rows) bytes, 8-byte aligned, a function of S = min(n, slab_rows) and part_rows
 *   only: 26240 B per slab row (64 + 4 x 512 + 144 activations and two 512-wide gradient buffers, doubles), 2101248 B (one 512 x 513
 *   partial) per partition of a slab, and 7160960 B of accumulators -- 148 MB at the Python defaults (4096, 256).  -1 on an argument
 *   error.  Contents are undefined before and after the call.
 * stats (HOST int[3], may be NULL): [0] kernels enqueued by the call, [1] the lowest layer differentiated (0..4; 5 when nothing was),
 *   [2] partitions of a full slab, ceil(min(n, slab_rows) / part_rows).
 * n == 0, or every entry of grads NULL, returns 0 without a launch and leaves grads untouched.
 * 1 <= part_rows <= slab_rows <= 2^20.
 * ------------------------------------------------------------------------------------------------------------ */
long rb_it_lobe_bwd_scratch_bytes(long n, long slab_rows, long part_rows);
int rb_it_lobe_bwd(const float* points, const float* hdr /* [n,1] or NULL */, long n, const float* const* params /* HOST[10] */,
                   const float* g_sgs, float* const* grads /* HOST[10] */, long slab_rows, long part_rows, void* scratch,
                   long scratch_bytes, int* stats /* HOST[3] */, rb_it_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * The spherical-Gaussian query and its reverse.
 * Replaces: query_indir_illum (model/loss.py:128-141) and torch autograd through its [n, S, L, 3] expansion.
 *   radiance[i, s, :] = sum_j mu_ij exp(lambda_ij (d_is . l_ij / |l_ij| - 1))
 *   sgs [n,L,7] = (l [3], lambda, mu [3]) per lobe, dirs [n,S,3], radiance [n,S,3];  1 <= L <= 32.  The lobe axis is divided by its norm,
 *   as the reference does (a zero axis gives the reference's NaN).
 * rb_it_sg_query: evaluated in fp64 from the fp32 inputs, lobes added in lobe order, one rounding per stored value.
 * rb_it_sg_query_bwd: g_sgs [n,L,7] = d <g_radiance, radiance> / d sgs: g_mu, g_lambda and g_l, the last through the normalisation (the
 *   tangential projection of the gradient on the unit axis, divided by |l|).  g_radiance [n,S,3] is dense: zeros at masked samples.  No
 *   gradient for dirs.  fp64 arithmetic, one rounding per stored value, no scratch, no atomics: one workgroup of 256 lanes owns one point,
 *   lane t adds the samples t, t + 256, ... in that order and the 256 lane sums meet in a fixed binary tree, so the association is a
 *   function of S alone and equal inputs give equal bytes.
 * n == 0 returns 0 without a launch, and so does S == 0 for rb_it_sg_query; rb_it_sg_query_bwd with S == 0 stores zeros.
 * ------------------------------------------------------------------------------------------------------------ */
int rb_it_sg_query(const float* sgs, const float* dirs, long n, int L, long S, float* radiance, rb_it_stream_t stream);
int rb_it_sg_query_bwd(const float* sgs, const float* dirs, const float* g_radiance, long n, int L, long S, float* g_sgs,
                       rb_it_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROBIR_HIP_ILLUMTRAIN_H */
