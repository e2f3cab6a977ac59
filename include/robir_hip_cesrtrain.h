/* robir_hip_cesrtrain.h -- C ABI of librobir_hip_cesrtrain.so: the training side of the two CESR networks (gfx950 / MI355X): the reverse
 * mode of shadow_net and normal_net, the 512 x 8 weight-normed softplus-100 SDFNetwork shapes of training/train_cesr.py:107-110.  A library
 * of its own next to robir_hip.h / robir_hip_legacy.h (ABI version 8), robir_hip_train.h, robir_hip_vistrain.h and robir_hip_illumtrain.h
 * (ABI version 1 each), whose export lists stay as they are.
 *
 * Conventions, as in robir_hip_vistrain.h:
 *   - every pointer is a DEVICE pointer unless marked HOST; tensors are dense row-major fp32 unless stated;
 *   - the library never allocates, never synchronises and keeps no state: scratch memory is the caller's (a size query says how
 *     much), kernels are enqueued on the given stream (rb_ct_stream_t == hipStream_t, 0 = default stream);
 *   - every entry point returns 0 on success, non-zero on error (text via rb_ct_last_error(), thread local), never throws, and
 *     validates its arguments BEFORE any launch -- the library loads and answers argument errors on a machine without a GPU;
 *   - plain HIP runtime dependency; no name of this header exists in the other five.
 */
#ifndef ROBIR_HIP_CESRTRAIN_H
#define ROBIR_HIP_CESRTRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

#define RB_CT_ABI_VERSION 1

typedef void* rb_ct_stream_t; /* hipStream_t */

int rb_ct_abi_version(void);
const char* rb_ct_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * Reverse mode of the CESR networks (robir_amd/csrc/cesrtrain/cesr_bwd.hip).
 * Replaces: torch autograd through model/neus_model.py:312-417 as training/train_cesr.py differentiates shadow_net / normal_net.
 * kind 0: normal_net, d_in = 63, d_out = 3.  kind 1: shadow_net, d_in = 191, d_out = 2.
 * The function differentiated, per row i < M:
 *   x      = [PE10(points[i / n_label]) | onehot(i % n_label, 128)]   kind 1, points form: 191 columns, rb_feat_pe10's column order
 *          = PE10(points[i])                                          kind 0, points form: 63 columns (n_label must be 1)
 *          = rows[i * ld .. i * ld + d_in - 1]                        dense form: the caller's rows, ld >= d_in
 *   h      = x;  for l in 0..8:  l == 4: h = [h | x] / sqrt(2);  h = W_l h + b_l;  l < 8: h = softplus(h, beta = 100)
 *   W_l    = g_l v_l / |v_l|_row                                      (weight norm over dim 0; lin3 has 512 - d_in rows)
 *   loss   = <g_out, head(h)>
 *   head 0: the raw output, g_out [M, d_out].
 *   head 1: the class-1 probability of the two-class softmax, g_out [M] (kind 1 only).
 *   head 2: raw / max(|raw|, 1e-4), g_out [M, 3] (kind 0 only).
 *   Exactly one of points / rows is non-NULL.  points [M / n_label, 3]; rows [M, ld].
 *   params     HOST array of 27 device pointers: lin{l}.weight_g [out,1], lin{l}.weight_v [out,in], lin{l}.bias [out] for l = 0..8 -- the
 *              module's own tensors; packed blobs are not read
 *   grads      HOST array of 27 device pointers in the order of params, each in its parameter's own shape; any may be NULL: that
 *              gradient is not formed.  The data path stops at the lowest layer that wants one.  No gradient for points or rows.
 * Arithmetic: the encoding is evaluated in fp64 from the fp32 coordinates (x 2^k is exact; sin / cos in double); the one-hot block of the
 *   points form is built from the row index.  The weight norm is folded in fp64 (W_l; the 1/sqrt(2) of the skip layer rides in W_4, which
 *   is the same function), the eight activations and the raw output are recomputed in fp64.  The stored activation follows torch's
 *   softplus: a = z where 100 z > 20, log1p(exp(100 z)) / 100 below.  ONE buffer per layer: the gate sigmoid(100 z) is recovered from
 *   the stored activation as -expm1(-100 a); above the threshold that is 1 - exp(-100 z) where torch's gate is exactly 1 (a difference
 *   below 2.1e-9), without a special case.  The head's derivative is written out in fp64 from the raw output.  The three product
 *   families -- activations, dZ_{l-1} = (dZ_l W_l) . gate, dW_l = dZ_l^T A_{l-1} with db_l = sum dZ_l as one more column -- are formed on
 *   v_mfma_f64_16x16x4_f64; the skip layer backpropagates into its first 512 - d_in input columns only.  The label columns of dW_0 and
 *   dW_4 are formed by the same product against the one-hot columns of x.  A last kernel maps the fp64 dW_l to
 *   dv_l = (g / |v|) (dW - (dW . v^) v^), dg_l = dW . v^ (v^ = v / |v|, per row) in fp64 and rounds each stored gradient to fp32 once.
 * Rows and reduction: rows are processed in slabs of slab_rows (the last one shorter).  Inside a slab the row range of a weight gradient
 *   is cut into contiguous partitions of part_rows rows (the last one shorter); one workgroup owns one (64 x 64 output tile, partition),
 *   sums the partition's rows in row order and stores an fp64 partial; a second kernel adds a slab's partials in partition order into the
 *   layer's fp64 accumulator, slabs add in slab order.  No atomics.  The association is a function of (M, slab_rows, part_rows) alone:
 *   the same arguments give the same bytes on every run; other slab_rows / part_rows change the fp64 association only.
 * Scratch: rb_ct_cesr_bwd_scratch_bytes(M, slab_rows, part_rows) bytes, 8-byte aligned, a function of S = min(M, slab_rows) and part_rows
 *   only (the same for both kinds): 42560 B per slab row (192 input columns, 8 x 512 activations, 8 for the raw output and two 512-wide
 *   gradient buffers, doubles), 2101248 B (one 512 x 513 partial) per partition of a slab, and 30986304 B of folded weights and
 *   accumulators.  -1 on an argument error.  Contents are undefined before and after the call.
 * stats (HOST int[3], may be NULL): [0] kernels enqueued by the call, [1] the lowest layer differentiated (0..8; 9 when nothing was),
 *   [2] partitions of a full slab, ceil(min(M, slab_rows) / part_rows).
 * M == 0, or every entry of grads NULL, returns 0 without a launch and leaves grads untouched.
 * 1 <= n_label <= 128, M % n_label == 0, 1 <= part_rows <= slab_rows <= 2^20.
 * ------------------------------------------------------------------------------------------------------------ */
long rb_ct_cesr_bwd_scratch_bytes(long M, long slab_rows, long part_rows);
int rb_ct_cesr_bwd(const float* points, const float* rows, long ld, long M, int kind, int n_label, int head,
                   const float* const* params /* HOST[27] */, const float* g_out, float* const* grads /* HOST[27] */, long slab_rows,
                   long part_rows, void* scratch, long scratch_bytes, int* stats /* HOST[3] */, rb_ct_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROBIR_HIP_CESRTRAIN_H */
