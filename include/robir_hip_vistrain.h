/* robir_hip_vistrain.h -- C ABI of librobir_hip_vistrain.so: the reverse mode of the visibility network (gfx950 / MI355X), a library of
 * its own next to robir_hip.h / robir_hip_legacy.h (ABI version 8) and robir_hip_train.h (ABI version 1), whose export lists stay as they are.
 *
 * Conventions, as in robir_hip_train.h:
 *   - every pointer is a DEVICE pointer unless marked HOST; tensors are dense row-major fp32 unless stated;
 *   - the library never allocates, never synchronises and keeps no state: scratch memory is the caller's (a size query says how
 *     much), kernels are enqueued on the given stream (rb_vt_stream_t == hipStream_t, 0 = default stream);
 *   - every entry point returns 0 on success, non-zero on error (text via rb_vt_last_error(), thread local), never throws, and
 *     validates its arguments BEFORE any launch -- the library loads and answers argument errors on a machine without a GPU;
 *   - plain HIP runtime dependency; no name of this header exists in the other three.
 */
#ifndef ROBIR_HIP_VISTRAIN_H
#define ROBIR_HIP_VISTRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

#define RB_VT_ABI_VERSION 1

typedef void* rb_vt_stream_t; /* hipStream_t */

int rb_vt_abi_version(void);
const char* rb_vt_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * Reverse mode of VisNetwork (robir_amd/csrc/vistrain/vis_bwd.hip).
 * Replaces: torch autograd through model/implicit_differentiable_renderer.py:250-258 (VisNetwork.forward) as the "Vis" stage
 *           (training/train_visibility.py:297-308, model/loss.py:173-177) differentiates it.
 * The function differentiated, per row i < M:
 *   x        = [PE10(p[i / rep]) | PE10(d[i])]                126 columns, PE10(v) = [v | sin 2^0 v | cos 2^0 v | ... | cos 2^9 v]
 *   logits   = W4 relu(W3 relu(W2 relu(W1 relu(W0 x + b0) + b1) + b2) + b3) + b4            126 -> 256 -> 256 -> 256 -> 256 -> 2
 *   loss     = <g_logits, logits>
 *   p [M/rep,3], d [M,3]   rep consecutive directions share one point (rep >= 1, M % rep == 0)
 *   params     HOST array of 10 device pointers: W0, b0, ..., W4, b4 -- the nn.Linear tensors themselves, weight row-major [out, in]
 *              (W0 [256,126], W4 [2,256]); packed blobs are not read
 *   g_logits [M,2]
 *   grads      HOST array of 10 device pointers in the order of params, each in its parameter's own shape; any may be NULL: that
 *              gradient is not formed.  The data path stops at the lowest layer that wants one.  No gradient with respect to p or d.
 * Arithmetic: the encoding is evaluated in fp64 from the fp32 coordinates (x 2^k is exact; sin / cos in double), the four hidden
 *   activations are recomputed in fp64 from the fp32 parameters, a ReLU gate is `pre-activation > 0` of that evaluation, and the three
 *   product families -- activations, dZ_{l-1} = (dZ_l W_l) . gate, dW_l = dZ_l^T A_{l-1} with db_l = sum dZ_l as one more column -- are
 *   formed in fp64 on v_mfma_f64_16x16x4_f64; each stored gradient is rounded to fp32 once.
 * Rows and reduction: rows are processed in slabs of slab_rows (the last one shorter).  Inside a slab the row range of a weight gradient
 *   is cut into contiguous partitions of part_rows rows (the last one shorter); one workgroup owns one (64 x 64 output tile, partition),
 *   sums the partition's rows in row order and stores an fp64 partial; a second kernel adds a slab's partials in partition order into the
 *   layer's fp64 accumulator, slabs add in slab order, a last kernel rounds.  No atomics.  The association is a function of
 *   (M, slab_rows, part_rows) alone -- never of the number of compute units or of occupancy: the same arguments give the same bytes on every
 *   run; other slab_rows / part_rows change the fp64 association only.  part_rows == slab_rows is the unsplit form.
 * Scratch: rb_vt_vis_bwd_scratch_bytes(M, slab_rows, part_rows) bytes, 8-byte aligned, a function of S = min(M, slab_rows) and part_rows
 *   only: 13312 B per slab row (128 + 4 x 256 activations and two 256-wide gradient buffers, doubles), 526336 B (one 256 x 257 partial) per
 *   partition of a slab, and 1.8 MB of accumulators -- 227 MB at the Python defaults (16384, 1024).  -1 on an argument error.  Contents
 *   are undefined before and after the call.
 * stats (HOST int[3], may be NULL): [0] kernels enqueued by the call, [1] the lowest layer differentiated (0..4; 5 when nothing was),
 *   [2] partitions of a full slab, ceil(min(M, slab_rows) / part_rows).
 * M == 0, or every entry of grads NULL, returns 0 without a launch and leaves grads untouched.
 * rep >= 1, M % rep == 0, 1 <= part_rows <= slab_rows <= 2^20.
 * ------------------------------------------------------------------------------------------------------------ */
long rb_vt_vis_bwd_scratch_bytes(long M, long slab_rows, long part_rows);
int rb_vt_vis_bwd(const float* p, const float* d, long M, int rep, const float* const* params /* HOST[10] */, const float* g_logits,
                  float* const* grads /* HOST[10] */, long slab_rows, long part_rows, void* scratch, long scratch_bytes,
                  int* stats /* HOST[3] */, rb_vt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROBIR_HIP_VISTRAIN_H */
