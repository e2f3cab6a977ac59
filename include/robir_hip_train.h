/* robir_hip_train.h -- C ABI of librobir_hip_train.so: the training-side kernels (gfx950 / MI355X), kept apart from the forward
 * renderer's two libraries (robir_hip.h, robir_hip_legacy.h: their export lists are frozen at ABI version 8).
 *
 * Conventions, as in robir_hip.h:
 *   - every pointer is a DEVICE pointer unless marked HOST; tensors are dense row-major fp32 unless stated;
 *   - the library never allocates, never synchronises and keeps no state: scratch memory is the caller's (a size query says how
 *     much), kernels are enqueued on the given stream (rb_train_stream_t == hipStream_t, 0 = default stream);
 *   - every entry point returns 0 on success, non-zero on error (text via rb_train_last_error(), thread local), never throws, and
 *     validates its arguments BEFORE any launch -- the library loads and answers argument errors on a machine without a GPU;
 *   - plain HIP runtime dependency; no name of this header exists in the other two.
 */
#ifndef ROBIR_HIP_TRAIN_H
#define ROBIR_HIP_TRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

#define RB_TRAIN_ABI_VERSION 1

typedef void* rb_train_stream_t; /* hipStream_t */

int rb_train_abi_version(void);
const char* rb_train_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * Reverse mode of one SparseAE with smooth_on_latent=True (robir_amd/csrc/train/ae_bwd.hip).
 * Replaces: torch autograd through model/sg_envmap_material.py:74-99 (SparseAE.forward / encode) as stage 3 of
 *           training/train_pbr.py:104-105,348-396 differentiates it.
 * The function differentiated, per row x = X[i, :in_dim]:
 *   encoder   in_dim -> 512 -> 512 -> 512 -> 512 -> 32, LeakyReLU(0.2) between the layers, none after the last
 *   e         = encoder(x) * (1 - var)                         the pre-activation latent, what SparseAE.encode returns
 *   lat       = sigmoid(e) (latent_act 0) | softplus(e) (1);   lat_xi = lat + noise[i] * noise_scale
 *   decoder   32 -> 128 -> 128 -> out_dim, LeakyReLU(0.2) between; out = f(decoder(lat)), out_xi = f(decoder(lat_xi)),
 *             f = sigmoid (out_act 1) | identity (0)
 *   loss      = <g_out, out> + <g_out_xi, out_xi> + <g_raw, e>       each upstream gradient may be NULL (absent term)
 *   X [n,64]       the fp32 feature rows the forward consumed (rb_feat_pe10's layout; columns >= in_dim are not read)
 *   noise [n,32]   may be NULL (lat_xi = lat);  var [32] may be NULL (zero)
 *   params         HOST array of 16 device pointers: encoder weight 0, bias 0, ..., weight 4, bias 4, decoder weight 0, bias 0, ...,
 *                  weight 2, bias 2 -- the nn.Linear tensors themselves, weight row-major [out, in] (the first one [512, in_dim],
 *                  NOT padded to 64); packed blobs are not read
 *   g_out, g_out_xi [n,out_dim], g_raw [n,32]
 *   grads          HOST array of 16 device pointers in the order of params, each in its parameter's own shape; any may be NULL:
 *                  that gradient is not formed.  The data path stops at the lowest layer that wants one -- with no encoder
 *                  gradient asked for, the backward stops at the latent and the encoder is only re-evaluated forwards.
 *                  No gradient with respect to X.
 * Arithmetic: the layer activations are recomputed from X and the fp32 parameters in fp64 (LeakyReLU side decisions are those of a
 *   float64 evaluation), and the three product families -- activations, dX = (dY . act') W, dW = dZ^T A with db = sum dZ as one more
 *   column -- are formed in fp64 on v_mfma_f64_16x16x4_f64; each stored gradient is rounded to fp32 once.
 * Reduction over rows: rows are processed in slabs of slab_rows (the last one shorter); within a slab one thread owns one element
 *   of a layer's fp64 accumulator and sums the slab's rows in row order (no atomics, no split of the row range); the slabs add into it
 *   in slab order.  The same (inputs, n, slab_rows) give the same bytes on every run; a different slab_rows changes the fp64
 *   association only.  The decoder's two passes are rows [0,S) and [S,2S) of one problem: their weight gradients are one sum.
 * Scratch: rb_train_ae_bwd_scratch_bytes(n, slab_rows, in_dim, out_dim) bytes, 8-byte aligned, a function of min(n, slab_rows) only
 *   (about 34.6 KB per slab row + 7 MB of accumulators); -1 on an argument error.  Contents are undefined before and after the call.
 * stats (HOST int[2], may be NULL): [0] kernels enqueued by the call, [1] 1 if the encoder was differentiated, 0 if the backward
 *   stopped at the latent.
 * n == 0 returns 0 without a launch and leaves grads untouched.  1 <= in_dim <= 64, 1 <= out_dim <= 16, 1 <= slab_rows <= 2^20.
 * ------------------------------------------------------------------------------------------------------------ */
long rb_train_ae_bwd_scratch_bytes(long n, long slab_rows, int in_dim, int out_dim);
int rb_train_ae_bwd(const float* X, long n, int in_dim, const float* noise, double noise_scale, const float* var, int latent_act,
                    int out_act, int out_dim, const float* const* params /* HOST[16] */, const float* g_out, const float* g_out_xi,
                    const float* g_raw, float* const* grads /* HOST[16] */, long slab_rows, void* scratch, long scratch_bytes,
                    int* stats /* HOST[2] */, rb_train_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROBIR_HIP_TRAIN_H */
