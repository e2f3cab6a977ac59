// librobir_hip_train.so: reverse mode of one SparseAE with smooth_on_latent=True (include/robir_hip_train.h).
//
// Everything is fp64: the layer activations are recomputed from the fp32 feature rows and the fp32 nn.Linear parameters, the three product
// families (activations, dX = (dY . act') W, dW = dZ^T A | db = sum dZ) run on v_mfma_f64_16x16x4_f64 through the training libraries' one
// tiled kernel (k_gemm64 of gemm64.h, instantiated here for LeakyReLU(0.2) and in-place accumulation) under the slab driver the four
// training libraries share (chain.h), and each stored gradient is rounded to fp32 once (k_finish).  This file holds what is particular to
// the auto-encoder: its latent and output kernels, its plan, its argument checks and the two-pass order of its slab loop.
//
// Reductions over rows: dW / db of a layer is a GEMM whose REDUCTION dimension is the slab's rows; one thread owns one element of the fp64
// accumulator (no atomics, no split over rows: wgrad_acc of chain.h), slabs are enqueued in order on one stream and add into that element
// in slab order.  The accumulation order is therefore a function of (n, slab_rows) alone.
//
// The decoder's two passes (clean latent | latent + noise * scale) are stacked as 2 S rows of one problem: their weight gradients are one sum.
#include "../../../include/robir_hip_train.h"
#include "chain.h"

namespace {

// LeakyReLU(0.2) where the act flag is set; weight gradients add in place, slab by slab
constexpr auto fwd = fwd_layer<ACT_LEAKY, RED_ACC>;
constexpr auto wgrad = wgrad_acc<ACT_LEAKY, RED_ACC>;
constexpr auto bwd = dgrad<ACT_LEAKY, RED_ACC>;

__device__ __forceinline__ double sigmoid64(double x) { return 1.0 / (1.0 + exp(-x)); }

// raw [S,32] (encoder output) -> E = raw (1 - var), LAT rows [0,S) = act(E), rows [S,2S) = act(E) + noise * scale
__global__ void k_latent(const double* raw, const float* var, const float* noise, double scale, int act, long S, double* E, double* LAT) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * 32) return;
    const int j = (int)(i & 31);
    const double e = raw[i] * (1.0 - (var ? (double)var[j] : 0.0));
    E[i] = e;
    const double lat = act == 0 ? sigmoid64(e) : (e > 20.0 ? e : log1p(exp(e)));      // F.softplus: beta 1, threshold 20
    LAT[i] = lat;
    LAT[S * 32 + i] = lat + (noise ? (double)noise[i] * scale : 0.0);
}

// Z [2S,od] pre-activation outputs -> in place d loss / d Z = upstream * out_act'(Z); rows [0,S) take g_out, rows [S,2S) g_xi; NULL = zero
__global__ void k_out_grad(double* Z, const float* g_out, const float* g_xi, int sig, long S, int od) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * S * od) return;
    const bool second = i >= S * od;
    const float* g = second ? g_xi : g_out;
    double v = 0.0;
    if (g) {
        v = (double)g[second ? i - S * od : i];
        if (sig) {
            const double s = sigmoid64(Z[i]);
            v *= s * (1.0 - s);
        }
    }
    Z[i] = v;
}

// d LAT [2S,32] (both passes; NULL: no decoder contribution) + upstream on E -> d raw [S,32]
__global__ void k_latent_grad(const double* dLAT, const double* E, const float* var, const float* g_raw, int act, long S, double* dRAW) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * 32) return;
    const int j = (int)(i & 31);
    const double e = E[i];
    const double s = sigmoid64(e);
    const double d = act == 0 ? s * (1.0 - s) : (e > 20.0 ? 1.0 : s);
    double de = dLAT ? (dLAT[i] + dLAT[S * 32 + i]) * d : 0.0;
    if (g_raw) de += (double)g_raw[i];
    dRAW[i] = de * (1.0 - (var ? (double)var[j] : 0.0));
}

struct Plan {
    Layer L[8];
    long acc_off[8];          // doubles
    long acc_total;
    // per-slab buffers, offsets in doubles (functions of S = slab rows and od)
    long A[4], RAW, E, LAT, H[2], Z, dH[2], dLAT, dRAW, dZ[2], total;
};

Plan make_plan(long S, int in_dim, int od) {
    Plan p;
    const int no[8] = {512, 512, 512, 512, 32, 128, 128, od};
    const int ki[8] = {in_dim, 512, 512, 512, 512, 32, 128, 128};
    const long ld[8] = {64, 512, 512, 512, 512, 32, 128, 128};
    long o = 0;
    for (int l = 0; l < 8; ++l) {
        p.L[l] = Layer{no[l], ki[l], ld[l]};
        p.acc_off[l] = o;
        o += (long)no[l] * (ki[l] + 1);
    }
    p.acc_total = o;
    Take take{o};
    for (int l = 0; l < 4; ++l) p.A[l] = take(S * 512);
    p.RAW = take(S * 32);
    p.E = take(S * 32);
    p.LAT = take(2 * S * 32);
    p.H[0] = take(2 * S * 128);
    p.H[1] = take(2 * S * 128);
    p.Z = take(2 * S * od);
    p.dH[0] = take(2 * S * 128);
    p.dH[1] = take(2 * S * 128);
    p.dLAT = take(2 * S * 32);
    p.dRAW = take(S * 32);
    p.dZ[0] = take(S * 512);
    p.dZ[1] = take(S * 512);
    p.total = take.o;
    return p;
}

bool check_dims(long n, long slab_rows, int in_dim, int out_dim) {
    if (!check_rows("n", n, slab_rows)) return false;
    if (in_dim < 1 || in_dim > 64) return fail("in_dim = %d outside [1, 64]", in_dim), false;
    if (out_dim < 1 || out_dim > 16) return fail("out_dim = %d outside [1, 16]", out_dim), false;
    return true;
}

}  // namespace

extern "C" {

int rb_train_abi_version(void) { return RB_TRAIN_ABI_VERSION; }

const char* rb_train_last_error(void) { return g_err; }

long rb_train_ae_bwd_scratch_bytes(long n, long slab_rows, int in_dim, int out_dim) {
    if (!check_dims(n, slab_rows, in_dim, out_dim)) return -1;
    return make_plan(query_slab_size(n, slab_rows), in_dim, out_dim).total * (long)sizeof(double);
}

int rb_train_ae_bwd(const float* X, long n, int in_dim, const float* noise, double noise_scale, const float* var, int latent_act, int out_act,
                    int out_dim, const float* const* params, const float* g_out, const float* g_out_xi, const float* g_raw,
                    float* const* grads, long slab_rows, void* scratch, long scratch_bytes, int* stats, rb_train_stream_t stream) {
    if (!check_dims(n, slab_rows, in_dim, out_dim)) return 1;
    if (latent_act != 0 && latent_act != 1) return fail("latent_act = %d: 0 (sigmoid) or 1 (softplus)", latent_act);
    if (out_act != 0 && out_act != 1) return fail("out_act = %d: 0 (none) or 1 (sigmoid)", out_act);
    if (!params || !grads) return fail("null pointer: params / grads (HOST arrays of 16 device pointers)");
    if (stats) stats[0] = stats[1] = 0;
    if (n == 0) return 0;
    if (!X) return fail("null pointer: X");
    for (int i = 0; i < 16; ++i)
        if (!params[i]) return fail("null pointer: params[%d]", i);
    bool want_layer[8];
    const int lowest = scan_wanted(grads, 8, 2, want_layer);      // first layer that wants a gradient: the data path stops there
    if (lowest == 8) return 0;
    const bool enc = lowest < 5;
    const long S0 = slab_size(n, slab_rows);
    const Plan p = make_plan(S0, in_dim, out_dim);
    if (check_scratch(scratch, scratch_bytes, p.total * (long)sizeof(double), "rb_train_ae_bwd_scratch_bytes")) return 1;
    hipStream_t st = (hipStream_t)stream;
    double* D = (double*)scratch;
    g_launches = 0;
    int bad = 0;

    for (long row0 = 0; row0 < n; row0 += S0) {
        const long S = n - row0 < S0 ? n - row0 : S0;
        const int first = row0 == 0;
        const float* Xs = X + row0 * 64;
        // input rows of layer l (fp32 features for l = 0, fp64 activations after), M rows
        const void* in[8] = {Xs, D + p.A[0], D + p.A[1], D + p.A[2], D + p.A[3], D + p.LAT, D + p.H[0], D + p.H[1]};
        double* out[8] = {D + p.A[0], D + p.A[1], D + p.A[2], D + p.A[3], D + p.RAW, D + p.H[0], D + p.H[1], D + p.Z};
        auto forward = [&](int l, long M) {
            bad |= fwd(p.L[l], M, in[l], l == 0, params[2 * l], 1, params[2 * l + 1], l != 4 && l != 7, out[l], p.L[l].n_out, st);
        };
        // d loss / d (pre-activation of layer l) sits in dz [M, n_out]: accumulate dW | db, and (to != NULL) hand the gradient to layer l - 1
        auto backward = [&](int l, long M, const double* dz, double* to, bool mask_prev) {
            const Layer& L = p.L[l];
            if (want_layer[l]) bad |= wgrad(L, M, dz, L.n_out, in[l], l == 0, D + p.acc_off[l], first, st);
            if (to) bad |= bwd(L, M, dz, 0, L.n_out, params[2 * l], 1, L.k_in, mask_prev, (const double*)in[l], to, st);
        };
        for (int l = 0; l < 5; ++l) forward(l, S);
        hipLaunchKernelGGL(k_latent, ew_grid(S * 32), dim3(256), 0, st, D + p.RAW, var, noise ? noise + row0 * 32 : nullptr, noise_scale,
                           latent_act, S, D + p.E, D + p.LAT);
        ++g_launches;
        const bool dec_grad = g_out || g_out_xi;      // without an upstream on either output the decoder's gradients are zero
        if (lowest < 8 && (dec_grad || first)) {
            // (a slab after the first adds nothing when there is no upstream; the first one must still store the zeros)
            for (int l = 5; l < 8; ++l) forward(l, 2 * S);
            hipLaunchKernelGGL(k_out_grad, ew_grid(2 * S * out_dim), dim3(256), 0, st, D + p.Z, g_out ? g_out + row0 * out_dim : nullptr,
                               g_out_xi ? g_out_xi + row0 * out_dim : nullptr, out_act, S, out_dim);
            ++g_launches;
            backward(7, 2 * S, D + p.Z, lowest < 7 ? D + p.dH[1] : nullptr, true);
            if (lowest < 7) backward(6, 2 * S, D + p.dH[1], lowest < 6 ? D + p.dH[0] : nullptr, true);
            if (lowest < 6) backward(5, 2 * S, D + p.dH[0], enc ? D + p.dLAT : nullptr, false);
        }
        if (!enc) continue;                           // no encoder parameter wants a gradient: the backward stops at the latent
        const bool through_decoder = dec_grad || first;
        hipLaunchKernelGGL(k_latent_grad, ew_grid(S * 32), dim3(256), 0, st, through_decoder ? D + p.dLAT : nullptr, D + p.E, var,
                           g_raw ? g_raw + row0 * 32 : nullptr, latent_act, S, D + p.dRAW);
        ++g_launches;
        const double* dz = D + p.dRAW;
        for (int l = 4; l >= lowest; --l) {
            double* to = l > lowest ? D + p.dZ[l & 1] : nullptr;
            backward(l, S, dz, to, true);
            dz = to;
        }
        if (stats) stats[1] = 1;
    }
    finish_layers(p.L, 8, D, p.acc_off, grads, st);
    if (stats) stats[0] = g_launches;
    if (bad || hipGetLastError() != hipSuccess) return fail("kernel launch failed");
    return 0;
}

}  // extern "C"
