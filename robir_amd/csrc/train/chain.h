// The slab driver of the training libraries, on top of the engine (gemm64.h): the host side that every reverse mode of a chain of layers
// repeats.  A library walks its rows slab by slab; per slab it runs the layers forward (fwd_layer), then from the top dZ downwards the
// weight gradient of every wanted layer (wgrad_parts or wgrad_acc) and the data gradient that hands dZ to the layer below (dgrad).  This
// file owns those three descriptor fill-ins, the partition / reduce scheme of DESIGN 4.5 (Z_GROUP, PART_ELEMS, k_reduce), the range check
// and the slab-size arithmetic of the entry points, the wanted-layer scan and the PE10 column.  Where a weight comes from, where dZ starts
// and what else runs between the products is the including library's.  Included once per library, like gemm64.h.
#pragma once
#include "gemm64.h"

namespace {

constexpr int Z_GROUP = 4096;                 // partitions per launch of the weight-gradient GEMM (grid.z)
template <int HID>
constexpr long PART_ELEMS = (long)HID * (HID + 1);      // the widest weight gradient of a HID-wide net with its bias column: one partial

// column c < 63 of PE10(src[0 .. 2]): x_c for c < 3, else with j = c - 3, k = j / 6: sin(2^k x_{j % 6}) for j % 6 < 3, cos(2^k x_{j % 6 - 3})
// otherwise (the oracle's encoding.pe, rb_feat_pe10's layout).  x 2^k is exact in double.
__device__ __forceinline__ double pe10_col(const float* src, int c) {
    if (c < 3) return (double)src[c];
    const int j = c - 3, k = j / 6, r = j % 6;
    const double a = (double)src[r % 3] * (double)(1 << k);
    return r < 3 ? sin(a) : cos(a);
}

// acc[e] (+)= partial[0][e] + partial[1][e] + ... in partition order; first = 1: the slab stores, else it adds to what the earlier slabs left
// (a template only so that a library that never partitions, the auto-encoder's, does not carry the kernel)
template <int RED>
__global__ void k_reduce(const double* partial, int nparts, long stride, long count, double* acc, int first) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    double s = first ? 0.0 : acc[e];
    for (int q = 0; q < nparts; ++q) s += partial[(long)q * stride + e];
    acc[e] = s;
}

// what the scratch query and the entry point check first; `name`: what the library's interface calls its row count.  Without part_rows:
// a library that does not partition its slabs
bool check_rows(const char* name, long rows, long slab_rows) {
    if (rows < 0) return fail("%s = %ld is negative", name, rows), false;
    if (slab_rows < 1 || slab_rows > (1L << 20)) return fail("slab_rows = %ld outside [1, 2^20]", slab_rows), false;
    return true;
}
bool check_rows(const char* name, long rows, long slab_rows, long part_rows) {
    if (!check_rows(name, rows, slab_rows)) return false;
    if (part_rows < 1 || part_rows > slab_rows) return fail("part_rows = %ld outside [1, slab_rows = %ld]", part_rows, slab_rows), false;
    return true;
}

// rows of a full slab: what the entry point plans for (rows > 0) | what the scratch query plans for (one row where there is none)
long slab_size(long rows, long slab_rows) { return rows < slab_rows ? rows : slab_rows; }
long query_slab_size(long rows, long slab_rows) { return rows > 0 ? slab_size(rows, slab_rows) : 1; }

// want_layer[l] = one of grads[per_layer l .. per_layer l + per_layer - 1] is wanted; -> the first such layer, where the data path stops
// (n_layers: nothing is wanted)
int scan_wanted(float* const* grads, int n_layers, int per_layer, bool* want_layer) {
    int lowest = n_layers;
    for (int l = n_layers - 1; l >= 0; --l) {
        want_layer[l] = false;
        for (int i = 0; i < per_layer; ++i) want_layer[l] |= grads[per_layer * l + i] != nullptr;
        if (want_layer[l]) lowest = l;
    }
    return lowest;
}

// The three product families of layer L over `rows` rows.  in: the layer's input rows [rows, k_in], row stride L.in_ld; W: its weight
// [n_out, k_in], row-major; dz: d loss / d (its pre-activation) [rows, n_out], row stride dz_ld; *_f32: fp32 elements, else fp64.

// out[rows, n_out] (row stride ldc) = act(in W^T + bias)
template <int ACT, int RED>
int fwd_layer(const Layer& L, long rows, const void* in, int in_f32, const void* W, int w_f32, const float* bias, int act, double* out, long ldc,
              hipStream_t st) {
    Gemm g{};
    g.A = in; g.sam = L.in_ld; g.sak = 1; g.a_f32 = in_f32;
    g.B = W; g.sbk = 1; g.sbn = L.k_in; g.b_f32 = w_f32;
    g.ones_col = -1;
    g.M = (int)rows; g.N = L.n_out; g.K = L.k_in;
    g.epi = EPI_FWD; g.C = out; g.ldc = ldc; g.bias = bias;
    g.act = act;
    return launch_gemm<ACT, RED>(g, 1, st);
}

// dW | db = dz^T [in | 1], a GEMM whose reduction dimension is the rows: A(m = neuron, k = row), B(k = row, n = input column), the bias
// column rides along as ones_col
Gemm wgrad_gemm(const Layer& L, long rows, const void* dz, int dz_f32, long dz_ld, const void* in, int in_f32, double* C) {
    Gemm g{};
    g.A = dz; g.sam = 1; g.sak = dz_ld; g.a_f32 = dz_f32;
    g.B = in; g.sbk = L.in_ld; g.sbn = 1; g.b_f32 = in_f32;
    g.ones_col = L.k_in;
    g.M = L.n_out; g.N = L.k_in + 1; g.K = (int)rows;
    g.epi = EPI_WGRAD; g.C = C; g.ldc = L.k_in + 1;
    return g;
}

// RED_PART: the rows are cut into partitions of part_rows, Z_GROUP of them per launch, each stores its partial at `partial`; k_reduce adds
// them in partition order into the layer's accumulator `acc` [n_out, k_in + 1] (first: stores)
template <int ACT, int RED>
int wgrad_parts(const Layer& L, long rows, const void* dz, int dz_f32, long dz_ld, const double* in, long part_rows, double* partial,
                double* acc, int first, hipStream_t st) {
    static_assert(RED == RED_PART, "per-partition partials");
    const long count = (long)L.n_out * (L.k_in + 1);
    const int nparts = (int)((rows + part_rows - 1) / part_rows);
    Gemm g = wgrad_gemm(L, rows, dz, dz_f32, dz_ld, in, 0, partial);
    g.part_rows = (int)part_rows; g.part_stride = count;
    int bad = 0;
    for (int q0 = 0; q0 < nparts; q0 += Z_GROUP) {
        g.part0 = q0;
        bad |= launch_gemm<ACT, RED>(g, nparts - q0 < Z_GROUP ? nparts - q0 : Z_GROUP, st);
    }
    hipLaunchKernelGGL(k_reduce<RED>, ew_grid(count), dim3(256), 0, st, partial, nparts, count, count, acc, first);
    ++g_launches;
    return bad;
}

// RED_ACC: one launch over all the rows, in place: stores (first) or adds to the layer's accumulator `acc`
template <int ACT, int RED>
int wgrad_acc(const Layer& L, long rows, const void* dz, long dz_ld, const void* in, int in_f32, double* acc, int first, hipStream_t st) {
    static_assert(RED == RED_ACC, "in-place accumulation");
    Gemm g = wgrad_gemm(L, rows, dz, 0, dz_ld, in, in_f32, acc);
    g.first = first;
    return launch_gemm<ACT, RED>(g, 1, st);
}

// to[rows, n_prev] (row stride k_in) = (dz W[:, :n_prev]) . act'(in), `in` being the stored activation of the layer below (act = 0: no
// gate).  n_prev = k_in, but for a layer whose input is only in part the output of the layer below
template <int ACT, int RED>
int dgrad(const Layer& L, long rows, const void* dz, int dz_f32, long dz_ld, const void* W, int w_f32, int n_prev, int act, const double* in,
          double* to, hipStream_t st) {
    Gemm g{};
    g.A = dz; g.sam = dz_ld; g.sak = 1; g.a_f32 = dz_f32;
    g.B = W; g.sbk = L.k_in; g.sbn = 1; g.b_f32 = w_f32;
    g.ones_col = -1;
    g.M = (int)rows; g.N = n_prev; g.K = L.n_out;
    g.epi = EPI_BWD; g.C = to; g.ldc = L.k_in;
    g.act = act; g.mask = in; g.ldm = L.in_ld;
    return launch_gemm<ACT, RED>(g, 1, st);
}

}  // namespace
