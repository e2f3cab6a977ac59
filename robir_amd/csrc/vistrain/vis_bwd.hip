// librobir_hip_vistrain.so: reverse mode of VisNetwork, PE10(p) | PE10(d) -> 256 x 4 ReLU -> 2 (include/robir_hip_vistrain.h).
//
// Everything is fp64: the encoding is evaluated in double from the fp32 coordinates (k_encode), the four hidden activations are recomputed
// from it and the fp32 nn.Linear parameters, and the three product families (activations, dZ_{l-1} = (dZ_l W_l) . gate, dW_l = dZ_l^T A_{l-1}
// | db_l = sum dZ_l) run on v_mfma_f64_16x16x4_f64 through the training libraries' one tiled kernel (k_gemm64 of ../train/gemm64.h,
// instantiated here for ReLU and per-partition partials), driven by the slab driver the four libraries share (../train/chain.h).  Each
// stored gradient is rounded to fp32 once (k_finish).  This file holds what is particular to the visibility network: k_encode, its plan,
// its argument checks and the order of its slab loop.
//
// Reductions over rows.  dW | db of a layer is a GEMM whose REDUCTION dimension is the slab's rows.  A Vis-stage step has 10^5 .. 10^6 rows, and
// a 256 x 257 gradient is 20 output tiles: the row range of a slab is therefore cut into contiguous partitions of part_rows rows, one
// workgroup per (output tile, partition) sums its rows in row order and stores an fp64 partial with plain vector stores, k_reduce adds the
// partials in partition order into the layer's accumulator (one thread per element), slabs add in slab order (wgrad_parts of chain.h).  No
// atomics: the association is a function of (M, slab_rows, part_rows) alone, never of the number of compute units or of occupancy.
#include "../../../include/robir_hip_vistrain.h"
#include "../train/chain.h"

namespace {

constexpr int HID = 256, IN = 126, IN_LD = 128, PE = 63;

// ReLU hidden layers (every forward and data-gradient launch has it); weight gradients leave as per-partition partials (k_reduce)
constexpr auto fwd = fwd_layer<ACT_RELU, RED_PART>;
constexpr auto wgrad = wgrad_parts<ACT_RELU, RED_PART>;
constexpr auto bwd = dgrad<ACT_RELU, RED_PART>;

// X[i, :] = [PE10(p[(row0 + i) / rep]) | PE10(d[row0 + i]) | 0 0], i < S (pe10_col: the column of one PE10 block)
__global__ void k_encode(const float* p, const float* d, long row0, int rep, long S, double* X) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * IN_LD) return;
    const long row = i / IN_LD;
    const int col = (int)(i % IN_LD);
    double v = 0.0;
    if (col < IN) {
        const bool dir = col >= PE;
        const int c = dir ? col - PE : col;
        v = pe10_col(dir ? d + (row0 + row) * 3 : p + ((row0 + row) / rep) * 3, c);
    }
    X[i] = v;
}

const Layer LAYERS[5] = {{HID, IN, IN_LD}, {HID, HID, HID}, {HID, HID, HID}, {HID, HID, HID}, {2, HID, HID}};

struct Plan {
    long acc_off[5];          // doubles
    long nparts;              // partitions of a full slab
    long partial, X, A[4], dZ[2], total;
};

Plan make_plan(long S, long part_rows) {
    Plan p;
    Take take;
    for (int l = 0; l < 5; ++l) p.acc_off[l] = take((long)LAYERS[l].n_out * (LAYERS[l].k_in + 1));
    p.nparts = (S + part_rows - 1) / part_rows;
    p.partial = take(p.nparts * PART_ELEMS<HID>);
    p.X = take(S * IN_LD);
    for (int l = 0; l < 4; ++l) p.A[l] = take(S * HID);
    p.dZ[0] = take(S * HID);
    p.dZ[1] = take(S * HID);
    p.total = take.o;
    return p;
}

}  // namespace

extern "C" {

int rb_vt_abi_version(void) { return RB_VT_ABI_VERSION; }

const char* rb_vt_last_error(void) { return g_err; }

long rb_vt_vis_bwd_scratch_bytes(long M, long slab_rows, long part_rows) {
    if (!check_rows("M", M, slab_rows, part_rows)) return -1;
    return make_plan(query_slab_size(M, slab_rows), part_rows).total * (long)sizeof(double);
}

int rb_vt_vis_bwd(const float* p, const float* d, long M, int rep, const float* const* params, const float* g_logits, float* const* grads,
                  long slab_rows, long part_rows, void* scratch, long scratch_bytes, int* stats, rb_vt_stream_t stream) {
    if (!check_rows("M", M, slab_rows, part_rows)) return 1;
    if (rep < 1) return fail("rep = %d: at least 1", rep);
    if (M % rep) return fail("M = %ld is not a multiple of rep = %d", M, rep);
    if (!params || !grads) return fail("null pointer: params / grads (HOST arrays of 10 device pointers)");
    if (stats) { stats[0] = 0; stats[1] = 5; stats[2] = 0; }
    if (M == 0) return 0;
    if (!p || !d || !g_logits) return fail("null pointer: p / d / g_logits");
    for (int i = 0; i < 10; ++i)
        if (!params[i]) return fail("null pointer: params[%d]", i);
    bool want_layer[5];
    const int lowest = scan_wanted(grads, 5, 2, want_layer);      // first layer that wants a gradient: the data path stops there
    if (lowest == 5) return 0;
    const long S0 = slab_size(M, slab_rows);
    const Plan pl = make_plan(S0, part_rows);
    if (check_scratch(scratch, scratch_bytes, pl.total * (long)sizeof(double), "rb_vt_vis_bwd_scratch_bytes")) return 1;
    hipStream_t st = (hipStream_t)stream;
    double* D = (double*)scratch;
    g_launches = 0;
    int bad = 0;

    for (long row0 = 0; row0 < M; row0 += S0) {
        const long S = M - row0 < S0 ? M - row0 : S0;
        const int first = row0 == 0;
        const double* in[5] = {D + pl.X, D + pl.A[0], D + pl.A[1], D + pl.A[2], D + pl.A[3]};      // input rows of layer l
        hipLaunchKernelGGL(k_encode, ew_grid(S * IN_LD), dim3(256), 0, st, p, d, row0, rep, S, D + pl.X);
        ++g_launches;
        for (int l = 0; l < 4; ++l) bad |= fwd(LAYERS[l], S, in[l], 0, params[2 * l], 1, params[2 * l + 1], 1, D + pl.A[l], HID, st);
        // d loss / d (pre-activation of layer l) sits in dz [S, dz_ld]: fp32 g_logits for the last layer, an fp64 scratch buffer below it
        const void* dz = g_logits + row0 * 2;
        int dz_f32 = 1;
        long dz_ld = 2;
        for (int l = 4; l >= lowest; --l) {
            const Layer& L = LAYERS[l];
            if (want_layer[l]) bad |= wgrad(L, S, dz, dz_f32, dz_ld, in[l], part_rows, D + pl.partial, D + pl.acc_off[l], first, st);
            if (l > lowest) {
                double* to = D + pl.dZ[l & 1];
                bad |= bwd(L, S, dz, dz_f32, dz_ld, params[2 * l], 1, L.k_in, 1, in[l], to, st);
                dz = to;
                dz_f32 = 0;
                dz_ld = HID;
            }
        }
    }
    finish_layers(LAYERS, 5, D, pl.acc_off, grads, st);
    if (stats) { stats[0] = g_launches; stats[1] = lowest; stats[2] = (int)pl.nparts; }
    if (bad || hipGetLastError() != hipSuccess) return fail("kernel launch failed");
    return 0;
}

}  // extern "C"
