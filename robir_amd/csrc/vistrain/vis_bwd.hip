// librobir_hip_vistrain.so: reverse mode of VisNetwork, PE10(p) | PE10(d) -> 256 x 4 ReLU -> 2 (include/robir_hip_vistrain.h).
//
// Everything is fp64: the encoding is evaluated in double from the fp32 coordinates (k_encode), the four hidden activations are recomputed
// from it and the fp32 nn.Linear parameters, and the three product families (activations, dZ_{l-1} = (dZ_l W_l) . gate, dW_l = dZ_l^T A_{l-1}
// | db_l = sum dZ_l) run on v_mfma_f64_16x16x4_f64 through the training libraries' one tiled kernel (k_gemm64 of ../train/gemm64.h, the
// engine csrc/train/ae_bwd.hip runs too; instantiated here for ReLU and per-partition partials).  Each stored gradient is rounded to fp32
// once (k_finish).  This file holds what is particular to the visibility network: k_encode, k_reduce, its plan and its slab loop.
//
// Reductions over rows.  dW | db of a layer is a GEMM whose REDUCTION dimension is the slab's rows.  A Vis-stage step has 10^5 .. 10^6 rows, and
// a 256 x 257 gradient is 20 output tiles: the row range of a slab is therefore cut into contiguous partitions of part_rows rows, one
// workgroup per (output tile, partition) sums its rows in row order and stores an fp64 partial with plain vector stores, k_reduce adds the
// partials in partition order into the layer's accumulator (one thread per element), slabs add in slab order.  No atomics: the association
// is a function of (M, slab_rows, part_rows) alone, never of the number of compute units or of occupancy.
#include "../../../include/robir_hip_vistrain.h"
#include "../train/gemm64.h"

namespace {

constexpr int HID = 256, IN = 126, IN_LD = 128, PE = 63;
constexpr long PART_ELEMS = (long)HID * (HID + 1);      // the widest weight gradient with its bias column: one partial
constexpr int Z_GROUP = 4096;                 // partitions per launch of the weight-gradient GEMM (grid.z)

constexpr auto gemm = launch_gemm<ACT_RELU, RED_PART>;      // ReLU hidden layers; weight gradients leave as per-partition partials (k_reduce)

// X[i, :] = [PE10(p[(row0 + i) / rep]) | PE10(d[row0 + i]) | 0 0], i < S: column c of one PE10 block is x_c for c < 3, else with j = c - 3,
// k = j / 6: sin(2^k x_{j % 6}) for j % 6 < 3, cos(2^k x_{j % 6 - 3}) otherwise (the oracle's encoding.pe).  x 2^k is exact in double.
__global__ void k_encode(const float* p, const float* d, long row0, int rep, long S, double* X) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * IN_LD) return;
    const long row = i / IN_LD;
    const int col = (int)(i % IN_LD);
    double v = 0.0;
    if (col < IN) {
        const bool dir = col >= PE;
        const int c = dir ? col - PE : col;
        const float* src = dir ? d + (row0 + row) * 3 : p + ((row0 + row) / rep) * 3;
        if (c < 3) {
            v = (double)src[c];
        } else {
            const int j = c - 3, k = j / 6, r = j % 6;
            const double a = (double)src[r % 3] * (double)(1 << k);
            v = r < 3 ? sin(a) : cos(a);
        }
    }
    X[i] = v;
}

// acc[e] (+)= partial[0][e] + partial[1][e] + ... in partition order; first = 1: the slab stores, else it adds to what the earlier slabs left
__global__ void k_reduce(const double* partial, int nparts, long stride, long count, double* acc, int first) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    double s = first ? 0.0 : acc[e];
    for (int q = 0; q < nparts; ++q) s += partial[(long)q * stride + e];
    acc[e] = s;
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
    p.partial = take(p.nparts * PART_ELEMS);
    p.X = take(S * IN_LD);
    for (int l = 0; l < 4; ++l) p.A[l] = take(S * HID);
    p.dZ[0] = take(S * HID);
    p.dZ[1] = take(S * HID);
    p.total = take.o;
    return p;
}

bool check_dims(long M, long slab_rows, long part_rows) {
    if (M < 0) return fail("M = %ld is negative", M), false;
    if (slab_rows < 1 || slab_rows > (1L << 20)) return fail("slab_rows = %ld outside [1, 2^20]", slab_rows), false;
    if (part_rows < 1 || part_rows > slab_rows) return fail("part_rows = %ld outside [1, slab_rows = %ld]", part_rows, slab_rows), false;
    return true;
}

}  // namespace

extern "C" {

int rb_vt_abi_version(void) { return RB_VT_ABI_VERSION; }

const char* rb_vt_last_error(void) { return g_err; }

long rb_vt_vis_bwd_scratch_bytes(long M, long slab_rows, long part_rows) {
    if (!check_dims(M, slab_rows, part_rows)) return -1;
    const long S = M < slab_rows ? (M > 0 ? M : 1) : slab_rows;
    return make_plan(S, part_rows).total * (long)sizeof(double);
}

int rb_vt_vis_bwd(const float* p, const float* d, long M, int rep, const float* const* params, const float* g_logits, float* const* grads,
                  long slab_rows, long part_rows, void* scratch, long scratch_bytes, int* stats, rb_vt_stream_t stream) {
    if (!check_dims(M, slab_rows, part_rows)) return 1;
    if (rep < 1) return fail("rep = %d: at least 1", rep);
    if (M % rep) return fail("M = %ld is not a multiple of rep = %d", M, rep);
    if (!params || !grads) return fail("null pointer: params / grads (HOST arrays of 10 device pointers)");
    if (stats) { stats[0] = 0; stats[1] = 5; stats[2] = 0; }
    if (M == 0) return 0;
    if (!p || !d || !g_logits) return fail("null pointer: p / d / g_logits");
    for (int i = 0; i < 10; ++i)
        if (!params[i]) return fail("null pointer: params[%d]", i);
    int lowest = 5;                                   // first layer that wants a gradient: the data path stops there
    for (int l = 4; l >= 0; --l)
        if (grads[2 * l] || grads[2 * l + 1]) lowest = l;
    if (lowest == 5) return 0;
    const long S0 = M < slab_rows ? M : slab_rows;
    const Plan pl = make_plan(S0, part_rows);
    if (check_scratch(scratch, scratch_bytes, pl.total * (long)sizeof(double), "rb_vt_vis_bwd_scratch_bytes")) return 1;
    hipStream_t st = (hipStream_t)stream;
    double* D = (double*)scratch;
    g_launches = 0;
    int bad = 0;
    bool want_layer[5];
    for (int l = 0; l < 5; ++l) want_layer[l] = grads[2 * l] || grads[2 * l + 1];

    for (long row0 = 0; row0 < M; row0 += S0) {
        const long S = M - row0 < S0 ? M - row0 : S0;
        const int first = row0 == 0;
        const double* in[5] = {D + pl.X, D + pl.A[0], D + pl.A[1], D + pl.A[2], D + pl.A[3]};      // input rows of layer l
        hipLaunchKernelGGL(k_encode, ew_grid(S * IN_LD), dim3(256), 0, st, p, d, row0, rep, S, D + pl.X);
        ++g_launches;
        for (int l = 0; l < 4; ++l) {
            const Layer& L = LAYERS[l];
            Gemm g{};
            g.A = in[l]; g.sam = L.in_ld; g.sak = 1; g.a_f32 = 0;
            g.B = params[2 * l]; g.sbk = 1; g.sbn = L.k_in; g.b_f32 = 1;
            g.ones_col = -1;
            g.M = (int)S; g.N = L.n_out; g.K = L.k_in;
            g.epi = EPI_FWD; g.C = D + pl.A[l]; g.ldc = HID; g.bias = params[2 * l + 1];
            bad |= gemm(g, 1, st);
        }
        // d loss / d (pre-activation of layer l) sits in dz [S, n_out]: fp32 g_logits for the last layer, an fp64 scratch buffer below it
        const void* dz = g_logits + row0 * 2;
        int dz_f32 = 1;
        for (int l = 4; l >= lowest; --l) {
            const Layer& L = LAYERS[l];
            if (want_layer[l]) {
                const long count = (long)L.n_out * (L.k_in + 1);
                const int nparts = (int)((S + part_rows - 1) / part_rows);
                Gemm g{};
                g.A = dz; g.sam = 1; g.sak = L.n_out; g.a_f32 = dz_f32;             // A(m = neuron, k = row)
                g.B = in[l]; g.sbk = L.in_ld; g.sbn = 1; g.b_f32 = 0;               // B(k = row, n = input column)
                g.ones_col = L.k_in;
                g.M = L.n_out; g.N = L.k_in + 1; g.K = (int)S;
                g.epi = EPI_WGRAD; g.C = D + pl.partial; g.ldc = L.k_in + 1;
                g.part_rows = (int)part_rows; g.part_stride = count;
                for (int q0 = 0; q0 < nparts; q0 += Z_GROUP) {
                    g.part0 = q0;
                    bad |= gemm(g, nparts - q0 < Z_GROUP ? nparts - q0 : Z_GROUP, st);
                }
                hipLaunchKernelGGL(k_reduce, ew_grid(count), dim3(256), 0, st, D + pl.partial, nparts, count, count, D + pl.acc_off[l], first);
                ++g_launches;
            }
            if (l > lowest) {
                double* to = D + pl.dZ[l & 1];
                Gemm g{};
                g.A = dz; g.sam = L.n_out; g.sak = 1; g.a_f32 = dz_f32;
                g.B = params[2 * l]; g.sbk = L.k_in; g.sbn = 1; g.b_f32 = 1;
                g.ones_col = -1;
                g.M = (int)S; g.N = L.k_in; g.K = L.n_out;
                g.epi = EPI_BWD; g.C = to; g.ldc = HID;
                g.mask = in[l]; g.ldm = HID;
                bad |= gemm(g, 1, st);
                dz = to;
                dz_f32 = 0;
            }
        }
    }
    finish_layers(LAYERS, 5, D, pl.acc_off, grads, st);
    if (stats) { stats[0] = g_launches; stats[1] = lowest; stats[2] = (int)pl.nparts; }
    if (bad || hipGetLastError() != hipSuccess) return fail("kernel launch failed");
    return 0;
}

}  // extern "C"
