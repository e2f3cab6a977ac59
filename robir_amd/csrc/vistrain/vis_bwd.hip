// librobir_hip_vistrain.so: reverse mode of VisNetwork, PE10(p) | PE10(d) -> 256 x 4 ReLU -> 2 (include/robir_hip_vistrain.h).
//
// Everything is fp64: the encoding is evaluated in double from the fp32 coordinates (k_encode), the four hidden activations are recomputed
// from it and the fp32 nn.Linear parameters, and the three product families (activations, dZ_{l-1} = (dZ_l W_l) . gate, dW_l = dZ_l^T A_{l-1}
// | db_l = sum dZ_l) run on v_mfma_f64_16x16x4_f64 through ONE tiled kernel (k_gemm64, modelled on csrc/train/ae_bwd.hip's: this translation
// unit carries its own so that the pinned training library is not touched).  Each stored gradient is rounded to fp32 once (k_finish).
//
// Reductions over rows.  dW | db of a layer is a GEMM whose REDUCTION dimension is the slab's rows.  A Vis-stage step has 10^5 .. 10^6 rows, and
// a 256 x 257 gradient is 20 output tiles: the row range of a slab is therefore cut into contiguous partitions of part_rows rows, one
// workgroup per (output tile, partition) sums its rows in row order and stores an fp64 partial with plain vector stores, k_reduce adds the
// partials in partition order into the layer's accumulator (one thread per element), slabs add in slab order.  No atomics: the association
// is a function of (M, slab_rows, part_rows) alone, never of the number of compute units or of occupancy.
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include "../../../include/robir_hip_vistrain.h"

namespace {

thread_local char g_err[512] = "";

int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return 1;
}

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int BM = 64, BN = 64, BK = 16;      // block tile: four waves, wave w owns rows 16 w .. 16 w + 15 and all 64 columns (4 MFMA tiles)
constexpr int LDS_LD = 80;                    // doubles per k-row of a tile in LDS: 160 dwords, consecutive k-rows start 32 banks apart
constexpr int HID = 256, IN = 126, IN_LD = 128, PE = 63;
constexpr long PART_ELEMS = (long)HID * (HID + 1);      // the widest weight gradient with its bias column: one partial
constexpr int Z_GROUP = 4096;                 // partitions per launch of the weight-gradient GEMM (grid.z)

enum { EPI_FWD = 0, EPI_BWD = 1, EPI_PART = 2 };

struct Gemm {
    // C[m,n] = sum_k A(m,k) B(k,n);  A(m,k) = A[m sam + k sak], B(k,n) = B[k sbk + n sbn] (fp32 or fp64 elements), zero outside M x K / K x N
    const void* A; long sam, sak; int a_f32;
    const void* B; long sbk, sbn; int b_f32;
    int ones_col;             // >= 0: B(k, ones_col) = 1 for every k < K and no memory is read for that column (db = dZ^T 1 rides along with dW)
    int M, N, K;
    int epi;
    double* C; long ldc;
    const float* bias;        // EPI_FWD: relu(result + bias[n])
    const double* mask; long ldm;      // EPI_BWD: result *= (mask[m,n] > 0), mask = the stored ReLU output (> 0 exactly where its pre-activation is)
    int part_rows, part0;     // EPI_PART: blockIdx.z + part0 = partition q, k in [q part_rows, min((q + 1) part_rows, K)); C += q part_stride
    long part_stride;
};

__device__ __forceinline__ double ld_elem(const void* p, long i, int f32) {
    return f32 ? (double)((const float*)p)[i] : ((const double*)p)[i];
}

__global__ __launch_bounds__(256) void k_gemm64(Gemm g) {
    __shared__ double As[BK][LDS_LD];
    __shared__ double Bs[BK][LDS_LD];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    int kb = 0, ke = g.K;
    double* C = g.C;
    if (g.epi == EPI_PART) {
        const long q = (long)blockIdx.z + g.part0;
        const long b = q * g.part_rows;
        kb = (int)b;
        ke = (int)(b + g.part_rows < (long)g.K ? b + g.part_rows : (long)g.K);
        C += q * g.part_stride;
    }
    double4_t acc[4];
    for (int i = 0; i < 4; ++i) acc[i] = double4_t{0.0, 0.0, 0.0, 0.0};
    const bool a_kfast = g.sak == 1, b_nfast = g.sbn == 1;
    for (int k0 = kb; k0 < ke; k0 += BK) {
        for (int i = 0; i < 4; ++i) {
            const int idx = t + 256 * i;
            int m, k;
            if (a_kfast) { k = idx & 15; m = idx >> 4; } else { m = idx & 63; k = idx >> 6; }
            const int gm = m0 + m, gk = k0 + k;
            As[k][m] = (gm < g.M && gk < ke) ? ld_elem(g.A, (long)gm * g.sam + (long)gk * g.sak, g.a_f32) : 0.0;
            int n;
            if (b_nfast) { n = idx & 63; k = idx >> 6; } else { k = idx & 15; n = idx >> 4; }
            const int gn = n0 + n;
            const int gk2 = k0 + k;
            double v = 0.0;
            if (gn < g.N && gk2 < ke) v = gn == g.ones_col ? 1.0 : ld_elem(g.B, (long)gk2 * g.sbk + (long)gn * g.sbn, g.b_f32);
            Bs[k][n] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BK; kk += 4) {
            // operand lane map of the 16x16x4 forms: lane l holds A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15]
            const double a = As[kk + (lane >> 4)][16 * w + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double b = Bs[kk + (lane >> 4)][16 * j + (lane & 15)];
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // C/D lane map of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 r  (NOT the f32 forms' 4 (lane >> 4) + r)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + 16 * j + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * w + (lane >> 4) + 4 * r;
            if (m >= g.M || n >= g.N) continue;
            double v = acc[j][r];
            if (g.epi == EPI_FWD) {
                v += (double)g.bias[n];
                v = v > 0.0 ? v : 0.0;
            } else if (g.epi == EPI_BWD) {
                v = g.mask[(long)m * g.ldm + n] > 0.0 ? v : 0.0;
            }
            C[(long)m * g.ldc + n] = v;
        }
    }
}

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

// fp64 accumulator [n_out, k_in + 1] (last column: bias) -> the parameter-shaped fp32 gradients, one rounding each
__global__ void k_finish(const double* acc, int n_out, int k_in, float* gW, float* gb) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n_out * (k_in + 1)) return;
    const int o = (int)(i / (k_in + 1)), c = (int)(i % (k_in + 1));
    if (c < k_in) {
        if (gW) gW[(long)o * k_in + c] = (float)acc[i];
    } else if (gb) {
        gb[o] = (float)acc[i];
    }
}

struct Layer { int n_out, k_in; long in_ld; };      // in_ld: row stride of the layer's input rows

const Layer LAYERS[5] = {{HID, IN, IN_LD}, {HID, HID, HID}, {HID, HID, HID}, {HID, HID, HID}, {2, HID, HID}};

struct Plan {
    long acc_off[5];          // doubles
    long nparts;              // partitions of a full slab
    long partial, X, A[4], dZ[2], total;
};

Plan make_plan(long S, long part_rows) {
    Plan p;
    long o = 0;
    auto take = [&](long n) { long at = o; o += (n + 7) & ~7L; return at; };
    for (int l = 0; l < 5; ++l) p.acc_off[l] = take((long)LAYERS[l].n_out * (LAYERS[l].k_in + 1));
    p.nparts = (S + part_rows - 1) / part_rows;
    p.partial = take(p.nparts * PART_ELEMS);
    p.X = take(S * IN_LD);
    for (int l = 0; l < 4; ++l) p.A[l] = take(S * HID);
    p.dZ[0] = take(S * HID);
    p.dZ[1] = take(S * HID);
    p.total = o;
    return p;
}

bool check_dims(long M, long slab_rows, long part_rows) {
    if (M < 0) return fail("M = %ld is negative", M), false;
    if (slab_rows < 1 || slab_rows > (1L << 20)) return fail("slab_rows = %ld outside [1, 2^20]", slab_rows), false;
    if (part_rows < 1 || part_rows > slab_rows) return fail("part_rows = %ld outside [1, slab_rows = %ld]", part_rows, slab_rows), false;
    return true;
}

thread_local int g_launches;

int launch_gemm(const Gemm& g, int nz, hipStream_t st) {
    if (g.M <= 0 || g.N <= 0 || nz <= 0) return 0;
    dim3 grid((g.N + BN - 1) / BN, (g.M + BM - 1) / BM, nz);
    hipLaunchKernelGGL(k_gemm64, grid, dim3(256), 0, st, g);
    ++g_launches;
    return hipGetLastError() != hipSuccess;
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
    if (!scratch) return fail("null pointer: scratch");
    if ((uintptr_t)scratch % 8) return fail("scratch is not 8-byte aligned");
    if (scratch_bytes < pl.total * (long)sizeof(double))
        return fail("scratch too small: %ld bytes given, %ld needed (rb_vt_vis_bwd_scratch_bytes)", scratch_bytes, pl.total * (long)sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    double* D = (double*)scratch;
    g_launches = 0;
    int bad = 0;
    auto ew_grid = [](long items) { return dim3((unsigned)((items + 255) / 256)); };
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
            bad |= launch_gemm(g, 1, st);
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
                g.epi = EPI_PART; g.C = D + pl.partial; g.ldc = L.k_in + 1;
                g.part_rows = (int)part_rows; g.part_stride = count;
                for (int q0 = 0; q0 < nparts; q0 += Z_GROUP) {
                    g.part0 = q0;
                    bad |= launch_gemm(g, nparts - q0 < Z_GROUP ? nparts - q0 : Z_GROUP, st);
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
                bad |= launch_gemm(g, 1, st);
                dz = to;
                dz_f32 = 0;
            }
        }
    }
    for (int l = 0; l < 5; ++l) {
        if (!want_layer[l]) continue;
        const Layer& L = LAYERS[l];
        hipLaunchKernelGGL(k_finish, ew_grid((long)L.n_out * (L.k_in + 1)), dim3(256), 0, st, D + pl.acc_off[l], L.n_out, L.k_in, grads[2 * l],
                           grads[2 * l + 1]);
        ++g_launches;
    }
    if (stats) { stats[0] = g_launches; stats[1] = lowest; stats[2] = (int)pl.nparts; }
    if (bad || hipGetLastError() != hipSuccess) return fail("kernel launch failed");
    return 0;
}

}  // extern "C"
