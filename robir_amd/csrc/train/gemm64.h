// The fp64 GEMM engine of the training libraries (librobir_hip_train.so: train/ae_bwd.hip, librobir_hip_vistrain.so: vistrain/vis_bwd.hip,
// librobir_hip_illumtrain.so: illumtrain/illum_bwd.hip, librobir_hip_cesrtrain.so: cesrtrain/cesr_bwd.hip).  A reverse mode is three product families -- activations, dX = (dY . act') W, dW = dZ^T A | db = sum dZ -- and all of them
// run on v_mfma_f64_16x16x4_f64 through ONE tiled kernel, k_gemm64, whose operands are addressed by (row stride, column stride).  Included
// once per library (through chain.h, the host-side slab driver on top of it): everything here is internal to the including translation
// unit (each library keeps its own last-error string and launch counter), and each library instantiates k_gemm64 for the one (activation
// family, reduction mode) it runs.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

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
constexpr double SLOPE = 0.2;                 // nn.LeakyReLU(0.2)

enum { EPI_FWD = 0, EPI_BWD = 1, EPI_WGRAD = 2 };      // Gemm::epi (run-time)
// compile-time: the activation of the hidden layers.  ACT_RELU_OPT: ReLU where Gemm::act is set, identity where it is not (a net whose
// last forward launch keeps its pre-activation: the lobe net's raw output).  ACT_SOFTPLUS100_OPT: softplus(beta = 100) where Gemm::act is
// set: the stored activation is a = z above torch's threshold (100 z > 20), log1p(exp(100 z)) / 100 below, and the gate is recovered from
// it as sigmoid(100 z) = -expm1(-100 a) (above the threshold that is 1 - exp(-100 z), within 2e-9 of torch's exact 1: no special case)
enum { ACT_LEAKY = 0, ACT_RELU = 1, ACT_RELU_OPT = 2, ACT_SOFTPLUS100_OPT = 3 };
// compile-time: how a weight gradient (EPI_WGRAD) leaves the kernel.  RED_ACC: its reduction dimension is not split, one thread owns one
// element of the fp64 accumulator and stores (first) or adds to it.  RED_PART: the reduction dimension is cut into partitions of part_rows,
// blockIdx.z + part0 = partition q stores its own partial at C + q part_stride with plain vector stores (the library adds them in order).
enum { RED_ACC = 0, RED_PART = 1 };

struct Gemm {
    // C[m,n] = sum_k A(m,k) B(k,n);  A(m,k) = A[m sam + k sak], B(k,n) = B[k sbk + n sbn] (fp32 or fp64 elements), zero outside M x K / K x N
    const void* A; long sam, sak; int a_f32;
    const void* B; long sbk, sbn; int b_f32;
    int ones_col;             // >= 0: B(k, ones_col) = 1 for every k < K and no memory is read for that column (db = dZ^T 1 rides along with dW)
    int M, N, K;
    int epi;
    double* C; long ldc;
    const float* bias;        // EPI_FWD: + bias[n]
    int act;                  // ACT_LEAKY / ACT_RELU_OPT, per layer: EPI_FWD: the activation on the result.  EPI_BWD: result . act'(mask[m,n]),
                              // mask = the stored activation.  An ACT_RELU library has no layer without it and applies it to every launch
    const double* mask; long ldm;
    int first;                // EPI_WGRAD, RED_ACC: 1 = store, 0 = add to what C holds (slab order)
    int part_rows, part0;     // EPI_WGRAD, RED_PART: k in [q part_rows, min((q + 1) part_rows, K))
    long part_stride;
};

__device__ __forceinline__ double ld_elem(const void* p, long i, int f32) {
    return f32 ? (double)((const float*)p)[i] : ((const double*)p)[i];
}

template <int ACT, int RED>
__global__ __launch_bounds__(256) void k_gemm64(Gemm g) {
    __shared__ double As[BK][LDS_LD];
    __shared__ double Bs[BK][LDS_LD];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    int kb = 0, ke = g.K;     // the k-range of this workgroup: all of K unless it owns one partition of a weight gradient
    double* C = g.C;
    if constexpr (RED == RED_PART) {
        if (g.epi == EPI_WGRAD) {
            const long q = (long)blockIdx.z + g.part0;
            const long b = q * g.part_rows;
            kb = (int)b;
            ke = (int)(b + g.part_rows < (long)g.K ? b + g.part_rows : (long)g.K);
            C += q * g.part_stride;
        }
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
            double* c = C + (long)m * g.ldc + n;
            // The two families keep their own expressions: a ReLU is NOT a LeakyReLU of slope 0 (0 * v is -0.0 for v < 0 and NaN for an
            // infinite v, where the select stores +0.0).  The stored activation has the sign of its pre-activation, and a(0) = 0 takes the
            // slope (LeakyReLU, like torch's leaky_relu) or the zero (ReLU).
            if (g.epi == EPI_FWD) {
                v += (double)g.bias[n];
                if constexpr (ACT == ACT_RELU) v = v > 0.0 ? v : 0.0;
                else if constexpr (ACT == ACT_RELU_OPT) v = !g.act || v > 0.0 ? v : 0.0;
                else if constexpr (ACT == ACT_SOFTPLUS100_OPT) v = !g.act || 100.0 * v > 20.0 ? v : log1p(exp(100.0 * v)) / 100.0;
                else if (g.act) v = v > 0.0 ? v : SLOPE * v;
            } else if (g.epi == EPI_BWD) {
                if constexpr (ACT == ACT_RELU) v = g.mask[(long)m * g.ldm + n] > 0.0 ? v : 0.0;
                else if constexpr (ACT == ACT_RELU_OPT) v = !g.act || g.mask[(long)m * g.ldm + n] > 0.0 ? v : 0.0;
                else if constexpr (ACT == ACT_SOFTPLUS100_OPT) v = g.act ? v * -expm1(-100.0 * g.mask[(long)m * g.ldm + n]) : v;
                else if (g.act) v *=g.mask[(long)m * g.ldm + n] > 0.0 ? 1.0 : SLOPE;
            } else if constexpr (RED == RED_ACC) {
                if (!g.first) v = *c + v;
            }
            *c = v;
        }
    }
}

thread_local int g_launches;      // kernels enqueued by the current call of the library's entry point (its stats[0])

// nz: grid.z, the partitions of one RED_PART weight-gradient launch; 1 for everything else
template <int ACT, int RED>
int launch_gemm(const Gemm& g, int nz, hipStream_t st) {
    if (g.M <= 0 || g.N <= 0 || nz <= 0) return 0;
    dim3 grid((g.N + BN - 1) / BN, (g.M + BM - 1) / BM, nz);
    hipLaunchKernelGGL((k_gemm64<ACT, RED>), grid, dim3(256), 0, st, g);
    ++g_launches;
    return hipGetLastError() != hipSuccess;
}

inline dim3 ew_grid(long items) { return dim3((unsigned)((items + 255) / 256)); }      // element-wise kernels: 256 threads, one item each

struct Layer { int n_out, k_in; long in_ld; };      // in_ld: row stride of the layer's input rows

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

// k_finish for every layer with a wanted gradient: grads[2 l] | grads[2 l + 1] = weight | bias of layer l (NULL: not wanted)
void finish_layers(const Layer* L, int n_layers, const double* D, const long* acc_off, float* const* grads, hipStream_t st) {
    for (int l = 0; l < n_layers; ++l) {
        if (!grads[2 * l] && !grads[2 * l + 1]) continue;
        hipLaunchKernelGGL(k_finish, ew_grid((long)L[l].n_out * (L[l].k_in + 1)), dim3(256), 0, st, D + acc_off[l], L[l].n_out, L[l].k_in,
                           grads[2 * l], grads[2 * l + 1]);
        ++g_launches;
    }
}

// the scratch allocator: offsets in doubles, every buffer starts a multiple of 8 doubles after the previous one
struct Take {
    long o = 0;
    long operator()(long n) { long at = o; o += (n + 7) & ~7L; return at; }
};

// what every entry point checks of the caller's scratch; `query`: the library's function that returns `need`
int check_scratch(const void* scratch, long scratch_bytes, long need, const char* query) {
    if (!scratch) return fail("null pointer: scratch");
    if ((uintptr_t)scratch % 8) return fail("scratch is not 8-byte aligned");
    if (scratch_bytes < need) return fail("scratch too small: %ld bytes given, %ld needed (%s)", scratch_bytes, need, query);
    return 0;
}

}  // namespace
