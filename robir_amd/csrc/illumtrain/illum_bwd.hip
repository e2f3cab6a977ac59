// librobir_hip_illumtrain.so: the training side of IndirctIllumNetwork (include/robir_hip_illumtrain.h) -- the reverse mode of
// its lobe net, [PE10(x) | hdr_shift] -> 512 x 4 ReLU -> 144 -> 24 lobes (two sigmoids to a unit axis, sigmoid 30 + 0.1, ReLU), and the
// spherical-Gaussian query of model/loss.py:128-141 with its reverse.
//
// The lobe net is vistrain/vis_bwd.hip's shape of problem and runs on the same engine (k_gemm64 of ../train/gemm64.h, instantiated here for
// the family with one layer that has no activation -- the raw output the head reads -- and per-partition partials) under the same slab
// driver (../train/chain.h): everything is fp64, the encoding is evaluated in double from the fp32 coordinates, the activations are
// recomputed, each stored gradient is rounded once (k_finish).  This file holds what is particular: k_encode, k_head_bwd, the plan, the
// argument checks and the order of the slab loop, and the two query kernels.
//
// Reductions over rows are DESIGN 4.5's (wgrad_parts of chain.h): no atomics, the association is a function of (n, slab_rows, part_rows)
// alone.
#include "../../../include/robir_hip_illumtrain.h"
#include "../train/chain.h"

namespace {

constexpr int HID = 512, IN_LD = 64, PE = 63, LOBES = 24, RAW = LOBES * 6, SG = 7;
constexpr double PI = 3.14159265358979323846;

// ReLU where the act flag is set (the raw output has none); weight gradients leave as per-partition partials (k_reduce)
constexpr auto fwd = fwd_layer<ACT_RELU_OPT, RED_PART>;
constexpr auto wgrad = wgrad_parts<ACT_RELU_OPT, RED_PART>;
constexpr auto bwd = dgrad<ACT_RELU_OPT, RED_PART>;

// X[i, :] = [PE10(points[row0 + i]) | hdr[row0 + i]], i < S (pe10_col: a column of PE10); column 63 is the hdr shift, 0 without one
__global__ void k_encode(const float* points, const float* hdr, long row0, long S, double* X) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * IN_LD) return;
    const long row = i / IN_LD;
    const int c = (int)(i % IN_LD);
    const float* src = points + (row0 + row) * 3;
    X[i] = c == PE ? (hdr ? (double)hdr[row0 + row] : 0.0) : pe10_col(src, c);
}

__device__ __forceinline__ double sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

// dZ[i, 6 j .. 6 j + 5] = d <g_sgs, lgt_sgs> / d raw[i, 6 j .. 6 j + 5], one thread per (row, lobe)
// (implicit_differentiable_renderer.py:206-218 written out: theta = 2 pi sigmoid(a), phi = pi sigmoid(b), axis = (cos theta sin phi,
// sin theta sin phi, cos phi), lambda = 30 sigmoid(c) + 0.1, mu = relu: gated by raw > 0)
__global__ void k_head_bwd(const double* raw, const float* g_sgs, long S, double* dZ) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * LOBES) return;
    const double* z = raw + i * 6;
    const float* g = g_sgs + i * SG;
    double* o = dZ + i * 6;
    const double sa = sigmoid(z[0]), sb = sigmoid(z[1]), sc = sigmoid(z[2]);
    const double theta = 2.0 * PI * sa, phi = PI * sb;
    const double ct = cos(theta), st = sin(theta), cp = cos(phi), sp = sin(phi);
    const double gx = (double)g[0], gy = (double)g[1], gz = (double)g[2];
    o[0] = (gy * ct - gx * st) * sp * (2.0 * PI * sa * (1.0 - sa));
    o[1] = ((gx * ct + gy * st) * cp - gz * sp) * (PI * sb * (1.0 - sb));
    o[2] = (double)g[3] * (30.0 * sc * (1.0 - sc));
    for (int c = 0; c < 3; ++c) o[3 + c] = z[3 + c] > 0.0 ? (double)g[4 + c] : 0.0;
}

struct Plan {
    long acc_off[5];          // doubles
    long nparts;              // partitions of a full slab
    long partial, X, A[4], raw, dZ[2], total;
};

// independent of hdr: the accumulator of layer 0 is sized for 64 input columns
Plan make_plan(long S, long part_rows) {
    Plan p;
    Take take;
    p.acc_off[0] = take((long)HID * (IN_LD + 1));
    for (int l = 1; l < 4; ++l) p.acc_off[l] = take((long)HID * (HID + 1));
    p.acc_off[4] = take((long)RAW * (HID + 1));
    p.nparts = (S + part_rows - 1) / part_rows;
    p.partial = take(p.nparts * PART_ELEMS<HID>);
    p.X = take(S * IN_LD);
    for (int l = 0; l < 4; ++l) p.A[l] = take(S * HID);
    p.raw = take(S * RAW);
    p.dZ[0] = take(S * HID);
    p.dZ[1] = take(S * HID);
    p.total = take.o;
    return p;
}

// ---------------------------------------------------------------------------------------------------------------- the SG query
constexpr int QT = 256;           // lanes of a query workgroup: one workgroup owns one point
constexpr int MAX_L = 32;

// lobes of point i -> LDS in fp64: unit axis [3], lambda, mu [3], and the norm of the stored axis
__device__ __forceinline__ void load_lobes(const float* sgs, long i, int L, double (*lobe)[8]) {
    for (int j = threadIdx.x; j < L; j += QT) {
        const float* s = sgs + (i * L + j) * SG;
        const double x = (double)s[0], y = (double)s[1], z = (double)s[2];
        const double nrm = sqrt(x * x + y * y + z * z);
        lobe[j][0] = x / nrm; lobe[j][1] = y / nrm; lobe[j][2] = z / nrm;
        lobe[j][3] = (double)s[3];
        lobe[j][4] = (double)s[4]; lobe[j][5] = (double)s[5]; lobe[j][6] = (double)s[6];
        lobe[j][7] = nrm;
    }
    __syncthreads();
}

__global__ __launch_bounds__(QT) void k_sg_query(const float* sgs, const float* dirs, int L, long S, float* radiance) {
    __shared__ double lobe[MAX_L][8];
    const long i = blockIdx.x;
    load_lobes(sgs, i, L, lobe);
    for (long s = threadIdx.x; s < S; s += QT) {
        const float* d = dirs + (i * S + s) * 3;
        const double dx = (double)d[0], dy = (double)d[1], dz = (double)d[2];
        double r0 = 0.0, r1 = 0.0, r2 = 0.0;
        for (int j = 0; j < L; ++j) {
            const double e = exp(lobe[j][3] * (dx * lobe[j][0] + dy * lobe[j][1] + dz * lobe[j][2] - 1.0));
            r0 += lobe[j][4] * e; r1 += lobe[j][5] * e; r2 += lobe[j][6] * e;
        }
        float* o = radiance + (i * S + s) * 3;
        o[0] = (float)r0; o[1] = (float)r1; o[2] = (float)r2;
    }
}

// With e = exp(lambda (c - 1)), c = d . axis and w = e <g, mu>:  g_mu = sum_s g e,  g_lambda = sum_s w (c - 1),  G = lambda sum_s w d is the
// gradient on the UNIT axis, and g_l = (G - axis <axis, G>) / |l|.  Per lobe: lane t adds its samples t, t + 256, ... in order, the 256
// lane sums of the seven quantities meet in one binary tree in LDS, lane 0 stores the lobe's seven floats.
__global__ __launch_bounds__(QT) void k_sg_query_bwd(const float* sgs, const float* dirs, const float* g_rad, int L, long S, float* g_sgs) {
    __shared__ double lobe[MAX_L][8];
    __shared__ double red[7][QT];
    const long i = blockIdx.x;
    const int t = threadIdx.x;
    load_lobes(sgs, i, L, lobe);
    for (int j = 0; j < L; ++j) {
        const double ax = lobe[j][0], ay = lobe[j][1], az = lobe[j][2], lam = lobe[j][3];
        const double m0 = lobe[j][4], m1 = lobe[j][5], m2 = lobe[j][6];
        double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // g_mu [3], g_lambda, sum w d [3]
        for (long s = t; s < S; s += QT) {
            const float* d = dirs + (i * S + s) * 3;
            const float* g = g_rad + (i * S + s) * 3;
            const double dx = (double)d[0], dy = (double)d[1], dz = (double)d[2];
            const double g0 = (double)g[0], g1 = (double)g[1], g2 = (double)g[2];
            const double c1 = dx * ax + dy * ay + dz * az - 1.0;
            const double e = exp(lam * c1);
            const double w = (g0 * m0 + g1 * m1 + g2 * m2) * e;
            a[0] += g0 * e; a[1] += g1 * e; a[2] += g2 * e;
            a[3] += w * c1;
            a[4] += w * dx; a[5] += w * dy; a[6] += w * dz;
        }
        for (int k = 0; k < 7; ++k) red[k][t] = a[k];
        __syncthreads();
        for (int off = QT / 2; off > 0; off >>= 1) {
            if (t < off)
                for (int k = 0; k < 7; ++k) red[k][t] += red[k][t + off];
            __syncthreads();
        }
        if (t == 0) {
            const double Gx = lam * red[4][0], Gy = lam * red[5][0], Gz = lam * red[6][0];
            const double along = ax * Gx + ay * Gy + az * Gz, nrm = lobe[j][7];
            float* o = g_sgs + (i * L + j) * SG;
            o[0] = (float)((Gx - ax * along) / nrm);
            o[1] = (float)((Gy - ay * along) / nrm);
            o[2] = (float)((Gz - az * along) / nrm);
            o[3] = (float)red[3][0];
            o[4] = (float)red[0][0]; o[5] = (float)red[1][0]; o[6] = (float)red[2][0];
        }
        __syncthreads();      // red is rewritten by the next lobe
    }
}

bool check_query(long n, int L, long S) {
    if (n < 0 || S < 0) return fail("n = %ld / S = %ld is negative", n, S), false;
    if (L < 1 || L > MAX_L) return fail("L = %d outside [1, %d]", L, MAX_L), false;
    if (n > 0x7fffffffL) return fail("n = %ld: at most 2^31 - 1 points per call (one workgroup each)", n), false;
    return true;
}

}  // namespace

extern "C" {

int rb_it_abi_version(void) { return RB_IT_ABI_VERSION; }

const char* rb_it_last_error(void) { return g_err; }

long rb_it_lobe_bwd_scratch_bytes(long n, long slab_rows, long part_rows) {
    if (!check_rows("n", n, slab_rows, part_rows)) return -1;
    return make_plan(query_slab_size(n, slab_rows), part_rows).total * (long)sizeof(double);
}

int rb_it_lobe_bwd(const float* points, const float* hdr, long n, const float* const* params, const float* g_sgs, float* const* grads,
                   long slab_rows, long part_rows, void* scratch, long scratch_bytes, int* stats, rb_it_stream_t stream) {
    if (!check_rows("n", n, slab_rows, part_rows)) return 1;
    if (!params || !grads) return fail("null pointer: params / grads (HOST arrays of 10 device pointers)");
    if (stats) { stats[0] = 0; stats[1] = 5; stats[2] = 0; }
    if (n == 0) return 0;
    if (!points || !g_sgs) return fail("null pointer: points / g_sgs");
    for (int i = 0; i < 10; ++i)
        if (!params[i]) return fail("null pointer: params[%d]", i);
    bool want_layer[5];
    const int lowest = scan_wanted(grads, 5, 2, want_layer);      // first layer that wants a gradient: the data path stops there
    if (lowest == 5) return 0;
    const long S0 = slab_size(n, slab_rows);
    const Plan pl = make_plan(S0, part_rows);
    if (check_scratch(scratch, scratch_bytes, pl.total * (long)sizeof(double), "rb_it_lobe_bwd_scratch_bytes")) return 1;
    hipStream_t st = (hipStream_t)stream;
    double* D = (double*)scratch;
    g_launches = 0;
    int bad = 0;
    // the no_hdr net has no weight column for the hdr shift: W0 is [512, 63] and column 63 of X is never read
    const Layer LAYERS[5] = {{HID, hdr ? IN_LD : PE, IN_LD}, {HID, HID, HID}, {HID, HID, HID}, {HID, HID, HID}, {RAW, HID, HID}};

    for (long row0 = 0; row0 < n; row0 += S0) {
        const long S = n - row0 < S0 ? n - row0 : S0;
        const int first = row0 == 0;
        const double* in[5] = {D + pl.X, D + pl.A[0], D + pl.A[1], D + pl.A[2], D + pl.A[3]};      // input rows of layer l
        hipLaunchKernelGGL(k_encode, ew_grid(S * IN_LD), dim3(256), 0, st, points, hdr, row0, S, D + pl.X);
        ++g_launches;
        for (int l = 0; l < 5; ++l)
            bad |= fwd(LAYERS[l], S, in[l], 0, params[2 * l], 1, params[2 * l + 1], l < 4, l < 4 ? D + pl.A[l] : D + pl.raw, LAYERS[l].n_out, st);
        // d loss / d (pre-activation of layer l) sits in dz [S, dz_ld]: the head's derivative for the last layer (dZ[1], 144 wide)
        hipLaunchKernelGGL(k_head_bwd, ew_grid(S * LOBES), dim3(256), 0, st, D + pl.raw, g_sgs + row0 * LOBES * SG, S, D + pl.dZ[1]);
        ++g_launches;
        const double* dz = D + pl.dZ[1];
        long dz_ld = RAW;
        for (int l = 4; l >= lowest; --l) {
            const Layer& L = LAYERS[l];
            if (want_layer[l]) bad |= wgrad(L, S, dz, 0, dz_ld, in[l], part_rows, D + pl.partial, D + pl.acc_off[l], first, st);
            if (l > lowest) {
                double* to = D + pl.dZ[l & 1];
                bad |= bwd(L, S, dz, 0, dz_ld, params[2 * l], 1, L.k_in, 1, in[l], to, st);
                dz = to;
                dz_ld = HID;
            }
        }
    }
    finish_layers(LAYERS, 5, D, pl.acc_off, grads, st);
    if (stats) { stats[0] = g_launches; stats[1] = lowest; stats[2] = (int)pl.nparts; }
    if (bad || hipGetLastError() != hipSuccess) return fail("kernel launch failed");
    return 0;
}

int rb_it_sg_query(const float* sgs, const float* dirs, long n, int L, long S, float* radiance, rb_it_stream_t stream) {
    if (!check_query(n, L, S)) return 1;
    if (n == 0 || S == 0) return 0;
    if (!sgs || !dirs || !radiance) return fail("null pointer: sgs / dirs / radiance");
    hipLaunchKernelGGL(k_sg_query, dim3((unsigned)n), dim3(QT), 0, (hipStream_t)stream, sgs, dirs, L, S, radiance);
    if (hipGetLastError() != hipSuccess) return fail("kernel launch failed");
    return 0;
}

int rb_it_sg_query_bwd(const float* sgs, const float* dirs, const float* g_radiance, long n, int L, long S, float* g_sgs,
                       rb_it_stream_t stream) {
    if (!check_query(n, L, S)) return 1;
    if (n == 0) return 0;
    if (!sgs || !dirs || !g_radiance || !g_sgs) return fail("null pointer: sgs / dirs / g_radiance / g_sgs");
    hipLaunchKernelGGL(k_sg_query_bwd, dim3((unsigned)n), dim3(QT), 0, (hipStream_t)stream, sgs, dirs, g_radiance, L, S, g_sgs);
    if (hipGetLastError() != hipSuccess) return fail("kernel launch failed");
    return 0;
}

}  // extern "C"
