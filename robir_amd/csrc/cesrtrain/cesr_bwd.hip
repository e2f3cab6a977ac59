// librobir_hip_cesrtrain.so: the training side of the two CESR networks (include/robir_hip_cesrtrain.h) -- the reverse mode of
// SDFNetwork(d_in, d_out, 512, 8, skip [4], multires 0): nine weight-normed layers, softplus(beta = 100) after the first eight, the input
// rejoining before layer 4 as [h | x] / sqrt(2); shadow_net (191 -> 2) and normal_net (63 -> 3) of training/train_cesr.py:107-110.
//
// vistrain/vis_bwd.hip's and illumtrain/illum_bwd.hip's shape of problem on the same engine (k_gemm64 of ../train/gemm64.h, instantiated
// here for the softplus-100 family with per-partition partials) under the same slab driver (../train/chain.h): everything is fp64, the
// encoding is evaluated in double from the fp32 coordinates, the activations are recomputed, each stored gradient is rounded once.  This
// file holds what is particular: the weight-norm fold (k_wnorm, tree_sum) and its reverse (k_finish_wn), k_encode / k_rows / k_skip_fill,
// k_head_bwd, the plan, the argument checks and the order of the slab loop.
//
// The skip layer: A[3] is a 512-wide buffer whose first 512 - d_in columns layer 3 writes and whose last d_in columns hold x, so layer 4
// reads [h | x] as it stands; the 1/sqrt(2) sits in the folded W_4 (the same function), comes back into dW_4 in k_finish_wn, and dZ_3 is
// the product with W_4's first 512 - d_in columns only.
//
// Reductions over rows are DESIGN 4.5's (wgrad_parts of chain.h): no atomics, the association is a function of (M, slab_rows, part_rows)
// alone.
#include "../../../include/robir_hip_cesrtrain.h"
#include "../train/chain.h"

namespace {

constexpr int HID = 512, PE = 63, LABELS = 128, X_LD = 192, RAW_LD = 8, NL = 9, SKIP = 4;
constexpr double RSQRT2 = 0.70710678118654752440;
constexpr int WT = 256;                       // lanes of a weight-norm workgroup: one workgroup owns one output row

// softplus-100 where the act flag is set (the raw output has none); weight gradients leave as per-partition partials (k_reduce)
constexpr auto fwd = fwd_layer<ACT_SOFTPLUS100_OPT, RED_PART>;
constexpr auto wgrad = wgrad_parts<ACT_SOFTPLUS100_OPT, RED_PART>;
constexpr auto bwd = dgrad<ACT_SOFTPLUS100_OPT, RED_PART>;

// X[i, :] of the points form, i < S, row stride ld: column c < 63 is PE10 of point (row0 + i) / n_label (pe10_col) and, kind 1, column
// 63 + j is 1 where j == (row0 + i) % n_label, else 0: built from the row index
__global__ void k_encode(const float* points, long row0, long S, int n_label, int d_in, int ld, double* X) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * d_in) return;
    const long row = i / d_in, grow = row0 + row;
    const int c = (int)(i % d_in);
    const float* src = points + (grow / n_label) * 3;
    X[row * ld + c] = c >= PE ? (c - PE == (int)(grow % n_label) ? 1.0 : 0.0) : pe10_col(src, c);
}

// the dense form: X[i, c] = rows[(row0 + i) rows_ld + c], c < d_in
__global__ void k_rows(const float* rows, long rows_ld, long row0, long S, int d_in, int ld, double* X) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * d_in) return;
    const long row = i / d_in;
    const int c = (int)(i % d_in);
    X[row * ld + c] = (double)rows[(row0 + row) * rows_ld + c];
}

// A3[i, 512 - d_in + c] = X[i, c]: the input's half of what the skip layer reads
__global__ void k_skip_fill(const double* X, int ld, long S, int d_in, double* A3) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * d_in) return;
    const long row = i / d_in;
    const int c = (int)(i % d_in);
    A3[row * HID + (HID - d_in) + c] = X[row * ld + c];
}

// sum over the WT lanes in one fixed binary tree; every lane returns the total
__device__ __forceinline__ double tree_sum(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();          // red may still be read from the previous sum
    red[t] = v;
    __syncthreads();
    for (int off = WT / 2; off > 0; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    return red[0];
}

// W[o, :] = scale g[o] v[o, :] / |v[o, :]| in fp64, one workgroup per output row: lane t adds its columns t, t + 256, ... in order
__global__ __launch_bounds__(WT) void k_wnorm(const float* v, const float* g, int k_in, double scale, double* W) {
    __shared__ double red[WT];
    const long o = blockIdx.x;
    const float* vr = v + o * k_in;
    double s2 = 0.0;
    for (int c = threadIdx.x; c < k_in; c += WT) s2 += (double)vr[c] * (double)vr[c];
    const double f = scale * (double)g[o] / sqrt(tree_sum(s2, red));
    for (int c = threadIdx.x; c < k_in; c += WT) W[o * k_in + c] = f * (double)vr[c];
}

// fp64 accumulator [n_out, k_in + 1] (last column: bias) -> the three parameter-shaped fp32 gradients of a weight-normed layer, one rounding
// each: with dW = scale acc[o, :k_in] and v^ = v / |v|:  dg = dW . v^,  dv = (g / |v|) (dW - dg v^),  db = acc[o, k_in]
__global__ __launch_bounds__(WT) void k_finish_wn(const double* acc, int k_in, const float* v, const float* g, double scale, float* gg, float* gv,
                                                  float* gb) {
    __shared__ double red[WT];
    const long o = blockIdx.x;
    const double* a = acc + o * (k_in + 1);
    const float* vr = v + o * k_in;
    double s2 = 0.0, sd = 0.0;
    for (int c = threadIdx.x; c < k_in; c += WT) {
        s2 += (double)vr[c] * (double)vr[c];
        sd += a[c] * (double)vr[c];
    }
    const double nrm = sqrt(tree_sum(s2, red));
    const double dg = scale * tree_sum(sd, red) / nrm;
    if (threadIdx.x == 0) {
        if (gg) gg[o] = (float)dg;
        if (gb) gb[o] = (float)a[k_in];
    }
    if (gv) {
        const double f = (double)g[o] / nrm;
        for (int c = threadIdx.x; c < k_in; c += WT) gv[o * k_in + c] = (float)(f * (scale * a[c] - dg * ((double)vr[c] / nrm)));
    }
}

// dZ[i, :d_out] = d <g_out, head(raw)> / d raw[i, :], one thread per row; raw has row stride RAW_LD, dZ row stride d_out
__global__ void k_head_bwd(const double* raw, const float* g_out, long S, int d_out, int head, double* dZ) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    const double* z = raw + i * RAW_LD;
    double* o = dZ + i * d_out;
    if (head == 0) {
        for (int c = 0; c < d_out; ++c) o[c] = (double)g_out[i * d_out + c];
    } else if (head == 1) {          // p = softmax(z)[1] = sigmoid(z1 - z0): dp / dz1 = p (1 - p) = -dp / dz0
        const double p = 1.0 / (1.0 + exp(z[0] - z[1]));
        const double d = (double)g_out[i] * p * (1.0 - p);
        o[0] = -d;
        o[1] = d;
    } else {                         // y = z / max(|z|, eps): (g - y <y, g>) / |z| where the norm decides, g / eps below
        const double gx = (double)g_out[3 * i], gy = (double)g_out[3 * i + 1], gz = (double)g_out[3 * i + 2];
        const double nrm = sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
        const double eps = 1e-4;
        if (nrm > eps) {
            const double y0 = z[0] / nrm, y1 = z[1] / nrm, y2 = z[2] / nrm;
            const double along = y0 * gx + y1 * gy + y2 * gz;
            o[0] = (gx - y0 * along) / nrm; o[1] = (gy - y1 * along) / nrm; o[2] = (gz - y2 * along) / nrm;
        } else {
            o[0] = gx / eps; o[1] = gy / eps; o[2] = gz / eps;
        }
    }
}

struct Plan {
    long W[NL], acc_off[NL];      // doubles
    long nparts;                  // partitions of a full slab
    long partial, X, A[8], raw, dZ[2], total;
};

// independent of the kind: layer 0 and the last layer are sized for the wider of the two nets
Plan make_plan(long S, long part_rows) {
    Plan p;
    Take take;
    for (int l = 0; l < NL; ++l) p.W[l] = take(l == 0 ? (long)HID * X_LD : l == 8 ? 3L * HID : (long)HID * HID);
    for (int l = 0; l < NL; ++l) p.acc_off[l] = take(l == 0 ? (long)HID * X_LD : l == 8 ? 3L * (HID + 1) : (long)HID * (HID + 1));
    p.nparts = (S + part_rows - 1) / part_rows;
    p.partial = take(p.nparts * PART_ELEMS<HID>);
    p.X = take(S * X_LD);
    for (int l = 0; l < 8; ++l) p.A[l] = take(S * HID);
    p.raw = take(S * RAW_LD);
    p.dZ[0] = take(S * HID);
    p.dZ[1] = take(S * HID);
    p.total = take.o;
    return p;
}

}  // namespace

extern "C" {

int rb_ct_abi_version(void) { return RB_CT_ABI_VERSION; }

const char* rb_ct_last_error(void) { return g_err; }

long rb_ct_cesr_bwd_scratch_bytes(long M, long slab_rows, long part_rows) {
    if (!check_rows("M", M, slab_rows, part_rows)) return -1;
    return make_plan(query_slab_size(M, slab_rows), part_rows).total * (long)sizeof(double);
}

int rb_ct_cesr_bwd(const float* points, const float* rows, long ld, long M, int kind, int n_label, int head, const float* const* params,
                   const float* g_out, float* const* grads, long slab_rows, long part_rows, void* scratch, long scratch_bytes, int* stats,
                   rb_ct_stream_t stream) {
    if (!check_rows("M", M, slab_rows, part_rows)) return 1;
    if (kind != 0 && kind != 1) return fail("kind = %d: 0 normal_net (63 -> 3), 1 shadow_net (191 -> 2)", kind);
    if (head < 0 || head > 2 || (head == 1 && kind != 1) || (head == 2 && kind != 0))
        return fail("head = %d with kind = %d: 0 raw output, 1 softmax class-1 probability (kind 1 only), 2 unit vector (kind 0 only)", head, kind);
    if (n_label < 1 || n_label > LABELS) return fail("n_label = %d outside [1, %d]", n_label, LABELS);
    if (kind == 0 && points && n_label != 1) return fail("n_label = %d: the points form of kind 0 has one row per point", n_label);
    if (M % n_label) return fail("M = %ld is not a multiple of n_label = %d", M, n_label);
    if (!params || !grads) return fail("null pointer: params / grads (HOST arrays of 27 device pointers)");
    if (stats) { stats[0] = 0; stats[1] = NL; stats[2] = 0; }
    if (M == 0) return 0;
    const int d_in = kind ? PE + LABELS : PE, d_out = kind ? 2 : 3, in_ld = kind ? X_LD : 64;
    if (!points == !rows) return fail("exactly one of points / rows is given (points form / dense form)");
    if (rows && ld < d_in) return fail("ld = %ld is smaller than d_in = %d", ld, d_in);
    if (!g_out) return fail("null pointer: g_out");
    for (int i = 0; i < 3 * NL; ++i)
        if (!params[i]) return fail("null pointer: params[%d]", i);
    bool want_layer[NL];
    const int lowest = scan_wanted(grads, NL, 3, want_layer);      // first layer that wants a gradient: the data path stops there
    if (lowest == NL) return 0;
    const long S0 = slab_size(M, slab_rows);
    const Plan pl = make_plan(S0, part_rows);
    if (check_scratch(scratch, scratch_bytes, pl.total * (long)sizeof(double), "rb_ct_cesr_bwd_scratch_bytes")) return 1;
    hipStream_t st = (hipStream_t)stream;
    double* D = (double*)scratch;
    g_launches = 0;
    int bad = 0;
    Layer LAYERS[NL];
    for (int l = 0; l < NL; ++l) LAYERS[l] = {l == 3 ? HID - d_in : l == 8 ? d_out : HID, l == 0 ? d_in : HID, l == 0 ? (long)in_ld : (long)HID};
    const float* const* G = params;                   // G[3 l] = weight_g, G[3 l + 1] = weight_v, G[3 l + 2] = bias
    for (int l = 0; l < NL; ++l) {
        hipLaunchKernelGGL(k_wnorm, dim3(LAYERS[l].n_out), dim3(WT), 0, st, G[3 * l + 1], G[3 * l], LAYERS[l].k_in, l == SKIP ? RSQRT2 : 1.0,
                           D + pl.W[l]);
        ++g_launches;
    }

    for (long row0 = 0; row0 < M; row0 += S0) {
        const long S = M - row0 < S0 ? M - row0 : S0;
        const int first = row0 == 0;
        const double* in[NL];                         // input rows of layer l
        in[0] = D + pl.X;
        for (int l = 1; l < NL; ++l) in[l] = D + pl.A[l - 1];
        if (points)
            hipLaunchKernelGGL(k_encode, ew_grid(S * d_in), dim3(256), 0, st, points, row0, S, n_label, d_in, in_ld, D + pl.X);
        else
            hipLaunchKernelGGL(k_rows, ew_grid(S * d_in), dim3(256), 0, st, rows, ld, row0, S, d_in, in_ld, D + pl.X);
        hipLaunchKernelGGL(k_skip_fill, ew_grid(S * d_in), dim3(256), 0, st, D + pl.X, in_ld, S, d_in, D + pl.A[3]);
        g_launches += 2;
        for (int l = 0; l < NL; ++l)
            bad |= fwd(LAYERS[l], S, in[l], 0, D + pl.W[l], 0, G[3 * l + 2], l < 8, l < 8 ? D + pl.A[l] : D + pl.raw, l < 8 ? HID : RAW_LD, st);
        // d loss / d (pre-activation of layer l) sits in dz [S, dz_ld]: the head's derivative for the last layer (dZ[1], d_out wide)
        const long g_w = head == 1 ? 1 : d_out;
        hipLaunchKernelGGL(k_head_bwd, ew_grid(S), dim3(256), 0, st, D + pl.raw, g_out + row0 * g_w, S, d_out, head, D + pl.dZ[1]);
        ++g_launches;
        const double* dz = D + pl.dZ[1];
        long dz_ld = d_out;
        for (int l = NL - 1; l >= lowest; --l) {
            const Layer& L = LAYERS[l];
            if (want_layer[l]) bad |= wgrad(L, S, dz, 0, dz_ld, in[l], part_rows, D + pl.partial, D + pl.acc_off[l], first, st);
            if (l > lowest) {
                // dZ_{l-1} = (dZ_l W_l) . gate(A_{l-1}); the skip layer: into the first 512 - d_in of its input columns only
                double* to = D + pl.dZ[l & 1];
                bad |= bwd(L, S, dz, 0, dz_ld, D + pl.W[l], 0, LAYERS[l - 1].n_out, 1, in[l], to, st);
                dz = to;
                dz_ld = HID;
            }
        }
    }
    for (int l = 0; l < NL; ++l) {
        if (!want_layer[l]) continue;
        hipLaunchKernelGGL(k_finish_wn, dim3(LAYERS[l].n_out), dim3(WT), 0, st, D + pl.acc_off[l], LAYERS[l].k_in, G[3 * l + 1], G[3 * l],
                           l == SKIP ? RSQRT2 : 1.0, grads[3 * l], grads[3 * l + 1], grads[3 * l + 2]);
        ++g_launches;
    }
    if (stats) { stats[0] = g_launches; stats[1] = lowest; stats[2] = (int)pl.nparts; }
    if (bad || hipGetLastError() != hipSuccess) return fail("kernel launch failed");
    return 0;
}

}  // extern "C"
