// identity.hip -- identity training for Gaussian grouping (Gaussian Grouping / Gaga; the reference's unfinished
// `GroupingClassifier.setup_train`, utils/grouping.py:110-136, restated from the published method): every Gaussian carries
// an identity vector of D <= 32 channels, a linear classifier (a 1 x 1 convolution, weight [K, D], bias [K]) maps a rendered
// pixel or a Gaussian's own vector onto K classes.
//   2-D loss:  z = W x + b per pixel, ce = logsumexp(z) - z[t - 1], loss = sum_labelled ce / max(n_labelled, 1)
//   3-D loss:  p_j = softmax(W e_j + b), loss = sum_pairs KL(p_sample || p_neighbour) / max(n_pairs, 1)
//   labels:    argmax_k z (+ 1), optionally max_k softmax(z)
// No [K, P] tensor exists in either direction.  lane = pixel (or pair side): the row's D values sit in registers across all
// classes, the classifier rows are wave-uniform and come through scalar loads, the contraction runs on the f32 VALU (f32-input
// MFMA has the VALU's rate on gfx950 and a reduced-precision format would change the loss).  The classes are walked in units of
// 16: a unit's logits, its maximum, one rescale of the running sum, 16 exponentials.  Backward recomputes the logits from the
// stored per-row log-sum-exp.  d/dx is per lane; d/dW is a sum over rows: grid (class units, row splits), a tile's 16 d/dz
// values and its rows go through LDS, thread = (channel, row group) accumulates, the row groups meet in ascending order and
// the splits' partial sums in fp64.  No floating-point atomic: two runs are equal bit for bit.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "misplat.h"
#include "rowlinear.h"
#include "wgprims.h"

namespace {

constexpr int kMaxD = 32;
constexpr int kMaxK = 4096;
constexpr int kMaxNb = 16;                      // widest neighbour table
constexpr int kUnit = 16;                       // classes walked at a time; the class unit of the weight-gradient grid
constexpr int kTile = 256;                      // rows of a workgroup (thread = row)
constexpr int kRS = kUnit + 4;                  // LDS row strides (floats), 16-byte aligned
constexpr int64_t kMaxRows = (int64_t)1 << 28;

// ---------------------------------------------------------------------------------------------------- the contraction
// A lane's row and one logit, bias + <row of W, x>: load_row and dot2 of rowlinear.h.

// log-sum-exp over the K classes, the maximum subtracted; *zt = the logit of class t (unchanged if t is not in 0 .. K - 1);
// *best = the first class that attains the maximum
template <int DP, bool kFull>
__device__ __forceinline__ void lse_walk(const float* __restrict__ W, const float* __restrict__ b, int K, int D, const float (&x)[DP],
                                         int t, float* lse, float* zt, int* best, float* conf) {
    float m = -INFINITY, s = 0.f, zsel = 0.f;
    int arg = 0;
    for (int k0 = 0; k0 < K; k0 += kUnit) {
        float z[kUnit], cm = m;
#pragma unroll
        for (int u = 0; u < kUnit; u++) {
            const int k = k0 + u;
            z[u] = -INFINITY;
            if (k < K) {
                z[u] = dot2<DP, kFull>(W + (size_t)k * D, b[k], x, D);
                zsel = k == t ? z[u] : zsel;
                arg = z[u] > cm ? k : arg;
                cm = fmaxf(cm, z[u]);
            }
        }
        s *= expf(m - cm);
#pragma unroll
        for (int u = 0; u < kUnit; u++) s += expf(z[u] - cm);
        m = cm;
    }
    *lse = m + logf(s);
    if (zt) *zt = zsel;
    if (best) *best = arg;
    if (conf) *conf = 1.0f / s;
}

// ---------------------------------------------------------------------------------------------------- 2-D: forward
// part [tiles][3] doubles: the tile's sum of ce, its labelled pixels and its pixels with a target outside 0 .. K
template <int DP, bool kFull>
__global__ __launch_bounds__(256) void ce_fwd_kernel(int64_t P, int D, int K, int stride, const float* __restrict__ features,
                                                     const float* __restrict__ W, const float* __restrict__ b,
                                                     const int32_t* __restrict__ target, float* __restrict__ lse_out,
                                                     double* __restrict__ part) {
    const int64_t p = (int64_t)blockIdx.x * kTile + threadIdx.x, pc = p < P ? p : P - 1;
    const int t = target[pc];
    const bool ok = p < P, lab = ok && t >= 1 && t <= K, bad = ok && (t < 0 || t > K);
    float lse = 0.f, zt = 0.f;
    if (__any(lab)) {
        float x[DP];
        load_row<DP, kFull>(x, features + pc * stride, D);
        lse_walk<DP, kFull>(W, b, K, D, x, t - 1, &lse, &zt, nullptr, nullptr);
    }
    if (ok) lse_out[p] = lse;
    double v[3] = {lab ? (double)(lse - zt) : 0.0, lab ? 1.0 : 0.0, bad ? 1.0 : 0.0};
    block_sums<3, 4>(v, part + 3 * (int64_t)blockIdx.x);
}

// loss = sum / max(n, 1); counts = (n, the rows outside the range)
__global__ __launch_bounds__(256) void loss_final_kernel(const double* __restrict__ part, int64_t nb, float* __restrict__ loss,
                                                         int32_t* __restrict__ counts) {
    __shared__ double out[3];
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < nb; i += 256)
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] += part[3 * i + k];
    block_sums<3, 4>(v, out);
    __syncthreads();
    if (threadIdx.x == 0) {
        *loss = (float)(out[0] / (out[1] > 1.0 ? out[1] : 1.0));
        counts[0] = (int32_t)out[1];
        counts[1] = (int32_t)out[2];
    }
}

__device__ __forceinline__ float grad_scale(const float* __restrict__ g_loss, const int32_t* __restrict__ counts) {
    const int32_t n = counts[0];
    return (g_loss ? *g_loss : 0.f) / (float)(n > 1 ? n : 1);
}

// ---------------------------------------------------------------------------------------------------- 2-D: d/dx
template <int DP, bool kFull>
__global__ __launch_bounds__(256) void ce_bwd_dx_kernel(int64_t P, int D, int K, int stride, const float* __restrict__ features,
                                                        const float* __restrict__ W, const float* __restrict__ b,
                                                        const int32_t* __restrict__ target, const float* __restrict__ lse_in,
                                                        const int32_t* __restrict__ counts, const float* __restrict__ g_loss,
                                                        float* __restrict__ v_features) {
    const int64_t p = (int64_t)blockIdx.x * kTile + threadIdx.x, pc = p < P ? p : P - 1;
    const int t = target[pc];
    const bool ok = p < P, lab = ok && t >= 1 && t <= K;
    const float ws = grad_scale(g_loss, counts);
    float dx[DP];
#pragma unroll
    for (int d = 0; d < DP; d++) dx[d] = 0.f;
    if (__any(lab)) {
        float x[DP];
        load_row<DP, kFull>(x, features + pc * stride, D);
        const float l = lse_in[pc];
#pragma unroll 2
        for (int k = 0; k < K; k++) {
            const float* wr = W + (size_t)k * D;
            const float z = dot2<DP, kFull>(wr, b[k], x, D);
            const float r = (expf(z - l) - (k == t - 1 ? 1.f : 0.f)) * ws;
#pragma unroll
            for (int d = 0; d < DP; d++)
                if (kFull || d < D) dx[d] = fmaf(wr[d], r, dx[d]);
        }
    }
    if (ok) {
        float* out = v_features + p * D;
#pragma unroll
        for (int d = 0; d < DP; d++)
            if (kFull || d < D) out[d] = lab ? dx[d] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------- 3-D: the pairs
struct Pairs {
    const float* e;                             // identities [N, D]
    const int64_t* sample;                      // [M]
    const int32_t* table;                       // [M, nb]
    int64_t N;
    int M, nb;
};

// pair q = (sample j, entry i): the two rows, or false for an entry that is -1, out of range or its own sample
__device__ __forceinline__ bool pair_rows(const Pairs& pr, int64_t q, int64_t* rs, int64_t* rt) {
    const int64_t j = q / pr.nb;
    const int64_t s = pr.sample[j];
    const int64_t t = pr.table[q];
    *rs = s; *rt = t;
    return s >= 0 && s < pr.N && t >= 0 && t < pr.N && t != s;
}

// pstat [pairs][3]: lse of the sample's logits, lse of the neighbour's, the pair's KL.  part as above (the third sum unused).
template <int DP, bool kFull>
__global__ __launch_bounds__(256) void kl_fwd_kernel(Pairs pr, int D, int K, const float* __restrict__ W, const float* __restrict__ b,
                                                     float* __restrict__ pstat, double* __restrict__ part) {
    const int64_t Q = (int64_t)pr.M * pr.nb, q = (int64_t)blockIdx.x * kTile + threadIdx.x, qc = q < Q ? q : Q - 1;
    int64_t rs, rt;
    const bool valid = pair_rows(pr, qc, &rs, &rt) && q < Q;
    float ls = 0.f, lt = 0.f, kl = 0.f;
    if (__any(valid)) {
        float xs[DP], xt[DP];
        load_row<DP, kFull>(xs, pr.e + (valid ? rs : 0) * D, D);
        load_row<DP, kFull>(xt, pr.e + (valid ? rt : 0) * D, D);
        lse_walk<DP, kFull>(W, b, K, D, xs, -1, &ls, nullptr, nullptr, nullptr);
        lse_walk<DP, kFull>(W, b, K, D, xt, -1, &lt, nullptr, nullptr, nullptr);
#pragma unroll 2
        for (int k = 0; k < K; k++) {
            const float* wr = W + (size_t)k * D;
            const float ps = dot2<DP, kFull>(wr, b[k], xs, D) - ls, pt = dot2<DP, kFull>(wr, b[k], xt, D) - lt;
            kl = fmaf(expf(ps), ps - pt, kl);
        }
    }
    if (q < Q) {
        pstat[3 * q] = ls; pstat[3 * q + 1] = lt; pstat[3 * q + 2] = valid ? kl : 0.f;
    }
    double v[3] = {valid ? (double)kl : 0.0, valid ? 1.0 : 0.0, 0.0};
    block_sums<3, 4>(v, part + 3 * (int64_t)blockIdx.x);
}

// d loss / d logit of one side of a pair, class k: the sample's side p (log p - log q - KL), the neighbour's q - p
__device__ __forceinline__ float pair_dz(int side, float lps, float lpt, float kl, float ws) {
    const float p = expf(lps);
    return (side == 0 ? p * ((lps - lpt) - kl) : expf(lpt) - p) * ws;
}

// slot = 2 * pair + side.  rowgrad [slots][D]: the gradient a pair sends to the row of that side (zeros for an invalid pair).
template <int DP, bool kFull>
__global__ __launch_bounds__(256) void kl_bwd_rows_kernel(Pairs pr, int D, int K, const float* __restrict__ W, const float* __restrict__ b,
                                                          const float* __restrict__ pstat, const int32_t* __restrict__ counts,
                                                          const float* __restrict__ g_loss, float* __restrict__ rowgrad) {
    const int64_t S = 2 * (int64_t)pr.M * pr.nb, sl = (int64_t)blockIdx.x * kTile + threadIdx.x, sc = sl < S ? sl : S - 1;
    const int64_t q = sc >> 1;
    const int side = (int)(sc & 1);
    int64_t rs, rt;
    const bool valid = pair_rows(pr, q, &rs, &rt) && sl < S;
    const float ws = grad_scale(g_loss, counts);
    float de[DP];
#pragma unroll
    for (int d = 0; d < DP; d++) de[d] = 0.f;
    if (__any(valid)) {
        float xs[DP], xt[DP];
        load_row<DP, kFull>(xs, pr.e + (valid ? rs : 0) * D, D);
        load_row<DP, kFull>(xt, pr.e + (valid ? rt : 0) * D, D);
        const float ls = pstat[3 * q], lt = pstat[3 * q + 1], kl = pstat[3 * q + 2];
#pragma unroll 2
        for (int k = 0; k < K; k++) {
            const float* wr = W + (size_t)k * D;
            const float r = pair_dz(side, dot2<DP, kFull>(wr, b[k], xs, D) - ls, dot2<DP, kFull>(wr, b[k], xt, D) - lt, kl, ws);
#pragma unroll
            for (int d = 0; d < DP; d++)
                if (kFull || d < D) de[d] = fmaf(wr[d], r, de[d]);
        }
    }
    if (sl < S) {
        float* out = rowgrad + sl * D;
#pragma unroll
        for (int d = 0; d < DP; d++)
            if (kFull || d < D) out[d] = valid ? de[d] : 0.f;
    }
}

// v_identities [N, D], every element: the slots of a row (a CSR over rows, ascending slots within a row) in that order
__global__ __launch_bounds__(256) void kl_gather_kernel(int64_t N, int D, const int64_t* __restrict__ rev_offsets,
                                                        const int32_t* __restrict__ rev_slots, int64_t n_slots,
                                                        const float* __restrict__ rowgrad, float* __restrict__ v_identities) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N * D) return;
    const int64_t n = e / D;
    const int d = (int)(e - n * D);
    int64_t lo = rev_offsets[n], hi = rev_offsets[n + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_slots ? n_slots : hi;
    float a = 0.f;
    for (int64_t i = lo; i < hi; i++) {
        const int64_t sl = rev_slots[i];
        if (sl >= 0 && sl < n_slots) a += rowgrad[sl * D + d];
    }
    v_identities[e] = a;
}

// ---------------------------------------------------------------------------------------------------- d/dW, d/db
// Both losses.  grid (class units, row splits); a workgroup walks the tiles split, split + PS, ... of 256 rows.  Per tile,
// thread = row forms the unit's 16 d/dz into LDS (and adds them to its own bias sums), the row itself goes to LDS as well;
// then thread = (channel d, row group g) walks the rows g, g + G, ...: acc[u] += dz[row][u] * x[row][d].  At the end the row
// groups are summed in ascending order, the bias sums by block_sums.  dwpart [PS][K][D + 1] (the last column: the bias).
struct Rows2D {
    const float* features; const int32_t* target; const float* lse;
    int64_t P; int stride;
};
struct Rows3D {
    Pairs pr; const float* pstat;
};

template <int DP, bool kFull, class Src>
__global__ __launch_bounds__(256) void wgrad_kernel(Src src, int64_t rows, int D, int K, int PS, const float* __restrict__ W,
                                                    const float* __restrict__ b, const int32_t* __restrict__ counts,
                                                    const float* __restrict__ g_loss, float* __restrict__ dwpart) {
    constexpr int XS = DP + 4, G = kTile / DP;
    __shared__ __attribute__((aligned(16))) float sdz[kTile * kRS];
    __shared__ __attribute__((aligned(16))) float sx[kTile * XS];
    __shared__ double sb[kUnit];
    const int c0 = blockIdx.x * kUnit;
    const int d = threadIdx.x % DP, grp = threadIdx.x / DP;
    const float ws = grad_scale(g_loss, counts);
    const int64_t tiles = (rows + kTile - 1) / kTile;
    float acc[kUnit];
    double rb[kUnit];
#pragma unroll
    for (int u = 0; u < kUnit; u++) { acc[u] = 0.f; rb[u] = 0.0; }
    for (int64_t tile = blockIdx.y; tile < tiles; tile += PS) {
        const int64_t r = tile * kTile + threadIdx.x, rc = r < rows ? r : rows - 1;
        float x[DP], dz[kUnit];
#pragma unroll
        for (int u = 0; u < kUnit; u++) dz[u] = 0.f;
#pragma unroll
        for (int dd = 0; dd < DP; dd++) x[dd] = 0.f;
        if constexpr (std::is_same<Src, Rows2D>::value) {
            const int t = src.target[rc];
            const bool lab = r < rows && t >= 1 && t <= K;
            if (__any(lab)) {
                load_row<DP, kFull>(x, src.features + rc * src.stride, D);
                const float l = src.lse[rc];
#pragma unroll
                for (int u = 0; u < kUnit; u++) {
                    const int k = c0 + u;
                    if (k < K) {
                        const float z = dot2<DP, kFull>(W + (size_t)k * D, b[k], x, D);
                        dz[u] = lab ? (expf(z - l) - (k == t - 1 ? 1.f : 0.f)) * ws : 0.f;
                    }
                }
                if (!lab) {
#pragma unroll
                    for (int dd = 0; dd < DP; dd++) x[dd] = 0.f;
                }
            }
        } else {
            const int64_t q = rc >> 1;
            const int side = (int)(rc & 1);
            int64_t rs, rt;
            const bool valid = pair_rows(src.pr, q, &rs, &rt) && r < rows;
            if (__any(valid)) {
                float xo[DP];
                load_row<DP, kFull>(x, src.pr.e + (valid ? (side ? rt : rs) : 0) * D, D);
                load_row<DP, kFull>(xo, src.pr.e + (valid ? (side ? rs : rt) : 0) * D, D);
                const float ls = src.pstat[3 * q], lt = src.pstat[3 * q + 1], kl = src.pstat[3 * q + 2];
#pragma unroll
                for (int u = 0; u < kUnit; u++) {
                    const int k = c0 + u;
                    if (k < K) {
                        const float* wr = W + (size_t)k * D;
                        const float zo = dot2<DP, kFull>(wr, b[k], x, D), zx = dot2<DP, kFull>(wr, b[k], xo, D);
                        const float lps = (side ? zx : zo) - ls, lpt = (side ? zo : zx) - lt;
                        dz[u] = valid ? pair_dz(side, lps, lpt, kl, ws) : 0.f;
                    }
                }
                if (!valid) {
#pragma unroll
                    for (int dd = 0; dd < DP; dd++) x[dd] = 0.f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kUnit; u++) { sdz[threadIdx.x * kRS + u] = dz[u]; rb[u] += (double)dz[u]; }
#pragma unroll
        for (int dd = 0; dd < DP; dd++) sx[threadIdx.x * XS + dd] = x[dd];
        __syncthreads();
        for (int i = 0; i < DP; i++) {                                    // kTile / G == DP rows per group
            const int row = grp + i * G;
            const float xv = sx[row * XS + d];
#pragma unroll
            for (int u = 0; u < kUnit; u++) acc[u] = fmaf(sdz[row * kRS + u], xv, acc[u]);
        }
        __syncthreads();
    }
    // the row groups in ascending order: buf [G][kUnit][DP] in sdz's place (G * kUnit * DP = 4096 floats)
    float* buf = sdz;
#pragma unroll
    for (int u = 0; u < kUnit; u++) buf[(grp * kUnit + u) * DP + d] = acc[u];
    __syncthreads();
    float* out = dwpart + (size_t)blockIdx.y * K * (D + 1);
    for (int o = threadIdx.x; o < kUnit * DP; o += 256) {
        const int u = o / DP, dd = o - u * DP;
        float s = buf[o];
        for (int g = 1; g < G; g++) s += buf[g * kUnit * DP + o];
        if (c0 + u < K && dd < D) out[(size_t)(c0 + u) * (D + 1) + dd] = s;
    }
    block_sums<kUnit, 4>(rb, sb);
    __syncthreads();
    if (threadIdx.x < kUnit && c0 + (int)threadIdx.x < K) out[(size_t)(c0 + threadIdx.x) * (D + 1) + D] = (float)sb[threadIdx.x];
}

// v_weight / v_bias: the splits' partial sums in fp64, ascending
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(int K, int D, int PS, const float* __restrict__ dwpart,
                                                           float* __restrict__ v_weight, float* __restrict__ v_bias) {
    const int64_t n = (int64_t)K * (D + 1), e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
    for (int ps = 0; ps < PS; ps++) s += (double)dwpart[(int64_t)ps * n + e];
    const int64_t c = e / (D + 1);
    const int d = (int)(e - c * (D + 1));
    if (d < D) v_weight[c * D + d] = (float)s;
    else v_bias[c] = (float)s;
}

// ---------------------------------------------------------------------------------------------------- inference
template <int DP, bool kFull>
__global__ __launch_bounds__(256) void labels_kernel(int64_t P, int D, int K, int stride, const float* __restrict__ features,
                                                     const float* __restrict__ W, const float* __restrict__ b,
                                                     int32_t* __restrict__ labels, float* __restrict__ confidence) {
    const int64_t p = (int64_t)blockIdx.x * kTile + threadIdx.x, pc = p < P ? p : P - 1;
    float x[DP], lse, conf;
    int best;
    load_row<DP, kFull>(x, features + pc * stride, D);
    lse_walk<DP, kFull>(W, b, K, D, x, -1, &lse, nullptr, &best, &conf);
    if (p < P) {
        labels[p] = best + 1;
        if (confidence) confidence[p] = conf;
    }
}

// ---------------------------------------------------------------------------------------------------- host
// The scratch layout and the launch shape: a function of the sizes alone.
struct Plan {
    int64_t rows, tiles;                        // rows of the weight-gradient kernel (pixels, or 2 * pairs) and their tiles
    int64_t loss_tiles;                         // tiles of the loss kernel (pixels, or pairs)
    int units, PS;
    int64_t part, stat, rowgrad, dwpart, total; // offsets in floats; part holds doubles and comes first
};

bool make_plan(int64_t n, int D, int K, int mode, Plan* pl) {
    if (n < 1 || n > kMaxRows || D < 1 || D > kMaxD || K < 1 || K > kMaxK || (mode != 0 && mode != 1)) return false;
    *pl = Plan{};
    pl->rows = mode == 0 ? n : 2 * n;
    pl->tiles = (pl->rows + kTile - 1) / kTile;
    pl->loss_tiles = (n + kTile - 1) / kTile;
    pl->units = (K + kUnit - 1) / kUnit;
    // row splits: enough workgroups for the device when the classes are few, a bounded partial buffer when they are many
    int cap = 512 / pl->units;
    cap = cap < 8 ? 8 : (cap > 64 ? 64 : cap);
    pl->PS = (int)(pl->tiles < cap ? pl->tiles : cap);
    int64_t off = 0;
    auto take = [&off](int64_t count) { const int64_t o = off; off += (count + 3) & ~(int64_t)3; return o; };
    pl->part = take(6 * pl->loss_tiles);
    pl->stat = take(mode == 0 ? n : 3 * n);
    pl->rowgrad = take(mode == 0 ? 0 : pl->rows * D);
    pl->dwpart = take((int64_t)pl->PS * K * (D + 1));
    pl->total = off;
    return true;
}

#define IDENTITY_DISPATCH(D, CALL)                                  \
    do {                                                            \
        if ((D) == 16) { CALL(16, true); }                          \
        else if ((D) < 16) { CALL(16, false); }                     \
        else if ((D) == 32) { CALL(32, true); }                     \
        else { CALL(32, false); }                                   \
    } while (0)

template <class Src>
void launch_wgrad(const Plan& pl, Src src, int D, int K, const float* W, const float* b, const int32_t* counts, const float* g_loss,
                  float* scratch, float* v_weight, float* v_bias, hipStream_t s) {
    const dim3 grid(pl.units, pl.PS);
    float* dwpart = scratch + pl.dwpart;
#define CALL(DP, FULL) hipLaunchKernelGGL((wgrad_kernel<DP, FULL, Src>), grid, dim3(256), 0, s, src, pl.rows, D, K, pl.PS, W, b, counts, \
                                          g_loss, dwpart)
    IDENTITY_DISPATCH(D, CALL);
#undef CALL
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks((int64_t)K * (D + 1), 256)), dim3(256), 0, s, K, D, pl.PS,
                       (const float*)dwpart, v_weight, v_bias);
}

}  // namespace

extern "C" int64_t misplat_identity_scratch_floats(int64_t rows, int32_t dim, int32_t classes, int32_t mode) {
    Plan pl;
    if (!make_plan(rows, dim, classes, mode, &pl)) return -1;
    return pl.total;
}

extern "C" int misplat_identity_loss_fwd(int32_t height, int32_t width, int32_t dim, int32_t pix_stride, const float* features,
                                         int32_t classes, const float* weight, const float* bias, const int32_t* target,
                                         float* scratch, int32_t* counts, float* loss, misplat_stream_t stream) {
    Plan pl;
    if (height < 1 || width < 1 || !make_plan((int64_t)height * width, dim, classes, 0, &pl)) return MISPLAT_EINVAL;
    if (pix_stride < dim || !features || !weight || !bias || !target || !scratch || !counts || !loss) return MISPLAT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t P = pl.rows;
    double* part = (double*)(scratch + pl.part);
    float* lse = scratch + pl.stat;
#define CALL(DP, FULL) hipLaunchKernelGGL((ce_fwd_kernel<DP, FULL>), dim3((unsigned)pl.loss_tiles), dim3(256), 0, s, P, (int)dim, \
                                          (int)classes, (int)pix_stride, features, weight, bias, target, lse, part)
    IDENTITY_DISPATCH(dim, CALL);
#undef CALL
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part, pl.loss_tiles, loss, counts);
    return launched();
}

extern "C" int misplat_identity_loss_bwd(int32_t height, int32_t width, int32_t dim, int32_t pix_stride, const float* features,
                                         int32_t classes, const float* weight, const float* bias, const int32_t* target,
                                         float* scratch, const int32_t* counts, const float* g_loss, float* v_features,
                                         float* v_weight, float* v_bias, misplat_stream_t stream) {
    Plan pl;
    if (height < 1 || width < 1 || !make_plan((int64_t)height * width, dim, classes, 0, &pl)) return MISPLAT_EINVAL;
    if (pix_stride < dim || !features || !weight || !bias || !target || !scratch || !counts || !v_features || !v_weight || !v_bias)
        return MISPLAT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t P = pl.rows;
    const float* lse = scratch + pl.stat;
#define CALL(DP, FULL) hipLaunchKernelGGL((ce_bwd_dx_kernel<DP, FULL>), dim3((unsigned)pl.loss_tiles), dim3(256), 0, s, P, (int)dim, \
                                          (int)classes, (int)pix_stride, features, weight, bias, target, lse, counts, g_loss, v_features)
    IDENTITY_DISPATCH(dim, CALL);
#undef CALL
    launch_wgrad(pl, Rows2D{features, target, lse, P, (int)pix_stride}, dim, classes, weight, bias, counts, g_loss, scratch, v_weight,
                 v_bias, s);
    return launched();
}

extern "C" int misplat_identity_labels(int64_t rows, int32_t dim, int32_t pix_stride, const float* features, int32_t classes,
                                       const float* weight, const float* bias, int32_t* labels, float* confidence,
                                       misplat_stream_t stream) {
    if (rows < 1 || rows > kMaxRows || dim < 1 || dim > kMaxD || classes < 1 || classes > kMaxK || pix_stride < dim) return MISPLAT_EINVAL;
    if (!features || !weight || !bias || !labels) return MISPLAT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
#define CALL(DP, FULL) hipLaunchKernelGGL((labels_kernel<DP, FULL>), dim3(blocks(rows, kTile)), dim3(256), 0, s, rows, (int)dim, \
                                          (int)classes, (int)pix_stride, features, weight, bias, labels, confidence)
    IDENTITY_DISPATCH(dim, CALL);
#undef CALL
    return launched();
}

extern "C" int misplat_identity_3d_fwd(int64_t n_rows, int32_t dim, const float* identities, int32_t classes, const float* weight,
                                       const float* bias, int32_t n_samples, int32_t k, const int64_t* sample, const int32_t* table,
                                       float* scratch, int32_t* counts, float* loss, misplat_stream_t stream) {
    Plan pl;
    if (n_rows < 1 || n_samples < 1 || k < 1 || k > kMaxNb || !make_plan((int64_t)n_samples * k, dim, classes, 1, &pl)) return MISPLAT_EINVAL;
    if (!identities || !weight || !bias || !sample || !table || !scratch || !counts || !loss) return MISPLAT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const Pairs pr{identities, sample, table, n_rows, (int)n_samples, (int)k};
    double* part = (double*)(scratch + pl.part);
    float* pstat = scratch + pl.stat;
#define CALL(DP, FULL) hipLaunchKernelGGL((kl_fwd_kernel<DP, FULL>), dim3((unsigned)pl.loss_tiles), dim3(256), 0, s, pr, (int)dim, \
                                          (int)classes, weight, bias, pstat, part)
    IDENTITY_DISPATCH(dim, CALL);
#undef CALL
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part, pl.loss_tiles, loss, counts);
    return launched();
}

extern "C" int misplat_identity_3d_bwd(int64_t n_rows, int32_t dim, const float* identities, int32_t classes, const float* weight,
                                       const float* bias, int32_t n_samples, int32_t k, const int64_t* sample, const int32_t* table,
                                       const int64_t* rev_offsets, const int32_t* rev_slots, float* scratch, const int32_t* counts,
                                       const float* g_loss, float* v_identities, float* v_weight, float* v_bias,
                                       misplat_stream_t stream) {
    Plan pl;
    if (n_rows < 1 || n_samples < 1 || k < 1 || k > kMaxNb || !make_plan((int64_t)n_samples * k, dim, classes, 1, &pl)) return MISPLAT_EINVAL;
    if (!identities || !weight || !bias || !sample || !table || !rev_offsets || !rev_slots || !scratch || !counts || !v_identities ||
        !v_weight || !v_bias)
        return MISPLAT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const Pairs pr{identities, sample, table, n_rows, (int)n_samples, (int)k};
    const float* pstat = scratch + pl.stat;
    float* rowgrad = scratch + pl.rowgrad;
#define CALL(DP, FULL) hipLaunchKernelGGL((kl_bwd_rows_kernel<DP, FULL>), dim3((unsigned)pl.tiles), dim3(256), 0, s, pr, (int)dim, \
                                          (int)classes, weight, bias, pstat, counts, g_loss, rowgrad)
    IDENTITY_DISPATCH(dim, CALL);
#undef CALL
    hipLaunchKernelGGL(kl_gather_kernel, dim3(blocks(n_rows * dim, 256)), dim3(256), 0, s, n_rows, (int)dim, rev_offsets, rev_slots,
                       pl.rows, (const float*)rowgrad, v_identities);
    launch_wgrad(pl, Rows3D{pr, pstat}, dim, classes, weight, bias, counts, g_loss, scratch, v_weight, v_bias, s);
    return launched();
}
