// featloss.hip -- the features model's decoder and cosine feature loss (rade_features_model.py:149-189 `decode_features`,
// :545-584 `get_loss_dict`; utils/features.py:408-478 `TwoLayerMLP`) as a handful of launches each way:
//   x   = bilinear(features [H,W,L] -> (Hm, Wm))                     (align_corners=False, no antialiasing)
//   h   = relu(w_hidden x + b_hidden)                                 per pixel of the main map
//   p_b = w_out[b] h_b + b_out[b], h_b = h resampled to (H_b, W_b)    per branch (h_b = h where the dims are the main map's)
//   features_loss = lambda * sum_b weight_b * mean_q (1 - <p_b, gt_b> / (max(|p_b|, 1e-8) max(|gt_b|, 1e-8)))
// The reference resizes the PREDICTIONS of a branch that is not the main one; bilinear weights sum to 1, so that equals
// the branch's linear layer applied to the resized h -- every branch is then "sample h at the branch's resolution,
// contract, compare", and no [C_b, H', W'] tensor exists in training.
//
// The Hd x C_b contraction per pixel runs on the f32 VALU: lane = pixel, a wave owns 16 channels at a time, the weights of
// those channels are wave-uniform (scalar loads), the pixel's hidden vector sits in 64 registers.  gfx950's f32-input
// MFMA has the VALU's peak rate (64 FLOP/clk/SIMD), so it would buy no throughput here, and at 7 296 pixels x 64 x 1 152
// (1.1 GFLOP a contraction) the kernels are bound by how many waves the pixel count can fill, not by the FMA rate.
// Backward: the predictions are recomputed (never stored); d/dh is accumulated per pixel in registers and summed over the
// channel splits in a fixed order; the weight gradients are sums over pixels in a fixed order (lane = hidden unit, the
// 16 d/dp values of a pixel broadcast from LDS), partial sums per pixel range, final sums in fp64.  The transposes of the
// two bilinear resizes are GATHERS (every output element looks up the samples whose taps touch it), so v_features is
// written whole, overlapping taps need no atomics, and two runs are equal bit for bit.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "bilinear.h"
#include "misplat.h"
#include "rowlinear.h"
#include "wgprims.h"

namespace {

constexpr int kMaxBranch = 4;
constexpr int kMaxLatent = 32;
constexpr int kMaxHidden = 256;
constexpr int kUnit = 16;                       // channels a wave contracts at a time
constexpr int kJ = 64;                          // hidden units held in registers at a time
constexpr int kPixTile = 64;                    // pixels of a workgroup of the per-branch kernels (lane = pixel)
constexpr int kHidPix = 16;                     // main-map pixels of a workgroup of the hidden-layer kernels
constexpr float kEps = 1e-8f;                   // F.cosine_similarity's eps, applied to each norm

struct Branch {
    const float* w;                             // [C, Hd]
    const float* b;                             // [C]
    const float* gt;                            // [C, Hb, Wb] (loss) or NULL
    float* out;                                 // decode: [C, Hb, Wb] or [Hb * Wb, C]
    float* v_w;                                 // backward: [C, Hd]
    float* v_b;                                 // backward: [C]
    int C, Hb, Wb, identity;                    // identity: (Hb, Wb) is the main map, h_b = h
    int S;                                      // channel splits (grid.y) of the per-pixel kernels
    int PS;                                     // pixel splits of the weight-gradient kernel
    float coef;                                 // lambda * weight_b / (Hb * Wb)
    size_t hqT, hqP;                            // offsets into scratch: h_b as [Hd, P] and [P, Hd]
    size_t part, stats;                         // [S, 3, P] partial and [3, P] final (|p|^2, <p, g>, |g|^2)
    size_t lossblk;                             // [ceil(P / 256)] block sums of 1 - cos
    size_t dhpart;                              // [S, P, Hd]
    size_t dwpart;                              // [PS, C, Hd + 1] (the last column: the bias)
};

struct Plan {
    Branch br[kMaxBranch];
    int n, L, Hd, Hm, Wm;
    size_t x, hT, hP, dpreT, dx;                // [Pm, L], [Hd, Pm], [Pm, Hd], [Hd, Pm], [Pm, L]
    size_t total;
    int max_tiles, max_S, max_units, max_PS, max_blk;
};

// ---- x and h on the main map.  One workgroup = 16 pixels: x through LDS, then one (pixel, hidden unit) per thread.
__global__ __launch_bounds__(256) void hidden_fwd_kernel(Plan pl, int H, int W, int pix_stride, const float* __restrict__ features,
                                                         const float* __restrict__ wh, const float* __restrict__ bh,
                                                         float* __restrict__ scratch) {
    __shared__ float sx[kHidPix][kMaxLatent + 1];
    const int L = pl.L, Hd = pl.Hd, Pm = pl.Hm * pl.Wm;
    const int m0 = blockIdx.x * kHidPix;
    const double sy = (double)H / pl.Hm, sxs = (double)W / pl.Wm;
    for (int t = threadIdx.x; t < kHidPix * L; t += 256) {
        const int pix = t / L, l = t - pix * L, m = m0 + pix;
        float v = 0.f;
        if (m < Pm) {
            const Taps ty = taps(m / pl.Wm, H, sy), tx = taps(m % pl.Wm, W, sxs);
            const float* f = features + l;
            const float v00 = f[((size_t)ty.i0 * W + tx.i0) * pix_stride], v01 = f[((size_t)ty.i0 * W + tx.i1) * pix_stride];
            const float v10 = f[((size_t)ty.i1 * W + tx.i0) * pix_stride], v11 = f[((size_t)ty.i1 * W + tx.i1) * pix_stride];
            v = bilerp(ty, tx, v00, v01, v10, v11);
            scratch[pl.x + (size_t)m * L + l] = v;
        }
        sx[pix][l] = v;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kHidPix * Hd; t += 256) {
        const int pix = t / Hd, j = t - pix * Hd, m = m0 + pix;
        if (m >= Pm) continue;
        float a = bh[j];
        for (int l = 0; l < L; l++) a = fmaf(wh[j * L + l], sx[pix][l], a);
        a = a > 0.f ? a : 0.f;
        scratch[pl.hT + (size_t)j * Pm + m] = a;
        scratch[pl.hP + (size_t)m * Hd + j] = a;
    }
}

// ---- h resampled to a branch's own resolution (branches whose dims differ from the main map's), both layouts
__global__ __launch_bounds__(256) void resample_kernel(Plan pl, float* __restrict__ scratch) {
    const Branch& br = pl.br[blockIdx.y];
    if (br.identity) return;
    const int Hd = pl.Hd;
    const size_t P = (size_t)br.Hb * br.Wb, e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= P * Hd) return;
    const size_t q = e / Hd;
    const int j = (int)(e - q * Hd);
    const Taps ty = taps((int)(q / br.Wb), pl.Hm, (double)pl.Hm / br.Hb), tx = taps((int)(q % br.Wb), pl.Wm, (double)pl.Wm / br.Wb);
    const float* h = scratch + pl.hP + j;
    const float v00 = h[((size_t)ty.i0 * pl.Wm + tx.i0) * Hd], v01 = h[((size_t)ty.i0 * pl.Wm + tx.i1) * Hd];
    const float v10 = h[((size_t)ty.i1 * pl.Wm + tx.i0) * Hd], v11 = h[((size_t)ty.i1 * pl.Wm + tx.i1) * Hd];
    const float v = bilerp(ty, tx, v00, v01, v10, v11);
    scratch[br.hqP + e] = v;
    scratch[br.hqT + (size_t)j * P + q] = v;
}

// One channel's prediction at one pixel, p = bias + <row of w_out, h_b(q)>.  The row is wave-uniform: it comes through scalar
// loads.  kH64 (Hd == 64, the default): the pixel's hidden vector stays in 64 registers for all channels (two chains of
// multiply-adds, rowlinear.h's dot2); any other Hd: it is read per channel (hT [Hd, P]: one coalesced load per hidden unit).
template <bool kH64>
__device__ __forceinline__ void load_hidden(float (&hv)[kJ], const float* __restrict__ hT, size_t P, size_t q) {
#pragma unroll
    for (int jj = 0; jj < kJ; jj++) hv[jj] = kH64 ? hT[(size_t)jj * P + q] : 0.f;
}
template <bool kH64>
__device__ __forceinline__ float predict(const float* __restrict__ wr, float bias, const float (&hv)[kJ], const float* __restrict__ hT,
                                         size_t P, size_t q, int Hd) {
    if (kH64) return dot2<kJ, true>(wr, bias, hv, kJ);
    float a = bias;
    for (int j = 0; j < Hd; j++) a = fmaf(wr[j], hT[(size_t)j * P + q], a);
    return a;
}

__device__ __forceinline__ const float* branch_hT(const Plan& pl, const Branch& br, const float* scratch) {
    return scratch + (br.identity ? pl.hT : br.hqT);
}
__device__ __forceinline__ const float* branch_hP(const Plan& pl, const Branch& br, const float* scratch) {
    return scratch + (br.identity ? pl.hP : br.hqP);
}

// ---- forward of a branch: grid (pixel tiles, channel splits, branches); wave w of split s takes the 16-channel units
// s * 4 + w, + 4 S, ...; per pixel the three sums |p|^2, <p, g>, |g|^2 over the split's channels
template <bool kH64>
__global__ __launch_bounds__(256) void branch_fwd_kernel(Plan pl, float* __restrict__ scratch) {
    __shared__ float red[3][256];
    const Branch& br = pl.br[blockIdx.z];
    const size_t P = (size_t)br.Hb * br.Wb;
    if ((int)blockIdx.y >= br.S || (size_t)blockIdx.x * kPixTile >= P) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t q = (size_t)blockIdx.x * kPixTile + lane, qc = q < P ? q : P - 1;
    const float* hT = branch_hT(pl, br, scratch);
    const int units = (br.C + kUnit - 1) / kUnit;
    float pp = 0.f, pg = 0.f, gg = 0.f, hv[kJ];
    load_hidden<kH64>(hv, hT, P, qc);
    for (int u = blockIdx.y * 4 + wave; u < units; u += 4 * br.S) {
#pragma unroll 1
        for (int c = u * kUnit; c < min((u + 1) * kUnit, br.C); c++) {
            const float p = predict<kH64>(br.w + (size_t)c * pl.Hd, br.b[c], hv, hT, P, qc, pl.Hd);
            const float g = br.gt[(size_t)c * P + qc];
            pp = fmaf(p, p, pp); pg = fmaf(p, g, pg); gg = fmaf(g, g, gg);
        }
    }
    red[0][threadIdx.x] = pp; red[1][threadIdx.x] = pg; red[2][threadIdx.x] = gg;
    __syncthreads();
    if (threadIdx.x < 64 && q < P) {
        float* part = scratch + br.part + (size_t)blockIdx.y * 3 * P;
#pragma unroll
        for (int v = 0; v < 3; v++)
            part[(size_t)v * P + q] = (red[v][lane] + red[v][64 + lane]) + (red[v][128 + lane] + red[v][192 + lane]);
    }
}

// ---- per pixel: the three sums over the splits (fixed order), 1 - cos, and the sum of it over the block's 256 pixels
__global__ __launch_bounds__(256) void pixel_stats_kernel(Plan pl, float* __restrict__ scratch) {
    __shared__ float sm[256];
    const Branch& br = pl.br[blockIdx.y];
    const size_t P = (size_t)br.Hb * br.Wb;
    if ((size_t)blockIdx.x * 256 >= P) return;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    float term = 0.f;
    if (q < P) {
        float s[3] = {0.f, 0.f, 0.f};
        for (int sp = 0; sp < br.S; sp++)
#pragma unroll
            for (int v = 0; v < 3; v++) s[v] += scratch[br.part + ((size_t)sp * 3 + v) * P + q];
#pragma unroll
        for (int v = 0; v < 3; v++) scratch[br.stats + (size_t)v * P + q] = s[v];
        const float np = fmaxf(sqrtf(s[0]), kEps), ng = fmaxf(sqrtf(s[2]), kEps);
        term = 1.0f - s[1] / (np * ng);
    }
    sm[threadIdx.x] = term;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) scratch[br.lossblk + blockIdx.x] = sm[0];
}

// ---- the block sums in fp64, a fixed order: branch_sums[b] = sum_q (1 - cos), features_loss = sum_b coef_b * that
__global__ __launch_bounds__(1024) void loss_final_kernel(Plan pl, const float* __restrict__ scratch, float* __restrict__ branch_sums,
                                                          float* __restrict__ features_loss) {
    __shared__ double sm[1024];
    double total = 0.0;
    for (int b = 0; b < pl.n; b++) {
        const Branch& br = pl.br[b];
        const int nblk = (int)(((size_t)br.Hb * br.Wb + 255) / 256);
        double s = 0.0;
        for (int i = threadIdx.x; i < nblk; i += 1024) s += (double)scratch[br.lossblk + i];
        sm[threadIdx.x] = s;
        __syncthreads();
        for (int w = 512; w >= 1; w >>= 1) {
            if ((int)threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            if (branch_sums) branch_sums[b] = (float)sm[0];
            total += (double)br.coef * sm[0];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && features_loss) *features_loss = (float)total;
}

// d loss / d p[k] = B p[k] - A g[k] of one pixel: A = s / (np ng), B = s <p, g> / (np^3 ng) where |p| is not clamped
// (the clamped norm is a constant), s = g_loss * coef_b
__device__ __forceinline__ void pixel_coefs(const float* __restrict__ stats, size_t P, size_t q, bool ok, float s, float* A, float* B) {
    *A = 0.f; *B = 0.f;
    if (!ok) return;
    const float pp = stats[q], pg = stats[P + q], gg = stats[2 * P + q];
    const float rp = sqrtf(pp), np = fmaxf(rp, kEps), ng = fmaxf(sqrtf(gg), kEps);
    const float a = s / (np * ng);
    *A = a;
    *B = rp >= kEps ? a * pg / (np * np) : 0.f;
}

// ---- backward, d/dh of a branch: the same grid as the forward.  Per wave and 16-channel unit: p again, d/dp, and
// dh[j] += sum_k W[c_k, j] dp[k] in 64 registers; the four waves are summed through LDS in wave order and the split's
// result goes out as [P, Hd].  Hd > 64: one pass per 64 hidden units.
template <bool kH64>
__global__ __launch_bounds__(256) void branch_bwd_dh_kernel(Plan pl, const float* __restrict__ g_loss, float* __restrict__ scratch) {
    __shared__ float red[kJ][kPixTile + 1];
    const Branch& br = pl.br[blockIdx.z];
    const size_t P = (size_t)br.Hb * br.Wb;
    if ((int)blockIdx.y >= br.S || (size_t)blockIdx.x * kPixTile >= P) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t q0 = (size_t)blockIdx.x * kPixTile, q = q0 + lane, qc = q < P ? q : P - 1;
    const float* hT = branch_hT(pl, br, scratch);
    const int Hd = pl.Hd, units = (br.C + kUnit - 1) / kUnit;
    float A, B;
    pixel_coefs(scratch + br.stats, P, qc, q < P, (g_loss ? *g_loss : 0.f) * br.coef, &A, &B);
    float* out = scratch + br.dhpart + (size_t)blockIdx.y * P * Hd;
    float hv[kJ];
    load_hidden<kH64>(hv, hT, P, qc);
    for (int jb = 0; jb < Hd; jb += kJ) {
        float dh[kJ];
#pragma unroll
        for (int jj = 0; jj < kJ; jj++) dh[jj] = 0.f;
        for (int u = blockIdx.y * 4 + wave; u < units; u += 4 * br.S) {
#pragma unroll 1
            for (int c = u * kUnit; c < min((u + 1) * kUnit, br.C); c++) {
                const float* wr = br.w + (size_t)c * Hd;
                const float p = predict<kH64>(wr, br.b[c], hv, hT, P, qc, Hd);
                const float dp = B * p - A * br.gt[(size_t)c * P + qc];
#pragma unroll
                for (int jj = 0; jj < kJ; jj++)
                    if (kH64 || jb + jj < Hd) dh[jj] = fmaf(wr[jb + jj], dp, dh[jj]);
            }
        }
        for (int w = 0; w < 4; w++) {
            if (wave == w) {
#pragma unroll
                for (int jj = 0; jj < kJ; jj++) red[jj][lane] = w == 0 ? dh[jj] : red[jj][lane] + dh[jj];
            }
            __syncthreads();
        }
        for (int t = threadIdx.x; t < kJ * kPixTile; t += 256) {
            const int jj = t & (kJ - 1), qq = t >> 6;
            if (q0 + qq < P && jb + jj < Hd) out[(q0 + qq) * Hd + jb + jj] = red[jj][qq];
        }
        __syncthreads();
    }
}

// ---- backward, d/dw_out and d/db_out of a branch: grid (16-channel units, pixel splits, branches).  Per tile of 256
// pixels: thread = pixel forms the unit's 16 d/dp values into LDS; then lane = hidden unit, each wave walks its own 64
// pixels: dw[k][j] += dp[q][k] * h_b[q][j].  Partial sums per pixel split, [PS, C, Hd + 1] (the last column: the bias).
template <bool kH64>
__global__ __launch_bounds__(256) void branch_bwd_dw_kernel(Plan pl, const float* __restrict__ g_loss, float* __restrict__ scratch) {
    __shared__ float sdp[256][kUnit];
    const Branch& br = pl.br[blockIdx.z];
    const int units = (br.C + kUnit - 1) / kUnit;
    if ((int)blockIdx.x >= units || (int)blockIdx.y >= br.PS) return;
    const size_t P = (size_t)br.Hb * br.Wb;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int Hd = pl.Hd, c0 = blockIdx.x * kUnit, chunks = (Hd + kJ - 1) / kJ;
    const float* hT = branch_hT(pl, br, scratch);
    const float* hP = branch_hP(pl, br, scratch);
    const float s = (g_loss ? *g_loss : 0.f) * br.coef;
    const size_t tiles = (P + 255) / 256;
    float acc[kMaxHidden / kJ][kUnit], accb = 0.f;                   // accb: lanes 0..15 of a wave, one channel's bias each
#pragma unroll
    for (int k = 0; k < kUnit; k++)
#pragma unroll
        for (int ci = 0; ci < kMaxHidden / kJ; ci++) acc[ci][k] = 0.f;
    for (size_t tile = blockIdx.y; tile < tiles; tile += br.PS) {
        const size_t q = tile * 256 + threadIdx.x, qc = q < P ? q : P - 1;
        float A, B, hv[kJ];
        pixel_coefs(scratch + br.stats, P, qc, q < P, s, &A, &B);
        load_hidden<kH64>(hv, hT, P, qc);
#pragma unroll 1
        for (int k = 0; k < kUnit; k++) {
            const int c = c0 + k;
            float dp = 0.f;
            if (c < br.C) dp = B * predict<kH64>(br.w + (size_t)c * Hd, br.b[c], hv, hT, P, qc, Hd) - A * br.gt[(size_t)c * P + qc];
            sdp[threadIdx.x][k] = dp;
        }
        __syncthreads();
        for (int qq = 0; qq < 64; qq++) {
            const size_t q2 = tile * 256 + wave * 64 + qq, q2c = q2 < P ? q2 : P - 1;   // (past P: dp is 0)
            float d[kUnit];
#pragma unroll
            for (int k = 0; k < kUnit; k++) d[k] = sdp[wave * 64 + qq][k];
            if (lane < kUnit) accb += sdp[wave * 64 + qq][lane];
#pragma unroll
            for (int ci = 0; ci < kMaxHidden / kJ; ci++) {
                if (ci < chunks) {
                    const int j = ci * kJ + lane;
                    const float hq = j < Hd ? hP[q2c * Hd + j] : 0.f;
#pragma unroll
                    for (int k = 0; k < kUnit; k++) acc[ci][k] = fmaf(d[k], hq, acc[ci][k]);
                }
            }
        }
        __syncthreads();
    }
    // the four waves (and, for the bias, the 256 threads) in a fixed order through LDS
    float* out = scratch + br.dwpart + ((size_t)blockIdx.y * br.C) * (Hd + 1);
    float* buf = &sdp[0][0];                                          // 4096 floats
#pragma unroll
    for (int ci = 0; ci < kMaxHidden / kJ; ci++) {
        if (ci < chunks) {
#pragma unroll
            for (int k = 0; k < kUnit; k++) buf[(wave * kUnit + k) * 64 + lane] = acc[ci][k];
            __syncthreads();
            for (int o = threadIdx.x; o < kUnit * 64; o += 256) {
                const int k = o >> 6, ln = o & 63, j = ci * kJ + ln;
                const float v = (buf[(0 * kUnit + k) * 64 + ln] + buf[(1 * kUnit + k) * 64 + ln]) +
                                (buf[(2 * kUnit + k) * 64 + ln] + buf[(3 * kUnit + k) * 64 + ln]);
                if (c0 + k < br.C && j < Hd) out[(size_t)(c0 + k) * (Hd + 1) + j] = v;
            }
            __syncthreads();
        }
    }
    if (lane < kUnit) buf[wave * kUnit + lane] = accb;
    __syncthreads();
    if (threadIdx.x < kUnit && c0 + (int)threadIdx.x < br.C)
        out[(size_t)(c0 + threadIdx.x) * (Hd + 1) + Hd] = (buf[threadIdx.x] + buf[kUnit + threadIdx.x]) +
                                                          (buf[2 * kUnit + threadIdx.x] + buf[3 * kUnit + threadIdx.x]);
}

// ---- v_w_out / v_b_out: the pixel splits' partial sums in fp64, a fixed order
__global__ __launch_bounds__(256) void wout_reduce_kernel(Plan pl, const float* __restrict__ scratch) {
    const Branch& br = pl.br[blockIdx.y];
    const int Hd = pl.Hd;
    const size_t n = (size_t)br.C * (Hd + 1), e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
    for (int ps = 0; ps < br.PS; ps++) s += (double)scratch[br.dwpart + (size_t)ps * n + e];
    const size_t c = e / (Hd + 1);
    const int j = (int)(e - c * (Hd + 1));
    if (j < Hd) br.v_w[c * Hd + j] = (float)s;
    else br.v_b[c] = (float)s;
}

// ---- d/dh on the main map = the branches' d/dh_b (summed over their splits) through the transpose of their resampling
// (a gather: the branch pixels whose taps touch this one), the relu's mask, and d/dx = w_hidden^T d/dpre
__global__ __launch_bounds__(256) void hidden_bwd_kernel(Plan pl, const float* __restrict__ wh, float* __restrict__ scratch) {
    __shared__ float sd[kHidPix][kMaxHidden + 1];
    const int L = pl.L, Hd = pl.Hd, Pm = pl.Hm * pl.Wm;
    const int m0 = blockIdx.x * kHidPix;
    for (int t = threadIdx.x; t < kHidPix * Hd; t += 256) {
        const int pix = t / Hd, j = t - pix * Hd, m = m0 + pix;
        float dh = 0.f;
        if (m < Pm) {
            const int my = m / pl.Wm, mx = m - my * pl.Wm;
            for (int b = 0; b < pl.n; b++) {
                const Branch& br = pl.br[b];
                const size_t P = (size_t)br.Hb * br.Wb;
                const float* part = scratch + br.dhpart + j;
                if (br.identity) {
                    float a = 0.f;
                    for (int sp = 0; sp < br.S; sp++) a += part[((size_t)sp * P + m) * Hd];
                    dh += a;
                    continue;
                }
                const double sy = (double)pl.Hm / br.Hb, sx = (double)pl.Wm / br.Wb;
                int rlo, rhi, clo, chi;
                touching(my, br.Hb, (double)br.Hb / pl.Hm, &rlo, &rhi);
                touching(mx, br.Wb, (double)br.Wb / pl.Wm, &clo, &chi);
                float a = 0.f;
                for (int r = rlo; r <= rhi; r++) {
                    const float wy = tap_weight(taps(r, pl.Hm, sy), my);
                    if (wy == 0.f) continue;
                    for (int c = clo; c <= chi; c++) {
                        const float wx = tap_weight(taps(c, pl.Wm, sx), mx);
                        if (wx == 0.f) continue;
                        const size_t q = (size_t)r * br.Wb + c;
                        float v = 0.f;
                        for (int sp = 0; sp < br.S; sp++) v += part[((size_t)sp * P + q) * Hd];
                        a = fmaf(wy * wx, v, a);
                    }
                }
                dh += a;
            }
            if (!(scratch[pl.hP + (size_t)m * Hd + j] > 0.f)) dh = 0.f;
            scratch[pl.dpreT + (size_t)j * Pm + m] = dh;
        }
        sd[pix][j] = dh;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kHidPix * L; t += 256) {
        const int pix = t / L, l = t - pix * L, m = m0 + pix;
        if (m >= Pm) continue;
        float a = 0.f;
        for (int j = 0; j < Hd; j++) a = fmaf(wh[j * L + l], sd[pix][j], a);
        scratch[pl.dx + (size_t)m * L + l] = a;
    }
}

// ---- v_w_hidden[j, :] = sum_m dpre[j, m] x[m, :], v_b_hidden[j] = sum_m dpre[j, m]: one workgroup per hidden unit,
// fp64, thread-strided pixels then a tree: a fixed order
__global__ __launch_bounds__(256) void hidden_wgrad_kernel(Plan pl, const float* __restrict__ scratch, float* __restrict__ v_wh,
                                                           float* __restrict__ v_bh) {
    __shared__ double sm[256];
    const int L = pl.L, Pm = pl.Hm * pl.Wm, j = blockIdx.x;
    double acc[kMaxLatent + 1];
#pragma unroll
    for (int l = 0; l <= kMaxLatent; l++) acc[l] = 0.0;
    for (int m = threadIdx.x; m < Pm; m += 256) {
        const double d = (double)scratch[pl.dpreT + (size_t)j * Pm + m];
        const float* x = scratch + pl.x + (size_t)m * L;
#pragma unroll
        for (int l = 0; l < kMaxLatent; l++)
            if (l < L) acc[l] += d * (double)x[l];
        acc[kMaxLatent] += d;
    }
#pragma unroll
    for (int l = 0; l <= kMaxLatent; l++) {
        if (l < L || l == kMaxLatent) {
            sm[threadIdx.x] = acc[l];
            __syncthreads();
            for (int w = 128; w >= 1; w >>= 1) {
                if ((int)threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                if (l < kMaxLatent) v_wh[j * L + l] = (float)sm[0];
                else v_bh[j] = (float)sm[0];
            }
            __syncthreads();
        }
    }
}

// ---- v_features [H, W, L], every element: the main-map pixels whose taps touch this render pixel (a gather; most rows of
// a downsample are touched by none and come out as exact zeros).  grid.y walks the rows (the row test is uniform in a
// workgroup), a thread owns one (column, channel) of the row; sy / sx and their inverses come from the host.
__global__ __launch_bounds__(256) void features_bwd_kernel(Plan pl, int H, int W, double sy, double sx, double inv_sy, double inv_sx,
                                                           const float* __restrict__ scratch, float* __restrict__ v_features) {
    const int L = pl.L, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= W * L) return;
    const int x = idx / L, l = idx - x * L;
    int clo, chi;
    touching(x, pl.Wm, inv_sx, &clo, &chi);
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        int rlo, rhi;
        touching(y, pl.Hm, inv_sy, &rlo, &rhi);
        float a = 0.f;
        for (int r = rlo; r <= rhi; r++) {
            const float wy = tap_weight(taps(r, H, sy), y);
            if (wy == 0.f) continue;
            for (int c = clo; c <= chi; c++) {
                const float wx = tap_weight(taps(c, W, sx), x);
                if (wx == 0.f) continue;
                a = fmaf(wy * wx, scratch[pl.dx + ((size_t)r * pl.Wm + c) * L + l], a);
            }
        }
        v_features[(size_t)y * W * L + idx] = a;
    }
}

// ---- inference: the predictions themselves, [C, P] or (channels_last) [P, C]
template <bool kH64>
__global__ __launch_bounds__(256) void branch_decode_kernel(Plan pl, int channels_last, const float* __restrict__ scratch) {
    const Branch& br = pl.br[blockIdx.z];
    const size_t P = (size_t)br.Hb * br.Wb;
    if ((int)blockIdx.y >= br.S || (size_t)blockIdx.x * kPixTile >= P) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t q = (size_t)blockIdx.x * kPixTile + lane, qc = q < P ? q : P - 1;
    const float* hT = branch_hT(pl, br, scratch);
    const int units = (br.C + kUnit - 1) / kUnit;
    float hv[kJ];
    load_hidden<kH64>(hv, hT, P, qc);
    for (int u = blockIdx.y * 4 + wave; u < units; u += 4 * br.S) {
#pragma unroll 1
        for (int c = u * kUnit; c < min((u + 1) * kUnit, br.C); c++) {
            const float p = predict<kH64>(br.w + (size_t)c * pl.Hd, br.b[c], hv, hT, P, qc, pl.Hd);
            if (q < P) br.out[channels_last ? q * br.C + c : (size_t)c * P + q] = p;
        }
    }
}

// The scratch layout and the launch shapes: a function of the sizes alone.  decode_only: the buffers of x, h and the
// resampled h only.  Returns false for sizes outside the documented limits.
bool make_plan(int L, int Hd, int Hm, int Wm, int n, const int32_t* dims, bool decode_only, Plan* pl) {
    if (L < 1 || L > kMaxLatent || Hd < 1 || Hd > kMaxHidden || Hm < 1 || Wm < 1 || n < 1 || n > kMaxBranch || !dims) return false;
    if ((int64_t)Hm * Wm > (1 << 28)) return false;
    *pl = Plan{};
    pl->n = n; pl->L = L; pl->Hd = Hd; pl->Hm = Hm; pl->Wm = Wm;
    const size_t Pm = (size_t)Hm * Wm;
    size_t off = 0;
    auto take = [&off](size_t count) { const size_t o = off; off += (count + 3) & ~(size_t)3; return o; };
    pl->x = take(Pm * L); pl->hT = take(Pm * Hd); pl->hP = take(Pm * Hd);
    if (!decode_only) { pl->dpreT = take(Pm * Hd); pl->dx = take(Pm * L); }
    for (int b = 0; b < n; b++) {
        Branch& br = pl->br[b];
        br.C = dims[3 * b]; br.Hb = dims[3 * b + 1]; br.Wb = dims[3 * b + 2];
        if (br.C < 1 || br.C > (1 << 20) || br.Hb < 1 || br.Wb < 1 || (int64_t)br.Hb * br.Wb > (1 << 28)) return false;
        br.identity = br.Hb == Hm && br.Wb == Wm;
        const size_t P = (size_t)br.Hb * br.Wb;
        const int units = (br.C + kUnit - 1) / kUnit;
        br.S = units / 8 < 1 ? 1 : (units / 8 > 8 ? 8 : units / 8);
        const size_t tiles256 = (P + 255) / 256;
        br.PS = tiles256 / 4 < 1 ? 1 : (tiles256 / 4 > 16 ? 16 : (int)(tiles256 / 4));
        if (!br.identity) { br.hqT = take(P * Hd); br.hqP = take(P * Hd); }
        if (!decode_only) {
            br.part = take((size_t)br.S * 3 * P); br.stats = take(3 * P); br.lossblk = take(tiles256);
            br.dhpart = take((size_t)br.S * P * Hd); br.dwpart = take((size_t)br.PS * br.C * (Hd + 1));
        }
        const int tiles = (int)((P + kPixTile - 1) / kPixTile);
        pl->max_tiles = tiles > pl->max_tiles ? tiles : pl->max_tiles;
        pl->max_S = br.S > pl->max_S ? br.S : pl->max_S;
        pl->max_units = units > pl->max_units ? units : pl->max_units;
        pl->max_PS = br.PS > pl->max_PS ? br.PS : pl->max_PS;
        pl->max_blk = (int)tiles256 > pl->max_blk ? (int)tiles256 : pl->max_blk;
    }
    pl->total = off;
    return true;
}

bool any_resampled(const Plan& pl) {
    for (int b = 0; b < pl.n; b++)
        if (!pl.br[b].identity) return true;
    return false;
}

void launch_hidden(const Plan& pl, int H, int W, int pix_stride, const float* features, const float* wh, const float* bh,
                   float* scratch, hipStream_t s) {
    const size_t Pm = (size_t)pl.Hm * pl.Wm;
    hipLaunchKernelGGL(hidden_fwd_kernel, dim3((unsigned)((Pm + kHidPix - 1) / kHidPix)), dim3(256), 0, s, pl, H, W, pix_stride,
                       features, wh, bh, scratch);
    if (any_resampled(pl)) {
        size_t most = 0;
        for (int b = 0; b < pl.n; b++)
            if (!pl.br[b].identity) most = std::max(most, (size_t)pl.br[b].Hb * pl.br[b].Wb * pl.Hd);
        hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((most + 255) / 256), pl.n), dim3(256), 0, s, pl, scratch);
    }
}

bool image_ok(int32_t H, int32_t W, int32_t L, int32_t pix_stride) {
    return H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 28) && pix_stride >= L;
}

}  // namespace

extern "C" int64_t misplat_featloss_scratch_floats(int32_t latent, int32_t hidden, int32_t main_h, int32_t main_w,
                                                   int32_t n_branches, const int32_t* dims, int32_t decode_only) {
    Plan pl;
    if (!make_plan(latent, hidden, main_h, main_w, n_branches, dims, decode_only != 0, &pl)) return -1;
    return (int64_t)pl.total;
}

extern "C" int misplat_featloss_fwd(int32_t height, int32_t width, int32_t latent, int32_t pix_stride, const float* features,
                                    int32_t hidden, const float* w_hidden, const float* b_hidden, int32_t main_h, int32_t main_w,
                                    int32_t n_branches, const int32_t* dims, const float* const* w_out,
                                    const float* const* b_out, const float* const* gt, const float* weights,
                                    float loss_lambda, float* scratch, float* branch_sums, float* features_loss,
                                    misplat_stream_t stream) {
    Plan pl;
    if (!make_plan(latent, hidden, main_h, main_w, n_branches, dims, false, &pl)) return MISPLAT_EINVAL;
    if (!image_ok(height, width, latent, pix_stride) || !features || !w_hidden || !b_hidden || !w_out || !b_out || !gt || !weights ||
        !scratch)
        return MISPLAT_EINVAL;
    for (int b = 0; b < pl.n; b++) {
        if (!w_out[b] || !b_out[b] || !gt[b]) return MISPLAT_EINVAL;
        pl.br[b].w = w_out[b]; pl.br[b].b = b_out[b]; pl.br[b].gt = gt[b];
        pl.br[b].coef = (float)((double)loss_lambda * (double)weights[b] / ((double)pl.br[b].Hb * (double)pl.br[b].Wb));
    }
    hipStream_t s = (hipStream_t)stream;
    launch_hidden(pl, height, width, pix_stride, features, w_hidden, b_hidden, scratch, s);
    const dim3 grid(pl.max_tiles, pl.max_S, pl.n);
    if (hidden == kJ) hipLaunchKernelGGL(branch_fwd_kernel<true>, grid, dim3(256), 0, s, pl, scratch);
    else hipLaunchKernelGGL(branch_fwd_kernel<false>, grid, dim3(256), 0, s, pl, scratch);
    hipLaunchKernelGGL(pixel_stats_kernel, dim3(pl.max_blk, pl.n), dim3(256), 0, s, pl, scratch);
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(1024), 0, s, pl, scratch, branch_sums, features_loss);
    return launched();
}

extern "C" int misplat_featloss_bwd(int32_t height, int32_t width, int32_t latent, int32_t hidden, const float* w_hidden,
                                    int32_t main_h, int32_t main_w, int32_t n_branches, const int32_t* dims,
                                    const float* const* w_out, const float* const* b_out, const float* const* gt,
                                    const float* weights, float loss_lambda, float* scratch, const float* g_loss,
                                    float* v_features, float* v_w_hidden, float* v_b_hidden, float* const* v_w_out,
                                    float* const* v_b_out, misplat_stream_t stream) {
    Plan pl;
    if (!make_plan(latent, hidden, main_h, main_w, n_branches, dims, false, &pl)) return MISPLAT_EINVAL;
    if (!image_ok(height, width, latent, latent) || (int64_t)width * latent > INT32_MAX || !w_hidden || !w_out || !b_out || !gt || !weights || !scratch || !v_features ||
        !v_w_hidden || !v_b_hidden || !v_w_out || !v_b_out)
        return MISPLAT_EINVAL;
    for (int b = 0; b < pl.n; b++) {
        if (!w_out[b] || !b_out[b] || !gt[b] || !v_w_out[b] || !v_b_out[b]) return MISPLAT_EINVAL;
        pl.br[b].w = w_out[b]; pl.br[b].b = b_out[b]; pl.br[b].gt = gt[b];
        pl.br[b].v_w = v_w_out[b]; pl.br[b].v_b = v_b_out[b];
        pl.br[b].coef = (float)((double)loss_lambda * (double)weights[b] / ((double)pl.br[b].Hb * (double)pl.br[b].Wb));
    }
    hipStream_t s = (hipStream_t)stream;
    const bool full = hidden == kJ;
    const dim3 grid(pl.max_tiles, pl.max_S, pl.n), grid_w(pl.max_units, pl.max_PS, pl.n);
    if (full) hipLaunchKernelGGL(branch_bwd_dh_kernel<true>, grid, dim3(256), 0, s, pl, g_loss, scratch);
    else hipLaunchKernelGGL(branch_bwd_dh_kernel<false>, grid, dim3(256), 0, s, pl, g_loss, scratch);
    if (full) hipLaunchKernelGGL(branch_bwd_dw_kernel<true>, grid_w, dim3(256), 0, s, pl, g_loss, scratch);
    else hipLaunchKernelGGL(branch_bwd_dw_kernel<false>, grid_w, dim3(256), 0, s, pl, g_loss, scratch);
    size_t most = 0;
    for (int b = 0; b < pl.n; b++) most = std::max(most, (size_t)pl.br[b].C * (hidden + 1));
    hipLaunchKernelGGL(wout_reduce_kernel, dim3((unsigned)((most + 255) / 256), pl.n), dim3(256), 0, s, pl, scratch);
    const size_t Pm = (size_t)main_h * main_w;
    hipLaunchKernelGGL(hidden_bwd_kernel, dim3((unsigned)((Pm + kHidPix - 1) / kHidPix)), dim3(256), 0, s, pl, w_hidden, scratch);
    hipLaunchKernelGGL(hidden_wgrad_kernel, dim3(hidden), dim3(256), 0, s, pl, scratch, v_w_hidden, v_b_hidden);
    const dim3 grid_f((unsigned)(((int64_t)width * latent + 255) / 256), (unsigned)std::min<int32_t>(height, 65535));
    hipLaunchKernelGGL(features_bwd_kernel, grid_f, dim3(256), 0, s, pl, (int)height, (int)width, (double)height / main_h,
                       (double)width / main_w, (double)main_h / height, (double)main_w / width, scratch, v_features);
    return launched();
}

extern "C" int misplat_feature_decode(int32_t height, int32_t width, int32_t latent, int32_t pix_stride, const float* features,
                                      int32_t hidden, const float* w_hidden, const float* b_hidden, int32_t main_h, int32_t main_w,
                                      int32_t n_branches, const int32_t* dims, const float* const* w_out,
                                      const float* const* b_out, float* const* out, int32_t channels_last, float* scratch,
                                      misplat_stream_t stream) {
    Plan pl;
    if (!make_plan(latent, hidden, main_h, main_w, n_branches, dims, true, &pl)) return MISPLAT_EINVAL;
    if (!image_ok(height, width, latent, pix_stride) || !features || !w_hidden || !b_hidden || !w_out || !b_out || !out || !scratch)
        return MISPLAT_EINVAL;
    for (int b = 0; b < pl.n; b++) {
        if (!w_out[b] || !b_out[b] || !out[b]) return MISPLAT_EINVAL;
        pl.br[b].w = w_out[b]; pl.br[b].b = b_out[b]; pl.br[b].out = out[b];
    }
    hipStream_t s = (hipStream_t)stream;
    launch_hidden(pl, height, width, pix_stride, features, w_hidden, b_hidden, scratch, s);
    const dim3 grid(pl.max_tiles, pl.max_S, pl.n);
    if (hidden == kJ) hipLaunchKernelGGL(branch_decode_kernel<true>, grid, dim3(256), 0, s, pl, channels_last, scratch);
    else hipLaunchKernelGGL(branch_decode_kernel<false>, grid, dim3(256), 0, s, pl, channels_last, scratch);
    return launched();
}
