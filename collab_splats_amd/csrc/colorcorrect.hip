// colorcorrect.hip -- colour-corrected evaluation: before a render of a model trained with per-camera
// bilateral grids is scored, it is warped onto its ground truth's colours by a small least-squares fit, so that PSNR / SSIM
// measure the reconstruction and not the colour offset.  The fit is multinerf's `color_correct` as nerfstudio carries it for
// Splatfacto's `color_corrected_metrics`; neither is on this machine or in the reference tree, the operation is restated
// from the published method and parity with that code is unpinned [UNVERIFIED-UPSTREAM].
//
// Per view, P = H W pixels, num_iters times:   a(x) = (r^2, rg, rb, g^2, gb, b^2, r, g, b, 1) of the current image x, in
// fp64 from the fp32 values;   for each output channel c the mask m_c = unclipped(pred_c) & unclipped(x_c) & unclipped(gt_c),
// unclipped(z) = eps <= z <= 1 - eps in fp32;   G_c = sum m_c a a^T,  r_c = sum m_c a gt_c;   w_c = G_c^+ r_c with the
// eigenvalues <= 2^-46 lambda_max dropped;   x'_c = clip(a . w_c, 0, 1) for every pixel, rounded once to fp32.
//
// Three launches per iteration on the caller's stream, no atomics, no host read:
//   accumulate  one pass over the pixels.  A thread keeps the 64 fp64 sums of ONE channel (the 54 products a_i a_j, i <= j,
//               without a_9 a_9 = 1, whose sum is the mask count, and the 10 products a_i gt_c) in registers: the three
//               channels go to three workgroups (grid.y), 65 accumulators fit a thread where 195 do not, and the inner
//               loop is 64 fp64 multiply-adds per pixel and channel with no LDS traffic.  A wave then folds its 64 x 64
//               values in 63 exchanges (half of the values change lanes per step; lane l ends with sum l), the four waves
//               are added in ascending order and the workgroup leaves 64 sums and its count.
//   solve       one workgroup per (view, channel): the workgroups' partials are added in an order that depends on H and W
//               only, then cyclic Jacobi on the 10 x 10 matrix in fp64 in round-robin order (9 rounds of 5 disjoint
//               rotations per sweep, thread (i, j) owns an element), until max |off-diagonal| <= 2^-80 max |diagonal| or
//               16 sweeps; the cut; w_c as [10, 3] per view.
//   apply       x' for every pixel; the last iteration's writes the output image.
// Contraction is OFF for this file (build.py): the apply's sum is ((a0 w0 + a1 w1) + a2 w2) + ... with every product and
// sum rounded on its own, which a numpy fp64 restatement reproduces bit for bit; where a multiply-add is meant it is an
// explicit fma.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "misplat.h"
#include "wgprims.h"

namespace {

constexpr int kMono = 10;                           // monomials = unknowns per channel
constexpr int kItems = 64;                          // fp64 sums per channel and workgroup
constexpr int kPart = kItems + 1;                   // ... and the mask count, as a double (an integer below 2^31: exact)
constexpr int kPairs = 54;                          // items 0..53: (i, j), i <= j, row-major, without (9, 9); 54 + i: a_i gt_c
constexpr int kAccumBlocks = 256;                   // workgroups per view and channel at most
constexpr int kSegs = 15;                           // the solve adds the partials in 15 segments of consecutive workgroups
constexpr int kSolveThreads = 1024;
constexpr int kMaxSweeps = 16;

inline int accum_blocks(int64_t hw) { return (int)((hw + 255) / 256 < kAccumBlocks ? (hw + 255) / 256 : kAccumBlocks); }

// the item of the pair (p, q), p <= q: row-major over the upper triangle; (9, 9) is kPairs, which is no item
__host__ __device__ constexpr int pair_item(int p, int q) { return kMono * p - p * (p - 1) / 2 + (q - p); }

__device__ __forceinline__ bool unclipped(float z, float lo, float hi) { return lo <= z && z <= hi; }

__device__ __forceinline__ void monomials(float rf, float gf, float bf, double (&a)[kMono]) {
    const double r = (double)rf, g = (double)gf, b = (double)bf;
    a[0] = r * r; a[1] = r * g; a[2] = r * b; a[3] = g * g; a[4] = g * b; a[5] = b * b;
    a[6] = r; a[7] = g; a[8] = b; a[9] = 1.0;
}

// one step of the wave's fold: N values per lane become N / 2, each the sum over a pair of lanes (l, l ^ N/2); the lane
// with that bit set keeps the upper half
template <int N>
__device__ __forceinline__ void fold(double (&a)[kItems], int lane) {
    constexpr int h = N / 2;
    const bool up = (lane & h) != 0;
#pragma unroll
    for (int k = 0; k < h; k++) {
        const double send = up ? a[k] : a[k + h];
        const double keep = up ? a[k + h] : a[k];
        a[k] = keep + __shfl_xor(send, h);
    }
}

// grid (nb, 3, B).  Workgroup (blk, c, view) takes the pixels (round nb + blk) 256 + thread of its view, round = 0, 1, ...
// partials: [view][c][blk][kPart].
__global__ __launch_bounds__(256) void cc_accumulate_kernel(int64_t hw, const float* __restrict__ x, const float* __restrict__ pred,
                                                            const float* __restrict__ gt, float lo, float hi,
                                                            double* __restrict__ partials) {
    __shared__ double ws[4][kItems];
    __shared__ int wc[4];
    const int c = blockIdx.y;
    const size_t view = 3 * (size_t)blockIdx.z * (size_t)hw;
    x += view;
    pred += view;
    gt += view;
    double acc[kItems];
#pragma unroll
    for (int k = 0; k < kItems; k++) acc[k] = 0.0;
    int count = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
        const float xr = x[3 * i], xg = x[3 * i + 1], xb = x[3 * i + 2];
        const float xc = c == 0 ? xr : (c == 1 ? xg : xb), pc = pred[3 * i + c], gc = gt[3 * i + c];
        if (unclipped(pc, lo, hi) && unclipped(xc, lo, hi) && unclipped(gc, lo, hi)) {
            double a[kMono];
            monomials(xr, xg, xb, a);
            const double g = (double)gc;
#pragma unroll
            for (int p = 0; p < kMono; p++)
#pragma unroll
                for (int q = p; q < kMono; q++)
                    if (pair_item(p, q) < kPairs) acc[pair_item(p, q)] = fma(a[p], a[q], acc[pair_item(p, q)]);
#pragma unroll
            for (int p = 0; p < kMono; p++) acc[kPairs + p] = fma(a[p], g, acc[kPairs + p]);
            count++;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    fold<64>(acc, lane); fold<32>(acc, lane); fold<16>(acc, lane); fold<8>(acc, lane); fold<4>(acc, lane); fold<2>(acc, lane);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off);
    ws[wave][lane] = acc[0];
    if (lane == 0) wc[wave] = count;
    __syncthreads();
    double* out = partials + (((size_t)blockIdx.z * 3 + c) * gridDim.x + blockIdx.x) * kPart;
    if (threadIdx.x < kItems) out[threadIdx.x] = ((ws[0][threadIdx.x] + ws[1][threadIdx.x]) + ws[2][threadIdx.x]) + ws[3][threadIdx.x];
    if (threadIdx.x == kItems) out[kItems] = (double)((wc[0] + wc[1]) + (wc[2] + wc[3]));
}

// the partner of index i in round r of the round-robin order over 10 indices (9 stays, the others turn)
__device__ __forceinline__ int partner(int i, int r) {
    if (i == 9) return r;
    if (i == r) return 9;
    return (2 * r - i + 9) % 9;
}

// grid (3 B).  warps, counts: this iteration's [10, 3] and [3] of view 0; a view's lie warp_stride / count_stride apart.
__global__ __launch_bounds__(kSolveThreads) void cc_solve_kernel(const double* __restrict__ partials, int nb, double* __restrict__ warps,
                                                                 int64_t warp_stride, int64_t* __restrict__ counts,
                                                                 int64_t count_stride) {
    __shared__ double seg[kSegs][kPart];
    __shared__ double tot[kPart];
    __shared__ double A[2][kMono][kMono], V[2][kMono][kMono];
    __shared__ double cs[kMono][2];
    __shared__ double proj[kMono];
    __shared__ int done;
    const int t = threadIdx.x, view = blockIdx.x / 3, c = blockIdx.x % 3;
    // ---- the view's sums: segment s adds workgroups s per .. (s + 1) per - 1 in ascending order, then the segments
    if (t < kSegs * kPart) {
        const int s = t / kPart, k = t - s * kPart, per = (nb + kSegs - 1) / kSegs;
        const int b0 = s * per, b1 = b0 + per < nb ? b0 + per : nb;
        const double* p = partials + (size_t)blockIdx.x * nb * kPart + k;
        double v = 0.0;
#pragma unroll 8
        for (int b = b0; b < b1; b++) v += p[(size_t)b * kPart];
        seg[s][k] = v;
    }
    __syncthreads();
    if (t < kPart) {
        double v = seg[0][t];
#pragma unroll
        for (int s = 1; s < kSegs; s++) v += seg[s][t];
        tot[t] = v;
    }
    __syncthreads();
    const int i = t / kMono, j = t - i * kMono;                          // t < 100: element (i, j) of A; 100 <= t < 200: of V
    if (t < 2 * kMono * kMono) {
        if (i < kMono) {
            const int p = i < j ? i : j, q = i < j ? j : i, k = pair_item(p, q);
            A[0][i][j] = k == kPairs ? tot[kItems] : tot[k];            // a_9 a_9 = 1: the count
        } else {
            V[0][i - kMono][j] = i - kMono == j ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    // ---- cyclic Jacobi, round-robin order: A <- J^T A J, V <- V J, J = five disjoint rotations per round
    int cur = 0;
    for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
        if (t == 0) {
            double off = 0.0, dg = 0.0;
            for (int p = 0; p < kMono; p++) {
                dg = fmax(dg, fabs(A[cur][p][p]));
                for (int q = p + 1; q < kMono; q++) off = fmax(off, fabs(A[cur][p][q]));
            }
            done = !(off > 0x1p-80 * dg);
        }
        __syncthreads();
        if (done) break;
        for (int r = 0; r < kMono - 1; r++) {
            if (t < kMono) {
                // column t of J: cs[t][0] e_t + cs[t][1] e_partner.  For the pair p < q: t = tan of the smaller angle that
                // zeroes a_pq, new column p = c col_p - s col_q, new column q = s col_p + c col_q
                const int o = partner(t, r), p = t < o ? t : o, q = t < o ? o : t;
                const double app = A[cur][p][p], aqq = A[cur][q][q], apq = A[cur][p][q];
                double co = 1.0, si = 0.0;
                if (apq != 0.0) {
                    const double d = aqq - app, b = 2.0 * apq, h = sqrt(d * d + b * b);
                    const double tn = (d >= 0.0 ? b : -b) / (fabs(d) + h);
                    co = 1.0 / sqrt(tn * tn + 1.0);
                    si = tn * co;
                }
                cs[t][0] = co;
                cs[t][1] = t == p ? -si : si;
            }
            __syncthreads();
            if (t < 2 * kMono * kMono) {
                if (i < kMono) {
                    // both (i, j) and (j, i) evaluate the expression of (min, max): A stays symmetric bit for bit
                    const int p = i < j ? i : j, q = i < j ? j : i, op = partner(p, r), oq = partner(q, r);
                    const double cp = cs[p][0], sp = cs[p][1], cq = cs[q][0], sq = cs[q][1];
                    const double v = (((cp * cq) * A[cur][p][q] + (cp * sq) * A[cur][p][oq]) + (sp * cq) * A[cur][op][q]) +
                                     (sp * sq) * A[cur][op][oq];
                    A[cur ^ 1][i][j] = (op == q && p != q) ? 0.0 : v;
                } else {
                    const int k = i - kMono, oj = partner(j, r);
                    V[cur ^ 1][k][j] = cs[j][0] * V[cur][k][j] + cs[j][1] * V[cur][k][oj];
                }
            }
            __syncthreads();
            cur ^= 1;
        }
    }
    // ---- w = sum over the kept eigenpairs of v (v . r) / lambda
    if (t < kMono) {
        double lmax = 0.0;
        for (int k = 0; k < kMono; k++) lmax = fmax(lmax, A[cur][k][k]);
        const double lam = A[cur][t][t];
        double d = 0.0;
        for (int k = 0; k < kMono; k++) d += V[cur][k][t] * tot[kPairs + k];
        proj[t] = (lam > 0.0 && lam > 0x1p-46 * lmax) ? d / lam : 0.0;
    }
    __syncthreads();
    if (t < kMono) {
        double w = 0.0;
        for (int k = 0; k < kMono; k++) w += V[cur][t][k] * proj[k];
        warps[(size_t)view * warp_stride + 3 * t + c] = w;
    }
    if (t == kMono) counts[(size_t)view * count_stride + c] = (int64_t)tot[kItems];
}

// grid (blocks, B).  x may be out: a thread reads its pixel before it writes it.
__global__ __launch_bounds__(256) void cc_apply_kernel(int64_t hw, const float* x, const double* __restrict__ warps, int64_t warp_stride,
                                                       float* out) {
    __shared__ double w[3 * kMono];
    if (threadIdx.x < 3 * kMono) w[threadIdx.x] = warps[(size_t)blockIdx.y * warp_stride + threadIdx.x];
    __syncthreads();
    const size_t view = 3 * (size_t)blockIdx.y * (size_t)hw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
        const size_t o = view + 3 * (size_t)i;
        double a[kMono];
        monomials(x[o], x[o + 1], x[o + 2], a);
        float y[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double s = a[0] * w[c];
#pragma unroll
            for (int k = 1; k < kMono; k++) s = s + a[k] * w[3 * k + c];
            y[c] = (float)fmin(fmax(s, 0.0), 1.0);
        }
        out[o] = y[0]; out[o + 1] = y[1]; out[o + 2] = y[2];
    }
}

inline bool sizes_ok(int32_t b, int32_t h, int32_t w) {
    return b >= 1 && b <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int64_t misplat_colorcorrect_scratch_floats(int32_t n_views, int32_t height, int32_t width) {
    if (!sizes_ok(n_views, height, width)) return -1;
    return 2 * (int64_t)kPart * 3 * accum_blocks((int64_t)height * width) * n_views;          // doubles
}

extern "C" int misplat_colorcorrect(int32_t n_views, int32_t height, int32_t width, const float* pred, const float* gt,
                                    int32_t num_iters, float eps, float* scratch, float* corrected, double* warps,
                                    int64_t* counts, misplat_stream_t stream) {
    if (!sizes_ok(n_views, height, width) || num_iters < 0 || num_iters > 64 || !(eps >= 0.0f && eps < 0.5f)) return MISPLAT_EINVAL;
    if (!pred || !gt || !corrected || pred == corrected || gt == corrected) return MISPLAT_EINVAL;
    if (num_iters > 0 && (!scratch || ((uintptr_t)scratch & 7) || !warps || !counts)) return MISPLAT_EINVAL;
    const int64_t hw = (int64_t)height * width;
    hipStream_t s = (hipStream_t)stream;
    if (num_iters == 0)
        return hipMemcpyAsync(corrected, pred, sizeof(float) * 3 * (size_t)hw * n_views, hipMemcpyDeviceToDevice, s) == hipSuccess
                   ? MISPLAT_OK : MISPLAT_ELAUNCH;
    const int nb = accum_blocks(hw);
    const float lo = eps, hi = 1.0f - eps;
    double* partials = (double*)scratch;
    const int64_t warp_stride = (int64_t)num_iters * 3 * kMono, count_stride = (int64_t)num_iters * 3;
    for (int it = 0; it < num_iters; it++) {
        const float* x = it == 0 ? pred : corrected;
        double* w = warps + (size_t)it * 3 * kMono;
        hipLaunchKernelGGL(cc_accumulate_kernel, dim3(nb, 3, n_views), dim3(256), 0, s, hw, x, pred, gt, lo, hi, partials);
        hipLaunchKernelGGL(cc_solve_kernel, dim3(3 * n_views), dim3(kSolveThreads), 0, s, (const double*)partials, nb, w, warp_stride,
                           counts + (size_t)it * 3, count_stride);
        hipLaunchKernelGGL(cc_apply_kernel, dim3(4 * nb, n_views), dim3(256), 0, s, hw, x, (const double*)w, warp_stride, corrected);
    }
    return launched();
}
