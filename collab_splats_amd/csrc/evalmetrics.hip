// evalmetrics.hip -- how good a render is: per-view PSNR / SSIM / MSE / L1 of B stacked views against their ground truth,
// and the angular and depth errors of the normal and depth maps.  These are the numbers nerfstudio's
// Splatfacto reports from get_metrics_dict and get_image_metrics_and_images, which the reference model inherits through
// super() (third-party and absent from the reference tree) [UNVERIFIED-UPSTREAM]:
//   psnr = torchmetrics PeakSignalNoiseRatio(data_range=1.0) = -10 log10(mean (pred - gt)^2), +inf for identical images;
//   ssim = torchmetrics structural_similarity_index_measure, which reflect-pads both images by the window's half width and
//          crops the same border off the index map again: what is left is the VALID (H - 10) x (W - 10) region, so the
//          number equals pytorch_msssim's valid-region mean, the SSIM of the training loss (ssim.hip).  Same window, same
//          C1 = 0.01^2, C2 = 0.03^2 (ssimwin.h).
// The angle map with no mask, no decoding and no normalisation is collab_splats/utils/utils.py:63-81 (mean_angular_error).
// The depth errors are the definitions of Eigen, Puhrsch & Fergus, "Depth map prediction from a single image using a
// multi-scale deep network" (NeurIPS 2014), restated from the paper; parity with any other code is unpinned.
//
// Every entry point is two launches on the caller's stream: workgroups of 256 threads leave partial sums, then ONE workgroup
// per view adds that view's partials in fp64 in an order that depends on H and W only (never on B or the view's index) and
// writes the view's row.  No atomics, no host read, no per-position maps: the image kernel brings 2 x 12 bytes per pixel
// in from HBM (the overlap of neighbouring patches comes from cache) and writes 12 bytes per 16 x 16 tile.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "misplat.h"
#include "ssimwin.h"
#include "wgprims.h"

namespace {

// ------------------------------------------------------------------------------------------------ the per-view finish
// K sums of one view: thread t adds partials t, t + 256, ... in ascending order in fp64, then block_sums' tree; thread 0
// hands the totals to `fin`, which writes the view's row.  part: [views][nb][K].
template <int K, typename T, class Fin>
__global__ __launch_bounds__(256) void view_final_kernel(const T* __restrict__ part, int nb, Fin fin, float* __restrict__ out) {
    __shared__ double tot[K];
    const T* p = part + (size_t)blockIdx.x * nb * K;
    double x[K];
#pragma unroll
    for (int k = 0; k < K; k++) x[k] = 0.0;
    // (eight trips' loads in flight at once; the additions stay in ascending order)
#pragma unroll 8
    for (int b = threadIdx.x; b < nb; b += 256)
#pragma unroll
        for (int k = 0; k < K; k++) x[k] += (double)p[(size_t)b * K + k];
    block_sums<K, 4>(x, tot);
    __syncthreads();
    if (threadIdx.x == 0) fin(tot, out, (int)blockIdx.x);
}

// ---------------------------------------------------------------------------------------------------------- images
constexpr int kImageSums = 3;                   // sum d^2, sum |d|, sum ssim

// The index of one window position from its five window means.  The variances are differences of nearly equal numbers, so
// the operations are kept exactly as written (no contraction): for x == y every pair of terms then has the same bits,
// numerator and denominator are equal and an identical pair scores exactly 1 -- a fused multiply-add on one side only
// leaves a rounding of E[xx] over C2, 1e-6 and more.  ONE quotient num / den, den >= C1 C2 > 0, as a reciprocal and one
// correction step (q += r (num - den q), the residual exact in the fma): within a rounding of the IEEE quotient -- and
// exactly 1 for num == den -- in four instructions (two IEEE divisions in its place measured the same time, within 2 us, at 1080p).
__device__ __forceinline__ float ssim_index(float m1, float m2, float xx, float yy, float xy) {
#pragma clang fp contract(off)
    const float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
    const float s11 = xx - m11, s22 = yy - m22, s12 = xy - m12;
    const float num = (2.0f * m12 + kSsimC1) * (2.0f * s12 + kSsimC2);
    const float den = ((m11 + m22) + kSsimC1) * ((s11 + s22) + kSsimC2);
    const float r = __builtin_amdgcn_rcpf(den), q = num * r;
    return fmaf(r, fmaf(-den, q, num), q);
}

// sum of squares and of magnitudes of one pixel's three differences: explicit operations, so that both code paths that
// call it (a tile with and without window positions) give the same bits
__device__ __forceinline__ void pixel_sums(float e0, float e1, float e2, float& d2, float& d1) {
    d2 = fmaf(e2, e2, fmaf(e1, e1, e0 * e0));
    d1 = (fabsf(e0) + fabsf(e1)) + fabsf(e2);
}

// One workgroup = one 16 x 16 tile of one view: the tile's PIXELS for the two difference sums, the tile's WINDOW POSITIONS
// (those inside the valid region) for the SSIM sum.  With positions: the 26 x 26 x 3 patch of both images goes through LDS
// once, zero beyond the image; the separable filter is ssim_fwd_kernel's (four outputs per thread and pass, the window
// folded around its centre), without the derivative maps.  Without (a tile right of or below the valid region, or the
// whole launch with SSIM = false, which then holds no LDS arrays at all): a thread reads its own pixel of both images and
// nothing else.  partials: [view][tile][3].
template <bool SSIM>
__global__ __launch_bounds__(256) void eval_image_kernel(int H, int Wd, const float* __restrict__ pred, const float* __restrict__ gt,
                                                         Window win, float* __restrict__ partials) {
    __shared__ float red[kImageSums][4];
    const int ox = blockIdx.x * kTile, oy = blockIdx.y * kTile;
    const int OW = Wd - (kWin - 1), OH = H - (kWin - 1);
    const int row_floats = 3 * Wd;
    const size_t image = (size_t)blockIdx.z * (size_t)H * (size_t)row_floats;
    pred += image;
    gt += image;
    const int lx = threadIdx.x & (kTile - 1), ly = threadIdx.x >> 4;
    const bool mine = ox + lx < Wd && oy + ly < H;                        // this thread's pixel of the tile
    const bool filter = SSIM && ox < OW && oy < OH;                       // (uniform over the workgroup)
    float d2 = 0.f, d1 = 0.f, s = 0.f;
    if (!filter) {
        if (mine) {
            const size_t o = (size_t)(oy + ly) * row_floats + 3 * (ox + lx);
            pixel_sums(pred[o] - gt[o], pred[o + 1] - gt[o + 1], pred[o + 2] - gt[o + 2], d2, d1);
        }
    }
    if constexpr (SSIM) if (filter) {
        __shared__ float sx[kPatch][kRowS], sy[kPatch][kRowS];
        __shared__ float hz[3][5][kPatch][kHzS];
        {
            // 234 threads = 3 patch rows of 78 floats per round, 9 rounds; all of a thread's loads before the first LDS store
            constexpr int kRowsPer = 256 / kRow3, kRounds = (kPatch + kRowsPer - 1) / kRowsPer;
            const int r0 = threadIdx.x / kRow3, q = threadIdx.x - r0 * kRow3;
            const int xf = 3 * ox + q;
            const bool lane_ok = r0 < kRowsPer && xf < row_floats;
            float va[kRounds], vb[kRounds];
#pragma unroll
            for (int i = 0; i < kRounds; i++) {
                const int r = r0 + kRowsPer * i, y = oy + r;
                va[i] = 0.f; vb[i] = 0.f;
                if (lane_ok && r < kPatch && y < H) {
                    const size_t o = (size_t)y * row_floats + xf;
                    va[i] = pred[o]; vb[i] = gt[o];
                }
            }
#pragma unroll
            for (int i = 0; i < kRounds; i++) {
                const int r = r0 + kRowsPer * i;
                if (r0 < kRowsPer && r < kPatch) { sx[r][q] = va[i]; sy[r][q] = vb[i]; }
            }
        }
        __syncthreads();
        // ---- the tile's own 16 x 16 pixels (the patch's first 16 rows and columns), all channels
        if (mine)
            pixel_sums(sx[ly][3 * lx] - sy[ly][3 * lx], sx[ly][3 * lx + 1] - sy[ly][3 * lx + 1],
                       sx[ly][3 * lx + 2] - sy[ly][3 * lx + 2], d2, d1);
        // ---- row pass: item = (channel, patch row, quad of output columns)
        for (int t = threadIdx.x; t < 3 * kPatch * kQuads; t += 256) {
            const int quad = t % kQuads, cr = t / kQuads;
            const int r = cr % kPatch, c = cr / kPatch;
            float v[5][kWin + 3];
#pragma unroll
            for (int j = 0; j < kWin + 3; j++) {
                const float a = sx[r][3 * (4 * quad + j) + c], b = sy[r][3 * (4 * quad + j) + c];
                v[0][j] = a; v[1][j] = b; v[2][j] = a * a; v[3][j] = b * b; v[4][j] = a * b;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int col = 4 * quad + u;
#pragma unroll
                for (int q = 0; q < 5; q++) {
                    float acc = win.w[5] * v[q][u + 5];
#pragma unroll
                    for (int k = 0; k < 5; k++) acc = fmaf(win.w[k], v[q][u + k] + v[q][u + 10 - k], acc);
                    hz[c][q][r][col] = acc;
                }
            }
        }
        __syncthreads();
        // ---- column pass: item = (channel, quad of output rows, column); four outputs per thread
        if (threadIdx.x < 3 * kQuads * kTile) {
            const int col = threadIdx.x % kTile, crq = threadIdx.x / kTile;
            const int rq = crq % kQuads, c = crq / kQuads;
            float acc[4][5];
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int q = 0; q < 5; q++) acc[u][q] = 0.f;
#pragma unroll
            for (int j = 0; j < kWin + 3; j++) {
                float v[5];
#pragma unroll
                for (int q = 0; q < 5; q++) v[q] = hz[c][q][4 * rq + j][col];
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (j - u >= 0 && j - u < kWin) {
#pragma unroll
                        for (int q = 0; q < 5; q++) acc[u][q] = fmaf(win.w[j - u], v[q], acc[u][q]);
                    }
            }
            const int px = ox + col;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int py = oy + 4 * rq + u;
                if (px < OW && py < OH) s += ssim_index(acc[u][0], acc[u][1], acc[u][2], acc[u][3], acc[u][4]);
            }
        }
    }
    d2 = wave_sum_xor(d2);
    d1 = wave_sum_xor(d1);
    s = wave_sum_xor(s);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = d2; red[1][threadIdx.x >> 6] = d1; red[2][threadIdx.x >> 6] = s; }
    __syncthreads();
    if (threadIdx.x < kImageSums) {
        const size_t nb = (size_t)gridDim.x * gridDim.y;
        const size_t b = (size_t)blockIdx.z * nb + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        partials[b * kImageSums + threadIdx.x] =
            (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
    }
}

struct ImageFinish {
    double inv_values, inv_positions;               // 1 / (3 H W), 1 / (3 OH OW) (0 without SSIM)
    int want_ssim;
    __device__ void operator()(const double* tot, float* out, int view) const {
        const double mse = tot[0] * inv_values;
        float* o = out + 4 * (size_t)view;
        o[0] = (float)mse;
        o[1] = (float)(tot[1] * inv_values);
        o[2] = want_ssim ? (float)(tot[2] * inv_positions) : __builtin_nanf("");
        o[3] = (float)(-10.0 * log10(mse));         // log10(0) = -inf: +inf for identical images
    }
};

// ---------------------------------------------------------------------------------------------- per-pixel metrics
constexpr int kPixelBlocks = 1024;                  // workgroups per view at most: a thread walks pixels i, i + stride, ...
constexpr int kNormalSums = 5;                      // sum theta, n < 11.25, n < 22.5, n < 30, count
constexpr int kDepthSums = 8;                       // abs_rel, sq_rel, sq, log^2, n delta_1..3, count

inline int pixel_blocks(int64_t hw) { return (int)((hw + 255) / 256 < kPixelBlocks ? (hw + 255) / 256 : kPixelBlocks); }

// The per-pixel arithmetic runs in fp64 on the fp32 inputs (products of floats are exact there): the angle and the log are
// rounded once, to the map's fp32.  Counts are integers per thread; as doubles they add exactly.  partials: [view][block][K].
__global__ __launch_bounds__(256) void eval_normals_kernel(int64_t hw, const float* __restrict__ pred, const float* __restrict__ gt,
                                                           const uint8_t* __restrict__ valid, int encoded, int normalize,
                                                           float* __restrict__ map, double* __restrict__ partials) {
    const size_t view = (size_t)blockIdx.y * (size_t)hw;
    pred += 3 * view;
    gt += 3 * view;
    if (valid) valid += view;
    if (map) map += view;
    constexpr double kDeg = 3.14159265358979323846 / 180.0;
    double sum = 0.0;
    int n11 = 0, n22 = 0, n30 = 0, count = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
        double a[3], b[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            a[c] = (double)pred[3 * i + c];
            b[c] = (double)gt[3 * i + c];
            if (encoded) { a[c] = 2.0 * a[c] - 1.0; b[c] = 2.0 * b[c] - 1.0; }
        }
        bool ok = !valid || valid[i] != 0;
        double dot = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
        if (normalize) {
            const double la = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], lb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
            ok = ok && la > 1e-12 && lb > 1e-12;
            dot = ok ? dot / sqrt(la * lb) : 0.0;
        }
        // (a NaN input gives a NaN angle: it is no smaller than any threshold and makes the mean NaN, as torch's would be)
        const double theta = acos(dot < -1.0 ? -1.0 : (dot > 1.0 ? 1.0 : dot));
        if (ok) {
            sum += theta;
            n11 += theta < 11.25 * kDeg; n22 += theta < 22.5 * kDeg; n30 += theta < 30.0 * kDeg;
            count++;
        }
        if (map) map[i] = ok ? (float)theta : __builtin_nanf("");
    }
    double x[kNormalSums] = {sum, (double)n11, (double)n22, (double)n30, (double)count};
    block_sums<kNormalSums, 4>(x, partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kNormalSums);
}

struct NormalFinish {
    __device__ void operator()(const double* tot, float* out, int view) const {
        float* o = out + kNormalSums * (size_t)view;
        const double n = tot[4];                    // 0 / 0 = NaN for a view without a counted pixel
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = (float)(tot[k] / n);
        o[4] = (float)n;
    }
};

__global__ __launch_bounds__(256) void eval_depth_kernel(int64_t hw, const float* __restrict__ pred, const float* __restrict__ gt,
                                                         const uint8_t* __restrict__ valid, float max_depth,
                                                         double* __restrict__ partials) {
    const size_t view = (size_t)blockIdx.y * (size_t)hw;
    pred += view;
    gt += view;
    if (valid) valid += view;
    double x[kDepthSums];
#pragma unroll
    for (int k = 0; k < kDepthSums; k++) x[k] = 0.0;
    int n1 = 0, n2 = 0, n3 = 0, count = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
        const float pf = pred[i], gf = gt[i];
        const bool ok = (!valid || valid[i] != 0) && isfinite(pf) && isfinite(gf) && pf > 0.f && gf > 0.f &&
                        (max_depth <= 0.f || gf <= max_depth);
        if (ok) {
            const double p = (double)pf, g = (double)gf, d = p - g, l = log(p) - log(g);
            x[0] += fabs(d) / g;
            x[1] += d * d / g;
            x[2] += d * d;
            x[3] += l * l;
            const double r = p > g ? p / g : g / p;
            n1 += r < 1.25; n2 += r < 1.5625; n3 += r < 1.953125;
            count++;
        }
    }
    x[4] = (double)n1; x[5] = (double)n2; x[6] = (double)n3; x[7] = (double)count;
    block_sums<kDepthSums, 4>(x, partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kDepthSums);
}

struct DepthFinish {
    __device__ void operator()(const double* tot, float* out, int view) const {
        float* o = out + kDepthSums * (size_t)view;
        const double n = tot[7];
        o[0] = (float)(tot[0] / n);
        o[1] = (float)(tot[1] / n);
        o[2] = (float)sqrt(tot[2] / n);
        o[3] = (float)sqrt(tot[3] / n);
#pragma unroll
        for (int k = 4; k < 7; k++) o[k] = (float)(tot[k] / n);
        o[7] = (float)n;
    }
};

inline bool views_ok(int32_t b, int32_t h, int32_t w) {
    return b >= 1 && b <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31) && (h + kTile - 1) / kTile <= 65535;
}

}  // namespace

extern "C" int64_t misplat_eval_image_scratch_floats(int32_t n_views, int32_t height, int32_t width) {
    if (!views_ok(n_views, height, width)) return -1;
    const int64_t gx = (width + kTile - 1) / kTile, gy = (height + kTile - 1) / kTile;
    return kImageSums * gx * gy * n_views;
}

extern "C" int misplat_eval_image(int32_t n_views, int32_t height, int32_t width, const float* pred, const float* gt,
                                  int32_t want_ssim, float* scratch, float* out, misplat_stream_t stream) {
    if (!views_ok(n_views, height, width) || !pred || !gt || !scratch || !out) return MISPLAT_EINVAL;
    if (want_ssim && (height < kWin || width < kWin)) return MISPLAT_EINVAL;
    // tiles of PIXELS: every pixel lies in one; a tile's window positions are those of its pixels inside the valid region
    const dim3 grid((width + kTile - 1) / kTile, (height + kTile - 1) / kTile, n_views);
    hipStream_t s = (hipStream_t)stream;
    if (want_ssim)
        hipLaunchKernelGGL(eval_image_kernel<true>, grid, dim3(256), 0, s, (int)height, (int)width, pred, gt, make_window(), scratch);
    else
        hipLaunchKernelGGL(eval_image_kernel<false>, grid, dim3(256), 0, s, (int)height, (int)width, pred, gt, make_window(), scratch);
    const double values = 3.0 * (double)height * (double)width;
    const double positions = want_ssim ? 3.0 * (double)(height - (kWin - 1)) * (double)(width - (kWin - 1)) : 0.0;
    const ImageFinish fin{1.0 / values, want_ssim ? 1.0 / positions : 0.0, (int)(want_ssim != 0)};
    hipLaunchKernelGGL((view_final_kernel<kImageSums, float, ImageFinish>), dim3(n_views), dim3(256), 0, s,
                       (const float*)scratch, (int)(grid.x * grid.y), fin, out);
    return launched();
}

extern "C" int64_t misplat_eval_pixels_scratch_floats(int32_t n_views, int32_t height, int32_t width) {
    if (!views_ok(n_views, height, width)) return -1;
    return 2 * (int64_t)kDepthSums * pixel_blocks((int64_t)height * width) * n_views;      // doubles, the wider of the two
}

extern "C" int misplat_eval_normals(int32_t n_views, int32_t height, int32_t width, const float* pred, const float* gt,
                                    const uint8_t* valid, int32_t encoded, int32_t normalize, float* map, float* scratch,
                                    float* out, misplat_stream_t stream) {
    if (!views_ok(n_views, height, width) || !pred || !gt || !scratch || !out || ((uintptr_t)scratch & 7)) return MISPLAT_EINVAL;
    const int64_t hw = (int64_t)height * width;
    const int nb = pixel_blocks(hw);
    hipStream_t s = (hipStream_t)stream;
    double* partials = (double*)scratch;
    hipLaunchKernelGGL(eval_normals_kernel, dim3(nb, n_views), dim3(256), 0, s, hw, pred, gt, valid, (int)(encoded != 0),
                       (int)(normalize != 0), map, partials);
    hipLaunchKernelGGL((view_final_kernel<kNormalSums, double, NormalFinish>), dim3(n_views), dim3(256), 0, s,
                       (const double*)partials, nb, NormalFinish{}, out);
    return launched();
}

extern "C" int misplat_eval_depth(int32_t n_views, int32_t height, int32_t width, const float* pred, const float* gt,
                                  const uint8_t* valid, float max_depth, float* scratch, float* out, misplat_stream_t stream) {
    if (!views_ok(n_views, height, width) || !pred || !gt || !scratch || !out || ((uintptr_t)scratch & 7)) return MISPLAT_EINVAL;
    const int64_t hw = (int64_t)height * width;
    const int nb = pixel_blocks(hw);
    hipStream_t s = (hipStream_t)stream;
    double* partials = (double*)scratch;
    hipLaunchKernelGGL(eval_depth_kernel, dim3(nb, n_views), dim3(256), 0, s, hw, pred, gt, valid, max_depth, partials);
    hipLaunchKernelGGL((view_final_kernel<kDepthSums, double, DepthFinish>), dim3(n_views), dim3(256), 0, s,
                       (const double*)partials, nb, DepthFinish{}, out);
    return launched();
}
