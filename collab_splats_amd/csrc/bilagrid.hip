// bilagrid.hip -- the bilateral-grid colour correction of a training view and the grids' total-variation loss (the
// `_apply_bilateral_grid` / `tv_loss` of the reference's call sites rade_gs_model.py:231-234, :284-289; the operation
// itself is nerfstudio's, restated from the published method [UNVERIFIED-UPSTREAM]):
//   x = px / (W - 1), y = py / (H - 1), z = 0.299 r + 0.587 g + 0.114 b            (0 where the image has one column / row)
//   A[12] = trilinear(grids[cam] at (z (L - 1), y (GH - 1), x (GW - 1))), border-clamped, lerp form a + t (b - a), x, y, z
//   out_c = A[c,0] r + A[c,1] g + A[c,2] b + A[c,3]
//   tv = (1 / num) sum_axis sum (G[i + 1] - G[i])^2 / count_axis
// Built without FMA contraction: z and with it the interval floor(gz) are the fp32 restatement's (tests/), black gives
// exactly 0 and white exactly 1, and a locally constant grid is reproduced bit for bit.
//
// Slice forward and its image-side backward: one pixel per lane, 32 x 8 pixels per workgroup.  The workgroup stages the
// (gy, gx) columns its pixels overlap -- all L levels, 12 channels -- in LDS (2 x 2 or 3 x 3 columns at 1080p) and every
// pixel reads its 8 corners from there; where an image is so small against the grid that the columns of a workgroup do
// not fit kStage floats, the same code reads the corners from global memory instead.  The backward recomputes A and the
// z-slope from rgb and the grid; nothing but rgb is saved.
// Grid-side backward: a GATHER.  A workgroup owns one (gy, gx) column, 8 levels of it and one slice of the rows of its
// support (the pixels within one cell in x and y); a lane keeps 8 x 12 private sums of dout (x) (r, g, b, 1) weighted by
// the column's trilinear weights, the lanes meet in a shuffle tree and the four waves in LDS, and a second kernel adds
// the row slices in order while it writes the whole [num, 12, L, GH, GW] gradient (zeros for the other cameras).  No
// atomics: two runs are equal bit for bit.
// TV: a grid-stride pass with per-lane fp64 sums per axis, a fixed tree per workgroup, partials that a one-workgroup
// kernel adds in order; the backward is the 3-axis stencil.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "misplat.h"
#include "wgprims.h"

namespace {

constexpr int kTileW = 32, kTileH = 8;          // pixels of a workgroup of the slice kernels
constexpr int kStage = 4096;                    // floats of grid a slice workgroup stages (16 KiB)
constexpr int kLev = 8;                         // levels a workgroup of the grid-side backward accumulates
constexpr int kMaxSplit = 16;                   // row slices of a column's support
constexpr int kSplitPixels = 4096;              // pixels of a typical support per row slice
constexpr int kMaxSide = 32768;                 // image rows / columns
constexpr float kWr = 0.299f, kWg = 0.587f, kWb = 0.114f;

struct Geo {
    int H, W, GW, GH, L;
};

bool geo_ok(int H, int W, int GW, int GH, int L) {
    return H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide && GW >= 1 && GW <= MISPLAT_BILAGRID_MAX_XY && GH >= 1 &&
           GH <= MISPLAT_BILAGRID_MAX_XY && L >= 1 && L <= MISPLAT_BILAGRID_MAX_L;
}

// position of pixel coordinate p (of n) on a grid axis of g vertices: the interval's two vertices and the fraction
__device__ __forceinline__ void axis_pos(int p, int n, int g, int* i0, int* i1, float* t) {
    const float u = n > 1 ? (float)p / (float)(n - 1) : 0.f;
    float c = u * (float)(g - 1);
    c = fminf(fmaxf(c, 0.f), (float)(g - 1));
    const float f = floorf(c);
    *i0 = (int)f;
    *i1 = min(*i0 + 1, g - 1);
    *t = c - f;
}

// the same along z from the pixel's colour; inside: 0 < gz < L - 1 (where the z-slope is not zero)
__device__ __forceinline__ void z_pos(float r, float g, float b, int L, int* i0, int* i1, float* t, bool* inside) {
    const float z = kWr * r + kWg * g + kWb * b;
    const float top = (float)(L - 1);
    const float c = fminf(fmaxf(z * top, 0.f), top);        // (a NaN lands on 0: every index stays inside the grid)
    const float f = floorf(c);
    *i0 = (int)f;
    *i1 = min(*i0 + 1, L - 1);
    *t = c - f;
    *inside = c > 0.f && c < top;
}

// the pixels whose position on a grid axis lies within one cell of vertex v: a superset [lo, hi] (the weight itself is
// computed per pixel with axis_pos, so the gather is the exact transpose of the sampling)
__device__ __forceinline__ void support(int v, int n, int g, int* lo, int* hi) {
    if (g == 1 || n == 1) {
        *lo = 0;
        *hi = n - 1;
        return;
    }
    const double s = (double)(n - 1) / (double)(g - 1);
    const int a = (int)floor((double)(v - 1) * s) - 1, b = (int)ceil((double)(v + 1) * s) + 1;
    *lo = max(a, 0);
    *hi = min(b, n - 1);
}

__device__ __forceinline__ float vertex_weight(int i0, int i1, float t, int v) {
    return (i0 == v ? 1.f - t : 0.f) + (i1 == v ? t : 0.f);
}

// P[12] = the grid bilinearly interpolated in (y, x) on level l.  kLds: from the staged columns ([ny][nx][L][12]).
template <bool kLds>
__device__ __forceinline__ void plane(float (&P)[12], const float* __restrict__ grid, const float* sg, const Geo& g, int l,
                                      int x0, int x1, int y0, int y1, float tx, float ty, int xlo, int ylo, int nx) {
    if (kLds) {
        const float* c00 = sg + ((size_t)((y0 - ylo) * nx + (x0 - xlo)) * g.L + l) * 12;
        const float* c01 = sg + ((size_t)((y0 - ylo) * nx + (x1 - xlo)) * g.L + l) * 12;
        const float* c10 = sg + ((size_t)((y1 - ylo) * nx + (x0 - xlo)) * g.L + l) * 12;
        const float* c11 = sg + ((size_t)((y1 - ylo) * nx + (x1 - xlo)) * g.L + l) * 12;
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const float r0 = c00[k] + tx * (c01[k] - c00[k]), r1 = c10[k] + tx * (c11[k] - c10[k]);
            P[k] = r0 + ty * (r1 - r0);
        }
    } else {
        const size_t lev = (size_t)g.GH * g.GW;
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const float* q = grid + ((size_t)k * g.L + l) * lev;
            const float a00 = q[(size_t)y0 * g.GW + x0], a01 = q[(size_t)y0 * g.GW + x1];
            const float a10 = q[(size_t)y1 * g.GW + x0], a11 = q[(size_t)y1 * g.GW + x1];
            const float r0 = a00 + tx * (a01 - a00), r1 = a10 + tx * (a11 - a10);
            P[k] = r0 + ty * (r1 - r0);
        }
    }
}

// ---- slice forward (kBwd = false: out = A (r, g, b, 1)) and image-side backward (kBwd = true: out = d rgb)
template <bool kBwd>
__global__ __launch_bounds__(256) void slice_kernel(Geo g, const float* __restrict__ rgb, const float* __restrict__ grid,
                                                    const float* __restrict__ v_out, float* __restrict__ out) {
    __shared__ float sg[kStage];
    const int tid = threadIdx.x;
    const int bx = blockIdx.x * kTileW, by = blockIdx.y * kTileH;
    // the columns the workgroup's pixels overlap (positions are monotone in the pixel index)
    int xlo, xhi, ylo, yhi, unused;
    float tunused;
    axis_pos(bx, g.W, g.GW, &xlo, &unused, &tunused);
    axis_pos(min(bx + kTileW, g.W) - 1, g.W, g.GW, &unused, &xhi, &tunused);
    axis_pos(by, g.H, g.GH, &ylo, &unused, &tunused);
    axis_pos(min(by + kTileH, g.H) - 1, g.H, g.GH, &unused, &yhi, &tunused);
    const int nx = xhi - xlo + 1, ny = yhi - ylo + 1;
    const int n_stage = nx * ny * g.L * 12;                       // <= 256 * 256 * 16 * 12 < 2^31
    const bool staged = n_stage <= kStage;                        // workgroup-uniform
    if (staged) {
        for (int i = tid; i < n_stage; i += 256) {
            const int lx = i % nx, r1 = i / nx, ly = r1 % ny, r2 = r1 / ny, l = r2 % g.L, k = r2 / g.L;
            sg[((ly * nx + lx) * g.L + l) * 12 + k] = grid[(((size_t)k * g.L + l) * g.GH + (ylo + ly)) * g.GW + (xlo + lx)];
        }
        __syncthreads();
    }
    const int px = bx + (tid & (kTileW - 1)), py = by + tid / kTileW;
    if (px >= g.W || py >= g.H) return;
    const size_t pix = ((size_t)py * g.W + px) * 3;
    const float r = rgb[pix], gr = rgb[pix + 1], b = rgb[pix + 2];
    int x0, x1, y0, y1, z0, z1;
    float tx, ty, tz;
    bool inside;
    axis_pos(px, g.W, g.GW, &x0, &x1, &tx);
    axis_pos(py, g.H, g.GH, &y0, &y1, &ty);
    z_pos(r, gr, b, g.L, &z0, &z1, &tz, &inside);
    float P0[12], P1[12], A[12];
    if (staged) {
        plane<true>(P0, grid, sg, g, z0, x0, x1, y0, y1, tx, ty, xlo, ylo, nx);
        plane<true>(P1, grid, sg, g, z1, x0, x1, y0, y1, tx, ty, xlo, ylo, nx);
    } else {
        plane<false>(P0, grid, sg, g, z0, x0, x1, y0, y1, tx, ty, xlo, ylo, nx);
        plane<false>(P1, grid, sg, g, z1, x0, x1, y0, y1, tx, ty, xlo, ylo, nx);
    }
#pragma unroll
    for (int k = 0; k < 12; k++) A[k] = P0[k] + tz * (P1[k] - P0[k]);
    if (!kBwd) {
#pragma unroll
        for (int c = 0; c < 3; c++) out[pix + c] = A[4 * c] * r + A[4 * c + 1] * gr + A[4 * c + 2] * b + A[4 * c + 3];
        return;
    }
    const float d0 = v_out[pix], d1 = v_out[pix + 1], d2 = v_out[pix + 2];
    const float d[3] = {d0, d1, d2};
    float vr = 0.f, vg = 0.f, vb = 0.f, q = 0.f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        vr += d[c] * A[4 * c];
        vg += d[c] * A[4 * c + 1];
        vb += d[c] * A[4 * c + 2];
        // the slope of the interval floor(gz); 0 at and beyond the two border planes
        q += d[c] * (r * (P1[4 * c] - P0[4 * c]) + gr * (P1[4 * c + 1] - P0[4 * c + 1]) + b * (P1[4 * c + 2] - P0[4 * c + 2]) +
                     (P1[4 * c + 3] - P0[4 * c + 3]));
    }
    q = inside ? q * (float)(g.L - 1) : 0.f;
    out[pix] = vr + kWr * q;
    out[pix + 1] = vg + kWg * q;
    out[pix + 2] = vb + kWb * q;
}

// ---- grid-side backward, pass 1: part[split][column][level (padded to kLev)][12]
__global__ __launch_bounds__(256) void grid_bwd_kernel(Geo g, const float* __restrict__ rgb, const float* __restrict__ v_out,
                                                       float* __restrict__ part, int n_split, int l_pad) {
    __shared__ float red[4][kLev * 12];
    const int tid = threadIdx.x, col = blockIdx.x, split = blockIdx.y, l0 = blockIdx.z * kLev;
    const int vx = col % g.GW, vy = col / g.GW;
    int c0, c1, r0, r1;
    support(vx, g.W, g.GW, &c0, &c1);
    support(vy, g.H, g.GH, &r0, &r1);
    const int per = (r1 - r0 + 1 + n_split - 1) / n_split;
    const int rs = r0 + split * per, re = min(r1, rs + per - 1);
    const int nc = c1 - c0 + 1;
    const int n = re >= rs ? (re - rs + 1) * nc : 0;              // <= 32768^2 = 2^30
    float acc[kLev][12];
#pragma unroll
    for (int l = 0; l < kLev; l++)
#pragma unroll
        for (int k = 0; k < 12; k++) acc[l][k] = 0.f;
    for (int i = tid; i < n; i += 256) {
        const int py = rs + i / nc, px = c0 + i % nc;
        int i0, i1;
        float t;
        axis_pos(px, g.W, g.GW, &i0, &i1, &t);
        const float wx = vertex_weight(i0, i1, t, vx);
        axis_pos(py, g.H, g.GH, &i0, &i1, &t);
        const float w = wx * vertex_weight(i0, i1, t, vy);
        if (w == 0.f) continue;
        const size_t pix = ((size_t)py * g.W + px) * 3;
        const float r = rgb[pix], gr = rgb[pix + 1], b = rgb[pix + 2];
        const float d0 = v_out[pix], d1 = v_out[pix + 1], d2 = v_out[pix + 2];
        bool inside;
        z_pos(r, gr, b, g.L, &i0, &i1, &t, &inside);
        const float m[12] = {d0 * r, d0 * gr, d0 * b, d0, d1 * r, d1 * gr, d1 * b, d1, d2 * r, d2 * gr, d2 * b, d2};
#pragma unroll
        for (int l = 0; l < kLev; l++) {
            const float wl = w * vertex_weight(i0, i1, t, l0 + l);
#pragma unroll
            for (int k = 0; k < 12; k++) acc[l][k] += wl * m[k];
        }
    }
    // the lanes of a wave in a fixed shuffle tree, then the four waves in order
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int l = 0; l < kLev; l++)
#pragma unroll
        for (int k = 0; k < 12; k++) {
            float v = acc[l][k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) red[wave][l * 12 + k] = v;
        }
    __syncthreads();
    if (tid < kLev * 12) {
        const float v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        const size_t n_col = (size_t)g.GW * g.GH;
        part[(((size_t)split * n_col + col) * l_pad + l0) * 12 + tid] = v;
    }
}

// ---- grid-side backward, pass 2: the whole gradient [num, 12, L, GH, GW]; the rendered camera's slice = the row slices
// added in order, every other camera's = 0
__global__ __launch_bounds__(256) void grid_bwd_finish_kernel(Geo g, const float* __restrict__ part, int n_split, int l_pad,
                                                              int64_t total, int cam, float* __restrict__ v_grids) {
    const int64_t per_cam = (int64_t)12 * g.L * g.GH * g.GW;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        float v = 0.f;
        if (e / per_cam == cam) {
            const int i = (int)(e - (int64_t)cam * per_cam);       // per_cam <= 12 * 16 * 256 * 256 < 2^31
            const int n_col = g.GH * g.GW;
            const int col = i % n_col, rest = i / n_col, l = rest % g.L, k = rest / g.L;
            for (int s = 0; s < n_split; s++) v += part[(((size_t)s * n_col + col) * l_pad + l) * 12 + k];
        }
        v_grids[e] = v;
    }
}

// ---- TV.  sums[3] per lane in fp64: the squared forward differences along GW, GH and L, each through wgprims.h's block_sum.

__global__ __launch_bounds__(256) void tv_fwd_kernel(Geo g, const float* __restrict__ grids, int64_t total,
                                                     double* __restrict__ partials) {
    __shared__ double red[4];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t row = g.GW, lev = (int64_t)g.GW * g.GH;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const int x = (int)(e % g.GW), y = (int)((e / row) % g.GH), l = (int)((e / lev) % g.L);
        const float v = grids[e];
        if (x + 1 < g.GW) {
            const float d = grids[e + 1] - v;
            sx += (double)(d * d);
        }
        if (y + 1 < g.GH) {
            const float d = grids[e + row] - v;
            sy += (double)(d * d);
        }
        if (l + 1 < g.L) {
            const float d = grids[e + lev] - v;
            sz += (double)(d * d);
        }
    }
    sx = block_sum<4>(sx, red);
    sy = block_sum<4>(sy, red);
    sz = block_sum<4>(sz, red);
    if (threadIdx.x == 0) {
        partials[3 * blockIdx.x] = sx;
        partials[3 * blockIdx.x + 1] = sy;
        partials[3 * blockIdx.x + 2] = sz;
    }
}

__device__ __forceinline__ double axis_count(int n_axis, int a, int b) {
    return 12.0 * (double)(n_axis - 1) * (double)a * (double)b;
}

__global__ __launch_bounds__(256) void tv_finish_kernel(Geo g, int num, const double* __restrict__ partials, int n_part,
                                                        float* __restrict__ loss) {
    __shared__ double red[4];
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n_part; i += 256)
        for (int a = 0; a < 3; a++) s[a] += partials[3 * i + a];
    const double sx = block_sum<4>(s[0], red), sy = block_sum<4>(s[1], red), sz = block_sum<4>(s[2], red);
    if (threadIdx.x == 0) {
        double tv = 0.0;
        if (g.GW > 1) tv += sx / axis_count(g.GW, g.GH, g.L);
        if (g.GH > 1) tv += sy / axis_count(g.GH, g.GW, g.L);
        if (g.L > 1) tv += sz / axis_count(g.L, g.GH, g.GW);
        *loss = (float)(tv / (double)num);
    }
}

__global__ __launch_bounds__(256) void tv_bwd_kernel(Geo g, int num, const float* __restrict__ grids, int64_t total,
                                                     const float* __restrict__ v_loss, float* __restrict__ v_grids) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t row = g.GW, lev = (int64_t)g.GW * g.GH;
    const float up = *v_loss;
    // d tv / d G[e] = (2 / num) sum_axis ((G[e] - G[e - 1]) - (G[e + 1] - G[e])) / count_axis, absent neighbours dropped
    const float kx = g.GW > 1 ? (float)(2.0 / ((double)num * axis_count(g.GW, g.GH, g.L))) : 0.f;
    const float ky = g.GH > 1 ? (float)(2.0 / ((double)num * axis_count(g.GH, g.GW, g.L))) : 0.f;
    const float kz = g.L > 1 ? (float)(2.0 / ((double)num * axis_count(g.L, g.GH, g.GW))) : 0.f;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const int x = (int)(e % g.GW), y = (int)((e / row) % g.GH), l = (int)((e / lev) % g.L);
        const float v = grids[e];
        float ax = 0.f, ay = 0.f, az = 0.f;
        if (x > 0) ax += v - grids[e - 1];
        if (x + 1 < g.GW) ax -= grids[e + 1] - v;
        if (y > 0) ay += v - grids[e - row];
        if (y + 1 < g.GH) ay -= grids[e + row] - v;
        if (l > 0) az += v - grids[e - lev];
        if (l + 1 < g.L) az -= grids[e + lev] - v;
        v_grids[e] = up * ((kx * ax + ky * ay) + kz * az);
    }
}

int split_count(int H, int W, int GW, int GH) {
    // a typical support: two cells each way (+ the margins of support())
    const int64_t rows = GH > 1 ? std::min<int64_t>(H, 2 * (int64_t)(H - 1) / (GH - 1) + 3) : H;
    const int64_t cols = GW > 1 ? std::min<int64_t>(W, 2 * (int64_t)(W - 1) / (GW - 1) + 3) : W;
    int64_t s = (rows * cols + kSplitPixels - 1) / kSplitPixels;
    s = std::min<int64_t>(s, std::min<int64_t>(kMaxSplit, rows));
    return (int)std::max<int64_t>(s, 1);
}

int stream_blocks(int64_t total) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, MISPLAT_BILAGRID_TV_BLOCKS));
}

}  // namespace

extern "C" {

int64_t misplat_bilagrid_scratch_floats(int32_t height, int32_t width, int32_t grid_w, int32_t grid_h, int32_t grid_l) {
    if (!geo_ok(height, width, grid_w, grid_h, grid_l)) return -1;
    const int64_t l_pad = (int64_t)((grid_l + kLev - 1) / kLev) * kLev;
    return (int64_t)split_count(height, width, grid_w, grid_h) * grid_w * grid_h * l_pad * 12;
}

int misplat_bilagrid_slice_fwd(int32_t height, int32_t width, const float* rgb, const float* grid, int32_t grid_w, int32_t grid_h,
                               int32_t grid_l, float* out, misplat_stream_t stream) {
    if (!geo_ok(height, width, grid_w, grid_h, grid_l) || !rgb || !grid || !out) return MISPLAT_EINVAL;
    const Geo g{height, width, grid_w, grid_h, grid_l};
    const dim3 blocks((width + kTileW - 1) / kTileW, (height + kTileH - 1) / kTileH);
    hipLaunchKernelGGL(slice_kernel<false>, blocks, dim3(256), 0, (hipStream_t)stream, g, rgb, grid, (const float*)nullptr, out);
    return launched();
}

int misplat_bilagrid_slice_bwd(int32_t height, int32_t width, const float* rgb, const float* grids, int32_t num, int32_t cam,
                               int32_t grid_w, int32_t grid_h, int32_t grid_l, const float* v_out, float* v_rgb, float* v_grids,
                               float* scratch, misplat_stream_t stream) {
    if (!geo_ok(height, width, grid_w, grid_h, grid_l) || num < 1 || cam < 0 || cam >= num || !rgb || !grids || !v_out || !v_rgb ||
        !v_grids || !scratch)
        return MISPLAT_EINVAL;
    const Geo g{height, width, grid_w, grid_h, grid_l};
    const int64_t per_cam = (int64_t)12 * grid_l * grid_h * grid_w;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 blocks((width + kTileW - 1) / kTileW, (height + kTileH - 1) / kTileH);
    hipLaunchKernelGGL(slice_kernel<true>, blocks, dim3(256), 0, s, g, rgb, grids + (int64_t)cam * per_cam, v_out, v_rgb);
    if (launched() != MISPLAT_OK) return MISPLAT_ELAUNCH;
    const int n_split = split_count(height, width, grid_w, grid_h), chunks = (grid_l + kLev - 1) / kLev;
    hipLaunchKernelGGL(grid_bwd_kernel, dim3(grid_w * grid_h, n_split, chunks), dim3(256), 0, s, g, rgb, v_out, scratch, n_split,
                       chunks * kLev);
    if (launched() != MISPLAT_OK) return MISPLAT_ELAUNCH;
    const int64_t total = per_cam * num;
    hipLaunchKernelGGL(grid_bwd_finish_kernel, dim3(stream_blocks(total) * 2), dim3(256), 0, s, g, (const float*)scratch, n_split,
                       chunks * kLev, total, cam, v_grids);
    return launched();
}

int misplat_bilagrid_tv_fwd(const float* grids, int32_t num, int32_t grid_w, int32_t grid_h, int32_t grid_l, double* partials,
                            float* loss, misplat_stream_t stream) {
    if (!geo_ok(1, 1, grid_w, grid_h, grid_l) || num < 1 || !grids || !partials || !loss) return MISPLAT_EINVAL;
    const Geo g{1, 1, grid_w, grid_h, grid_l};
    const int64_t total = (int64_t)12 * grid_l * grid_h * grid_w * num;
    const int n_part = stream_blocks(total);
    hipLaunchKernelGGL(tv_fwd_kernel, dim3(n_part), dim3(256), 0, (hipStream_t)stream, g, grids, total, partials);
    if (launched() != MISPLAT_OK) return MISPLAT_ELAUNCH;
    hipLaunchKernelGGL(tv_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, g, num, (const double*)partials, n_part, loss);
    return launched();
}

int misplat_bilagrid_tv_bwd(const float* grids, int32_t num, int32_t grid_w, int32_t grid_h, int32_t grid_l, const float* v_loss,
                            float* v_grids, misplat_stream_t stream) {
    if (!geo_ok(1, 1, grid_w, grid_h, grid_l) || num < 1 || !grids || !v_loss || !v_grids) return MISPLAT_EINVAL;
    const Geo g{1, 1, grid_w, grid_h, grid_l};
    const int64_t total = (int64_t)12 * grid_l * grid_h * grid_w * num;
    hipLaunchKernelGGL(tv_bwd_kernel, dim3(stream_blocks(total) * 2), dim3(256), 0, (hipStream_t)stream, g, num, grids, total, v_loss,
                       v_grids);
    return launched();
}

}  // extern "C"
