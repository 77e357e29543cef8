// poisson.hip -- dense-grid screened Poisson surface reconstruction of an oriented point cloud.
//
// Semantics: a restated uniform-grid solve (tests/poisson_restatement.py is the oracle); neither Kazhdan's adaptive octree nor
// Open3D's code.  Compiled with -ffp-contract=off; every fp32 expression of the splat, the system and the sampler is evaluated
// in the written order, so the int64 grids, b and D equal the restatement's bit for bit.
//
// Grid: G = 2^depth cells per axis, cell (i, j, k) has its centre at o + (idx + 0.5) h, linear index i + G (j + G k).
// Pipeline: splat (int64 fixed-point atomics) -> system (W, b, D) -> Jacobi-preconditioned CG (stencil / update / direction,
// each dot product a fixed two-level reduction) -> sample (iso value, vertex density and colour) -> pool (chi - iso laid out as
// a fully allocated TSDF unit map, which misplat_tsdf_mc_count / misplat_tsdf_mc_emit extract).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"
#include "wgprims.h"
#include "unitgrid.h"

namespace {

constexpr int kBlock = 256;
constexpr int kCellsPerBlock = 1024;                  // 4 consecutive cells per lane
constexpr int kFinal = 1024;                          // threads of the one workgroup that sums the partials
constexpr float kFix = 1073741824.f;                  // 2^30: the fixed point of the splat
constexpr float kInvFix = 1.f / 1073741824.f;

// solver state: 8 doubles at the head of the workspace
enum { S_RZ = 0, S_PAP, S_RR, S_BB, S_ALPHA, S_BETA, S_DONE, S_ITERS };
constexpr int64_t kStateBytes = 64, kSumsBytes = 64;  // state, then {sum of W, cells with W > 0} as uint64

// the one-workgroup second level: thread t adds partials t, t + 1024, ... in ascending order, then wgprims.h's block_sum (the
// workgroup sum in a fixed tree; every thread gets it).  A device function, not sum_final_kernel: the callers go on computing.
__device__ __forceinline__ double final_sum(const double* __restrict__ partials, int64_t n, double* sh) {
    double v = 0.0;
#pragma unroll 8
    for (int64_t i = threadIdx.x; i < n; i += kFinal) v += partials[i];      // (unrolled: the loads of 8 steps are in flight together)
    return block_sum<kFinal / 64>(v, sh);
}

// two sums at once (their loads overlap); each in final_sum's order
__device__ __forceinline__ void final_sum2(const double* __restrict__ pa, const double* __restrict__ pb, int64_t n, double* sh,
                                           double& sa, double& sb) {
    double va = 0.0, vb = 0.0;
#pragma unroll 8
    for (int64_t i = threadIdx.x; i < n; i += kFinal) { va += pa[i]; vb += pb[i]; }
    sa = block_sum<kFinal / 64>(va, sh);
    sb = block_sum<kFinal / 64>(vb, sh);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// --------------------------------------------------------------------------------------------------------------- splat
// One thread per point: g = (p - o) / h - 0.5, i0 = floor(g), f = g - i0; corner weight w = (wx wy) wz; W += w, V_a += w n_a,
// C_c += w c_c as q = llrint(x 2^30) with 64-bit integer atomics (exact, order-free).  Corner indices are clamped to the grid.
__global__ __launch_bounds__(kBlock) void poisson_splat_kernel(const float* __restrict__ points, const float* __restrict__ normals,
                                                               const float* __restrict__ colors, int64_t n, int G, float ox, float oy,
                                                               float oz, float h, unsigned long long* __restrict__ Wq,
                                                               unsigned long long* __restrict__ Vq,
                                                               unsigned long long* __restrict__ Cq) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float o[3] = {ox, oy, oz};
    int i0[3];
    float f[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float g = (points[3 * i + a] - o[a]) / h - 0.5f;
        const float fl = floorf(g);
        i0[a] = (int)fl;
        f[a] = g - fl;
    }
    float ch[6];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        ch[a] = normals[3 * i + a];
        ch[3 + a] = colors ? colors[3 * i + a] : 0.f;
    }
    const int64_t n3 = (int64_t)G * G * G;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
        const float wx = dx ? f[0] : 1.f - f[0], wy = dy ? f[1] : 1.f - f[1], wz = dz ? f[2] : 1.f - f[2];
        const float w = (wx * wy) * wz;
        const int64_t cell = (int64_t)clampi(i0[0] + dx, 0, G - 1) +
                             (int64_t)G * (clampi(i0[1] + dy, 0, G - 1) + (int64_t)G * clampi(i0[2] + dz, 0, G - 1));
        const long long qw = llrintf(w * kFix);
        if (qw != 0) atomicAdd(&Wq[cell], (unsigned long long)qw);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const long long q = llrintf((w * ch[a]) * kFix);
            if (q != 0) atomicAdd(&Vq[a * n3 + cell], (unsigned long long)q);
        }
        if (colors) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const long long q = llrintf((w * ch[3 + a]) * kFix);
                if (q != 0) atomicAdd(&Cq[a * n3 + cell], (unsigned long long)q);
            }
        }
    }
}

// sums[0] += sum of Wq, sums[1] += cells with Wq > 0: integer, so exact in any order
__global__ __launch_bounds__(kBlock) void poisson_wsum_kernel(const long long* __restrict__ Wq, unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long sh[2][kBlock / 64];
    const int64_t c = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
    unsigned long long s = 0ull, k = 0ull;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const long long q = Wq[c + j];
        s += (unsigned long long)q;
        k += q > 0 ? 1ull : 0ull;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off);
        k += __shfl_down(k, off);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sh[0][wave] = s; sh[1][wave] = k; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&sums[0], sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3]);
        atomicAdd(&sums[1], sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3]);
    }
}

// -------------------------------------------------------------------------------------------------------------- system
// W = float(Wq) 2^-30; wbar = float((double(sum Wq) 2^-30) / double(#{Wq > 0})); D = float(in-grid neighbours) + (pw W) / wbar;
// b = -0.5 ((dVx + dVy) + dVz), dV_a = V_a(i + e_a) - V_a(i - e_a) with V = float(Vq) 2^-30 and 0 outside the grid.
__global__ __launch_bounds__(kBlock) void poisson_system_kernel(const long long* __restrict__ Wq, const long long* __restrict__ Vq,
                                                                const unsigned long long* __restrict__ sums, int depth, float pw,
                                                                float* __restrict__ W, float* __restrict__ b, float* __restrict__ D) {
    const int G = 1 << depth;
    const int64_t n3 = (int64_t)1 << (3 * depth);
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int x = (int)(c & (G - 1)), y = (int)((c >> depth) & (G - 1)), z = (int)(c >> (2 * depth));
    const int64_t step[3] = {1, (int64_t)G, (int64_t)G * G};
    const int pos[3] = {x, y, z};
    const float w = (float)Wq[c] * kInvFix;
    const unsigned long long cnt = sums[1];
    int nn = 0;
    float dv[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const bool up = pos[a] < G - 1, dn = pos[a] > 0;
        nn += (up ? 1 : 0) + (dn ? 1 : 0);
        const float vp = up ? (float)Vq[a * n3 + c + step[a]] * kInvFix : 0.f;
        const float vm = dn ? (float)Vq[a * n3 + c - step[a]] * kInvFix : 0.f;
        dv[a] = vp - vm;
    }
    float d = (float)nn;
    if (cnt > 0ull) {
        const float wbar = (float)(((double)sums[0] * (1.0 / 1073741824.0)) / (double)cnt);
        d = d + (pw * w) / wbar;
    }
    W[c] = w;
    D[c] = d;
    b[c] = -0.5f * ((dv[0] + dv[1]) + dv[2]);
}

// ------------------------------------------------------------------------------------------------------------------ CG
__device__ __forceinline__ float4 ld4(const float* __restrict__ p, int64_t i) { return *reinterpret_cast<const float4*>(p + i); }
__device__ __forceinline__ void st4(float* __restrict__ p, int64_t i, float4 v) { *reinterpret_cast<float4*>(p + i) = v; }

// x = 0, r = b, z = r / D, p = z; partials of r.z and b.b
__global__ __launch_bounds__(kBlock) void cg_init_kernel(const float* __restrict__ b, const float* __restrict__ D, float* __restrict__ x,
                                                         float* __restrict__ r, float* __restrict__ z, float* __restrict__ p,
                                                         double* __restrict__ partials, int64_t nb) {
    __shared__ double sh[kBlock / 64];
    const int64_t c = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
    const float4 bv = ld4(b, c), dv = ld4(D, c);
    const float4 zv = make_float4(bv.x / dv.x, bv.y / dv.y, bv.z / dv.z, bv.w / dv.w);
    st4(x, c, make_float4(0.f, 0.f, 0.f, 0.f));
    st4(r, c, bv);
    st4(z, c, zv);
    st4(p, c, zv);
    const double rz = (((double)bv.x * zv.x + (double)bv.y * zv.y) + (double)bv.z * zv.z) + (double)bv.w * zv.w;
    const double bb = (((double)bv.x * bv.x + (double)bv.y * bv.y) + (double)bv.z * bv.z) + (double)bv.w * bv.w;
    const double s0 = block_sum<kBlock / 64>(rz, sh), s1 = block_sum<kBlock / 64>(bb, sh);
    if (threadIdx.x == 0) { partials[blockIdx.x] = s0; partials[nb + blockIdx.x] = s1; }
}

__global__ __launch_bounds__(kFinal) void cg_init_reduce_kernel(const double* __restrict__ partials, int64_t nb, double* __restrict__ state,
                                                                int max_iters) {
    __shared__ double sh[kFinal / 64];
    double rz, bb;
    final_sum2(partials, partials + nb, nb, sh, rz, bb);
    if (threadIdx.x == 0) {
        state[S_RZ] = rz; state[S_PAP] = 0.0; state[S_RR] = bb; state[S_BB] = bb; state[S_ALPHA] = 0.0; state[S_BETA] = 0.0;
        state[S_ITERS] = 0.0;
        state[S_DONE] = bb == 0.0 ? 1.0 : (max_iters <= 0 ? 2.0 : 0.0);      // b = 0: chi = 0 is the solution
    }
}

// Ap = D p - (the in-grid neighbours of p); partials of p.Ap.  A lane holds 4 cells of one x row.
__global__ __launch_bounds__(kBlock) void cg_stencil_kernel(const float* __restrict__ p, const float* __restrict__ D, float* __restrict__ Ap,
                                                            double* __restrict__ partials, const double* __restrict__ state, int depth) {
    __shared__ double sh[kBlock / 64];
    if (state[S_DONE] != 0.0) return;
    const int G = 1 << depth;
    const int64_t c = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
    const int x = (int)(c & (G - 1)), y = (int)((c >> depth) & (G - 1)), z = (int)(c >> (2 * depth));
    const int64_t sy = G, sz = (int64_t)G * G;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 pc = ld4(p, c), dv = ld4(D, c);
    const float xm = x > 0 ? p[c - 1] : 0.f, xp = x + 4 < G ? p[c + 4] : 0.f;
    const float4 ym = y > 0 ? ld4(p, c - sy) : zero, yp = y < G - 1 ? ld4(p, c + sy) : zero;
    const float4 zm = z > 0 ? ld4(p, c - sz) : zero, zp = z < G - 1 ? ld4(p, c + sz) : zero;
    float4 a;
    a.x = dv.x * pc.x - (((((xm + pc.y) + ym.x) + yp.x) + zm.x) + zp.x);
    a.y = dv.y * pc.y - (((((pc.x + pc.z) + ym.y) + yp.y) + zm.y) + zp.y);
    a.z = dv.z * pc.z - (((((pc.y + pc.w) + ym.z) + yp.z) + zm.z) + zp.z);
    a.w = dv.w * pc.w - (((((pc.z + xp) + ym.w) + yp.w) + zm.w) + zp.w);
    st4(Ap, c, a);
    const double d = (((double)pc.x * a.x + (double)pc.y * a.y) + (double)pc.z * a.z) + (double)pc.w * a.w;
    const double s = block_sum<kBlock / 64>(d, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// alpha = r.z / p.Ap; p.Ap = 0 or r.z = 0 ends the solve (no 0 / 0 is ever formed)
__global__ __launch_bounds__(kFinal) void cg_alpha_kernel(const double* __restrict__ partials, int64_t nb, double* __restrict__ state) {
    __shared__ double sh[kFinal / 64];
    if (state[S_DONE] != 0.0) return;
    const double pAp = final_sum(partials, nb, sh);
    if (threadIdx.x == 0) {
        const double rz = state[S_RZ];
        state[S_PAP] = pAp;
        if (pAp == 0.0 || rz == 0.0) {
            state[S_ALPHA] = 0.0;
            state[S_DONE] = 3.0;
        } else {
            state[S_ALPHA] = (double)(float)(rz / pAp);
        }
    }
}

// x += alpha p, r -= alpha Ap, z = r / D; partials of r.z and r.r
__global__ __launch_bounds__(kBlock) void cg_update_kernel(float* __restrict__ x, float* __restrict__ r, float* __restrict__ z,
                                                           const float* __restrict__ p, const float* __restrict__ Ap,
                                                           const float* __restrict__ D, double* __restrict__ partials, int64_t nb,
                                                           const double* __restrict__ state) {
    __shared__ double sh[kBlock / 64];
    if (state[S_DONE] != 0.0) return;
    const float alpha = (float)state[S_ALPHA];
    const int64_t c = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
    float4 xv = ld4(x, c), rv = ld4(r, c);
    const float4 pv = ld4(p, c), av = ld4(Ap, c), dv = ld4(D, c);
    xv.x = xv.x + alpha * pv.x; xv.y = xv.y + alpha * pv.y; xv.z = xv.z + alpha * pv.z; xv.w = xv.w + alpha * pv.w;
    rv.x = rv.x - alpha * av.x; rv.y = rv.y - alpha * av.y; rv.z = rv.z - alpha * av.z; rv.w = rv.w - alpha * av.w;
    const float4 zv = make_float4(rv.x / dv.x, rv.y / dv.y, rv.z / dv.z, rv.w / dv.w);
    st4(x, c, xv);
    st4(r, c, rv);
    st4(z, c, zv);
    const double rz = (((double)rv.x * zv.x + (double)rv.y * zv.y) + (double)rv.z * zv.z) + (double)rv.w * zv.w;
    const double rr = (((double)rv.x * rv.x + (double)rv.y * rv.y) + (double)rv.z * rv.z) + (double)rv.w * rv.w;
    const double s0 = block_sum<kBlock / 64>(rz, sh), s1 = block_sum<kBlock / 64>(rr, sh);
    if (threadIdx.x == 0) { partials[blockIdx.x] = s0; partials[nb + blockIdx.x] = s1; }
}

// beta = (r.z)_new / (r.z)_old; the iteration count; done = 1 once r.r <= tol^2 b.b, 2 at the iteration cap
__global__ __launch_bounds__(kFinal) void cg_beta_kernel(const double* __restrict__ partials, int64_t nb, double* __restrict__ state,
                                                         double tol2, int max_iters) {
    __shared__ double sh[kFinal / 64];
    if (state[S_DONE] != 0.0) return;
    double rz, rr;
    final_sum2(partials, partials + nb, nb, sh, rz, rr);
    if (threadIdx.x == 0) {
        const double iters = state[S_ITERS] + 1.0;
        state[S_BETA] = (double)(float)(rz / state[S_RZ]);               // (the old r.z is not 0: cg_alpha_kernel ended the solve)
        state[S_RZ] = rz;
        state[S_RR] = rr;
        state[S_ITERS] = iters;
        if (rr <= tol2 * state[S_BB]) state[S_DONE] = 1.0;
        else if (iters >= (double)max_iters) state[S_DONE] = 2.0;
    }
}

// p = z + beta p
__global__ __launch_bounds__(kBlock) void cg_direction_kernel(const float* __restrict__ z, float* __restrict__ p,
                                                              const double* __restrict__ state) {
    if (state[S_DONE] != 0.0) return;
    const float beta = (float)state[S_BETA];
    const int64_t c = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
    const float4 zv = ld4(z, c);
    float4 pv = ld4(p, c);
    pv.x = zv.x + beta * pv.x; pv.y = zv.y + beta * pv.y; pv.z = zv.z + beta * pv.z; pv.w = zv.w + beta * pv.w;
    st4(p, c, pv);
}

// -------------------------------------------------------------------------------------------------------------- sample
// Trilinear reads of cell-centred fields at world positions: g = (q - o) / h - 0.5, i0 = floor(g) clamped to 0 .. G - 2, f = g - i0
// clamped to [0, 1]; along x: v0 (1 - fx) + v1 fx, then y, then z.  One thread per query, all channels.
__global__ __launch_bounds__(kBlock) void poisson_sample_kernel(const float* __restrict__ field, int nch, int G, float ox, float oy,
                                                                float oz, float h, const float* __restrict__ queries, int64_t nq,
                                                                float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nq) return;
    const float o[3] = {ox, oy, oz};
    int i0[3];
    float f[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float g = (queries[3 * i + a] - o[a]) / h - 0.5f;
        float fl = floorf(g);
        fl = fl < 0.f ? 0.f : (fl > (float)(G - 2) ? (float)(G - 2) : fl);
        i0[a] = (int)fl;
        float t = g - fl;
        t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
        f[a] = t;
    }
    const int64_t sy = G, sz = (int64_t)G * G, n3 = sz * G;
    const int64_t base = i0[0] + sy * i0[1] + sz * i0[2];
    const float gx = 1.f - f[0], gy = 1.f - f[1], gz = 1.f - f[2];
    for (int ch = 0; ch < nch; ch++) {
        const float* __restrict__ F = field + ch * n3 + base;
        const float x00 = F[0] * gx + F[1] * f[0], x10 = F[sy] * gx + F[sy + 1] * f[0];
        const float x01 = F[sz] * gx + F[sz + 1] * f[0], x11 = F[sz + sy] * gx + F[sz + sy + 1] * f[0];
        const float y0 = x00 * gy + x10 * f[1], y1 = x01 * gy + x11 * f[1];
        out[i * nch + ch] = y0 * gz + y1 * f[2];
    }
}

// partials[b] = the fp64 sum of values 1024 b .. 1024 b + 1023 (those below n) in the fixed tree
__global__ __launch_bounds__(kBlock) void mean_partial_kernel(const float* __restrict__ values, int64_t n, double* __restrict__ partials) {
    __shared__ double sh[kBlock / 64];
    const int64_t c = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) v += c + j < n ? (double)values[c + j] : 0.0;
    const double s = block_sum<kBlock / 64>(v, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(kFinal) void mean_final_kernel(const double* __restrict__ partials, int64_t nb, int64_t n, double* __restrict__ out) {
    __shared__ double sh[kFinal / 64];
    const double s = final_sum(partials, nb, sh);
    if (threadIdx.x == 0) out[0] = s / (double)n;
}

// ---------------------------------------------------------------------------------------------------------------- pool
// chi - float(iso) as the tsdf plane of a fully allocated unit map (unit u = ux + U (uy + U uz), slot = u, voxel i = lx + 16 ly + 256
// lz), weight 1, colour 0: the layout misplat_tsdf_mc_count / _emit read.  One thread per voxel in pool order.
__global__ __launch_bounds__(kBlock) void poisson_pool_kernel(const float* __restrict__ chi, int depth, float iso, float* __restrict__ pool) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t slot = t / kUnitVoxels;
    const int i = (int)(t % kUnitVoxels);
    const int U = 1 << (depth - 4);
    const int ux = (int)(slot % U), uy = (int)((slot / U) % U), uz = (int)(slot / ((int64_t)U * U));
    const int64_t x = ux * 16 + (i & 15), y = uy * 16 + ((i >> 4) & 15), z = uz * 16 + (i >> 8);
    const float v = chi[x + (y << depth) + (z << (2 * depth))] - iso;
    float* __restrict__ base = pool + pool_index(slot, 0, 0) + i;
    base[0] = v;
    base[kUnitVoxels] = 1.f;
#pragma unroll
    for (int c = 2; c < kPlanes; c++) base[c * kUnitVoxels] = 0.f;
}

inline bool depth_ok(int32_t depth) { return depth >= MISPLAT_POISSON_MIN_DEPTH && depth <= MISPLAT_POISSON_MAX_DEPTH; }
inline int64_t cells(int32_t depth) { return (int64_t)1 << (3 * depth); }
inline int64_t partial_count(int32_t depth, int64_t n_points) {
    const int64_t a = cells(depth) / kCellsPerBlock, b = (n_points + kCellsPerBlock - 1) / kCellsPerBlock;
    return a > b ? a : b;
}
inline int64_t workspace_bytes(int32_t depth, int64_t n_points) {
    return kStateBytes + kSumsBytes + 2 * partial_count(depth, n_points) * (int64_t)sizeof(double);
}
inline double* ws_state(void* ws) { return (double*)ws; }
inline unsigned long long* ws_sums(void* ws) { return (unsigned long long*)((char*)ws + kStateBytes); }
inline double* ws_partials(void* ws) { return (double*)((char*)ws + kStateBytes + kSumsBytes); }
inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace

extern "C" int64_t misplat_poisson_workspace(int32_t depth, int64_t n_points) {
    if (!depth_ok(depth) || n_points < 0 || n_points >= (1ll << 31)) return -1;
    return workspace_bytes(depth, n_points);
}

extern "C" int misplat_poisson_splat(const float* points, const float* normals, const float* colors, int64_t n_points, int32_t depth,
                                     float origin_x, float origin_y, float origin_z, float h, int64_t* w_grid, int64_t* v_grid,
                                     int64_t* c_grid, misplat_stream_t stream) {
    if (!depth_ok(depth) || n_points < 1 || n_points >= (1ll << 31) || !points || !normals || !w_grid || !v_grid ||
        (colors && !c_grid) || !(h > 0.f))
        return MISPLAT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n3 = cells(depth);
    if (hipMemsetAsync(w_grid, 0, n3 * sizeof(int64_t), s) != hipSuccess) return MISPLAT_ELAUNCH;
    if (hipMemsetAsync(v_grid, 0, 3 * n3 * sizeof(int64_t), s) != hipSuccess) return MISPLAT_ELAUNCH;
    if (colors && hipMemsetAsync(c_grid, 0, 3 * n3 * sizeof(int64_t), s) != hipSuccess) return MISPLAT_ELAUNCH;
    hipLaunchKernelGGL(poisson_splat_kernel, dim3((unsigned)((n_points + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, points, normals,
                       colors, n_points, 1 << depth, origin_x, origin_y, origin_z, h, (unsigned long long*)w_grid,
                       (unsigned long long*)v_grid, (unsigned long long*)c_grid);
    return launched();
}

extern "C" int misplat_poisson_system(const int64_t* w_grid, const int64_t* v_grid, int32_t depth, float point_weight, void* workspace,
                                      int64_t workspace_bytes_, float* w, float* b, float* d, misplat_stream_t stream) {
    if (!depth_ok(depth) || !w_grid || !v_grid || !workspace || !w || !b || !d || !(point_weight >= 0.f) ||
        workspace_bytes_ < workspace_bytes(depth, 0))
        return MISPLAT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n3 = cells(depth);
    if (hipMemsetAsync(ws_sums(workspace), 0, kSumsBytes, s) != hipSuccess) return MISPLAT_ELAUNCH;
    hipLaunchKernelGGL(poisson_wsum_kernel, dim3((unsigned)(n3 / kCellsPerBlock)), dim3(kBlock), 0, s, (const long long*)w_grid,
                       ws_sums(workspace));
    hipLaunchKernelGGL(poisson_system_kernel, dim3((unsigned)(n3 / kBlock)), dim3(kBlock), 0, s, (const long long*)w_grid,
                       (const long long*)v_grid, (const unsigned long long*)ws_sums(workspace), (int)depth, point_weight, w, b, d);
    return launched();
}

extern "C" int misplat_poisson_cg_init(const float* b, const float* d, int32_t depth, int32_t max_iters, void* workspace,
                                       int64_t workspace_bytes_, float* x, float* r, float* z, float* p, misplat_stream_t stream) {
    if (!depth_ok(depth) || !b || !d || !workspace || !x || !r || !z || !p || max_iters < 0 ||
        workspace_bytes_ < workspace_bytes(depth, 0) || !aligned16(b) || !aligned16(d) || !aligned16(x) || !aligned16(r) ||
        !aligned16(z) || !aligned16(p))
        return MISPLAT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = cells(depth) / kCellsPerBlock;
    hipLaunchKernelGGL(cg_init_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, b, d, x, r, z, p, ws_partials(workspace), nb);
    hipLaunchKernelGGL(cg_init_reduce_kernel, dim3(1), dim3(kFinal), 0, s, (const double*)ws_partials(workspace), nb,
                       ws_state(workspace), (int)max_iters);
    return launched();
}

extern "C" int misplat_poisson_cg_iterate(const float* d, int32_t depth, int32_t n_iters, double tol, int32_t max_iters,
                                          void* workspace, int64_t workspace_bytes_, float* x, float* r, float* z, float* p,
                                          float* ap, misplat_stream_t stream) {
    if (!depth_ok(depth) || !d || !workspace || !x || !r || !z || !p || !ap || n_iters < 0 || n_iters > 4096 || max_iters < 0 ||
        !(tol >= 0.0) || workspace_bytes_ < workspace_bytes(depth, 0) || !aligned16(d) || !aligned16(x) || !aligned16(r) ||
        !aligned16(z) || !aligned16(p) || !aligned16(ap))
        return MISPLAT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = cells(depth) / kCellsPerBlock;
    double* state = ws_state(workspace);
    double* partials = ws_partials(workspace);
    for (int it = 0; it < n_iters; it++) {
        hipLaunchKernelGGL(cg_stencil_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, (const float*)p, d, ap, partials,
                           (const double*)state, (int)depth);
        hipLaunchKernelGGL(cg_alpha_kernel, dim3(1), dim3(kFinal), 0, s, (const double*)partials, nb, state);
        hipLaunchKernelGGL(cg_update_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, x, r, z, (const float*)p, (const float*)ap, d,
                           partials, nb, (const double*)state);
        hipLaunchKernelGGL(cg_beta_kernel, dim3(1), dim3(kFinal), 0, s, (const double*)partials, nb, state, tol * tol, (int)max_iters);
        hipLaunchKernelGGL(cg_direction_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, (const float*)z, p, (const double*)state);
    }
    return launched();
}

extern "C" int misplat_poisson_sample(const float* field, int32_t n_channels, int32_t depth, float origin_x, float origin_y,
                                      float origin_z, float h, const float* queries, int64_t n_queries, float* out,
                                      misplat_stream_t stream) {
    if (!depth_ok(depth) || !field || n_channels < 1 || n_channels > 16 || n_queries < 0 || n_queries >= (1ll << 31) || !(h > 0.f) ||
        (n_queries > 0 && (!queries || !out)))
        return MISPLAT_EINVAL;
    if (n_queries == 0) return MISPLAT_OK;
    hipLaunchKernelGGL(poisson_sample_kernel, dim3((unsigned)((n_queries + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       field, (int)n_channels, 1 << depth, origin_x, origin_y, origin_z, h, queries, n_queries, out);
    return launched();
}

extern "C" int misplat_poisson_mean(const float* values, int64_t n, void* workspace, int64_t workspace_bytes_, double* mean,
                                    misplat_stream_t stream) {
    if (!values || n < 1 || n >= (1ll << 31) || !workspace || !mean) return MISPLAT_EINVAL;
    const int64_t nb = (n + kCellsPerBlock - 1) / kCellsPerBlock;
    if (workspace_bytes_ < kStateBytes + kSumsBytes + nb * (int64_t)sizeof(double)) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mean_partial_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, values, n, ws_partials(workspace));
    hipLaunchKernelGGL(mean_final_kernel, dim3(1), dim3(kFinal), 0, s, (const double*)ws_partials(workspace), nb, n, mean);
    return launched();
}

extern "C" int misplat_poisson_mc_pool(const float* chi, int32_t depth, float iso, float* pool, misplat_stream_t stream) {
    if (!depth_ok(depth) || !chi || !pool) return MISPLAT_EINVAL;
    hipLaunchKernelGGL(poisson_pool_kernel, dim3((unsigned)(cells(depth) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, chi,
                       (int)depth, iso, pool);
    return launched();
}
