// density.hip -- the density of the Gaussian mixture itself on the TSDF volume's lattice, and at arbitrary points (DESIGN.md
// section 25), and the search for its level sets along rays (section 26).
//
// Field (restated from the published definition, SuGaR's density; tests/density_restatement.py holds the fp64 oracle and the
// fp32 restatement of everything integer here): with R = R(q / |q|) (columns e_a), m_g(x) = sum_a ((e_a . (x - mu)) / s_a)^2,
//   k_g(x) = o_g (exp(-m_g / 2) - exp(-r^2 / 2))  where m_g < r^2, else 0      (continuous at the cut-off r)
//   d(x) = sum_g k_g(x) in ascending g,   grad d(x) = -sum_{m_g < r^2} o_g exp(-m_g / 2) A_g^T A_g (x - mu_g),  A = diag(1 / s) R^T.
//
// Lattice: the TSDF volume's (csrc/unitgrid.h), h its voxel size and L = fl32(16 h) its unit length; plane 0 of the pool takes
// d, plane 1 the weight 1, planes 2..4 zero, so misplat_tsdf_mc_count / _emit extract level sets of it unchanged.
//
// Lists: a Gaussian reaches a unit by a conservative test evaluated in fp32 in the written order (compiled with
// -ffp-contract=off, as every binning-like file), so the integer structures equal the restatement's bit for bit:
//   E_i = r sqrt(sum_a (R[i][a] s_a)^2);  range per axis: units floor(((mu_i - E_i) - h) / L) .. floor(((mu_i + E_i) + h) / L),
//   clipped to the map;  slab test: keep unit u iff for each a  |e_a . (c - mu)| <= r s_a + H sum_i |R[i][a]|,
//   c = (u + 0.5) L,  H = 0.5 L + h  (the unit's box widened by one voxel: marching cubes needs all 8 corners of a cell).
// Pipeline: records -> the list layer of unitlists.h (count, emit in Gaussian order, misplat_tsdf_alloc, misplat_unit_lists: the
// sort being stable, every list is ascending in g) -> accumulate.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"
#include "unitlists.h"

namespace {

constexpr int kRec = MISPLAT_DENSITY_REC;
constexpr int kBatch = MISPLAT_DENSITY_BATCH;
using Grid = UnitGrid;

bool make_grid(const misplat_tsdf_grid* p, Grid& g, int64_t& n) { return make_unit_grid(p, g, n) && p->voxel_size < 1e30f; }

inline bool cutoff_ok(float r) { return r > 0.f && r <= 6.f; }

__device__ __forceinline__ bool is_fin(float x) { return fabsf(x) < __builtin_inff(); }

// The Gaussian's frame in the fixed operation order of the restatement.  False: the Gaussian takes no part (opacity below
// min_opacity, a non-finite parameter, a non-positive scale or a zero quaternion).
struct Geom {
    float mu[3], R[3][3], s[3], o, E[3];
};
__device__ __forceinline__ bool gauss_geom(const float* __restrict__ means, const float* __restrict__ quats,
                                           const float* __restrict__ scales, const float* __restrict__ opacities, int64_t g,
                                           float r, float min_opacity, Geom& G) {
    const float w = quats[4 * g], x = quats[4 * g + 1], y = quats[4 * g + 2], z = quats[4 * g + 3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        G.mu[a] = means[3 * g + a];
        G.s[a] = scales[3 * g + a];
        ok = ok && is_fin(G.mu[a]) && is_fin(G.s[a]) && G.s[a] > 0.f;
    }
    G.o = opacities[g];
    ok = ok && is_fin(G.o) && G.o >= min_opacity && is_fin(w) && is_fin(x) && is_fin(y) && is_fin(z);
    const float n = sqrtf(((w * w + x * x) + y * y) + z * z);
    ok = ok && n > 0.f && is_fin(n);
    if (!ok) return false;
    const float qr = w / n, qx = x / n, qy = y / n, qz = z / n;
    G.R[0][0] = 1.f - 2.f * (qy * qy + qz * qz); G.R[0][1] = 2.f * (qx * qy - qr * qz); G.R[0][2] = 2.f * (qx * qz + qr * qy);
    G.R[1][0] = 2.f * (qx * qy + qr * qz); G.R[1][1] = 1.f - 2.f * (qx * qx + qz * qz); G.R[1][2] = 2.f * (qy * qz - qr * qx);
    G.R[2][0] = 2.f * (qx * qz - qr * qy); G.R[2][1] = 2.f * (qy * qz + qr * qx); G.R[2][2] = 1.f - 2.f * (qx * qx + qy * qy);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float a0 = G.R[i][0] * G.s[0], a1 = G.R[i][1] * G.s[1], a2 = G.R[i][2] * G.s[2];
        G.E[i] = r * sqrtf((a0 * a0 + a1 * a1) + a2 * a2);
        ok = ok && is_fin(G.E[i]);
    }
    return ok;
}

// record: [0:3] mu, [3:12] A = diag(1 / s) R^T row-major (A[a][i] = R[i][a] / s_a), [12] o, [13:16] E; a Gaussian that takes
// no part: o = 0, E = -1, the rest 0
__global__ __launch_bounds__(256) void density_records_kernel(const float* __restrict__ means, const float* __restrict__ quats,
                                                              const float* __restrict__ scales,
                                                              const float* __restrict__ opacities, int64_t N, float r,
                                                              float min_opacity, float* __restrict__ records) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= N) return;
    Geom G;
    float rec[kRec];
    if (gauss_geom(means, quats, scales, opacities, g, r, min_opacity, G)) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            rec[a] = G.mu[a];
            rec[13 + a] = G.E[a];
#pragma unroll
            for (int i = 0; i < 3; i++) rec[3 + 3 * a + i] = G.R[i][a] / G.s[a];
        }
        rec[12] = G.o;
    } else {
#pragma unroll
        for (int k = 0; k < 13; k++) rec[k] = 0.f;
        rec[13] = rec[14] = rec[15] = -1.f;
    }
    float4* out = reinterpret_cast<float4*>(records + kRec * g);
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = make_float4(rec[4 * k], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3]);
}

// the clipped unit range of a Gaussian; false: empty
__device__ __forceinline__ bool unit_range(const Grid& g, const Geom& G, int (&lo)[3], int (&hi)[3]) {
    bool any = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        // (clamped before the conversion: a far Gaussian must not overflow the int)
        int l = (int)fminf(fmaxf(floorf(((G.mu[a] - G.E[a]) - g.vs) / g.ulen), -1e6f), 1e6f);
        int h = (int)fminf(fmaxf(floorf(((G.mu[a] + G.E[a]) + g.vs) / g.ulen), -1e6f), 1e6f);
        clamp_units(g, a, l, h);
        lo[a] = l; hi[a] = h;
        any = any && l <= h;
    }
    return any;
}

struct Slabs {
    float bound[3];
};
__device__ __forceinline__ Slabs slab_bounds(const Grid& g, const Geom& G, float r) {
    const float H = 0.5f * g.ulen + g.vs;
    Slabs S;
#pragma unroll
    for (int a = 0; a < 3; a++) S.bound[a] = r * G.s[a] + H * ((fabsf(G.R[0][a]) + fabsf(G.R[1][a])) + fabsf(G.R[2][a]));
    return S;
}
__device__ __forceinline__ bool slab_keep(const Grid& g, const Geom& G, const Slabs& S, int ux, int uy, int uz) {
    const float d0 = ((float)ux + 0.5f) * g.ulen - G.mu[0];
    const float d1 = ((float)uy + 0.5f) * g.ulen - G.mu[1];
    const float d2 = ((float)uz + 0.5f) * g.ulen - G.mu[2];
    bool keep = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float p = (G.R[0][a] * d0 + G.R[1][a] * d1) + G.R[2][a] * d2;
        keep = keep && fabsf(p) <= S.bound[a];
    }
    return keep;
}

// One lane per Gaussian: its pairs (PairSink, unitlists.h), units in z, y, x order (ascending map index)
template <bool EMIT>
__global__ __launch_bounds__(256) void density_pairs_kernel(Grid g, const float* __restrict__ means, const float* __restrict__ quats,
                                                            const float* __restrict__ scales, const float* __restrict__ opacities,
                                                            int64_t N, float r, float min_opacity, PairBufs bufs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    Geom G;
    int lo[3], hi[3];
    PairSink<EMIT> sink(bufs);
    if (gauss_geom(means, quats, scales, opacities, i, r, min_opacity, G) && unit_range(g, G, lo, hi)) {
        const Slabs S = slab_bounds(g, G, r);
        sink.open(i);
        for (int uz = lo[2]; uz <= hi[2]; uz++)
            for (int uy = lo[1]; uy <= hi[1]; uy++)
                for (int ux = lo[0]; ux <= hi[0]; ux++)
                    if (slab_keep(g, G, S, ux, uy, uz))
                        sink.add(EMIT ? map_index(g, ux, uy, uz) : 0, i);   // (inside the map: the range is clipped to it)
    }
    sink.finish(i);
}

// ---------------------------------------------------------------------------------------------------------- accumulate
// One workgroup of 256 threads per allocated unit.  Wave w holds the 8 x 8 x 16 brick (x half w & 1, y half w >> 1); lane l its
// column lx = 8 (w & 1) + (l & 7), ly = 8 (w >> 1) + (l >> 3), all 16 z, in registers.  The unit's list is staged through LDS in
// batches of kBatch records; every voxel adds its terms in list order.  SKIP: a wave passes over a record whose slabs miss its
// brick (the test of the lists in the record's scaled form, on wave-uniform values, with a margin for its own rounding):
// a skipped term is zero: SKIP = false gives the same bits (tests/test_density_regimes_gpu.py).
template <bool SKIP>
__global__ __launch_bounds__(256) void density_accumulate_kernel(Grid g, const int32_t* __restrict__ touched,
                                                                 const float* __restrict__ records, const int32_t* __restrict__ ids,
                                                                 const int32_t* __restrict__ ranges, float r,
                                                                 float* __restrict__ pool) {
    __shared__ float4 stage[kBatch * 4];
    const int64_t m = touched[2 * blockIdx.x];
    const int64_t slot = touched[2 * blockIdx.x + 1];
    int ux, uy, uz;
    unit_coords(g, m, ux, uy, uz);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int lx = 8 * (wave & 1) + (lane & 7), ly = 8 * (wave >> 1) + (lane >> 3);
    const float x = ((float)(ux * 16 + lx) + 0.5f) * g.vs;
    const float y = ((float)(uy * 16 + ly) + 0.5f) * g.vs;
    float zc[16];
#pragma unroll
    for (int k = 0; k < 16; k++) zc[k] = ((float)(uz * 16 + k) + 0.5f) * g.vs;
    // the wave's brick: centre and half sides (voxel centres only: 3.5 and 7.5 voxels), padded by a relative 2^-20 of the
    // coordinates' size so that rounding cannot drop a voxel
    const float bx = ((float)(ux * 16 + 8 * (wave & 1)) + 4.f) * g.vs, by = ((float)(uy * 16 + 8 * (wave >> 1)) + 4.f) * g.vs;
    const float bz = ((float)(uz * 16) + 8.f) * g.vs;
    const float slack = 9.5367431640625e-7f * (((fabsf(bx) + fabsf(by)) + fabsf(bz)) + 16.f * g.vs);
    const float hx = 3.5f * g.vs + slack, hy = hx, hz = 7.5f * g.vs + slack;
    const float r2 = r * r, ecut = __expf(-0.5f * r2);
    float acc[16];
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = 0.f;
    const int e0 = ranges[2 * slot], e1 = ranges[2 * slot + 1];
    for (int b0 = e0; b0 < e1; b0 += kBatch) {
        const int nb = e1 - b0 < kBatch ? e1 - b0 : kBatch;
        __syncthreads();                                   // the previous batch has been read
        if ((t >> 2) < nb) stage[t] = reinterpret_cast<const float4*>(records + (int64_t)kRec * ids[b0 + (t >> 2)])[t & 3];
        __syncthreads();
        for (int j = 0; j < nb; j++) {
            const float4 q0 = stage[4 * j], q1 = stage[4 * j + 1], q2 = stage[4 * j + 2], q3 = stage[4 * j + 3];
            // q0 = mu.xyz, A00; q1 = A01 A02 A10 A11; q2 = A12 A20 A21 A22; q3 = o, E
            if (SKIP) {
                const float cx = bx - q0.x, cy = by - q0.y, cz = bz - q0.z;
                const float p0 = __builtin_fmaf(q1.y, cz, __builtin_fmaf(q1.x, cy, q0.w * cx));
                const float p1 = __builtin_fmaf(q2.x, cz, __builtin_fmaf(q1.w, cy, q1.z * cx));
                const float p2 = __builtin_fmaf(q2.w, cz, __builtin_fmaf(q2.z, cy, q2.y * cx));
                const float w0 = __builtin_fmaf(fabsf(q1.y), hz, __builtin_fmaf(fabsf(q1.x), hy, fabsf(q0.w) * hx));
                const float w1 = __builtin_fmaf(fabsf(q2.x), hz, __builtin_fmaf(fabsf(q1.w), hy, fabsf(q1.z) * hx));
                const float w2 = __builtin_fmaf(fabsf(q2.w), hz, __builtin_fmaf(fabsf(q2.z), hy, fabsf(q2.y) * hx));
                // (1 + 2^-16: the products above round)
                if (fabsf(p0) > (r + w0) * 1.0000152587890625f || fabsf(p1) > (r + w1) * 1.0000152587890625f ||
                    fabsf(p2) > (r + w2) * 1.0000152587890625f)
                    continue;
            }
            const float dx = x - q0.x, dy = y - q0.y;
            const float pa0 = __builtin_fmaf(q1.x, dy, q0.w * dx);
            const float pa1 = __builtin_fmaf(q1.w, dy, q1.z * dx);
            const float pa2 = __builtin_fmaf(q2.z, dy, q2.y * dx);
            const float o = q3.x;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const float dz = zc[k] - q0.z;
                const float t0 = __builtin_fmaf(q1.y, dz, pa0), t1 = __builtin_fmaf(q2.x, dz, pa1), t2 = __builtin_fmaf(q2.w, dz, pa2);
                const float mm = __builtin_fmaf(t2, t2, __builtin_fmaf(t1, t1, t0 * t0));
                const float term = o * (__expf(-0.5f * mm) - ecut);
                acc[k] += mm < r2 ? term : 0.f;
            }
        }
    }
    float* base = pool + pool_index(slot, 0, 0) + lx + 16 * ly;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        base[0 * kUnitVoxels + 256 * k] = acc[k];
        base[1 * kUnitVoxels + 256 * k] = 1.f;
        base[2 * kUnitVoxels + 256 * k] = 0.f;
        base[3 * kUnitVoxels + 256 * k] = 0.f;
        base[4 * kUnitVoxels + 256 * k] = 0.f;
    }
}

// --------------------------------------------------------------------------------------------------------------- query
// One lane per point: the point's voxel floor(p / h) names its unit, the unit's list is walked from global memory.  The first
// walk gives density, gradient and the dominant Gaussian; values take one more walk per four channels.
__device__ __forceinline__ bool gauss_term(const float* __restrict__ rec, float px, float py, float pz, float r2, float ecut,
                                           float& k, float& e, float (&tv)[3]) {
    const float dx = px - rec[0], dy = py - rec[1], dz = pz - rec[2];
#pragma unroll
    for (int a = 0; a < 3; a++) tv[a] = (rec[3 + 3 * a] * dx + rec[4 + 3 * a] * dy) + rec[5 + 3 * a] * dz;
    const float mm = (tv[0] * tv[0] + tv[1] * tv[1]) + tv[2] * tv[2];
    if (!(mm < r2)) return false;
    // exp(-m / 2) - exp(-r^2 / 2) = exp(-r^2 / 2) expm1((r^2 - m) / 2): no cancellation near the cut-off, where a ratio of two
    // small terms (values) would otherwise lose its digits
    const float em1 = expm1f(0.5f * (r2 - mm));
    e = ecut * (em1 + 1.f);
    k = rec[12] * (ecut * em1);
    return true;
}

// the pool slot of the unit that holds the point's voxel floor(p / h); -1: a non-finite point, outside the map, or an
// unallocated unit.  Shared by query and raycast.
__device__ __forceinline__ int point_slot(const Grid& g, const int32_t* __restrict__ slot_map, float px, float py, float pz) {
    if (!(is_fin(px) && is_fin(py) && is_fin(pz))) return -1;
    // (clamped before the conversion, as the ranges)
    const int vx = (int)fminf(fmaxf(floorf(px / g.vs), -3e7f), 3e7f);
    const int vy = (int)fminf(fmaxf(floorf(py / g.vs), -3e7f), 3e7f);
    const int vz = (int)fminf(fmaxf(floorf(pz / g.vs), -3e7f), 3e7f);
    const int64_t m = map_index(g, vx >> 4, vy >> 4, vz >> 4);
    return m < 0 ? -1 : slot_map[m];
}

__global__ __launch_bounds__(256) void density_query_kernel(Grid g, const int32_t* __restrict__ slot_map,
                                                            const float* __restrict__ records, const int32_t* __restrict__ ids,
                                                            const int32_t* __restrict__ ranges, float r,
                                                            const float* __restrict__ points, int64_t P,
                                                            const float* __restrict__ values, int D, float* __restrict__ density,
                                                            float* __restrict__ grad, int32_t* __restrict__ dominant,
                                                            float* __restrict__ values_out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float px = points[3 * p], py = points[3 * p + 1], pz = points[3 * p + 2];
    int e0 = 0, e1 = 0;
    const int s = point_slot(g, slot_map, px, py, pz);
    if (s >= 0) { e0 = ranges[2 * s]; e1 = ranges[2 * s + 1]; }
    const float r2 = r * r, ecut = expf(-0.5f * r2);
    float d = 0.f, gx = 0.f, gy = 0.f, gz = 0.f, best = 0.f;
    int32_t dom = -1;
    for (int e = e0; e < e1; e++) {
        const int32_t id = ids[e];
        const float* rec = records + (int64_t)kRec * id;
        float k, ex, tv[3];
        if (!gauss_term(rec, px, py, pz, r2, ecut, k, ex, tv)) continue;
        d += k;
        const float w = rec[12] * ex;
        gx -= w * ((rec[3] * tv[0] + rec[6] * tv[1]) + rec[9] * tv[2]);
        gy -= w * ((rec[4] * tv[0] + rec[7] * tv[1]) + rec[10] * tv[2]);
        gz -= w * ((rec[5] * tv[0] + rec[8] * tv[1]) + rec[11] * tv[2]);
        if (k > best) { best = k; dom = id; }
    }
    if (density) density[p] = d;
    if (grad) { grad[3 * p] = gx; grad[3 * p + 1] = gy; grad[3 * p + 2] = gz; }
    if (dominant) dominant[p] = d > 0.f ? dom : -1;
    if (!values_out) return;
    for (int c0 = 0; c0 < D; c0 += 4) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        const int nc = D - c0 < 4 ? D - c0 : 4;
        if (d > 0.f)
            for (int e = e0; e < e1; e++) {
                const int32_t id = ids[e];
                float k, ex, tv[3];
                if (!gauss_term(records + (int64_t)kRec * id, px, py, pz, r2, ecut, k, ex, tv)) continue;
                for (int c = 0; c < nc; c++) v[c] += k * values[(int64_t)D * id + c0 + c];
            }
        for (int c = 0; c < nc; c++) values_out[(int64_t)D * p + c0 + c] = d > 0.f ? v[c] / d : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------------------- raycast
// The level-set search along rays.  One wave per ray, four rays per workgroup; lane k owns sample k.
// d at the wave's 64 points, bit for bit what query gives at each: the wave walks its distinct units one at a time (the slot
// of the first pending lane, the lanes that share it), the unit's list with a wave-uniform index, so the id and the record
// are uniform loads that serve the whole group; each lane adds its terms in its own unit's list order.  need: the lanes
// whose sample is evaluated (the others return 0).
__device__ __forceinline__ float wave_density(const Grid& g, const int32_t* __restrict__ slot_map, const float* __restrict__ records,
                                              const int32_t* __restrict__ ids, const int32_t* __restrict__ ranges, float r2,
                                              float ecut, bool need, float px, float py, float pz) {
    const int slot = need ? point_slot(g, slot_map, px, py, pz) : -1;
    bool pending = slot >= 0;
    float d = 0.f;
    while (true) {
        const unsigned long long todo = __ballot(pending);
        if (!todo) break;
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        const int s = __builtin_amdgcn_readlane(slot, leader);
        const bool mine = pending && slot == s;
        const int e0 = __builtin_amdgcn_readfirstlane(ranges[2 * s]), e1 = __builtin_amdgcn_readfirstlane(ranges[2 * s + 1]);
        for (int e = e0; e < e1; e++) {
            const float* rec = records + (int64_t)kRec * __builtin_amdgcn_readfirstlane(ids[e]);
            float k, ex, tv[3];
            if (mine && gauss_term(rec, px, py, pz, r2, ecut, k, ex, tv)) d += k;
        }
        if (mine) pending = false;
    }
    return d;
}

struct Levels {
    float v[4];
};

// lane k's value (k wave-uniform)
__device__ __forceinline__ float read_lane(float x, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), k)); }

// t_out [L, M], hit_out [L, M]: per level the first crossing from below, front to back: a coarse pass of 64 samples over
// [t0, t1] shared by the levels, then per level 64 samples over its bracket (the ends reuse the coarse values), then the
// linear interpolation inside the fine bracket.  Every expression in the one order DESIGN.md section 26 writes.
__global__ __launch_bounds__(256) void density_raycast_kernel(Grid g, const int32_t* __restrict__ slot_map,
                                                              const float* __restrict__ records, const int32_t* __restrict__ ids,
                                                              const int32_t* __restrict__ ranges, float r,
                                                              const float* __restrict__ origins, const float* __restrict__ dirs,
                                                              const float* __restrict__ t0s, const float* __restrict__ t1s, int64_t M,
                                                              Levels levels, int L, float* __restrict__ t_out,
                                                              uint8_t* __restrict__ hit_out) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (ray >= M) return;                                  // (the whole wave)
    const float ox = origins[3 * ray], oy = origins[3 * ray + 1], oz = origins[3 * ray + 2];
    const float vx = dirs[3 * ray], vy = dirs[3 * ray + 1], vz = dirs[3 * ray + 2];
    const float t0 = t0s[ray], t1 = t1s[ray];
    const bool ok = is_fin(ox) && is_fin(oy) && is_fin(oz) && is_fin(vx) && is_fin(vy) && is_fin(vz) && is_fin(t0) && is_fin(t1) &&
                    t1 > t0;
    if (!ok) {
        if (lane < L) { t_out[(int64_t)lane * M + ray] = 0.f; hit_out[(int64_t)lane * M + ray] = 0; }
        return;
    }
    const float r2 = r * r, ecut = expf(-0.5f * r2);
    const float step = (t1 - t0) / 63.f;
    const float tk = t0 + (float)lane * step;
    const float D = wave_density(g, slot_map, records, ids, ranges, r2, ecut, true, ox + tk * vx, oy + tk * vy, oz + tk * vz);
    const float Dn = __shfl_down(D, 1);
    for (int l = 0; l < L; l++) {
        const float lev = l == 0 ? levels.v[0] : l == 1 ? levels.v[1] : l == 2 ? levels.v[2] : levels.v[3];
        float t = 0.f;
        int hit_lane = 0;                                  // (without a bracket: lane 0 writes the miss)
        bool hit = false;
        const unsigned long long bracket = __ballot(lane < 63 && D < lev && lev <= Dn);
        if (bracket) {
            const int k = __builtin_amdgcn_readfirstlane(__ffsll((long long)bracket) - 1);
            const float a = read_lane(tk, k), b = read_lane(tk, k + 1);
            const float Da = read_lane(D, k), Db = read_lane(D, k + 1);
            const float fstep = (b - a) / 63.f;
            const float u = lane == 0 ? a : lane == 63 ? b : a + (float)lane * fstep;
            float F = wave_density(g, slot_map, records, ids, ranges, r2, ecut, lane > 0 && lane < 63, ox + u * vx, oy + u * vy,
                                   oz + u * vz);
            F = lane == 0 ? Da : lane == 63 ? Db : F;
            const float un = __shfl_down(u, 1), Fn = __shfl_down(F, 1);
            const unsigned long long fine = __ballot(lane < 63 && F < lev && lev <= Fn);
            if (fine) {                                    // (always: F_0 < lev <= F_63)
                hit = true;
                hit_lane = __builtin_amdgcn_readfirstlane(__ffsll((long long)fine) - 1);
                t = u + (un - u) * ((lev - F) / (Fn - F));
            }
        }
        if (lane == hit_lane) {
            t_out[(int64_t)l * M + ray] = t;
            hit_out[(int64_t)l * M + ray] = hit ? 1 : 0;
        }
    }
}

}  // namespace

extern "C" int64_t misplat_density_workspace(int64_t n_gauss, int64_t n_pairs) { return work_bytes(n_gauss, n_pairs); }

extern "C" int misplat_density_records(const float* means, const float* quats, const float* scales, const float* opacities,
                                       int64_t n_gauss, float cutoff, float min_opacity, float* records,
                                       misplat_stream_t stream) {
    if (!sizes_ok(n_gauss, 0) || !cutoff_ok(cutoff) || !(min_opacity == min_opacity) || (((uintptr_t)records) & 15)) return MISPLAT_EINVAL;
    if (n_gauss == 0) return MISPLAT_OK;
    if (!means || !quats || !scales || !opacities || !records) return MISPLAT_EINVAL;
    hipLaunchKernelGGL(density_records_kernel, dim3(blocks(n_gauss, 256)), dim3(256), 0, (hipStream_t)stream, means, quats, scales,
                       opacities, n_gauss, cutoff, min_opacity, records);
    return launched();
}

extern "C" int misplat_density_count(const misplat_tsdf_grid* grid, const float* means, const float* quats, const float* scales,
                                     const float* opacities, int64_t n_gauss, float cutoff, float min_opacity, void* workspace,
                                     int64_t workspace_bytes, int32_t* pair_off, int64_t* n_pairs, misplat_stream_t stream) {
    Grid g;
    int64_t n_map;
    if (!make_grid(grid, g, n_map) || !sizes_ok(n_gauss, 0) || n_gauss < 1 || !cutoff_ok(cutoff) || !(min_opacity == min_opacity) ||
        !means || !quats || !scales || !opacities || !workspace || !pair_off || !n_pairs)
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, n_gauss, 0);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    count_pairs(W, n_gauss, pair_off, n_pairs, s, [&](PairBufs bufs) {
        hipLaunchKernelGGL(density_pairs_kernel<false>, dim3(blocks(n_gauss, 256)), dim3(256), 0, s, g, means, quats, scales,
                           opacities, n_gauss, cutoff, min_opacity, bufs);
    });
    return launched();
}

extern "C" int misplat_density_emit(const misplat_tsdf_grid* grid, const float* means, const float* quats, const float* scales,
                                    const float* opacities, int64_t n_gauss, float cutoff, float min_opacity,
                                    const int32_t* pair_off, int64_t n_pairs, int32_t* keys, int32_t* ids, uint64_t* words,
                                    misplat_stream_t stream) {
    Grid g;
    int64_t n_map;
    if (!make_grid(grid, g, n_map) || !sizes_ok(n_gauss, n_pairs) || n_gauss < 1 || n_pairs < 1 || !cutoff_ok(cutoff) ||
        !(min_opacity == min_opacity) || !means || !quats || !scales || !opacities || !pair_off || !keys || !ids || !words)
        return MISPLAT_EINVAL;
    hipLaunchKernelGGL(density_pairs_kernel<true>, dim3(blocks(n_gauss, 256)), dim3(256), 0, (hipStream_t)stream, g, means, quats,
                       scales, opacities, n_gauss, cutoff, min_opacity,
                       PairBufs{nullptr, nullptr, pair_off, n_pairs, keys, ids, (unsigned long long*)words});
    return launched();
}

// The list layer's sort and ranges (unitlists.h), exported once, for this file's pairs and pointtsdf.hip's (DESIGN.md section
// 14.5 says why here).  Of the grid only voxel_size, lo and dims are read.
extern "C" int misplat_unit_lists(const misplat_tsdf_grid* grid, const int32_t* slot_map, int32_t* keys, int32_t* ids,
                                  int64_t n_pairs, int32_t n_units, void* workspace, int64_t workspace_bytes, int32_t* keys_sorted,
                                  int32_t* ids_sorted, int32_t* ranges, misplat_stream_t stream) {
    UnitGrid g;
    int64_t n_map;
    if (!make_unit_grid(grid, g, n_map) || !(grid->voxel_size < 1e30f) || !sizes_ok(0, n_pairs) || n_pairs < 1 || n_units < 1 ||
        n_units > n_map || !slot_map || !keys || !ids || !workspace || !keys_sorted || !ids_sorted || !ranges)
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, 0, n_pairs);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    unit_lists(n_map, slot_map, keys, ids, n_pairs, keys_sorted, ids_sorted, ranges, W, (hipStream_t)stream);
    return launched();
}

extern "C" int misplat_density_accumulate(const misplat_tsdf_grid* grid, const int32_t* touched, int32_t n_units,
                                          const float* records, const int32_t* ids_sorted, const int32_t* ranges, float cutoff,
                                          int32_t flags, float* pool, misplat_stream_t stream) {
    Grid g;
    int64_t n_map;
    if (!make_grid(grid, g, n_map) || n_units < 0 || n_units > n_map || !cutoff_ok(cutoff) || (((uintptr_t)records) & 15)) return MISPLAT_EINVAL;
    if (n_units == 0) return MISPLAT_OK;
    if (!touched || !records || !ids_sorted || !ranges || !pool) return MISPLAT_EINVAL;
    if (flags & 1)
        hipLaunchKernelGGL(density_accumulate_kernel<false>, dim3((unsigned)n_units), dim3(256), 0, (hipStream_t)stream, g, touched,
                           records, ids_sorted, ranges, cutoff, pool);
    else
        hipLaunchKernelGGL(density_accumulate_kernel<true>, dim3((unsigned)n_units), dim3(256), 0, (hipStream_t)stream, g, touched,
                           records, ids_sorted, ranges, cutoff, pool);
    return launched();
}

extern "C" int misplat_density_query(const misplat_tsdf_grid* grid, const int32_t* slot_map, const float* records,
                                     const int32_t* ids_sorted, const int32_t* ranges, float cutoff, const float* points,
                                     int64_t n_points, const float* values, int32_t n_channels, float* density, float* grad,
                                     int32_t* dominant, float* values_out, misplat_stream_t stream) {
    Grid g;
    int64_t n_map;
    if (!make_grid(grid, g, n_map) || n_points < 0 || n_points >= (1ll << 31) || !cutoff_ok(cutoff) ||
        ((values_out != nullptr) != (values != nullptr)) || (values && (n_channels < 1 || n_channels > MISPLAT_DENSITY_MAX_CHANNELS)))
        return MISPLAT_EINVAL;
    if (n_points == 0) return MISPLAT_OK;
    if (!slot_map || !points) return MISPLAT_EINVAL;       // (records / ids / ranges may be NULL for a field without pairs:
                                                           //  every unit is then unallocated and no list is read)
    hipLaunchKernelGGL(density_query_kernel, dim3(blocks(n_points, 256)), dim3(256), 0, (hipStream_t)stream, g, slot_map, records,
                       ids_sorted, ranges, cutoff, points, n_points, values, (int)n_channels, density, grad, dominant, values_out);
    return launched();
}

extern "C" int misplat_density_raycast(const misplat_tsdf_grid* grid, const int32_t* slot_map, const float* records,
                                       const int32_t* ids_sorted, const int32_t* ranges, float cutoff, const float* origins,
                                       const float* dirs, const float* t0, const float* t1, int64_t n_rays, float level0,
                                       float level1, float level2, float level3, int32_t n_levels, float* t_out, uint8_t* hit_out,
                                       misplat_stream_t stream) {
    Grid g;
    int64_t n_map;
    if (!make_grid(grid, g, n_map) || n_rays < 0 || n_rays >= (1ll << 31) || !cutoff_ok(cutoff) || n_levels < 1 || n_levels > 4)
        return MISPLAT_EINVAL;
    const Levels levels = {{level0, level1, level2, level3}};
    for (int l = 0; l < n_levels; l++)
        if (!(levels.v[l] > 0.f && levels.v[l] < __builtin_inff())) return MISPLAT_EINVAL;
    if (n_rays == 0) return MISPLAT_OK;
    if (!slot_map || !origins || !dirs || !t0 || !t1 || !t_out || !hit_out) return MISPLAT_EINVAL;   // (records / ids / ranges: as query)
    hipLaunchKernelGGL(density_raycast_kernel, dim3(blocks(n_rays, 4)), dim3(256), 0, (hipStream_t)stream, g, slot_map, records,
                       ids_sorted, ranges, cutoff, origins, dirs, t0, t1, n_rays, levels, (int)n_levels, t_out, hit_out);
    return launched();
}
