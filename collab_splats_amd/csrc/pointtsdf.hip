// pointtsdf.hip -- TSDF fusion of point clouds with origins, with space carving: what the reference's
// TSDFFusion asks of vdbfusion's VDBVolume::Integrate, restated on this project's lattice (csrc/unitgrid.h).  The oracle is
// tests/pointtsdf_restatement.py; vdbfusion itself is unpinned.
//
// Ray (fp32, this order, compiled with -ffp-contract=off): v = p - o, L = sqrtf((vx vx + vy vy) + vz vz), d = v / L,
// ol = o / h, dl = d / h (h the voxel size), s0 = 0 with carving, else fmaxf(L - trunc, 0), s1 = L + trunc.  A ray with a
// non-finite coordinate, L = 0 or non-finite, or |o / h| or |p / h| >= 2^22 on an axis is skipped.
// Walk: from voxel floorf(ol + s0 dl); per axis with dl != 0 the next boundary k (g + 1 going up, g going down) lies at
// t(k) = ((float)k - ol) / dl, always from the integer; step along the smallest t, ties to the lowest axis; stop when the
// smallest t > s1.  Every t(k) of an axis is monotone in k, so the walk is the merge of three sorted event lists by the key
// (t, axis): the state after any event is a function of that event alone, and enter_box finds the walk's first voxel inside
// a box (the unit map, a unit) without walking up to it.
// Voxel with centre c = ((float)g + 0.5f) h: sdf = +-sqrtf(|p - c|^2), + iff ((c - o) . (p - c)) >= 0 (sums as above);
// where sdf > -trunc: sum_q += (int)rintf((fminf(trunc, sdf) / trunc) * 16384.f), count += 1; where |sdf| < trunc the
// colour sums take uint8(rgb 255) and the band count 1.  Integer sums: the result depends on no order.
// Pipeline per chunk of rays: the list layer of unitlists.h (count, emit, misplat_tsdf_alloc, misplat_unit_lists) ->
// accumulate, one workgroup per piece of a touched unit's list.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"
#include "unitlists.h"

namespace {

constexpr float kMaxCoord = 4194304.f;      // 2^22 voxels: lattice coordinates keep half a voxel of fp32 resolution
constexpr int kFlush = 65536;               // terms a voxel's 32-bit LDS sums may take before they are flushed
constexpr int kChunk = 8192;                // rays of a unit's list per workgroup
constexpr float kQ = 16384.f;               // fixed point of tsdf / trunc

struct Grid {
    float vs, ulen;
    int lo[3], dims[3];
    float trunc;
    int carve;
};

bool make_grid(const misplat_tsdf_grid* p, int carve, Grid& g, int64_t& n) {
    if (!make_unit_grid(p, g, n) || !(p->voxel_size < 1e30f) || !(p->sdf_trunc > 0.f) || !(p->sdf_trunc < 1e30f)) return false;
    g.trunc = p->sdf_trunc;
    g.carve = carve ? 1 : 0;
    return true;
}

__device__ __forceinline__ bool is_fin(float x) { return fabsf(x) < __builtin_inff(); }

struct Ray {
    float o[3], p[3], ol[3], dl[3], s1;
    int g0[3], step[3];
};

// false: the ray is skipped
__device__ __forceinline__ bool make_ray(const Grid& g, const float* __restrict__ points, const float* __restrict__ origins,
                                         int ostride, int64_t i, Ray& R) {
    bool ok = true;
    float v[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        R.p[a] = points[3 * i + a];
        R.o[a] = origins[(int64_t)ostride * i + a];
        ok = ok && is_fin(R.p[a]) && is_fin(R.o[a]);
        v[a] = R.p[a] - R.o[a];
    }
    const float L = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (!ok || !(L > 0.f) || !is_fin(L)) return false;
    const float s0 = g.carve ? 0.f : fmaxf(L - g.trunc, 0.f);
    R.s1 = L + g.trunc;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float d = v[a] / L;
        R.ol[a] = R.o[a] / g.vs;
        R.dl[a] = d / g.vs;
        ok = ok && fabsf(R.ol[a]) < kMaxCoord && fabsf(R.p[a] / g.vs) < kMaxCoord;
        R.step[a] = R.dl[a] > 0.f ? 1 : R.dl[a] < 0.f ? -1 : 0;
    }
    if (!ok) return false;
#pragma unroll
    for (int a = 0; a < 3; a++) R.g0[a] = (int)floorf(R.ol[a] + s0 * R.dl[a]);   // (|.| < 2^23: p and o are below 2^22)
    return true;
}

// the ray parameter of boundary k of axis A (dl[A] != 0)
template <int A> __device__ __forceinline__ float tb(const Ray& R, int k) { return ((float)k - R.ol[A]) / R.dl[A]; }
// the boundary the walk crosses next from coordinate c of axis A; +inf for an axis it never leaves
template <int A> __device__ __forceinline__ float t_next(const Ray& R, int c) {
    return R.step[A] > 0 ? tb<A>(R, c + 1) : R.step[A] < 0 ? tb<A>(R, c) : __builtin_inff();
}

// event (t, A) comes before event (tE, aE)
template <int A> __device__ __forceinline__ bool before(float t, float tE, int aE) { return t < tE || (t == tE && A < aE); }

// The coordinate of axis A after every event of the walk that comes before (tE, aE); false once it has passed the box.
template <int A>
__device__ __forceinline__ bool coord_at(const Ray& R, float tE, int aE, int blo, int bhi, int& c) {
    c = R.g0[A];
    if (R.step[A] == 0 || A == aE) return true;
    const int st = R.step[A];
    // a guess from the line, kept on the walk's side of its start; then exact, by the events themselves
    const float x = fminf(fmaxf(floorf(R.ol[A] + tE * R.dl[A]), -8388608.f), 8388608.f);
    c = (int)x;
    if ((c - R.g0[A]) * st < 0) c = R.g0[A];
    if (st > 0 ? c > bhi + 1 : c < blo - 1) c = st > 0 ? bhi + 1 : blo - 1;      // (past the box is past the box)
    if ((c - R.g0[A]) * st < 0) c = R.g0[A];
    while (before<A>(t_next<A>(R, c), tE, aE)) {
        c += st;
        if (st > 0 ? c > bhi : c < blo) return false;
    }
    // (the event that led into c: boundary c going up, c + 1 going down)
    while (c != R.g0[A] && !before<A>(tb<A>(R, st > 0 ? c : c + 1), tE, aE)) c -= st;
    return true;
}

// axis A's entry into blo .. bhi as an event: updates the latest entry (tE, aE); false: the walk never has that coordinate
template <int A>
__device__ __forceinline__ bool entry_event(const Ray& R, int blo, int bhi, float& tE, int& aE) {
    const int c = R.g0[A];
    if (c >= blo && c <= bhi) return true;
    if (R.step[A] == 0 || (R.step[A] > 0 ? c > bhi : c < blo)) return false;
    const float t = tb<A>(R, R.step[A] > 0 ? blo : bhi + 1);
    if (t >= tE) { tE = t; aE = A; }                     // (axes come in ascending order: a tie goes to the later event)
    return true;
}

// The first voxel of the walk inside the box blo .. bhi (inclusive); false: the walk has none.
__device__ __forceinline__ bool enter_box(const Ray& R, const int (&blo)[3], const int (&bhi)[3], int& ex, int& ey, int& ez) {
    float tE = -__builtin_inff();
    int aE = -1;
    if (!entry_event<0>(R, blo[0], bhi[0], tE, aE) || !entry_event<1>(R, blo[1], bhi[1], tE, aE) ||
        !entry_event<2>(R, blo[2], bhi[2], tE, aE))
        return false;
    if (aE < 0) {                                         // the walk starts inside
        ex = R.g0[0]; ey = R.g0[1]; ez = R.g0[2];
        return true;
    }
    if (!(tE <= R.s1)) return false;                      // the walk stops before the entry
    if (!coord_at<0>(R, tE, aE, blo[0], bhi[0], ex) || !coord_at<1>(R, tE, aE, blo[1], bhi[1], ey) ||
        !coord_at<2>(R, tE, aE, blo[2], bhi[2], ez))
        return false;
    if (aE == 0) ex = R.step[0] > 0 ? blo[0] : bhi[0];
    if (aE == 1) ey = R.step[1] > 0 ? blo[1] : bhi[1];
    if (aE == 2) ez = R.step[2] > 0 ? blo[2] : bhi[2];
    return ex >= blo[0] && ex <= bhi[0] && ey >= blo[1] && ey <= bhi[1] && ez >= blo[2] && ez <= bhi[2];
}

// The walk from voxel (gx, gy, gz) (a voxel of the walk) while it stays inside the box: visit(gx, gy, gz) per voxel.
template <class V>
__device__ __forceinline__ void walk_box(const Ray& R, int gx, int gy, int gz, const int (&blo)[3], const int (&bhi)[3], V visit) {
    float tx = t_next<0>(R, gx), ty = t_next<1>(R, gy), tz = t_next<2>(R, gz);
    while (true) {
        visit(gx, gy, gz);
        int a = 0;
        float tm = tx;
        if (ty < tm) { a = 1; tm = ty; }
        if (tz < tm) { a = 2; tm = tz; }
        if (!(tm <= R.s1)) break;
        if (a == 0) {
            gx += R.step[0];
            if (gx < blo[0] || gx > bhi[0]) break;
            tx = t_next<0>(R, gx);
        } else if (a == 1) {
            gy += R.step[1];
            if (gy < blo[1] || gy > bhi[1]) break;
            ty = t_next<1>(R, gy);
        } else {
            gz += R.step[2];
            if (gz < blo[2] || gz > bhi[2]) break;
            tz = t_next<2>(R, gz);
        }
    }
}

__device__ __forceinline__ int to_u8(float x) {          // uint8(rgb * 255) with truncation, clamped to [0, 255] (as tsdf.hip)
    float c = x * 255.f;
    c = c > 0.f ? c : 0.f;                                // (NaN -> 0)
    c = c < 255.f ? c : 255.f;
    return (int)c;
}

// ------------------------------------------------------------------------------------------------------------- pairs
// One lane per ray: the voxel walk inside the unit map, reduced to the units it passes (each once: the walk is monotone per
// axis), handed to the PairSink (unitlists.h) in walk order.
template <bool EMIT>
__global__ __launch_bounds__(256) void ptsdf_pairs_kernel(Grid g, const float* __restrict__ points, const float* __restrict__ origins,
                                                          int ostride, int64_t N, PairBufs bufs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    Ray R;
    PairSink<EMIT> sink(bufs);
    if (make_ray(g, points, origins, ostride, i, R)) {
        const int blo[3] = {g.lo[0] * 16, g.lo[1] * 16, g.lo[2] * 16};
        const int bhi[3] = {(g.lo[0] + g.dims[0]) * 16 - 1, (g.lo[1] + g.dims[1]) * 16 - 1, (g.lo[2] + g.dims[2]) * 16 - 1};
        int ex, ey, ez;
        if (enter_box(R, blo, bhi, ex, ey, ez)) {
            sink.open(i);
            int lx = 0, ly = 0, lz = 0;
            bool have = false;
            walk_box(R, ex, ey, ez, blo, bhi, [&](int gx, int gy, int gz) {
                const int ux = gx >> 4, uy = gy >> 4, uz = gz >> 4;
                if (have && ux == lx && uy == ly && uz == lz) return;
                have = true; lx = ux; ly = uy; lz = uz;
                sink.add(EMIT ? map_index(g, ux, uy, uz) : 0, i);       // (inside the map: the walk is confined to it)
            });
        }
    }
    sink.finish(i);
}

// -------------------------------------------------------------------------------------------------------- accumulate
// chunks[t] = the number of pieces of kChunk rays the list of touched unit t is cut into
__global__ __launch_bounds__(256) void ptsdf_chunks_kernel(const int32_t* __restrict__ touched, int n_touched,
                                                           const int32_t* __restrict__ ranges, int32_t* __restrict__ chunks) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_touched) return;
    const int64_t slot = touched[2 * t + 1];
    chunks[t] = (ranges[2 * slot + 1] - ranges[2 * slot] + kChunk - 1) / kChunk;
}

// One workgroup of 256 threads per piece of at most kChunk rays of a touched unit's list (with carving every ray of a view
// passes its camera's unit: one workgroup per unit would leave the whole view to a handful of workgroups).  The unit's 4096
// (sum_q, count) pairs live in LDS as 2 x int32 (32 KiB: up to five workgroups share a CU's 160 KiB).  Lanes take the piece's
// rays, re-enter the walk at the unit's box and add with LDS integer atomics.  Overflow: a ray passes a voxel at most once
// (the walk is monotone per axis) and |q| <= 16384 = 2^14, so a voxel's 32-bit partial sum takes at most kChunk <= kFlush =
// 2^16 terms before it is flushed: |sum| <= 2^30 < 2^31, count <= 2^16.  The flush adds LDS into the global int64 / int32
// planes: with plain loads and stores where the unit's list is one piece (no other workgroup of the launch owns the unit),
// with integer atomics where it is several.  The colour sums touch the voxels of the band only: global integer atomics.
// chunk_off: the exclusive scan of the pieces per touched unit, [n_touched + 1]; the grid may be longer than their number.
__global__ __launch_bounds__(256) void ptsdf_accumulate_kernel(Grid g, const int32_t* __restrict__ touched, int n_touched,
                                                               const int32_t* __restrict__ chunk_off,
                                                               const float* __restrict__ points, const float* __restrict__ origins,
                                                               int ostride, const float* __restrict__ colors,
                                                               const int32_t* __restrict__ ids, const int32_t* __restrict__ ranges,
                                                               long long* __restrict__ sum_q, int32_t* __restrict__ count,
                                                               int32_t* __restrict__ rgb_sum, int32_t* __restrict__ rgb_count) {
    static_assert(kChunk <= kFlush, "a piece is flushed once, at its end");
    __shared__ int32_t sq[kUnitVoxels], sc[kUnitVoxels];
    const int piece = blockIdx.x;
    if (piece >= chunk_off[n_touched]) return;             // (the whole workgroup)
    int lo = 0, hi = n_touched - 1;                        // the last unit whose pieces begin at or before this one
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (chunk_off[mid] <= piece) lo = mid; else hi = mid - 1;
    }
    const bool shared = chunk_off[lo + 1] - chunk_off[lo] > 1;
    const int64_t m = touched[2 * lo];
    const int64_t slot = touched[2 * lo + 1];
    int ux, uy, uz;
    unit_coords(g, m, ux, uy, uz);
    const int blo[3] = {ux * 16, uy * 16, uz * 16}, bhi[3] = {ux * 16 + 15, uy * 16 + 15, uz * 16 + 15};
    const int t = threadIdx.x;
    for (int i = t; i < kUnitVoxels; i += 256) { sq[i] = 0; sc[i] = 0; }
    __syncthreads();
    const int e1 = ranges[2 * slot + 1];
    const int c0 = ranges[2 * slot] + (piece - chunk_off[lo]) * kChunk;
    const int c1 = e1 - c0 < kChunk ? e1 : c0 + kChunk;
    for (int e = c0 + t; e < c1; e += 256) {
        const int64_t ray = ids[e];
        Ray R;
        int ex, ey, ez;
        if (!make_ray(g, points, origins, ostride, ray, R) || !enter_box(R, blo, bhi, ex, ey, ez)) continue;   // (never: the ray was listed)
        int cr = 0, cg = 0, cb = 0;
        if (colors) { cr = to_u8(colors[3 * ray]); cg = to_u8(colors[3 * ray + 1]); cb = to_u8(colors[3 * ray + 2]); }
        walk_box(R, ex, ey, ez, blo, bhi, [&](int gx, int gy, int gz) {
            const float cx = ((float)gx + 0.5f) * g.vs, cy = ((float)gy + 0.5f) * g.vs, cz = ((float)gz + 0.5f) * g.vs;
            const float px = R.p[0] - cx, py = R.p[1] - cy, pz = R.p[2] - cz;
            const float dot = ((cx - R.o[0]) * px + (cy - R.o[1]) * py) + (cz - R.o[2]) * pz;
            const float dist = sqrtf((px * px + py * py) + pz * pz);
            const float sdf = dot >= 0.f ? dist : -dist;
            if (!(sdf > -g.trunc)) return;
            const int i = (gx & 15) | ((gy & 15) << 4) | ((gz & 15) << 8);
            const int q = (int)rintf((fminf(g.trunc, sdf) / g.trunc) * kQ);
            atomicAdd(&sq[i], q);
            atomicAdd(&sc[i], 1);
            if (fabsf(sdf) < g.trunc) {
                const int64_t j = slot * kUnitVoxels + i;
                if (colors) {
                    atomicAdd(&rgb_sum[3 * slot * kUnitVoxels + i], cr);
                    atomicAdd(&rgb_sum[(3 * slot + 1) * kUnitVoxels + i], cg);
                    atomicAdd(&rgb_sum[(3 * slot + 2) * kUnitVoxels + i], cb);
                }
                atomicAdd(&rgb_count[j], 1);
            }
        });
    }
    __syncthreads();
    for (int i = t; i < kUnitVoxels; i += 256) {
        const int c = sc[i];
        if (!c) continue;
        const int64_t j = slot * kUnitVoxels + i;
        if (shared) {
            atomicAdd((unsigned long long*)&sum_q[j], (unsigned long long)(long long)sq[i]);      // (two's complement: the sum is the same)
            atomicAdd(&count[j], c);
        } else {
            sum_q[j] += (long long)sq[i];
            count[j] += c;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- finalise
// the integer planes into the fp32 pool of unitgrid.h (colours 0..255, as tsdf.hip's pool: the marching cubes divide by 255)
__global__ __launch_bounds__(256) void ptsdf_finalize_kernel(int64_t n, const long long* __restrict__ sum_q,
                                                             const int32_t* __restrict__ count, const int32_t* __restrict__ rgb_sum,
                                                             const int32_t* __restrict__ rgb_count, int min_weight,
                                                             float* __restrict__ pool) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int64_t slot = j >> 12, i = j & 4095;
    const int c = count[j], bc = rgb_count[j];
    pool[pool_index(slot, 0, i)] = c > 0 ? (float)((double)sum_q[j] / (double)c) * (1.f / kQ) : 0.f;
    pool[pool_index(slot, 1, i)] = c >= min_weight ? (float)c : 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++)
        pool[pool_index(slot, 2 + k, i)] = bc > 0 ? (float)((double)rgb_sum[(3 * slot + k) * kUnitVoxels + i] / (double)bc) : 0.f;
}

inline bool stride_ok(int32_t s) { return s == 0 || s == 3; }

}  // namespace

// (unitlists.h's workspace: N rays for count, N touched units for accumulate's piece scan)
extern "C" int64_t misplat_ptsdf_workspace(int64_t n_rays, int64_t n_pairs) { return work_bytes(n_rays, n_pairs); }

extern "C" int misplat_ptsdf_count(const misplat_tsdf_grid* grid, const float* points, const float* origins, int32_t origin_stride,
                                   int64_t n_rays, int32_t space_carving, void* workspace, int64_t workspace_bytes,
                                   int32_t* pair_off, int64_t* n_pairs, misplat_stream_t stream) {
    Grid g;
    int64_t n_map;
    if (!make_grid(grid, space_carving, g, n_map) || !sizes_ok(n_rays, 0) || n_rays < 1 || !stride_ok(origin_stride) || !points ||
        !origins || !workspace || !pair_off || !n_pairs)
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, n_rays, 0);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    count_pairs(W, n_rays, pair_off, n_pairs, s, [&](PairBufs bufs) {
        hipLaunchKernelGGL(ptsdf_pairs_kernel<false>, dim3(blocks(n_rays, 256)), dim3(256), 0, s, g, points, origins,
                           (int)origin_stride, n_rays, bufs);
    });
    return launched();
}

extern "C" int misplat_ptsdf_emit(const misplat_tsdf_grid* grid, const float* points, const float* origins, int32_t origin_stride,
                                  int64_t n_rays, int32_t space_carving, const int32_t* pair_off, int64_t n_pairs, int32_t* keys,
                                  int32_t* ids, uint64_t* words, misplat_stream_t stream) {
    Grid g;
    int64_t n_map;
    if (!make_grid(grid, space_carving, g, n_map) || !sizes_ok(n_rays, n_pairs) || n_rays < 1 || n_pairs < 1 ||
        !stride_ok(origin_stride) || !points || !origins || !pair_off || !keys || !ids || !words)
        return MISPLAT_EINVAL;
    hipLaunchKernelGGL(ptsdf_pairs_kernel<true>, dim3(blocks(n_rays, 256)), dim3(256), 0, (hipStream_t)stream, g, points, origins,
                       (int)origin_stride, n_rays, PairBufs{nullptr, nullptr, pair_off, n_pairs, keys, ids, (unsigned long long*)words});
    return launched();
}

extern "C" int misplat_ptsdf_accumulate(const misplat_tsdf_grid* grid, const int32_t* touched, int32_t n_touched,
                                        const float* points, const float* origins, int32_t origin_stride, const float* colors,
                                        int32_t space_carving, const int32_t* ids_sorted, const int32_t* ranges, int64_t n_pairs,
                                        void* workspace, int64_t workspace_bytes, int64_t* sum_q, int32_t* count,
                                        int32_t* rgb_sum, int32_t* rgb_count, misplat_stream_t stream) {
    Grid g;
    int64_t n_map;
    if (!make_grid(grid, space_carving, g, n_map) || n_touched < 0 || n_touched > n_map || !stride_ok(origin_stride) ||
        !sizes_ok(n_touched, n_pairs))
        return MISPLAT_EINVAL;
    if (n_touched == 0) return MISPLAT_OK;
    if (!touched || !points || !origins || !ids_sorted || !ranges || !workspace || !sum_q || !count || !rgb_sum || !rgb_count)
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, n_touched, 0);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ptsdf_chunks_kernel, dim3(blocks(n_touched, 256)), dim3(256), 0, s, touched, (int)n_touched, ranges, W.counts);
    scan(W.counts, n_touched, W.offs, W.scr, s);
    // (the pieces number at most n_touched + n_pairs / kChunk: each list ends in at most one short piece)
    const int64_t pieces = n_touched + n_pairs / kChunk;
    hipLaunchKernelGGL(ptsdf_accumulate_kernel, dim3((unsigned)pieces), dim3(256), 0, s, g, touched, (int)n_touched,
                       (const int32_t*)W.offs, points, origins, (int)origin_stride, colors, ids_sorted, ranges, (long long*)sum_q, count,
                       rgb_sum, rgb_count);
    return launched();
}

extern "C" int misplat_ptsdf_finalize(int32_t n_units, const int64_t* sum_q, const int32_t* count, const int32_t* rgb_sum,
                                      const int32_t* rgb_count, int32_t min_weight, float* pool, misplat_stream_t stream) {
    if (n_units < 0 || n_units > MISPLAT_TSDF_MAX_UNITS) return MISPLAT_EINVAL;
    if (n_units == 0) return MISPLAT_OK;
    if (!sum_q || !count || !rgb_sum || !rgb_count || !pool) return MISPLAT_EINVAL;
    const int64_t n = (int64_t)n_units * kUnitVoxels;
    hipLaunchKernelGGL(ptsdf_finalize_kernel, dim3(blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, n, (const long long*)sum_q,
                       count, rgb_sum, rgb_count, (int)min_weight, pool);
    return launched();
}
