// pointcloud.hip -- point-cloud cleaning on the device: unbounded k-nearest mean distance, the
// statistical-outlier threshold, radius counts and the voxel reduction.
//
// Semantics (tests/pointcloud_restatement.py is the oracle).  d2 = ((dx dx + dy dy) + dz dz) in fp32, compiled with
// -ffp-contract=off: every expression is evaluated in the written order.
//   knn:     per query the k smallest d2 among all points (a multiset: no tie rule); mean = the fp32 sum of sqrtf(d2) in
//            ascending order / float(k), nearest = sqrtf of the smallest.
//   outlier: mu and sigma of the positive means in fp64 in a fixed reduction order; keep iff avg > 0 and double(avg) < thr.
//   radius:  the number of points with d2 < r2, r2 = r r in fp32 (strict).
//   voxel:   cell = floor((double(p) - origin) / voxel) in fp64; voxels numbered in ascending order of their smallest member;
//            the members of a voxel summed in fp64 in ascending point index, the quotient rounded to fp32.
// No float atomics anywhere: two runs are bitwise equal.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"
#include "internal.h"
#include "cellhash.h"
#include "radixsort.h"

namespace {

constexpr int kLevels = 3;            // hashes of edge h, 8 h, 64 h over the same points
constexpr float kCoarser = 8.f;
constexpr int kRings = 2;             // rings around the query's cell at each level (a box of 5^3 cells) before the next level
constexpr uint32_t kUnset = 0xffffffffu;
constexpr int kSubR = 8;              // lanes per query of the radius count (as cluster.hip's union)

// --------------------------------------------------------------------------------------------------------- best list
// The k smallest d2 seen, as the bits of the (non-negative) floats (cellhash.h's KBest).  Unset slots hold kUnset (above
// +inf's bits).
template <int KC>
using Best = KBest<uint32_t, KC>;

// the k smallest of what the L lanes of a query hold together (every lane gets the same list): a butterfly over disjoint sets
template <int KC, int L>
__device__ __forceinline__ Best<KC> merged(const Best<KC>& own, int k) {
    Best<KC> m = own;
    if constexpr (L > 1) {
#pragma unroll
        for (int off = 1; off < L; off <<= 1) {
            uint32_t o[KC];
#pragma unroll
            for (int j = 0; j < KC; j++) o[j] = (uint32_t)__shfl_xor((int)m.b[j], off);
#pragma unroll
            for (int j = 0; j < KC; j++)
                if (j >= KC - k) m.offer(o[j]);
        }
    }
    return m;
}

struct Levels {
    Index ix[kLevels];
    float h[kLevels], inv_h[kLevels];
};

// The query's side of every rounding argument below.  u = 2^-24.  A point x is in cell c of an axis iff
// floorf(fl(x inv_h)) = c.  With H = 1 / inv_h (exact) and h = fl(1 / inv_h) = H (1 + e), |e| <= u:
//   * fl(x inv_h) >= F (an integer) gives x >= F H - |F| H u (1 + 2 u); likewise fl(x inv_h) < F gives x < F H + |F| H u;
//   * the face is computed as fl(fl(F h) - p): off the true F H - p by at most |F| H (2 u + u^2) + u |result|;
//   * every F used is within kRings + 1 cells of the query's own, so |F| H <= amax (1 + u) + (kRings + 2) h.
// So a point outside the box lo .. hi of an axis lies at least g = gap_c - 4.2 u (amax + (kRings + 2) h) from p on that axis,
// gap_c the computed distance to the face.  Its computed d2 is at least g^2 (1 - u)^5: dx = fl(p - x) >= g (1 - u), the
// product and the two sums of non-negative terms each lose at most a factor (1 - u), and rounding is monotone.  The test
// kth < fl(t t), t = fl(gap_c - margin), therefore proves d2 >= kth for every unvisited point as soon as
// t (1 + u) <= g (1 - 3.1 u), i.e. margin >= 4.2 u (amax + (kRings + 2) h) + 5.3 u gap_c; gap_c <= (kRings + 2) h gives
// margin >= 9.5 u (amax + (kRings + 2) h).  The kernel takes 16 u = 2^-20 of it (the margin's own rounding is 3 u of it).
// The same bound serves the per-cell test of visit(): a point of cell c is at least max(t_a, 0) from p on axis a, t_a the
// computed distance to the nearer face less the margin, so its computed d2 is at least (1 - 16 u) times the computed
// (tx tx + ty ty) + tz tz.
struct Query {
    float p[3];
    float margin;
    uint32_t cut;                     // no key above it can be among the k smallest (kUnset: unknown)
    int sub;
};

template <int KC, int L>
__device__ __forceinline__ void visit(const Index& ix, float h, int cx, int cy, int cz, const Query& q, Best<KC>& best) {
    const int c[3] = {cx, cy, cz};
    float t[3];
#pragma unroll
    for (int a = 0; a < 3; a++)
        t[a] = fmaxf(fmaxf((float)c[a] * h - q.p[a], q.p[a] - (float)(c[a] + 1) * h) - q.margin, 0.f);
    const float lb = ((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) * 0.99999905f;
    if (lb > __uint_as_float(q.cut)) return;                        // (cut unset is a NaN: never skipped)
    const int s = find_cell(ix.keys, ix.mask, cell_key(cx, cy, cz));
    if (s < 0) return;
    const int e1 = ix.starts[s + 1];
    for (int e = ix.starts[s] + q.sub; e < e1; e += L) {
        const float4 v = ix.pts[e];
        const float dx = q.p[0] - v.x, dy = q.p[1] - v.y, dz = q.p[2] - v.z;
        const uint32_t key = __float_as_uint((dx * dx + dy * dy) + dz * dz);
        if (key <= q.cut) best.offer(key);
    }
}

// cells of the box c0 - R .. c0 + R that are not in the box of R - 1
template <int KC, int L>
__device__ __forceinline__ void visit_shell(const Index& ix, float h, const int (&c0)[3], int R, const Query& q, Best<KC>& best) {
    for (int cz = c0[2] - R; cz <= c0[2] + R; cz++)
        for (int cy = c0[1] - R; cy <= c0[1] + R; cy++) {
            const bool inner = R > 0 && cz > c0[2] - R && cz < c0[2] + R && cy > c0[1] - R && cy < c0[1] + R;
            const int step = inner ? 2 * R : 1;
            for (int cx = c0[0] - R; cx <= c0[0] + R; cx += step) visit<KC, L>(ix, h, cx, cy, cz, q, best);
        }
}

// L lanes per query, each taking every L-th point of every cell.  Q NULL: the points query themselves, in the cell order of
// level 0 (neighbouring lanes walk the same cells), and the result goes to the point's own row.
template <int KC, int L>
__global__ __launch_bounds__(256) void knn_mean_kernel(Levels lv, int64_t N, const float* __restrict__ Q, int64_t Nq, int k,
                                                       float* __restrict__ mean, float* __restrict__ nearest) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t t = g / L;
    if (t >= Nq) return;
    Query q;
    q.sub = (int)(g % L);
    q.cut = kUnset;
    int64_t row = t;
    if (Q) {
        q.p[0] = Q[3 * t]; q.p[1] = Q[3 * t + 1]; q.p[2] = Q[3 * t + 2];
    } else {
        const float4 v = lv.ix[0].pts[t];
        q.p[0] = v.x; q.p[1] = v.y; q.p[2] = v.z;
        row = __float_as_int(v.w);
    }
    const float amax = fmaxf(fmaxf(fabsf(q.p[0]), fabsf(q.p[1])), fabsf(q.p[2]));
    Best<KC> best, m;
    bool done = false;
    for (int l = 0; l < kLevels && !done; l++) {
        const float h = lv.h[l], inv_h = lv.inv_h[l];
        q.margin = 9.5367432e-7f * (amax + (float)(kRings + 2) * h);
        best.reset(k);
        int c0[3];
#pragma unroll
        for (int a = 0; a < 3; a++) c0[a] = cell_of(q.p[a], inv_h);
        for (int R = 0; R <= kRings && !done; R++) {
            visit_shell<KC, L>(lv.ix[l], h, c0, R, q, best);
            m = merged<KC, L>(best, k);
            const uint32_t kth = m.b[KC - 1];
            if (kth == kUnset) continue;
            q.cut = kth < q.cut ? kth : q.cut;
            float gap = 3.4e38f;
#pragma unroll
            for (int a = 0; a < 3; a++)
                gap = fminf(gap, fminf(q.p[a] - (float)(c0[a] - R) * h, (float)(c0[a] + R + 1) * h - q.p[a]));
            const float tt = gap - q.margin;
            done = tt > 0.f && __uint_as_float(kth) < tt * tt;
        }
    }
    if (!done) {                                                    // the last resort: every point, once
        best.reset(k);
        for (int64_t e = q.sub; e < N; e += L) {
            const float4 v = lv.ix[0].pts[e];
            const float dx = q.p[0] - v.x, dy = q.p[1] - v.y, dz = q.p[2] - v.z;
            const uint32_t key = __float_as_uint((dx * dx + dy * dy) + dz * dz);
            if (key <= q.cut) best.offer(key);
        }
        m = merged<KC, L>(best, k);
    }
    if (q.sub != 0) return;
    float sum = 0.f, first = 0.f;
#pragma unroll
    for (int j = 0; j < KC; j++) {
        if (j < KC - k) continue;
        const float d = sqrtf(__uint_as_float(m.b[j]));
        if (j == KC - k) first = d;
        sum += d;
    }
    mean[row] = sum / (float)k;
    nearest[row] = first;
}

// ------------------------------------------------------------------------------------------------------ radius count
// As cluster.hip's union_kernel: the box comes from the coordinates, cells cell_of(x - t) .. cell_of(x + t), t = r + margin,
// margin = 2^-22 (amax + r) (the derivation stands there); a query outside the index's range has no point within r.
__global__ __launch_bounds__(256) void radius_count_kernel(Index ix, const float* __restrict__ Q, int64_t Nq, float r, float r2,
                                                           float inv_h, int32_t* __restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t t = g / kSubR;
    const int sub = (int)(g % kSubR);
    if (t >= Nq) return;
    float p[3];
    int64_t row = t;
    if (Q) {
        p[0] = Q[3 * t]; p[1] = Q[3 * t + 1]; p[2] = Q[3 * t + 2];
    } else {
        const float4 v = ix.pts[t];
        p[0] = v.x; p[1] = v.y; p[2] = v.z;
        row = __float_as_int(v.w);
    }
    const float amax = fmaxf(fmaxf(fabsf(p[0]), fabsf(p[1])), fabsf(p[2]));
    int cnt = 0;
    if (amax * inv_h < kCoordCells + 2.f) {
        const float reach = r + 2.3841858e-7f * (amax + r);
        int lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; a++) { lo[a] = cell_of(p[a] - reach, inv_h); hi[a] = cell_of(p[a] + reach, inv_h); }
        for (int cz = lo[2]; cz <= hi[2]; cz++)
            for (int cy = lo[1]; cy <= hi[1]; cy++)
                for (int cx = lo[0]; cx <= hi[0]; cx++) {
                    const int s = find_cell(ix.keys, ix.mask, cell_key(cx, cy, cz));
                    if (s < 0) continue;
                    const int e1 = ix.starts[s + 1];
                    for (int e = ix.starts[s] + sub; e < e1; e += kSubR) {
                        const float4 c = ix.pts[e];
                        const float dx = p[0] - c.x, dy = p[1] - c.y, dz = p[2] - c.z;
                        cnt += ((dx * dx + dy * dy) + dz * dz) < r2 ? 1 : 0;
                    }
                }
    }
#pragma unroll
    for (int off = 1; off < kSubR; off <<= 1) cnt += __shfl_xor(cnt, off);
    if (sub == 0) out[row] = cnt;
}

// --------------------------------------------------------------------------------------------------- occupied cells
__global__ __launch_bounds__(256) void occupied_kernel(const unsigned long long* __restrict__ keys, int64_t cap,
                                                       int32_t* __restrict__ n_cells) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long any = __ballot(s < cap && keys[s] != kEmpty);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(n_cells, __popcll(any));
}

// ---------------------------------------------------------------------------------------------------- outlier stats
// wgprims.h's fixed-order sums: 256 values per workgroup in a fixed tree (block_sums), the workgroup sums strided over one
// workgroup and through the same tree (sum_final_kernel<2, 256>).  Pass 0: (sum of the positive avg, their number); pass 1:
// (sum of (avg - mu)^2, 0).

__global__ __launch_bounds__(256) void stat_partial_kernel(const float* __restrict__ avg, int64_t N, int pass,
                                                           const double* __restrict__ stats, double* __restrict__ part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double sc[2] = {0.0, 0.0};
    if (i < N && avg[i] > 0.f) {
        if (pass == 0) { sc[0] = (double)avg[i]; sc[1] = 1.0; }
        else { const double d = (double)avg[i] - stats[0] / stats[1]; sc[0] = d * d; }
    }
    block_sums<2>(sc, part + 2 * blockIdx.x);
}

// stats: 0 sum, 1 n_valid, 2 sum of squares, 3 (unused), 4 threshold.  n_valid <= 1: no threshold (every positive avg stays).
__global__ __launch_bounds__(256) void outlier_mask_kernel(const float* __restrict__ avg, int64_t N, double std_ratio,
                                                           double* __restrict__ stats, uint8_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const double n = stats[1];
    double thr = __longlong_as_double(0x7ff0000000000000ll);
    if (n > 1.0) thr = stats[0] / n + std_ratio * sqrt(stats[2] / (n - 1.0));
    if (i == 0) stats[4] = thr;
    if (i >= N) return;
    const float a = avg[i];
    keep[i] = (a > 0.f && (double)a < thr) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ voxel
__device__ __forceinline__ long long voxel_cell(float x, double origin, double voxel) {
    const double c = floor(((double)x - origin) / voxel);
    return (long long)fmin(fmax(c, -1048576.0), 1048575.0);       // (the host checks the range: never clamped)
}

__global__ __launch_bounds__(256) void voxel_insert_kernel(const float* __restrict__ P, int64_t N, double ox, double oy, double oz,
                                                           double voxel, unsigned long long* __restrict__ keys, uint32_t mask,
                                                           int32_t* __restrict__ vslot, int32_t* __restrict__ first) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const unsigned long long key = (unsigned long long)(voxel_cell(P[3 * i], ox, voxel) + 1048576) |
                                   ((unsigned long long)(voxel_cell(P[3 * i + 1], oy, voxel) + 1048576) << 21) |
                                   ((unsigned long long)(voxel_cell(P[3 * i + 2], oz, voxel) + 1048576) << 42);
    const uint32_t s = claim_slot(keys, mask, hash_slot(key, mask), key);
    vslot[i] = (int32_t)s;
    atomicMin(&first[s], (int32_t)i);
}

__global__ __launch_bounds__(256) void voxel_flag_kernel(const int32_t* __restrict__ vslot, const int32_t* __restrict__ first,
                                                         int64_t N, int32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) flag[i] = first[vslot[i]] == (int32_t)i ? 1 : 0;
}

// key = the voxel's number (the rank of its smallest member among the smallest members), value = the point
__global__ __launch_bounds__(256) void voxel_key_kernel(const int32_t* __restrict__ vslot, const int32_t* __restrict__ first,
                                                        const int32_t* __restrict__ rank, int64_t N, int32_t* __restrict__ keys,
                                                        int32_t* __restrict__ vals, int32_t* __restrict__ n_voxels) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *n_voxels = rank[N];
    if (i >= N) return;
    keys[i] = rank[first[vslot[i]]];
    vals[i] = (int32_t)i;
}

// order = the sorted points; offs[v] = first sorted position whose voxel is >= v, v = 0 .. N
__global__ __launch_bounds__(256) void voxel_finish_kernel(const int32_t* __restrict__ skeys, const int32_t* __restrict__ svals,
                                                           int64_t N, int32_t* __restrict__ order, int32_t* __restrict__ offs) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v > N) return;
    if (v < N) order[v] = svals[v];
    int64_t a = 0, b = N;
    while (a < b) {
        const int64_t m = (a + b) >> 1;
        if (skeys[m] < v) a = m + 1;
        else b = m;
    }
    offs[v] = (int32_t)a;
}

// one thread per (voxel, channel): fp64 sum in ascending point index, the quotient rounded to fp32
__global__ __launch_bounds__(256) void voxel_mean_kernel(const float* __restrict__ X, int D, const int32_t* __restrict__ order,
                                                         const int32_t* __restrict__ offs, int64_t V, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t v = t / D;
    const int c = (int)(t - v * D);
    if (v >= V) return;
    const int32_t e0 = offs[v], e1 = offs[v + 1];
    double acc = 0.0;
    for (int32_t e = e0; e < e1; e++) acc += (double)X[(int64_t)order[e] * D + c];
    out[t] = (float)(acc / (double)(e1 - e0));
}

// ------------------------------------------------------------------------------------------------------- workspace
enum { kKindCells = 0, kKindKnn = 1, kKindRadius = 2, kKindOutlier = 3, kKindVoxel = 4 };

inline bool sizes_ok(int64_t N) { return N >= 0 && N < (1ll << 30); }

// what a kind does not use stays null
struct Work {
    IndexBufs lv[kLevels];            // kKindKnn: all of them; kKindCells, kKindRadius: lv[0]
    int32_t *vslot, *scr;
    double *part, *stats;             // kKindOutlier
    unsigned long long* vkeys;        // kKindVoxel: the voxel hash (capacity cap), ...
    int32_t *first, *flag, *rank, *ka, *va, *kb, *vb;
    SortBufs sort;                    // ... and the sort of the points by voxel
    int64_t cap;
};

inline Work carve(Carver& c, int64_t N, int kind) {
    Work W = {};
    W.cap = hash_capacity(N);
    const int64_t n_hist = 256 * ((N + kTile - 1) / kTile);
    const int levels = kind == kKindKnn ? kLevels : (kind == kKindCells || kind == kKindRadius) ? 1 : 0;
    for (int l = 0; l < levels; l++) W.lv[l] = take_index(c, N);
    W.vslot = c.take<int32_t>(N);
    W.scr = take_scan(c, W.cap > n_hist ? W.cap : n_hist);
    if (kind == kKindOutlier) {
        W.part = c.take<double>(2 * ((N + 255) / 256) + 2);
        W.stats = c.take<double>(8);
    }
    if (kind == kKindVoxel) {
        W.vkeys = c.take<unsigned long long>(W.cap);
        W.first = c.take<int32_t>(W.cap);
        W.flag = c.take<int32_t>(N);
        W.rank = c.take<int32_t>(N + 1);
        W.ka = c.take<int32_t>(N);
        W.va = c.take<int32_t>(N);
        W.kb = c.take<int32_t>(N);
        W.vb = c.take<int32_t>(N);
        W.sort = take_sort(c, N);
    }
    return W;
}

inline bool edge_ok(float h) { return h > 0.f && h < 3.0e35f && 1.f / h < 3.0e38f; }

template <int KC>
void launch_knn(const Levels& lv, int64_t N, const float* Q, int64_t Nq, int k, int lanes, float* mean, float* nearest,
                hipStream_t s) {
    if (lanes == 1)
        hipLaunchKernelGGL((knn_mean_kernel<KC, 1>), dim3(blocks(Nq, 256)), dim3(256), 0, s, lv, N, Q, Nq, k, mean, nearest);
    else
        hipLaunchKernelGGL((knn_mean_kernel<KC, 8>), dim3(blocks(Nq * 8, 256)), dim3(256), 0, s, lv, N, Q, Nq, k, mean, nearest);
}

}  // namespace

extern "C" int64_t misplat_pointcloud_workspace(int64_t n_points, int32_t kind) {
    if (!sizes_ok(n_points) || kind < kKindCells || kind > kKindVoxel) return -1;
    Carver c{nullptr};
    carve(c, n_points, kind);
    return c.o;
}

extern "C" int misplat_pointcloud_cells(const float* points, int64_t n_points, float edge, void* workspace,
                                        int64_t workspace_bytes, int32_t* n_cells, misplat_stream_t stream) {
    const int64_t N = n_points;
    if (!sizes_ok(N) || N < 1 || !edge_ok(edge) || !points || !workspace || !n_cells) return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, N, kKindCells);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const Index ix = build_index(points, N, nullptr, 1.f / edge, W.lv[0], W.vslot, W.scr, s);
    misplat_internal::fill_bytes(n_cells, 4, 0u, s);
    hipLaunchKernelGGL(occupied_kernel, dim3(blocks(W.cap, 256)), dim3(256), 0, s, ix.keys, W.cap, n_cells);
    return launched();
}

extern "C" int misplat_pointcloud_knn(const float* points, int64_t n_points, const float* queries, int64_t n_queries, int32_t k,
                                      float edge, int32_t lanes, void* workspace, int64_t workspace_bytes, float* mean,
                                      float* nearest, misplat_stream_t stream) {
    const int64_t N = n_points, Nq = queries ? n_queries : n_points;
    if (!sizes_ok(N) || !sizes_ok(Nq) || N < 1 || k < 1 || k > 32 || k > N || !(lanes == 1 || lanes == 8) || !edge_ok(edge) ||
        !points || !workspace || (Nq > 0 && (!mean || !nearest)))
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, N, kKindKnn);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    if (Nq == 0) return MISPLAT_OK;
    hipStream_t s = (hipStream_t)stream;
    Levels lv;
    float h = edge;
    for (int l = 0; l < kLevels; l++, h *= kCoarser) {
        lv.h[l] = h;
        lv.inv_h[l] = 1.f / h;
        lv.ix[l] = build_index(points, N, nullptr, lv.inv_h[l], W.lv[l], W.vslot, W.scr, s);
    }
    if (k <= 4) launch_knn<4>(lv, N, queries, Nq, k, lanes, mean, nearest, s);
    else if (k <= 8) launch_knn<8>(lv, N, queries, Nq, k, lanes, mean, nearest, s);
    else if (k <= 16) launch_knn<16>(lv, N, queries, Nq, k, lanes, mean, nearest, s);
    else launch_knn<32>(lv, N, queries, Nq, k, lanes, mean, nearest, s);
    return launched();
}

extern "C" int misplat_pointcloud_radius_count(const float* points, int64_t n_points, const float* queries, int64_t n_queries,
                                               float radius, void* workspace, int64_t workspace_bytes, int32_t* counts,
                                               misplat_stream_t stream) {
    const int64_t N = n_points, Nq = queries ? n_queries : n_points;
    if (!sizes_ok(N) || !sizes_ok(Nq) || N < 1 || !(radius > 0.f) || !(radius < 3.0e37f) || !(1.f / radius < 3.0e38f) || !points ||
        !workspace || (Nq > 0 && !counts))
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, N, kKindRadius);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    if (Nq == 0) return MISPLAT_OK;
    hipStream_t s = (hipStream_t)stream;
    const float inv_h = 1.f / radius;
    const Index ix = build_index(points, N, nullptr, inv_h, W.lv[0], W.vslot, W.scr, s);
    hipLaunchKernelGGL(radius_count_kernel, dim3(blocks(Nq * kSubR, 256)), dim3(256), 0, s, ix, queries, Nq, radius,
                       radius * radius, inv_h, counts);
    return launched();
}

extern "C" int misplat_pointcloud_outlier_mask(const float* avg, int64_t n_points, double std_ratio, void* workspace,
                                               int64_t workspace_bytes, uint8_t* keep, misplat_stream_t stream) {
    const int64_t N = n_points;
    if (!sizes_ok(N) || N < 1 || !(std_ratio == std_ratio) || !avg || !workspace || !keep) return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, N, kKindOutlier);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = (N + 255) / 256;
    for (int pass = 0; pass < 2; pass++) {
        hipLaunchKernelGGL(stat_partial_kernel, dim3((unsigned)nb), dim3(256), 0, s, avg, N, pass, (const double*)W.stats, W.part);
        hipLaunchKernelGGL((sum_final_kernel<2, 256>), dim3(1), dim3(256), 0, s, (const double*)W.part, nb, W.stats + 2 * pass);
    }
    hipLaunchKernelGGL(outlier_mask_kernel, dim3(blocks(N, 256)), dim3(256), 0, s, avg, N, std_ratio, W.stats, keep);
    return launched();
}

extern "C" int misplat_pointcloud_voxel_group(const float* points, int64_t n_points, double origin_x, double origin_y,
                                              double origin_z, double voxel_size, void* workspace, int64_t workspace_bytes,
                                              int32_t* order, int32_t* offsets, int32_t* n_voxels, misplat_stream_t stream) {
    const int64_t N = n_points;
    if (!sizes_ok(N) || N < 1 || !(voxel_size > 0.0) || !(voxel_size < 1e300) || !points || !workspace || !order || !offsets ||
        !n_voxels)
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, N, kKindVoxel);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const unsigned nb = blocks(N, 256);
    misplat_internal::fill_bytes(W.vkeys, 8 * W.cap, 0xffffffffu, s);
    misplat_internal::fill_bytes(W.first, 4 * W.cap, 0x7fffffffu, s);
    hipLaunchKernelGGL(voxel_insert_kernel, dim3(nb), dim3(256), 0, s, points, N, origin_x, origin_y, origin_z, voxel_size, W.vkeys,
                       (uint32_t)(W.cap - 1), W.vslot, W.first);
    hipLaunchKernelGGL(voxel_flag_kernel, dim3(nb), dim3(256), 0, s, (const int32_t*)W.vslot, (const int32_t*)W.first, N, W.flag);
    scan(W.flag, N, W.rank, W.scr, s);
    int32_t *ka = W.ka, *va = W.va, *kb = W.kb, *vb = W.vb;
    hipLaunchKernelGGL(voxel_key_kernel, dim3(nb), dim3(256), 0, s, (const int32_t*)W.vslot, (const int32_t*)W.first,
                       (const int32_t*)W.rank, N, ka, va, n_voxels);
    radix_sort(ka, va, kb, vb, N, radix_passes(N - 1), W.sort, W.scr, s);      // (the keys are voxel numbers: 0 .. N - 1)
    hipLaunchKernelGGL(voxel_finish_kernel, dim3(blocks(N + 1, 256)), dim3(256), 0, s, (const int32_t*)ka, (const int32_t*)va, N,
                       order, offsets);
    return launched();
}

extern "C" int misplat_pointcloud_voxel_mean(const float* values, int64_t n_points, int32_t n_channels, const int32_t* order,
                                             const int32_t* offsets, int64_t n_voxels, float* out, misplat_stream_t stream) {
    const int64_t N = n_points, V = n_voxels;
    if (!sizes_ok(N) || N < 1 || V < 0 || V > N || n_channels < 1 || n_channels > 4096 || V * n_channels >= (1ll << 38) || !values ||
        !order || !offsets || (V > 0 && !out))
        return MISPLAT_EINVAL;
    if (V == 0) return MISPLAT_OK;
    hipLaunchKernelGGL(voxel_mean_kernel, dim3(blocks(V * n_channels, 256)), dim3(256), 0, (hipStream_t)stream, values,
                       (int)n_channels, order, offsets, V, out);
    return launched();
}
