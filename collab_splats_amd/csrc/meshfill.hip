// meshfill.hip -- hole patches at the mesh's own resolution: longest-edge bisection of a face region in
// rounds of edges that share no face, and membrane fairing (uniform-weight Jacobi with everything that is not free held
// fixed) of patches of free vertices, each to its own tolerance; at the end of the file, curvature (thin-plate) fairing by
// conjugate gradients, one persistent workgroup per patch (section 31).
//
// Semantics: tests/meshfill_restatement.py is the oracle, bit for bit.  Compiled with -ffp-contract=off: every fp32 and fp64
// expression is evaluated in the written order.  Integer atomics only (the edge table's counts and faces, the maxima of the
// displacement's bits); every fp64 sum runs over a sorted CSR row in ascending order: two runs are bitwise equal.
//
// Subdivision, one round (misplat_meshfill_round): the edge table of the current mesh -- meshclean.hip's, with the largest
// incident face beside the smallest, which names both faces of a two-face edge (facetable.h, shared with meshtri.hip, as are
// the priority and the selection); per corner the length bits of a splittable
// edge; per face the corner of its first splittable edge in priority; per face again whether that edge is first in its other
// face too (it is then selected); two scans number the selected edges and the faces they split.  The host reads the two
// totals, makes room, and misplat_meshfill_apply writes the midpoints and the faces.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"
#include "internal.h"
#include "wgprims.h"
#include "radixsort.h"
#include "unionfind.h"
#include "hashmix.h"
#include "meshedge.h"
#include "facetable.h"
#include "meshadj.h"

namespace {

// ------------------------------------------------------------------------------------------------------ selection
// sbits[h] = the fp32 bits of the length of corner h's edge if it is splittable (one incident face or two distinct ones, all
// in the region, none with a repeated corner, length > max_len), else 0 (no length above max_len > 0 has these bits)
__global__ __launch_bounds__(256) void splittable_kernel(const float* __restrict__ V, const int32_t* __restrict__ tri, int64_t T,
                                                         const uint8_t* __restrict__ region, EdgeTable E, float max_len,
                                                         uint32_t* __restrict__ sbits) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= 3 * T) return;
    const int64_t f = h / 3;
    int32_t a, b;
    corner_edge(tri, f, (int)(h - 3 * f), a, b);
    uint32_t bits = 0;
    if (a != b) {
        const int64_t s = edge_find(E, edge_key(a, b));
        const int32_t n = E.cnt[s], f0 = E.fmin[s], f1 = E.fmax[s];
        if ((n == 1 || (n == 2 && f0 != f1)) && region[f0] && region[f1] && !repeated(tri, f0) && !repeated(tri, f1)) {
            const float len = edge_length(V, a, b);
            if (len > max_len) bits = __float_as_uint(len);
        }
    }
    sbits[h] = bits;
}

__global__ void totals_kernel(const int32_t* __restrict__ spos, const int32_t* __restrict__ frank, int64_t T, int32_t* __restrict__ counts) {
    counts[0] = spos[3 * T];
    counts[1] = frank[T];
}

// ---------------------------------------------------------------------------------------------------------- landing
// one 32-bit digit of the priority of the listed edges: 0 hi, 1 lo, 2 mix, 3 the complement of the length bits
__global__ __launch_bounds__(256) void digit_kernel(const int32_t* __restrict__ tri, const uint32_t* __restrict__ sbits,
                                                    const int32_t* __restrict__ list, int64_t S, int which, int32_t* __restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    const int32_t h = list[i];
    const int64_t f = h / 3;
    int32_t a, b;
    corner_edge(tri, f, (int)(h - 3 * f), a, b);
    const PrioOf<uint32_t> p = prio_of(sbits[h], a, b);
    key[i] = (int32_t)(which == 0 ? (uint32_t)p.key : which == 1 ? (uint32_t)(p.key >> 32) : which == 2 ? p.mix : ~p.bits);
}

// the listed edges are in priority order: those from `limit` on are dropped
__global__ __launch_bounds__(256) void drop_kernel(const int32_t* __restrict__ list, int64_t S, int64_t limit, int32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < S && i >= limit) flag[list[i]] = 0;
}

__global__ __launch_bounds__(256) void restrict_kernel(int64_t T, const int32_t* __restrict__ flag, int32_t* __restrict__ owner,
                                                       int32_t* __restrict__ fsplit) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= T || owner[f] < 0 || flag[owner[f]]) return;
    owner[f] = -1;
    fsplit[f] = 0;
}

// ------------------------------------------------------------------------------------------------------------ apply
// owner slot h, number s: vertex M + s = 0.5f (x_lo + x_hi), every attribute channel the same
__global__ __launch_bounds__(256) void midpoint_kernel(float* __restrict__ V, int64_t M, const int32_t* __restrict__ tri, int64_t T,
                                                       const int32_t* __restrict__ flag, const int32_t* __restrict__ spos,
                                                       float* __restrict__ att, int D) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= 3 * T || !flag[h]) return;
    const int64_t f = h / 3;
    int32_t a, b;
    corner_edge(tri, f, (int)(h - 3 * f), a, b);
    const int64_t lo = a < b ? a : b, hi = a < b ? b : a, m = M + spos[h];
    for (int k = 0; k < 3; k++) V[3 * m + k] = 0.5f * (V[3 * lo + k] + V[3 * hi + k]);
    for (int k = 0; k < D; k++) att[m * D + k] = 0.5f * (att[lo * D + k] + att[hi * D + k]);
}

// face f = (a, b, c) rotated so that a -> b is its selected edge: (a, m, c) in slot f, (m, b, c) in slot T + rank(f)
__global__ __launch_bounds__(256) void split_kernel(int32_t* __restrict__ tri, int64_t M, int64_t T, const int32_t* __restrict__ best,
                                                    const int32_t* __restrict__ owner, const int32_t* __restrict__ spos,
                                                    const int32_t* __restrict__ frank, uint8_t* __restrict__ region,
                                                    int32_t* __restrict__ origin) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= T || owner[f] < 0) return;
    const int c = best[f];
    const int32_t a = tri[3 * f + c], b = tri[3 * f + (c + 1) % 3], d = tri[3 * f + (c + 2) % 3];
    const int32_t m = (int32_t)(M + spos[owner[f]]);
    const int64_t g = T + frank[f];
    tri[3 * f] = a; tri[3 * f + 1] = m; tri[3 * f + 2] = d;
    tri[3 * g] = m; tri[3 * g + 1] = b; tri[3 * g + 2] = d;
    region[g] = region[f];
    origin[g] = origin[f];
}

// ------------------------------------------------------------------------------------------------------- workspace
inline int64_t max2(int64_t a, int64_t b) { return a > b ? a : b; }

struct Work {
    EdgeTable edges;
    uint32_t* sbits;
    int32_t *best, *owner, *fsplit, *flag, *spos, *frank;
    int32_t *sk, *sv, *skb, *svb;                 // the landing sort of the selected edges (at most one per face)
    int32_t* scr;
    SortBufs sort;
};

inline Work carve(Carver& c, int64_t T) {
    Work W = {};
    W.edges = take_edge_table(c, T);
    W.sbits = c.take<uint32_t>(3 * T);
    W.best = c.take<int32_t>(T);
    W.owner = c.take<int32_t>(T);
    W.fsplit = c.take<int32_t>(T);
    W.flag = c.take<int32_t>(3 * T);
    W.spos = c.take<int32_t>(3 * T + 1);
    W.frank = c.take<int32_t>(T + 1);
    W.sk = c.take<int32_t>(T); W.sv = c.take<int32_t>(T); W.skb = c.take<int32_t>(T); W.svb = c.take<int32_t>(T);
    W.scr = take_scan(c, max2(3 * T + 1, 256 * ((T + kTile - 1) / kTile) + 1));
    W.sort = take_sort(c, T);
    return W;
}

inline bool sizes_ok(int64_t M, int64_t T) { return M >= 1 && M < (1ll << 31) && T >= 1 && 6 * T < (1ll << 31) - kTile; }

inline void number(const Work& W, int64_t T, int32_t* counts, hipStream_t s) {
    scan(W.flag, 3 * T, W.spos, W.scr, s);
    scan(W.fsplit, T, W.frank, W.scr, s);
    hipLaunchKernelGGL(totals_kernel, dim3(1), dim3(1), 0, s, (const int32_t*)W.spos, (const int32_t*)W.frank, T, counts);
}

// ========================================================================================================== fairing
// The free vertices in ascending order (fl[k]); a CSR of their rows only: the directed edges whose source is free, as (key =
// target, value = the source's free index), sorted by target and then stably by source; patches = the components of the free
// vertices under edges with both ends free (union-find over the free indices: a patch's root is its smallest vertex).
__global__ __launch_bounds__(256) void free_flag_kernel(const uint8_t* __restrict__ free, int64_t M, int32_t* __restrict__ f32) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < M) f32[v] = free[v] ? 1 : 0;
}

__global__ __launch_bounds__(256) void free_edge_flag_kernel(const int32_t* __restrict__ tri, int64_t E6, const uint8_t* __restrict__ free,
                                                             int32_t* __restrict__ eflag) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E6) return;
    int32_t src, tgt;
    directed(tri, e, src, tgt);
    eflag[e] = (src != tgt && free[src]) ? 1 : 0;
}

__global__ void fair_totals_kernel(const int32_t* __restrict__ fidx, int64_t M, const int32_t* __restrict__ epos, int64_t E6,
                                   int32_t* __restrict__ counts) {
    counts[0] = fidx[M];
    counts[1] = epos[E6];
}

__global__ __launch_bounds__(256) void free_edge_emit_kernel(const int32_t* __restrict__ tri, int64_t E6, const int32_t* __restrict__ eflag,
                                                             const int32_t* __restrict__ epos, const int32_t* __restrict__ fidx,
                                                             int64_t Ef, int32_t* __restrict__ tgt_out, int32_t* __restrict__ src_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E6 || !eflag[e] || epos[e] >= Ef) return;
    int32_t src, tgt;
    directed(tri, e, src, tgt);
    tgt_out[epos[e]] = tgt;
    src_out[epos[e]] = fidx[src];
}

__global__ __launch_bounds__(256) void patch_init_kernel(int64_t n, int32_t* __restrict__ parent, int32_t* __restrict__ iters,
                                                         uint32_t* __restrict__ disp) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    parent[k] = (int32_t)k;
    iters[k] = 0;
    disp[k] = 0xffffffffu;                                  // "iteration 0" moved every patch: nothing has stopped before 1
    disp[n + k] = 0u;
    disp[2 * n + k] = 0u;
}

__global__ __launch_bounds__(256) void patch_union_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ tgt, int64_t Ef,
                                                          const uint8_t* __restrict__ free, const int32_t* __restrict__ fidx,
                                                          int32_t* __restrict__ parent) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= Ef) return;
    const int32_t j = tgt[e];
    if (free[j]) (void)unite(parent, src[e], fidx[j]);
}

__global__ __launch_bounds__(256) void patch_root_kernel(const int32_t* __restrict__ parent, int64_t n, int32_t* __restrict__ root,
                                                         int32_t* __restrict__ isroot) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int32_t r = walk_root(parent, (int32_t)k);
    root[k] = r;
    isroot[k] = r == (int32_t)k ? 1 : 0;
}

__global__ __launch_bounds__(256) void patch_label_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ rank, int64_t n,
                                                          int32_t* __restrict__ pid, int32_t* __restrict__ counts) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k == 0) counts[2] = rank[n];
    if (k < n) pid[k] = rank[root[k]];
}

// What an iteration reads (built once per call, kept in the workspace).
struct Fair {
    const int32_t *fl, *rows, *nbr, *pid, *isroot;
};

// x_i' = fp32(sum_j (double) x_j / |N(i)|) over the distinct neighbours in ascending order (a repeat follows its twin); no
// neighbour: unchanged.  The row is read kRowChunk entries at a time, the entries first and then their values: loads that do
// not wait for each other (every launch finds the values cold: another XCD's L2 wrote them), then the sum in order.  (Chunks
// of 8 and of 32 measured the same on the hole-fill timing script: the rows are not what a launch waits for.)
constexpr int kRowChunk = 32;
constexpr int kLdsRowChunk = 16;                            // (the LDS kernel holds three values per entry in registers)
constexpr int32_t kNoEntry = INT32_MIN;                     // no vertex, no place in a patch and no complement of a vertex

__device__ __forceinline__ float membrane(const float* __restrict__ in, int D, int c, const Fair& F, int64_t k, float x) {
    double S = 0.0;
    int32_t cnt = 0, prev = kNoEntry;
    const int32_t r0 = F.rows[2 * k], r1 = F.rows[2 * k + 1];
    for (int32_t e0 = r0; e0 < r1; e0 += kRowChunk) {
        int32_t j[kRowChunk];
        float v[kRowChunk];
#pragma unroll
        for (int u = 0; u < kRowChunk; u++) j[u] = e0 + u < r1 ? F.nbr[e0 + u] : kNoEntry;
#pragma unroll
        for (int u = 0; u < kRowChunk; u++) v[u] = j[u] != kNoEntry ? in[(int64_t)j[u] * D + c] : 0.f;
#pragma unroll
        for (int u = 0; u < kRowChunk; u++)
            if (j[u] != kNoEntry && j[u] != prev) {
                prev = j[u];
                S += (double)v[u];
                cnt++;
            }
    }
    return cnt ? (float)(S / (double)cnt) : x;
}

// Iteration n, one lane per (free vertex k, channel c) of values [M, D].  Measured mode (fixed = 0): patch p has stopped iff
// iters[p] is set or the displacement of iteration n - 1 (d_prev, complete: the previous launch) is below the tolerance; its
// root then records n - 1 once.  A stopped patch is copied.  A running one moves, and the bits of max |x' - x| go into
// d_cur[p] by an integer maximum; the root clears d_next[p] for iteration n + 1 (d_next was last read in iteration n - 1).
// Counted mode (fixed = 1): patch p runs iff n <= iters[p].
constexpr int kStepThreads = 256;

__global__ __launch_bounds__(kStepThreads) void fair_step_kernel(const float* __restrict__ in, float* __restrict__ out, int D,
                                                                 int64_t n_free, Fair F, int32_t* __restrict__ iters,
                                                                 const uint32_t* __restrict__ d_prev, uint32_t* __restrict__ d_cur,
                                                                 uint32_t* __restrict__ d_next, uint32_t tol_bits, int32_t n, int fixed) {
    __shared__ int32_t wave_p[kStepThreads / 64];
    __shared__ uint32_t wave_m[kStepThreads / 64];
    const int64_t idx = (int64_t)blockIdx.x * kStepThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool moving = false;                                    // (no lane leaves before the workgroup's maxima below)
    int32_t p = -1;
    uint32_t bits = 0u;
    if (idx < n_free * D) {
        const int64_t k = idx / D;
        const int c = (int)(idx - k * D);
        const int64_t at = (int64_t)F.fl[k] * D + c;
        p = F.pid[k];
        // A plain load beside the root's store below: in the one launch that stores, `now` holds for every lane of the patch,
        // so either value read gives the same answer; every later launch sees the store.
        const int32_t it = iters[p];
        if (fixed) {
            moving = n <= it;
        } else {
            const bool now = d_prev[p] < tol_bits;
            moving = it == 0 && !now;
            if (c == 0 && F.isroot[k]) {
                if (it == 0 && now) iters[p] = n - 1;
                d_next[p] = 0u;
            }
        }
        const float x = in[at];
        const float y = moving ? membrane(in, D, c, F, k, x) : x;
        out[at] = y;
        bits = __float_as_uint(fabsf(y - x));
    }
    if (fixed) return;                                      // (uniform)
    // The maxima reach memory as few integer atomics as the patches allow.  A wave whose moving lanes are of one patch hands
    // (patch, maximum) to the workgroup, where lane 0 merges neighbouring waves of one patch into one atomic; a wave of several
    // patches (subdivision numbers a round's vertices across all holes, so late rounds interleave the patches in the list)
    // issues one per lane, and none where the patch's word is already as large.
    const unsigned long long mv = __ballot(moving);
    int32_t wp = -1;
    uint32_t m = 0u;
    if (mv) {
        const int leader = __ffsll((long long)mv) - 1;
        const int32_t p0 = __shfl(p, leader);
        if (__ballot(moving && p != p0) == 0ull) {
            wp = p0;
            m = wave_max(moving ? bits : 0u);
        } else if (moving && bits > __hip_atomic_load(d_cur + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            atomicMax(d_cur + p, bits);                     // (none where the patch's word is already as large)
        }
    }
    if (lane == 0) { wave_p[threadIdx.x >> 6] = wp; wave_m[threadIdx.x >> 6] = m; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t cp = -1;
        uint32_t cm = 0u;
        for (int w = 0; w < kStepThreads / 64; w++) {
            if (wave_p[w] < 0) continue;
            if (wave_p[w] != cp) {
                if (cp >= 0) atomicMax(d_cur + cp, cm);
                cp = wave_p[w];
                cm = 0u;
            }
            cm = wave_m[w] > cm ? wave_m[w] : cm;
        }
        if (cp >= 0) atomicMax(d_cur + cp, cm);
    }
}

// counts[3] = the patches that are still running after the iteration whose displacements are d_last
__global__ __launch_bounds__(256) void running_kernel(const int32_t* __restrict__ iters, const uint32_t* __restrict__ d_last,
                                                      uint32_t tol_bits, int32_t* __restrict__ counts) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < counts[2] && iters[p] == 0 && !(d_last[p] < tol_bits)) atomicAdd(&counts[3], 1);
}

// a patch that was never seen stopped took every iteration that ran
__global__ __launch_bounds__(256) void finish_kernel(int32_t* __restrict__ iters, int32_t n_done, const int32_t* __restrict__ counts) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < counts[2] && iters[p] == 0) iters[p] = n_done;
}


// ------------------------------------------------------------------------------------------------------- LDS path
// A patch of at most MISPLAT_MESHFILL_LDS_VERTICES free vertices runs ALL its iterations in one workgroup: both iterates of
// its vertices in LDS (24 B a vertex), a barrier between iterations instead of a launch.  The patch's vertices are listed by
// patch (plist, prow); every CSR entry is translated once (lnbr): >= 0 the neighbour's place in its patch's list (a free
// neighbour is in the same patch by definition), < 0 the complement of a fixed vertex, read from memory (it never changes).
// Same rows, same order, same arithmetic as fair_step_kernel: the same bits and the same iteration counts.
constexpr int kLdsVertices = MISPLAT_MESHFILL_LDS_VERTICES;
constexpr int kLdsThreads = 1024;

__global__ __launch_bounds__(256) void patch_keys_kernel(const int32_t* __restrict__ pid, int64_t n, int32_t* __restrict__ key,
                                                         int32_t* __restrict__ val) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) { key[k] = pid[k]; val[k] = (int32_t)k; }
}

__global__ __launch_bounds__(256) void patch_place_kernel(const int32_t* __restrict__ plist, const int32_t* __restrict__ pkey,
                                                          const int32_t* __restrict__ prow, int64_t n, int32_t* __restrict__ loc) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q < n) loc[plist[q]] = (int32_t)(q - prow[2 * (int64_t)pkey[q]]);
}

__global__ __launch_bounds__(256) void local_edges_kernel(const int32_t* __restrict__ nbr, int64_t Ef, const int32_t* __restrict__ f32,
                                                          const int32_t* __restrict__ fidx, const int32_t* __restrict__ loc,
                                                          int32_t* __restrict__ lnbr) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= Ef) return;
    const int32_t j = nbr[e];
    lnbr[e] = f32[j] ? loc[fidx[j]] : ~j;
}

__global__ __launch_bounds__(kLdsThreads) void fair_lds_kernel(float* __restrict__ pos, Fair F, const int32_t* __restrict__ plist,
                                                               const int32_t* __restrict__ prow, const int32_t* __restrict__ lnbr,
                                                               uint32_t tol_bits, int32_t max_it, int32_t* __restrict__ iters,
                                                               int32_t* __restrict__ counts) {
    __shared__ float X[2][3 * kLdsVertices];
    __shared__ uint32_t wmax[kLdsThreads / 64];
    const int32_t p = blockIdx.x;
    const int32_t k0 = prow[2 * (int64_t)p], nv = prow[2 * (int64_t)p + 1] - k0;
    if (nv > kLdsVertices) {                                     // (uniform) left to the launches per iteration
        if (threadIdx.x == 0) atomicAdd(&counts[3], 1);
        return;
    }
    for (int32_t idx = threadIdx.x; idx < 3 * nv; idx += kLdsThreads) {
        const int32_t l = idx / 3;
        X[0][idx] = pos[3 * (int64_t)F.fl[plist[k0 + l]] + (idx - 3 * l)];
    }
    __syncthreads();
    int32_t it = 0;
    while (it < max_it) {
        const float* in = X[it & 1];
        float* out = X[(it & 1) ^ 1];
        uint32_t mine = 0u;
        for (int32_t l = threadIdx.x; l < nv; l += kLdsThreads) {            // one lane per vertex: its row is read once
            const int64_t k = plist[k0 + l];
            double S[3] = {0.0, 0.0, 0.0};
            int32_t cnt = 0, prev = kNoEntry;
            const int32_t r0 = F.rows[2 * k], r1 = F.rows[2 * k + 1];
            for (int32_t e0 = r0; e0 < r1; e0 += kLdsRowChunk) {              // as membrane(): entries, then values, then the sum
                int32_t q[kLdsRowChunk];
                float v[kLdsRowChunk][3];
#pragma unroll
                for (int u = 0; u < kLdsRowChunk; u++) q[u] = e0 + u < r1 ? lnbr[e0 + u] : kNoEntry;
#pragma unroll
                for (int u = 0; u < kLdsRowChunk; u++) {
                    const float* from = q[u] >= 0 ? in + 3 * q[u] : q[u] != kNoEntry ? pos + 3 * (int64_t)(~q[u]) : in;
#pragma unroll
                    for (int c = 0; c < 3; c++) v[u][c] = from[c];
                }
#pragma unroll
                for (int u = 0; u < kLdsRowChunk; u++)
                    if (q[u] != kNoEntry && q[u] != prev) {
                        prev = q[u];
#pragma unroll
                        for (int c = 0; c < 3; c++) S[c] += (double)v[u][c];
                        cnt++;
                    }
            }
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float x = in[3 * l + c];
                const float y = cnt ? (float)(S[c] / (double)cnt) : x;
                out[3 * l + c] = y;
                const uint32_t bits = __float_as_uint(fabsf(y - x));
                mine = bits > mine ? bits : mine;
            }
        }
        mine = wave_max(mine);
        if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mine;
        __syncthreads();                                         // the new iterate and the waves' maxima are written
        uint32_t all = 0u;
#pragma unroll
        for (int w = 0; w < kLdsThreads / 64; w++) all = wmax[w] > all ? wmax[w] : all;
        __syncthreads();                                         // wmax is read before the next iteration writes it
        it++;
        if (all < tol_bits) break;                               // (uniform)
    }
    const float* fin = X[it & 1];
    for (int32_t idx = threadIdx.x; idx < 3 * nv; idx += kLdsThreads) {
        const int32_t l = idx / 3;
        pos[3 * (int64_t)F.fl[plist[k0 + l]] + (idx - 3 * l)] = fin[idx];
    }
    if (threadIdx.x == 0) iters[p] = it;
}

struct FairWork {
    int32_t *f32, *fidx, *eflag, *epos;           // the part the count call uses: M and T alone size it
    int32_t *fl, *ka, *va, *kb, *vb, *rows, *parent, *root, *isroot, *rank, *pid;
    uint32_t* disp;                               // three rotating rows [n_free] of displacement bits, one entry per patch
    int32_t *pk, *pv, *pkb, *pvb, *prow, *loc, *lnbr;     // the LDS path: the free vertices by patch, the translated entries
    int32_t* scr;
    SortBufs sort;
};

inline FairWork carve_fair(Carver& c, int64_t M, int64_t T, int64_t n, int64_t Ef) {
    FairWork W = {};
    W.f32 = c.take<int32_t>(M);
    W.fidx = c.take<int32_t>(M + 1);
    W.eflag = c.take<int32_t>(6 * T);
    W.epos = c.take<int32_t>(6 * T + 1);
    const int64_t most = max2(n, Ef);                           // (both sorts: the edges, the free vertices by patch)
    W.scr = take_scan(c, max2(max2(M, 6 * T), max2(n, 256 * ((most + kTile - 1) / kTile)) + 1));
    W.fl = c.take<int32_t>(n);
    W.ka = c.take<int32_t>(Ef); W.va = c.take<int32_t>(Ef); W.kb = c.take<int32_t>(Ef); W.vb = c.take<int32_t>(Ef);
    W.rows = c.take<int32_t>(2 * n);
    W.parent = c.take<int32_t>(n);
    W.root = c.take<int32_t>(n);
    W.isroot = c.take<int32_t>(n);
    W.rank = c.take<int32_t>(n + 1);
    W.pid = c.take<int32_t>(n);
    W.disp = c.take<uint32_t>(3 * n);
    W.pk = c.take<int32_t>(n); W.pv = c.take<int32_t>(n); W.pkb = c.take<int32_t>(n); W.pvb = c.take<int32_t>(n);
    W.prow = c.take<int32_t>(2 * n);
    W.loc = c.take<int32_t>(n);
    W.lnbr = c.take<int32_t>(Ef);
    W.sort = take_sort(c, most);
    return W;
}

inline bool fair_ok(int64_t M, int64_t T, int64_t n, int64_t Ef) {
    return M >= 1 && M < (1ll << 31) && T >= 0 && 6 * T < (1ll << 31) - kTile && n >= 0 && n <= M && Ef >= 0 && Ef <= 6 * T;
}

// the free indices and the edge positions (two scans)
inline void fair_scans(const FairWork& W, const int32_t* tri, int64_t T, const uint8_t* free, int64_t M, hipStream_t s) {
    hipLaunchKernelGGL(free_flag_kernel, dim3(blocks(M, 256)), dim3(256), 0, s, free, M, W.f32);
    scan(W.f32, M, W.fidx, W.scr, s);
    if (T > 0) hipLaunchKernelGGL(free_edge_flag_kernel, dim3(blocks(6 * T, 256)), dim3(256), 0, s, tri, 6 * T, free, W.eflag);
    scan(W.eflag, 6 * T, W.epos, W.scr, s);
}

// the sorted targets (the rows' entries), where the two sorts of the build left them
inline const int32_t* sorted_targets(const FairWork& W, int64_t M, int64_t n) {
    int32_t *ka = W.ka, *va = W.va, *kb = W.kb, *vb = W.vb;
    sorted_directed_names(ka, va, kb, vb, radix_passes(M - 1), radix_passes(n - 1));
    return ka;
}

}  // namespace

extern "C" int64_t misplat_meshfill_workspace(int64_t n_vertices, int64_t n_triangles) {
    if (!sizes_ok(n_vertices, n_triangles)) return -1;
    Carver c{nullptr};
    carve(c, n_triangles);
    return c.o;
}

extern "C" int misplat_meshfill_round(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                      const uint8_t* region, float max_edge_len, void* workspace, int64_t workspace_bytes,
                                      int32_t* counts, misplat_stream_t stream) {
    const int64_t M = n_vertices, T = n_triangles;
    if (!sizes_ok(M, T) || !(max_edge_len > 0.f) || !vertices || !triangles || !region || !workspace || !counts) return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, T);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const unsigned nh = blocks(3 * T, 256), nf = blocks(T, 256);
    const EdgeTable& E = W.edges;
    build_edge_table(triangles, T, E, s);
    hipLaunchKernelGGL(splittable_kernel, dim3(nh), dim3(256), 0, s, vertices, triangles, T, region, E, max_edge_len, W.sbits);
    hipLaunchKernelGGL(face_best_kernel<uint32_t>, dim3(nf), dim3(256), 0, s, triangles, T, (const uint32_t*)W.sbits, W.best);
    hipLaunchKernelGGL(select_kernel, dim3(nf), dim3(256), 0, s, triangles, T, E, (const int32_t*)W.best, W.owner, W.fsplit, W.flag);
    number(W, T, counts, s);
    return launched();
}

extern "C" int misplat_meshfill_apply(float* vertices, int64_t n_vertices, int32_t* triangles, int64_t n_triangles, uint8_t* region,
                                      int32_t* origin, float* attributes, int32_t n_channels, int64_t n_selected, int64_t limit,
                                      void* workspace, int64_t workspace_bytes, int32_t* counts, misplat_stream_t stream) {
    const int64_t M = n_vertices, T = n_triangles, S = n_selected;
    const int D = n_channels;
    if (!sizes_ok(M, T) || S < 1 || S > T || M + S >= (1ll << 31) || limit == 0 || limit > S || D < 0 || D > 4096 ||
        (M + S) * (int64_t)(D > 3 ? D : 3) >= (1ll << 39) || !vertices || !triangles || !region || !origin || (D > 0 && !attributes) ||
        !workspace || !counts)
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, T);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const unsigned nh = blocks(3 * T, 256), nf = blocks(T, 256);
    if (limit > 0 && limit < S) {
        // Only the `limit` first in priority: the owner slots in slot order, sorted stably by the four 32-bit digits of the
        // priority from the least significant on (hi, lo, the mixed key, the complement of the length bits).
        int32_t *sk = W.sk, *sv = W.sv, *skb = W.skb, *svb = W.svb;
        misplat_internal::fill_bytes(sv, 4 * (size_t)S, 0u, s);         // (a wrong n_selected reads slot 0)
        hipLaunchKernelGGL(compact_kernel<int32_t>, dim3(nh), dim3(256), 0, s, (const int32_t*)W.flag, (const int32_t*)W.spos, 3 * T, S,
                           sv);                                         // (the owner slots in slot order)
        const SortBufs sb = sort_for(W.sort, S);
        const int index_passes = radix_passes(M - 1);
        for (int which = 0; which < 4; which++) {
            hipLaunchKernelGGL(digit_kernel, dim3(blocks(S, 256)), dim3(256), 0, s, (const int32_t*)triangles, (const uint32_t*)W.sbits,
                               (const int32_t*)sv, S, which, sk);
            radix_sort(sk, sv, skb, svb, S, which < 2 ? index_passes : 4, sb, W.scr, s);
        }
        hipLaunchKernelGGL(drop_kernel, dim3(blocks(S, 256)), dim3(256), 0, s, (const int32_t*)sv, S, limit, W.flag);
        hipLaunchKernelGGL(restrict_kernel, dim3(nf), dim3(256), 0, s, T, (const int32_t*)W.flag, W.owner, W.fsplit);
        number(W, T, counts, s);
    }
    hipLaunchKernelGGL(midpoint_kernel, dim3(nh), dim3(256), 0, s, vertices, M, (const int32_t*)triangles, T, (const int32_t*)W.flag,
                       (const int32_t*)W.spos, attributes, D);
    hipLaunchKernelGGL(split_kernel, dim3(nf), dim3(256), 0, s, triangles, M, T, (const int32_t*)W.best, (const int32_t*)W.owner,
                       (const int32_t*)W.spos, (const int32_t*)W.frank, region, origin);
    return launched();
}

extern "C" int64_t misplat_meshfill_fair_workspace(int64_t n_vertices, int64_t n_triangles, int64_t n_free, int64_t n_edges) {
    if (!fair_ok(n_vertices, n_triangles, n_free, n_edges)) return -1;
    Carver c{nullptr};
    carve_fair(c, n_vertices, n_triangles, n_free, n_edges);
    return c.o;
}

extern "C" int misplat_meshfill_fair_count(const int32_t* triangles, int64_t n_triangles, const uint8_t* free, int64_t n_vertices,
                                           void* workspace, int64_t workspace_bytes, int32_t* counts, misplat_stream_t stream) {
    const int64_t M = n_vertices, T = n_triangles;
    if (!fair_ok(M, T, 0, 0) || !free || (T > 0 && !triangles) || !workspace || !counts) return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const FairWork W = carve_fair(c, M, T, 0, 0);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    fair_scans(W, triangles, T, free, M, s);
    hipLaunchKernelGGL(fair_totals_kernel, dim3(1), dim3(1), 0, s, (const int32_t*)W.fidx, M, (const int32_t*)W.epos, 6 * T, counts);
    return launched();
}

extern "C" int misplat_meshfill_fair_build(const int32_t* triangles, int64_t n_triangles, const uint8_t* free, int64_t n_vertices,
                                           int64_t n_free, int64_t n_edges, void* workspace, int64_t workspace_bytes, int32_t* iterations,
                                           int32_t* counts, misplat_stream_t stream) {
    const int64_t M = n_vertices, T = n_triangles, n = n_free, Ef = n_edges;
    if (!fair_ok(M, T, n, Ef) || n < 1 || !free || (T > 0 && !triangles) || !workspace || !iterations || !counts) return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const FairWork W = carve_fair(c, M, T, n, Ef);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    fair_scans(W, triangles, T, free, M, s);
    const unsigned nk = blocks(n, 256);
    misplat_internal::fill_bytes(W.fl, 4 * (size_t)n, 0u, s);           // (a wrong n_free reads vertex 0, never beyond the list)
    hipLaunchKernelGGL(compact_kernel<int32_t>, dim3(blocks(M, 256)), dim3(256), 0, s, (const int32_t*)W.f32, (const int32_t*)W.fidx, M, n,
                       W.fl);
    hipLaunchKernelGGL(patch_init_kernel, dim3(nk), dim3(256), 0, s, n, W.parent, iterations, W.disp);
    misplat_internal::fill_bytes(W.rows, 8 * (size_t)n, 0u, s);
    if (Ef > 0) {
        int32_t *ka = W.ka, *va = W.va, *kb = W.kb, *vb = W.vb;
        misplat_internal::fill_bytes(ka, 4 * (size_t)Ef, 0u, s);        // (a wrong n_edges leaves edges 0 -> 0 of free vertex 0)
        misplat_internal::fill_bytes(va, 4 * (size_t)Ef, 0u, s);
        hipLaunchKernelGGL(free_edge_emit_kernel, dim3(blocks(6 * T, 256)), dim3(256), 0, s, triangles, 6 * T, (const int32_t*)W.eflag,
                           (const int32_t*)W.epos, (const int32_t*)W.fidx, Ef, ka, va);
        sort_directed(ka, va, kb, vb, Ef, radix_passes(M - 1), radix_passes(n - 1), W.sort, W.scr, s);     // va sources, ka targets
        hipLaunchKernelGGL(rows_kernel, dim3(blocks(Ef, 256)), dim3(256), 0, s, (const int32_t*)va, Ef, W.rows);
        hipLaunchKernelGGL(patch_union_kernel, dim3(blocks(Ef, 256)), dim3(256), 0, s, (const int32_t*)va, (const int32_t*)ka, Ef, free,
                           (const int32_t*)W.fidx, W.parent);
    }
    hipLaunchKernelGGL(patch_root_kernel, dim3(nk), dim3(256), 0, s, (const int32_t*)W.parent, n, W.root, W.isroot);
    scan(W.isroot, n, W.rank, W.scr, s);
    hipLaunchKernelGGL(patch_label_kernel, dim3(nk), dim3(256), 0, s, (const int32_t*)W.root, (const int32_t*)W.rank, n, W.pid, counts);
    return launched();
}

extern "C" int misplat_meshfill_fair_step(float* values_a, float* values_b, int64_t n_vertices, int64_t n_triangles, int32_t n_channels,
                                          int64_t n_free, int64_t n_edges, int32_t first, int32_t count, float tolerance, int32_t fixed,
                                          void* workspace, int64_t workspace_bytes, int32_t* iterations, int32_t* counts,
                                          misplat_stream_t stream) {
    const int64_t M = n_vertices, T = n_triangles, n = n_free, Ef = n_edges;
    const int D = n_channels;
    if (!fair_ok(M, T, n, Ef) || n < 1 || D < 1 || D > 4096 || M * (int64_t)D >= (1ll << 39) || first < 1 || count < 1 ||
        (int64_t)first + count > (1ll << 31) - 1 || !(tolerance > 0.f) || !values_a || !values_b || !workspace || !iterations || !counts)
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const FairWork W = carve_fair(c, M, T, n, Ef);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const Fair F{W.fl, W.rows, sorted_targets(W, M, n), W.pid, W.isroot};
    uint32_t tol_bits;
    __builtin_memcpy(&tol_bits, &tolerance, 4);
    const unsigned nb = blocks(n * D, kStepThreads);
    for (int32_t it = first; it < first + count; it++) {
        const float* in = (it & 1) ? values_a : values_b;       // iteration 1 reads a
        float* out = (it & 1) ? values_b : values_a;
        hipLaunchKernelGGL(fair_step_kernel, dim3(nb), dim3(kStepThreads), 0, s, in, out, D, n, F, iterations,
                           (const uint32_t*)(W.disp + (int64_t)((it + 2) % 3) * n), W.disp + (int64_t)(it % 3) * n,
                           W.disp + (int64_t)((it + 1) % 3) * n, tol_bits, it, (int)(fixed != 0));
    }
    if (!fixed) {
        const int32_t last = first + count - 1;
        misplat_internal::fill_bytes(counts + 3, 4, 0u, s);
        hipLaunchKernelGGL(running_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, (const int32_t*)iterations,
                           (const uint32_t*)(W.disp + (int64_t)(last % 3) * n), tol_bits, counts);
    }
    return launched();
}

extern "C" int misplat_meshfill_fair_lds(float* vertices, int64_t n_vertices, int64_t n_triangles, int64_t n_free, int64_t n_edges,
                                         int32_t n_patches, float tolerance, int32_t max_iterations, void* workspace,
                                         int64_t workspace_bytes, int32_t* iterations, int32_t* counts, misplat_stream_t stream) {
    const int64_t M = n_vertices, T = n_triangles, n = n_free, Ef = n_edges;
    if (!fair_ok(M, T, n, Ef) || n < 1 || n_patches < 1 || n_patches > n || !(tolerance > 0.f) || max_iterations < 1 || !vertices ||
        !workspace || !iterations || !counts)
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const FairWork W = carve_fair(c, M, T, n, Ef);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const Fair F{W.fl, W.rows, sorted_targets(W, M, n), W.pid, W.isroot};
    uint32_t tol_bits;
    __builtin_memcpy(&tol_bits, &tolerance, 4);
    const unsigned nk = blocks(n, 256);
    int32_t *pk = W.pk, *pv = W.pv, *pkb = W.pkb, *pvb = W.pvb;
    hipLaunchKernelGGL(patch_keys_kernel, dim3(nk), dim3(256), 0, s, (const int32_t*)W.pid, n, pk, pv);
    radix_sort(pk, pv, pkb, pvb, n, radix_passes(n_patches - 1), sort_for(W.sort, n), W.scr, s);    // (a patch's vertices stay ascending)
    misplat_internal::fill_bytes(W.prow, 8 * (size_t)n, 0u, s);
    hipLaunchKernelGGL(rows_kernel, dim3(nk), dim3(256), 0, s, (const int32_t*)pk, n, W.prow);
    hipLaunchKernelGGL(patch_place_kernel, dim3(nk), dim3(256), 0, s, (const int32_t*)pv, (const int32_t*)pk, (const int32_t*)W.prow, n,
                       W.loc);
    if (Ef > 0)
        hipLaunchKernelGGL(local_edges_kernel, dim3(blocks(Ef, 256)), dim3(256), 0, s, F.nbr, Ef, (const int32_t*)W.f32,
                           (const int32_t*)W.fidx, (const int32_t*)W.loc, W.lnbr);
    misplat_internal::fill_bytes(counts + 3, 4, 0u, s);
    hipLaunchKernelGGL(fair_lds_kernel, dim3((unsigned)n_patches), dim3(kLdsThreads), 0, s, vertices, F, (const int32_t*)pv,
                       (const int32_t*)W.prow, (const int32_t*)W.lnbr, tol_bits, max_iterations, iterations, counts);
    return launched();
}

extern "C" int misplat_meshfill_fair_finish(int64_t n_free, int32_t n_done, int32_t* iterations, const int32_t* counts,
                                            misplat_stream_t stream) {
    if (n_free < 1 || n_free >= (1ll << 31) || n_done < 0 || !iterations || !counts) return MISPLAT_EINVAL;
    hipLaunchKernelGGL(finish_kernel, dim3(blocks(n_free, 256)), dim3(256), 0, (hipStream_t)stream, iterations, n_done, counts);
    return launched();
}

// ================================================================================================ curvature fairing
// Thin-plate fairing of the free vertices: the energy sum over S of |U_i|^2, U the umbrella operator, S the
// free vertices F and the fixed vertices R with a free neighbour, minimised over the free coordinates by conjugate gradients
// on A = L^T L.  The oracle is tests/meshsmooth_restatement.py, bit for bit.
//
// The S-list holds the free vertices by patch and then by vertex (places 0 .. nF - 1), then the rows of R the same way (places nF
// .. nS - 1); a CSR row per place lists its vertex's distinct neighbours in ascending order, as vertices (nbr) and as places
// (place: -1 for a fixed vertex outside S).  One persistent workgroup per patch runs the whole solve: x, r, p, q over the
// patch's free places and t, t / n over its places of S are its part of the workspace, touched by this workgroup only and read
// after the barrier that follows their writes; every dot product is summed in a fixed order (thread t adds the patch's elements
// t, t + B, ... in ascending order, then block_sum); alpha, beta and the stop are computed once by thread 0 and broadcast from
// LDS, so the loop's bound and exit are uniform and every barrier sits outside divergent code.
namespace {

constexpr int kCgThreads = 1024;

__global__ __launch_bounds__(256) void curv_union_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ tgt, int64_t n_edges,
                                                         const uint8_t* __restrict__ free, int64_t M, int32_t* __restrict__ parent) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const int32_t a = src[e], b = tgt[e];
    if (a < 0 || a >= M || b < 0 || b >= M || !free[b]) return;
    (void)unite(parent, a, b);                                  // a row of S and a free neighbour of it: one patch
}

__global__ __launch_bounds__(256) void curv_root_kernel(const int32_t* __restrict__ parent, int64_t M, int32_t* __restrict__ root) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= M) return;
    root[v] = walk_root(parent, (int32_t)v);
}

struct Curv {
    const int32_t *foff, *roff, *vertex, *row, *deg, *nbr, *place, *code;
    int64_t nF, nS;
    double *x, *r, *p, *q, *t, *tn;
};

struct CurvCtl {
    double alpha[3], beta[3], rr[3], rr0, ratio;
    int32_t stop;
};

// place number idx of patch p's part of the S-list: its free places first, then its rows of R
__device__ __forceinline__ int64_t curv_place(const Curv& C, int32_t f0, int32_t nf, int32_t r0, int32_t idx) {
    return idx < nf ? (int64_t)f0 + idx : C.nF + r0 + (idx - nf);
}

__global__ __launch_bounds__(kCgThreads) void curv_solve_kernel(const float* __restrict__ pos, float* __restrict__ out, Curv C,
                                                                double rtol2, int32_t max_it, int32_t* __restrict__ iterations,
                                                                uint8_t* __restrict__ converged, double* __restrict__ residual) {
    __shared__ double sh[kCgThreads / 64];
    __shared__ CurvCtl ctl;
    const int32_t pt = blockIdx.x, tid = threadIdx.x;
    const int32_t f0 = C.foff[pt], nf = C.foff[pt + 1] - f0, r0 = C.roff[pt], nr = C.roff[pt + 1] - r0;
    bool ok = C.code[pt] == 0 && f0 >= 0 && nf >= 1 && (int64_t)f0 + nf <= C.nF && r0 >= 0 && nr >= 0 && C.nF + r0 + nr <= C.nS;
    if (!ok) {                                                  // (uniform) codes 1, 2, 3: unchanged
        if (tid == 0) { iterations[pt] = 0; converged[pt] = 0; residual[pt] = 0.0; }
        return;
    }
    const int32_t ns = nf + nr;
    const int32_t limit = max_it < 0 ? nf : max_it;
    // t = U(x0) over the patch's places of S, from the fp32 positions
    for (int32_t idx = tid; idx < ns; idx += kCgThreads) {
        const int64_t s = curv_place(C, f0, nf, r0, idx);
        const int64_t v = C.vertex[s];
        const int32_t e0 = C.row[s], n = C.deg[s];
        double sum[3] = {0.0, 0.0, 0.0};
        for (int32_t e = e0; e < e0 + n; e++) {
            const int64_t j = C.nbr[e];
            for (int c = 0; c < 3; c++) sum[c] += (double)pos[3 * j + c];
        }
        for (int c = 0; c < 3; c++) {
            const double t = sum[c] / (double)n - (double)pos[3 * v + c];
            C.t[3 * s + c] = t;
            C.tn[3 * s + c] = t / (double)n;
        }
    }
    __syncthreads();
    // r0 = -L^T t, p = r, x = x0
    double acc[3] = {0.0, 0.0, 0.0};
    for (int32_t idx = tid; idx < nf; idx += kCgThreads) {
        const int64_t s = (int64_t)f0 + idx;
        const int64_t v = C.vertex[s];
        const int32_t e0 = C.row[s], n = C.deg[s];
        double sum[3] = {0.0, 0.0, 0.0};
        for (int32_t e = e0; e < e0 + n; e++) {
            const int64_t j = C.place[e];
            for (int c = 0; c < 3; c++) sum[c] += C.tn[3 * j + c];
        }
        for (int c = 0; c < 3; c++) {
            const double r = -(sum[c] - C.t[3 * s + c]);
            C.x[3 * s + c] = (double)pos[3 * v + c];
            C.r[3 * s + c] = r;
            C.p[3 * s + c] = r;
            acc[c] += r * r;
        }
    }
    double rr[3];
    for (int c = 0; c < 3; c++) rr[c] = block_sum<kCgThreads / 64>(acc[c], sh);
    if (tid == 0) {
        for (int c = 0; c < 3; c++) ctl.rr[c] = rr[c];
        ctl.rr0 = (rr[0] + rr[1]) + rr[2];
        ctl.ratio = 0.0;
        ctl.stop = ctl.rr0 == 0.0 ? 1 : 0;                      // a right-hand side of 0: no iteration
    }
    __syncthreads();
    int32_t it = 0;
    while (it < limit && !ctl.stop) {                           // (uniform: ctl is written by thread 0 between barriers)
        // t = L p over the places of S (p is zero off F)
        for (int32_t idx = tid; idx < ns; idx += kCgThreads) {
            const int64_t s = curv_place(C, f0, nf, r0, idx);
            const int32_t e0 = C.row[s], n = C.deg[s];
            double sum[3] = {0.0, 0.0, 0.0};
            for (int32_t e = e0; e < e0 + n; e++) {
                const int64_t j = C.place[e];
                if (j >= 0 && j < C.nF)
                    for (int c = 0; c < 3; c++) sum[c] += C.p[3 * j + c];
            }
            for (int c = 0; c < 3; c++) {
                double t = sum[c] / (double)n;
                if (idx < nf) t = t - C.p[3 * s + c];
                C.t[3 * s + c] = t;
                C.tn[3 * s + c] = t / (double)n;
            }
        }
        __syncthreads();
        // q = L^T t over the free places, and p . q
        for (int c = 0; c < 3; c++) acc[c] = 0.0;
        for (int32_t idx = tid; idx < nf; idx += kCgThreads) {
            const int64_t s = (int64_t)f0 + idx;
            const int32_t e0 = C.row[s], n = C.deg[s];
            double sum[3] = {0.0, 0.0, 0.0};
            for (int32_t e = e0; e < e0 + n; e++) {
                const int64_t j = C.place[e];
                for (int c = 0; c < 3; c++) sum[c] += C.tn[3 * j + c];
            }
            for (int c = 0; c < 3; c++) {
                const double q = sum[c] - C.t[3 * s + c];
                C.q[3 * s + c] = q;
                acc[c] += C.p[3 * s + c] * q;
            }
        }
        double pq[3];
        for (int c = 0; c < 3; c++) pq[c] = block_sum<kCgThreads / 64>(acc[c], sh);
        if (tid == 0)
            for (int c = 0; c < 3; c++) ctl.alpha[c] = pq[c] == 0.0 ? 0.0 : ctl.rr[c] / pq[c];
        __syncthreads();
        for (int c = 0; c < 3; c++) acc[c] = 0.0;
        for (int32_t idx = tid; idx < nf; idx += kCgThreads) {
            const int64_t s = (int64_t)f0 + idx;
            for (int c = 0; c < 3; c++) {
                const double a = ctl.alpha[c];
                C.x[3 * s + c] = C.x[3 * s + c] + a * C.p[3 * s + c];
                const double r = C.r[3 * s + c] - a * C.q[3 * s + c];
                C.r[3 * s + c] = r;
                acc[c] += r * r;
            }
        }
        for (int c = 0; c < 3; c++) rr[c] = block_sum<kCgThreads / 64>(acc[c], sh);
        if (tid == 0) {
            for (int c = 0; c < 3; c++) {
                ctl.beta[c] = pq[c] == 0.0 ? 0.0 : rr[c] / ctl.rr[c];
                ctl.rr[c] = rr[c];
            }
            const double now = (rr[0] + rr[1]) + rr[2];
            ctl.ratio = now / ctl.rr0;
            ctl.stop = now <= rtol2 * ctl.rr0 ? 1 : 0;
        }
        __syncthreads();
        for (int32_t idx = tid; idx < nf; idx += kCgThreads) {
            const int64_t s = (int64_t)f0 + idx;
            for (int c = 0; c < 3; c++) C.p[3 * s + c] = C.r[3 * s + c] + ctl.beta[c] * C.p[3 * s + c];
        }
        it++;
        __syncthreads();                                        // p is written before the next pass gathers it; ctl is read
    }
    if (it > 0)
        for (int32_t idx = tid; idx < nf; idx += kCgThreads) {
            const int64_t s = (int64_t)f0 + idx;
            const int64_t v = C.vertex[s];
            for (int c = 0; c < 3; c++) out[3 * v + c] = (float)C.x[3 * s + c];
        }
    if (tid == 0) {
        iterations[pt] = it;
        converged[pt] = (uint8_t)ctl.stop;
        residual[pt] = sqrt(ctl.ratio);
    }
}

inline bool curv_ok(int64_t M, int64_t nF, int64_t nS, int64_t nE, int64_t P) {
    return M >= 1 && M < (1ll << 31) && nF >= 1 && nF <= nS && nS <= M && nE >= 0 && nE < (1ll << 31) && P >= 1 && P <= nF;
}

inline Curv carve_curv(Carver& c, int64_t nF, int64_t nS) {
    Curv C = {};
    C.x = c.take<double>(3 * nF);
    C.r = c.take<double>(3 * nF);
    C.p = c.take<double>(3 * nF);
    C.q = c.take<double>(3 * nF);
    C.t = c.take<double>(3 * nS);
    C.tn = c.take<double>(3 * nS);
    return C;
}

}  // namespace

extern "C" int misplat_meshfill_curv_patches(const int32_t* src, const int32_t* tgt, int64_t n_edges, const uint8_t* free,
                                             int64_t n_vertices, int32_t* parent, int32_t* root, misplat_stream_t stream) {
    const int64_t M = n_vertices;
    if (M < 1 || M >= (1ll << 31) || n_edges < 0 || n_edges >= (1ll << 31) || (n_edges > 0 && (!src || !tgt)) || !free || !parent || !root)
        return MISPLAT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (n_edges > 0)
        hipLaunchKernelGGL(curv_union_kernel, dim3(blocks(n_edges, 256)), dim3(256), 0, s, src, tgt, n_edges, free, M, parent);
    hipLaunchKernelGGL(curv_root_kernel, dim3(blocks(M, 256)), dim3(256), 0, s, (const int32_t*)parent, M, root);
    return launched();
}

extern "C" int64_t misplat_meshfill_curv_workspace(int64_t n_free, int64_t n_rows) {
    if (n_free < 1 || n_rows < n_free || n_rows >= (1ll << 31)) return -1;
    Carver c{nullptr};
    carve_curv(c, n_free, n_rows);
    return c.o;
}

extern "C" int misplat_meshfill_curv_solve(const float* vertices, float* out, int64_t n_vertices, const int32_t* free_offset,
                                           const int32_t* rim_offset, const int32_t* vertex, const int32_t* row, const int32_t* degree,
                                           const int32_t* neighbour, const int32_t* place, int64_t n_free, int64_t n_rows,
                                           int64_t n_entries, const int32_t* code, int32_t n_patches, double rtol,
                                           int32_t max_iterations, void* workspace, int64_t workspace_bytes, int32_t* iterations,
                                           uint8_t* converged, double* residual, misplat_stream_t stream) {
    if (!curv_ok(n_vertices, n_free, n_rows, n_entries, n_patches) || !(rtol >= 0.0) || !vertices || !out || !free_offset || !rim_offset ||
        !vertex || !row || !degree || (n_entries > 0 && (!neighbour || !place)) || !code || !workspace || !iterations || !converged || !residual)
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    Curv C = carve_curv(c, n_free, n_rows);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    C.foff = free_offset; C.roff = rim_offset; C.vertex = vertex; C.row = row; C.deg = degree; C.nbr = neighbour; C.place = place;
    C.code = code; C.nF = n_free; C.nS = n_rows;
    hipLaunchKernelGGL(curv_solve_kernel, dim3((unsigned)n_patches), dim3(kCgThreads), 0, (hipStream_t)stream, vertices, out, C,
                       rtol * rtol, max_iterations, iterations, converged, residual);
    return launched();
}
