// facetable.h -- the edge table of a triangle mesh, shared by meshclean.hip, meshfill.hip (section 29)
// and meshtri.hip (section 30): per undirected edge its count of incidences, its smallest and, where the caller takes it, its
// largest incident face, which names both faces of a two-face edge (meshclean.hip takes none: 4 B a slot and one atomic the
// less); the priority (bits, mixed key, key) by which meshfill.hip and meshtri.hip pick one edge per face.  In an unnamed
// namespace, as wgprims.h: each translation unit compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "internal.h"
#include "wgprims.h"
#include "hashmix.h"
#include "meshedge.h"

namespace {

typedef unsigned long long u64;

struct EdgeTable {
    u64* keys;
    int32_t *cnt, *fmin, *fmax;                             // fmax: null in a table that keeps the smallest face only
    u64 mask;                                               // capacity - 1
};

// the slot of an edge that was inserted
__device__ __forceinline__ int64_t edge_find(const EdgeTable& E, u64 key) {
    u64 s = edge_home(key, E.mask);
    while (E.keys[s] != key) s = (s + 1) & E.mask;
    return (int64_t)s;
}

// whether `key` is an edge of the table at all (the table is never full: a probe ends at a free slot)
__device__ __forceinline__ bool edge_present(const EdgeTable& E, u64 key) {
    u64 s = edge_home(key, E.mask);
    while (true) {
        const u64 k = E.keys[s];
        if (k == key) return true;
        if (k == kEmpty) return false;
        s = (s + 1) & E.mask;
    }
}

__global__ __launch_bounds__(256) void edge_insert_kernel(const int32_t* __restrict__ tri, int64_t T, EdgeTable E) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= 3 * T) return;
    const int64_t f = h / 3;
    int32_t a, b;
    corner_edge(tri, f, (int)(h - 3 * f), a, b);
    if (a == b) return;
    const u64 key = edge_key(a, b);
    const u64 s = claim_slot(E.keys, E.mask, edge_home(key, E.mask), key);
    atomicAdd(&E.cnt[s], 1);
    atomicMin(&E.fmin[s], (int32_t)f);
    if (E.fmax) atomicMax(&E.fmax[s], (int32_t)f);
}

__device__ __forceinline__ bool repeated(const int32_t* __restrict__ tri, int64_t f) {
    const int32_t a = tri[3 * f], b = tri[3 * f + 1], c = tri[3 * f + 2];
    return a == b || b == c || a == c;
}

inline int64_t edge_capacity(int64_t T) {
    int64_t cap = 64;
    while (cap < 6 * T) cap <<= 1;
    return cap;
}

// the storage of the table of T faces, `both`: with the largest incident face
inline EdgeTable take_edge_table(Carver& c, int64_t T, bool both = true) {
    const int64_t cap = edge_capacity(T);
    EdgeTable E = {};
    E.keys = c.take<u64>(cap);
    E.cnt = c.take<int32_t>(cap);
    E.fmin = c.take<int32_t>(cap);
    if (both) E.fmax = c.take<int32_t>(cap);
    E.mask = (u64)(cap - 1);
    return E;
}

// fills the table with the T faces of `tri` (cleared by kernels, not memsets: internal.h); an empty mesh launches no insertion
inline void build_edge_table(const int32_t* tri, int64_t T, const EdgeTable& E, hipStream_t s) {
    const size_t cap = (size_t)E.mask + 1;
    misplat_internal::fill_bytes(E.keys, 8 * cap, 0xffffffffu, s);
    misplat_internal::fill_bytes(E.cnt, 4 * cap, 0u, s);
    misplat_internal::fill_bytes(E.fmin, 4 * cap, 0x7fffffffu, s);
    if (E.fmax) misplat_internal::fill_bytes(E.fmax, 4 * cap, 0u, s);
    if (T > 0) hipLaunchKernelGGL(edge_insert_kernel, dim3(blocks(3 * T, 256)), dim3(256), 0, s, tri, T, E);
}

// The priority of an edge among the candidates of a round: larger bits first (the fp32 length's in meshfill.hip, the fp64
// violation's in meshtri.hip), then the smaller mix32(lo, hi, 0), then the smaller key.
template <typename B>
struct PrioOf {
    B bits;
    uint32_t mix;
    u64 key;
};
template <typename B>
__device__ __forceinline__ PrioOf<B> prio_of(B bits, int32_t a, int32_t b) {
    const u64 key = edge_key(a, b);
    return PrioOf<B>{bits, mix32((uint32_t)(key >> 32), (uint32_t)key, 0u), key};
}
template <typename B>
__device__ __forceinline__ bool before(const PrioOf<B>& x, const PrioOf<B>& y) {
    if (x.bits != y.bits) return x.bits > y.bits;
    if (x.mix != y.mix) return x.mix < y.mix;
    return x.key < y.key;
}

// best[f] = the corner of face f's first candidate edge in priority (bits[3 f + c] != 0 marks a candidate), -1 if it has none
template <typename B>
__global__ __launch_bounds__(256) void face_best_kernel(const int32_t* __restrict__ tri, int64_t T, const B* __restrict__ bits,
                                                        int32_t* __restrict__ best) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= T) return;
    int32_t bc = -1;
    PrioOf<B> bp = {};
    for (int c = 0; c < 3; c++) {
        const B x = bits[3 * f + c];
        if (!x) continue;
        int32_t a, b;
        corner_edge(tri, f, c, a, b);
        const PrioOf<B> p = prio_of(x, a, b);
        if (bc < 0 || before(p, bp)) { bc = c; bp = p; }
    }
    best[f] = bc;
}

// Face f's first edge is selected iff it is the first edge of its other face too.  owner[f] = the slot (3 face + corner, at
// the edge's smallest face) that numbers the selected edge, -1 if f's first edge is not selected; fsel[f] = 1 / 0; flag[3 f +
// c] = 1 at the owner slots.
__global__ __launch_bounds__(256) void select_kernel(const int32_t* __restrict__ tri, int64_t T, EdgeTable E,
                                                     const int32_t* __restrict__ best, int32_t* __restrict__ owner,
                                                     int32_t* __restrict__ fsel, int32_t* __restrict__ flag) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= T) return;
    const int32_t c = best[f];
    int32_t own = -1;
    if (c >= 0) {
        int32_t a, b;
        corner_edge(tri, f, c, a, b);
        const u64 key = edge_key(a, b);
        const int64_t s = edge_find(E, key);
        const int32_t f0 = E.fmin[s], f1 = E.fmax[s];
        const int32_t g = f0 == (int32_t)f ? f1 : f0;
        bool sel = true;
        int32_t c0 = c;                                     // the edge's corner in its smallest face
        if (g != (int32_t)f) {
            const int32_t cg = best[g];
            sel = false;
            if (cg >= 0) {
                int32_t ga, gb;
                corner_edge(tri, g, cg, ga, gb);
                sel = edge_key(ga, gb) == key;
            }
            if (g == f0) c0 = cg;
        }
        if (sel) own = 3 * f0 + c0;
    }
    owner[f] = own;
    fsel[f] = own >= 0 ? 1 : 0;
    for (int k = 0; k < 3; k++) flag[3 * f + k] = (own == (int32_t)(3 * f + k)) ? 1 : 0;
}

}  // namespace
