// cellhash.h -- the spatial index shared by meshmap.hip (kNN vertex map), cluster.hip (radius-graph
// clustering, section 16) and pointcloud.hip (section 17): a hash of the OCCUPIED cells of edge h (open addressing, capacity
// a power of two >= 2 M, 64-bit keys) and the vertices regrouped by cell (count, scan, fill).  Memory O(M) whatever the
// extent of the scene.  The scan, the claim loop of the insertion and the host helpers are wgprims.h's.
//
// Besides the two kernels: the host side of an index (IndexBufs, take_index, build_index: all three files), the k smallest
// keys in registers (KBest: meshmap.hip and pointcloud.hip).
//
// Everything sits in an unnamed namespace on purpose: each translation unit that includes this header compiles its own
// copy of the kernels into its own code object (the library is built without relocatable device code).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"
#include "internal.h"
#include "wgprims.h"

namespace {

constexpr float kCoordCells = 262144.f;   // |v| / h < 2^18 for every vertex (the host checks it)

__device__ __forceinline__ unsigned long long cell_key(int cx, int cy, int cz) {
    return (unsigned long long)(uint32_t)(cx + (1 << 20)) | ((unsigned long long)(uint32_t)(cy + (1 << 20)) << 21) |
           ((unsigned long long)(uint32_t)(cz + (1 << 20)) << 42);
}

__device__ __forceinline__ uint32_t hash_slot(unsigned long long key, uint32_t mask) {
    key ^= key >> 31;
    key *= 0x7fb5d329728ea185ull;
    key ^= key >> 27;
    return (uint32_t)key & mask;
}

__device__ __forceinline__ int cell_of(float x, float inv_h) { return (int)floorf(x * inv_h); }

// slot of an occupied cell, -1 if the cell holds no vertex
__device__ __forceinline__ int find_cell(const unsigned long long* __restrict__ keys, uint32_t mask, unsigned long long key) {
    uint32_t s = hash_slot(key, mask);
    while (true) {
        const unsigned long long k = keys[s];
        if (k == key) return (int)s;
        if (k == kEmpty) return -1;
        s = (s + 1) & mask;
    }
}

// ----------------------------------------------------------------------------------------------------- k smallest
// The k smallest keys offered, ascending in b[KC - k .. KC - 1]; the KC - k slots in front hold 0 and never move (a real
// key is never below them).  Unset slots hold ~Key(0).  An equal key is inserted behind its equals.  meshmap.hip packs
// (d2 bits, vertex index) into 64 bits; pointcloud.hip keeps the d2 bits alone.
template <class Key, int KC>
struct KBest {
    Key b[KC];
    __device__ __forceinline__ void reset(int k) {
#pragma unroll
        for (int j = 0; j < KC; j++) b[j] = (j >= KC - k) ? ~Key(0) : Key(0);
    }
    __device__ __forceinline__ Key nearest(int k) const {      // b[KC - k] without a dynamic register index
        Key r = 0;
#pragma unroll
        for (int j = 0; j < KC; j++) r = (j == KC - k) ? b[j] : r;
        return r;
    }
    __device__ __forceinline__ void offer(Key key) {
        if (key >= b[KC - 1]) return;
#pragma unroll
        for (int j = KC - 1; j > 0; j--) b[j] = (b[j - 1] > key) ? b[j - 1] : (b[j] > key ? key : b[j]);
        b[0] = b[0] > key ? key : b[0];
    }
};

// --------------------------------------------------------------------------------------------------------- index
// Insert every vertex's cell into the hash and count the vertices per slot.  Which slot a cell takes depends on the
// insertion order; the lookups and every result do not.  select (or NULL: every vertex): only the vertices with a
// non-zero byte enter the index; the others get vslot -1.
__global__ __launch_bounds__(256) void index_insert_kernel(const float* __restrict__ V, int64_t M,
                                                           const uint8_t* __restrict__ select, float inv_h,
                                                           unsigned long long* __restrict__ keys, uint32_t mask,
                                                           int32_t* __restrict__ vslot, int32_t* __restrict__ counts) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= M) return;
    if (select && !select[v]) { vslot[v] = -1; return; }
    const unsigned long long key = cell_key(cell_of(V[3 * v], inv_h), cell_of(V[3 * v + 1], inv_h), cell_of(V[3 * v + 2], inv_h));
    const uint32_t s = claim_slot(keys, mask, hash_slot(key, mask), key);
    vslot[v] = (int32_t)s;
    atomicAdd(&counts[s], 1);
}

// vertices regrouped by cell: cellpts[starts[s] ..) = (x, y, z, index bits); counts are consumed as cursors.  The order
// inside a cell is arbitrary: no result depends on it.  A vertex with vslot -1 is not in the index.
__global__ __launch_bounds__(256) void index_fill_kernel(const float* __restrict__ V, int64_t M, const int32_t* __restrict__ vslot,
                                                         const int32_t* __restrict__ starts, int32_t* __restrict__ cursor,
                                                         float4* __restrict__ cellpts) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= M) return;
    const int s = vslot[v];
    if (s < 0) return;
    const int pos = starts[s] + atomicSub(&cursor[s], 1) - 1;
    cellpts[pos] = make_float4(V[3 * v], V[3 * v + 1], V[3 * v + 2], __int_as_float((int)v));
}

struct Index {
    const unsigned long long* keys;
    const int32_t* starts;
    const float4* pts;
    uint32_t mask;
};

// ---------------------------------------------------------------------------------------------------------- host
// capacity of the hash for n vertices: the power of two >= max(64, 2 n)
inline int64_t hash_capacity(int64_t n) {
    int64_t cap = 64;
    while (cap < 2 * n) cap <<= 1;
    return cap;
}

// The buffers of one index over n vertices.  Besides them a build needs vslot [n] and a scan scratch for cap counts
// (take_scan(c, cap) or longer); both may be shared by several indices built one after the other.
struct IndexBufs {
    unsigned long long* keys;
    int32_t *counts, *starts;
    float4* pts;
    int64_t cap;
};

inline IndexBufs take_index(Carver& c, int64_t n) {
    IndexBufs b;
    b.cap = hash_capacity(n);
    b.keys = c.take<unsigned long long>(b.cap);
    b.counts = c.take<int32_t>(b.cap);
    b.starts = c.take<int32_t>(b.cap + 1);
    b.pts = c.take<float4>(n);
    return b;
}

// the hash of the occupied cells of edge 1 / inv_h over V [n, 3] (select: see index_insert_kernel) and the vertices regrouped
// by cell; starts[cap] = the number of vertices in the index
inline Index build_index(const float* V, int64_t n, const uint8_t* select, float inv_h, const IndexBufs& b, int32_t* vslot,
                         int32_t* scan_scratch, hipStream_t s) {
    const uint32_t mask = (uint32_t)(b.cap - 1);
    misplat_internal::fill_bytes(b.keys, 8 * b.cap, 0xffffffffu, s);          // (kernels, not memsets: internal.h)
    misplat_internal::fill_bytes(b.counts, 4 * b.cap, 0u, s);
    hipLaunchKernelGGL(index_insert_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, V, n, select, inv_h, b.keys, mask, vslot, b.counts);
    scan(b.counts, b.cap, b.starts, scan_scratch, s);
    hipLaunchKernelGGL(index_fill_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, V, n, (const int32_t*)vslot,
                       (const int32_t*)b.starts, b.counts, b.pts);
    return Index{b.keys, b.starts, b.pts, mask};
}

}  // namespace
