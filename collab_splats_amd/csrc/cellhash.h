// cellhash.h -- the spatial index shared by meshmap.hip (kNN vertex map), cluster.hip (radius-graph
// clustering, section 16) and pointcloud.hip (section 17): a hash of the OCCUPIED cells of edge h (open addressing, capacity
// a power of two >= 2 M, 64-bit keys) and the vertices regrouped by cell (count, scan, fill).  Memory O(M) whatever the
// extent of the scene.  The scan, the claim loop of the insertion and the host helpers are wgprims.h's.
//
// Everything sits in an unnamed namespace on purpose: each translation unit that includes this header compiles its own
// copy of the kernels into its own code object (the library is built without relocatable device code).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"
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

// capacity of the hash for n vertices: the power of two >= max(64, 2 n)
inline int64_t hash_capacity(int64_t n) {
    int64_t cap = 64;
    while (cap < 2 * n) cap <<= 1;
    return cap;
}

}  // namespace
