// meshedge.h -- what meshclean.hip and meshfill.hip (section 29) share about a triangle mesh's edges:
// the key of an undirected edge, its home slot in an open-addressing table, the directed edge of a corner and the fp32 edge
// length in its written operation order.  In an unnamed namespace, as wgprims.h: each translation unit compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ unsigned long long edge_key(int32_t a, int32_t b) {
    const uint32_t lo = (uint32_t)(a < b ? a : b), hi = (uint32_t)(a < b ? b : a);
    return ((unsigned long long)lo << 32) | hi;
}

__device__ __forceinline__ unsigned long long edge_home(unsigned long long key, unsigned long long mask) {
    key ^= key >> 31;
    key *= 0x7fb5d329728ea185ull;
    key ^= key >> 27;
    return key & mask;
}

// corner c of face f: the directed edge tri[3 f + c] -> tri[3 f + (c + 1) % 3]
__device__ __forceinline__ void corner_edge(const int32_t* __restrict__ tri, int64_t f, int c, int32_t& a, int32_t& b) {
    a = tri[3 * f + c];
    b = tri[3 * f + (c == 2 ? 0 : c + 1)];
}

__device__ __forceinline__ float edge_length(const float* __restrict__ V, int32_t a, int32_t b) {
    const float dx = V[3 * (int64_t)b] - V[3 * (int64_t)a], dy = V[3 * (int64_t)b + 1] - V[3 * (int64_t)a + 1],
                dz = V[3 * (int64_t)b + 2] - V[3 * (int64_t)a + 2];
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

}  // namespace
