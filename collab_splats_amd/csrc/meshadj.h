// meshadj.h -- vertex adjacency as sorted CSR rows, shared by meshclean.hip (Laplacian smoothing),
// decimate.hip (the corner and neighbour tables of a round, section 27) and meshfill.hip (the rows of the free vertices, the free
// vertices by patch, section 29).  The directed edges of all corners, both ways, as (key = target, value = source): sorted by
// target, then stably by source, they form a CSR over the sources with every row ascending in its target.  In an unnamed
// namespace, as wgprims.h: each translation unit compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wgprims.h"
#include "radixsort.h"
#include "meshedge.h"

namespace {

// directed edge e = 2 h + d of corner h = 3 f + c: d = 0 as the face runs, d = 1 against it
__device__ __forceinline__ void directed(const int32_t* __restrict__ tri, int64_t e, int32_t& src, int32_t& tgt) {
    const int64_t h = e >> 1, f = h / 3;
    int32_t a, b;
    corner_edge(tri, f, (int)(h - 3 * f), a, b);
    src = (e & 1) ? b : a;
    tgt = (e & 1) ? a : b;
}

// Both directed edges of corner c of face f, written as entries 2 h and 2 h + 1 of (key = target, value = source): with h = 3 f + c
// entry e is directed(e).  The kernels that emit all 6 n edges of n faces stay with their files (one lane per corner: all the
// faces in meshclean.hip; the live faces, and their corner keys beside, in decimate.hip: a launch of its own for them measured
// 2 % on a round).
__device__ __forceinline__ void emit_corner_edges(const int32_t* __restrict__ tri, int64_t f, int c, int64_t h, int32_t* __restrict__ tgt,
                                                  int32_t* __restrict__ src) {
    int32_t a, b;
    corner_edge(tri, f, c, a, b);
    tgt[2 * h] = b; src[2 * h] = a;
    tgt[2 * h + 1] = a; src[2 * h + 1] = b;
}

// rows[2 i], rows[2 i + 1] = item i's part of the sorted keys (zeroed by the caller: an item without an entry keeps 0, 0)
__global__ __launch_bounds__(256) void rows_kernel(const int32_t* __restrict__ key, int64_t E, int32_t* __restrict__ rows) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int32_t s = key[e];
    if (e == 0 || key[e - 1] != s) rows[2 * (int64_t)s] = (int32_t)e;
    if (e == E - 1 || key[e + 1] != s) rows[2 * (int64_t)s + 1] = (int32_t)(e + 1);
}

// E directed edges (tgt, src) and a second pair of buffers: sorted by target in `tgt_passes` passes, then stably by source in
// `src_passes`.  On return src and tgt name the sorted sources and targets, as radix_sort leaves its names.
inline void sort_directed(int32_t*& tgt, int32_t*& src, int32_t*& tgt_b, int32_t*& src_b, int64_t E, int tgt_passes, int src_passes,
                          const SortBufs& b, int32_t* scan_scratch, hipStream_t s) {
    radix_sort(tgt, src, tgt_b, src_b, E, tgt_passes, b, scan_scratch, s);
    radix_sort(src, tgt, src_b, tgt_b, E, src_passes, b, scan_scratch, s);
}

// the same names for a later call that sorts nothing
inline void sorted_directed_names(int32_t*& tgt, int32_t*& src, int32_t*& tgt_b, int32_t*& src_b, int tgt_passes, int src_passes) {
    sorted_names(tgt, src, tgt_b, src_b, tgt_passes);
    sorted_names(src, tgt, src_b, tgt_b, src_passes);
}

}  // namespace
