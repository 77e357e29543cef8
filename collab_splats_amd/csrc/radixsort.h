// radixsort.h -- the stable radix sort of (int32 key, int32 value) pairs and its host driver.  Used by meshmap.hip
// (contributions by vertex), pointcloud.hip (points by voxel, section 17), grouping.hip (Gaussians by
// depth, then by cell, section 22), through unitlists.h the unit lists of density.hip and pointtsdf.hip (pairs by unit, sorted in
// density.hip's misplat_unit_lists; sections 14.5, 25 and 32) and, through meshadj.h, the mesh files (adjacency rows, sections
// 26.5, 27 and 29).  What a caller must know about the sort lives here too: which of its two pairs holds the
// result (sorted_names) and the buffers of a shorter sort (sort_for).  In an unnamed namespace, as cellhash.h: each
// translation unit that includes this header compiles its own copy of the kernels into its own code object.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wgprims.h"

namespace {

constexpr int kTile = 4096;           // radix sort: items per workgroup (256 threads x 16 rounds)

// Stable LSD radix sort of (key, value) by key, 8 bits per pass: per-workgroup digit histograms (digit-major, so one scan
// gives every workgroup's stable offsets), then a scatter that ranks each round of 256 items in item order (ballots inside a
// wave, per-wave counts across the workgroup).  Equal keys keep the order in which they entered.
__global__ __launch_bounds__(256) void radix_hist_kernel(const int32_t* __restrict__ keys, int64_t E, int shift, int64_t nblk,
                                                         int32_t* __restrict__ hist) {
    __shared__ int32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * kTile;
    for (int r = 0; r < kTile / 256; r++) {
        const int64_t e = e0 + r * 256 + threadIdx.x;
        if (e < E) atomicAdd(&h[(keys[e] >> shift) & 255], 1);
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(256) void radix_scatter_kernel(const int32_t* __restrict__ keys, const int32_t* __restrict__ vals,
                                                            int64_t E, int shift, int64_t nblk, const int32_t* __restrict__ hoff,
                                                            int32_t* __restrict__ keys_out, int32_t* __restrict__ vals_out) {
    __shared__ int32_t run[256];
    __shared__ int32_t wcnt[4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    run[threadIdx.x] = hoff[(int64_t)threadIdx.x * nblk + blockIdx.x];
    const int64_t e0 = (int64_t)blockIdx.x * kTile;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int r = 0; r < kTile / 256; r++) {
#pragma unroll
        for (int w = 0; w < 4; w++) wcnt[w][threadIdx.x] = 0;
        __syncthreads();
        const int64_t e = e0 + r * 256 + threadIdx.x;
        const bool act = e < E;
        int32_t key = 0, val = 0;
        int digit = 0;
        if (act) { key = keys[e]; val = vals[e]; digit = (key >> shift) & 255; }
        unsigned long long same = __ballot(act);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const unsigned long long set = __ballot(act && ((digit >> b) & 1));
            same &= ((digit >> b) & 1) ? set : ~set;
        }
        const int rank = __popcll(same & lt);
        if (act && (same >> lane) == 1ull) wcnt[wave][digit] = __popcll(same);      // the group's highest lane
        __syncthreads();
        if (act) {
            int before = run[digit] + rank;
            for (int w = 0; w < wave; w++) before += wcnt[w][digit];
            keys_out[before] = key;
            vals_out[before] = val;
        }
        __syncthreads();
        run[threadIdx.x] += ((wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x]) + wcnt[2][threadIdx.x]) + wcnt[3][threadIdx.x];
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------- host
// What a sort of E items needs besides its two (key, value) pairs and a scan scratch for 256 nblk counts
// (take_scan(c, 256 * nblk) or longer).
struct SortBufs {
    int32_t *hist, *hoff;
    int64_t nblk;
};

inline SortBufs take_sort(Carver& c, int64_t E) {
    SortBufs b;
    b.nblk = (E + kTile - 1) / kTile;
    b.hist = c.take<int32_t>(256 * b.nblk);
    b.hoff = c.take<int32_t>(256 * b.nblk + 1);
    return b;
}

// The number of 8-bit passes that cover every key in 0 .. max_key: at least 1, at most 4 (an int32 key).  Pass p >= 1 is
// needed iff some key has a bit at or above 8 p, i.e. iff (max_key >> 8 p) > 0, and these conditions are nested: the count
// is 1 + the number of p in 1 .. 3 with (max_key >> 8 p) > 0.  That is what the loop
//     for (shift = 0; shift == 0 || (max_key >> shift) > 0; shift += 8)
// runs for 0 <= max_key < 2^31 (it stops at shift 32 at the latest, max_key being held in 64 bits), and what
//     for (shift = 0; shift < 32 && (max_key >> shift) > 0; shift += 8)
// runs for 1 <= max_key < 2^31 (for max_key = 0 that loop runs no pass: a caller that can see 0 must ask for itself).
inline int radix_passes(int64_t max_key) {
    int passes = 1;
    while (passes < 4 && (max_key >> (8 * passes)) > 0) passes++;
    return passes;
}

// `passes` passes over E items, pass p on the digit at shift min(8 p, 24) (a pass beyond the fourth repeats the top byte: the
// sort being stable, the identity).  Every pass reads (ka, va), writes (kb, vb) and swaps the two pairs: on return (ka, va)
// name the sorted pair -- the caller's second pair if `passes` is odd, its first if even -- and (kb, vb) the other.
inline void radix_sort(int32_t*& ka, int32_t*& va, int32_t*& kb, int32_t*& vb, int64_t E, int passes, const SortBufs& b,
                       int32_t* scan_scratch, hipStream_t s) {
    for (int pass = 0; pass < passes; pass++) {
        const int shift = 8 * pass < 24 ? 8 * pass : 24;
        hipLaunchKernelGGL(radix_hist_kernel, dim3((unsigned)b.nblk), dim3(256), 0, s, (const int32_t*)ka, E, shift, b.nblk, b.hist);
        scan(b.hist, 256 * b.nblk, b.hoff, scan_scratch, s);
        hipLaunchKernelGGL(radix_scatter_kernel, dim3((unsigned)b.nblk), dim3(256), 0, s, (const int32_t*)ka, (const int32_t*)va, E,
                           shift, b.nblk, (const int32_t*)b.hoff, kb, vb);
        int32_t* t = ka; ka = kb; kb = t;
        t = va; va = vb; vb = t;
    }
}

// The same renaming without the sort: where radix_sort left the sorted pair after `passes` passes, for a later call that
// reads what an earlier one sorted.
inline void sorted_names(int32_t*& ka, int32_t*& va, int32_t*& kb, int32_t*& vb, int passes) {
    if (passes & 1) {
        int32_t* t = ka; ka = kb; kb = t;
        t = va; va = vb; vb = t;
    }
}

// the buffers of a sort of fewer items than `b` was taken for
inline SortBufs sort_for(SortBufs b, int64_t items) {
    b.nblk = (items + kTile - 1) / kTile;
    return b;
}

}  // namespace
