// unitlists.h -- the per-unit item lists over the sparse unit volume (unitgrid.h): what density.hip
// (Gaussians per unit, section 25) and pointtsdf.hip (rays per unit, section 32) share of the pipeline
//   count + scan -> emit (unit map index, item) pairs, marking the unit's word -> misplat_tsdf_alloc -> stable radix sort by
//   unit + per-slot ranges -> one workgroup per list.
// A user keeps its own pairs kernel (how an item finds its units) and hands every pair to a PairSink; the workspace, the
// count driver, the sort and the ranges are here, once.  misplat_unit_lists (density.hip) exports unit_lists.  In an unnamed
// namespace, as unitgrid.h and radixsort.h: each translation unit compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"
#include "wgprims.h"
#include "radixsort.h"
#include "unitgrid.h"

namespace {

// What a pairs kernel takes as its last argument: counts and total for the count (EMIT = false), the rest for the emit.
struct PairBufs {
    int32_t* counts;
    unsigned long long* total;
    const int32_t* pair_off;
    int64_t n_pairs;
    int32_t *keys, *ids;
    unsigned long long* words;
};

// Where a lane of a pairs kernel puts the pairs of its item i, in the order it meets them.  EMIT = false: counts[i] = pairs of
// item i (and the 64-bit total); EMIT = true: the pairs from pair_off[i] on, and the unit's word set.  open(i) before the first
// pair, add per pair, finish(i) on every lane.
template <bool EMIT>
struct PairSink {
    const PairBufs& b;
    int64_t pos = 0, n = 0;

    __device__ __forceinline__ explicit PairSink(const PairBufs& bufs) : b(bufs) {}

    __device__ __forceinline__ void open(int64_t i) { pos = EMIT ? (int64_t)b.pair_off[i] : 0; }

    // m: the unit's map index (map_index's).  Both guards always hold: m >= 0 because each walk is confined to the map,
    // pos + n < n_pairs because the offsets are the scan of the same walk's counts.  This is pointtsdf.hip's form as it was;
    // density.hip tested only the second and set the word outside it, which under the two invariants is the same stores.
    __device__ __forceinline__ void add(int64_t m, int64_t i) {
        if (EMIT) {
            if (m >= 0 && pos + n < b.n_pairs) {
                b.keys[pos + n] = (int32_t)m;
                b.ids[pos + n] = (int32_t)i;
                b.words[m] = 1ull;                         // (every writer stores the same value)
            }
        }
        n++;
    }

    __device__ __forceinline__ void finish(int64_t i) {
        if (!EMIT) {
            b.counts[i] = (int32_t)(n < 0x7fffffffll ? n : 0x7fffffffll);
            if (n) atomicAdd(b.total, (unsigned long long)n);
        }
    }
};

// ranges[2 slot], ranges[2 slot + 1] = the unit's part of the sorted pairs
__global__ __launch_bounds__(256) void unit_ranges_kernel(const int32_t* __restrict__ keys, int64_t E,
                                                          const int32_t* __restrict__ slot_map, int32_t* __restrict__ ranges) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int32_t k = keys[e];
    const bool first = e == 0 || keys[e - 1] != k, last = e == E - 1 || keys[e + 1] != k;
    if (!first && !last) return;
    const int32_t s = slot_map[k];
    if (s < 0) return;                                     // (never: emit marked the unit and alloc gave it a slot)
    if (first) ranges[2 * s] = (int32_t)e;
    if (last) ranges[2 * s + 1] = (int32_t)(e + 1);
}

__global__ void unit_clear_total_kernel(unsigned long long* total) { *total = 0ull; }
__global__ void unit_copy_total_kernel(const unsigned long long* total, int64_t* out) { *out = (int64_t)*total; }

// ----------------------------------------------------------------------------------------------------------- workspace
// N items (count_pairs; a user's own scan of N counts into offs, as pointtsdf.hip's pieces) and E pairs (unit_lists): either
// may be 0 for the call that does not use it.  The one description of the layout: every *_workspace size and every user.
struct Work {
    int32_t *counts, *offs, *scr;
    unsigned long long* total;
    SortBufs sort;
};
inline Work carve(Carver& c, int64_t N, int64_t E) {
    Work W;
    const int64_t n_hist = 256 * ((E + kTile - 1) / kTile);
    W.counts = c.take<int32_t>(N + 1);
    W.offs = c.take<int32_t>(N + 1);
    W.scr = take_scan(c, (N > n_hist ? N : n_hist) + 1);
    W.total = c.take<unsigned long long>(1);
    W.sort = take_sort(c, E);
    return W;
}
inline bool sizes_ok(int64_t N, int64_t E) { return N >= 0 && N < (1ll << 31) && E >= 0 && E < (1ll << 31) - kTile; }

// the bytes of carve(c, N, E), or -1 for sizes the library refuses: what a *_workspace entry point returns
inline int64_t work_bytes(int64_t N, int64_t E) {
    if (!sizes_ok(N, E)) return -1;
    Carver c{nullptr};
    carve(c, N, E);
    return c.o;
}

// --------------------------------------------------------------------------------------------------------------- host
// pair_off [N + 1] = the exclusive scan of the pairs per item, *n_pairs (device) = their exact number.  launch(bufs): the
// caller's pairs<false> kernel over its N items.
template <class L>
inline void count_pairs(const Work& W, int64_t N, int32_t* pair_off, int64_t* n_pairs, hipStream_t s, L launch) {
    hipLaunchKernelGGL(unit_clear_total_kernel, dim3(1), dim3(1), 0, s, W.total);
    launch(PairBufs{W.counts, W.total, nullptr, 0, nullptr, nullptr, nullptr});
    scan(W.counts, N, pair_off, W.scr, s);
    hipLaunchKernelGGL(unit_copy_total_kernel, dim3(1), dim3(1), 0, s, (const unsigned long long*)W.total, n_pairs);
}

// The E pairs sorted by unit, stable, into keys_sorted / ids_sorted (keys and ids are used as scratch), and the range of
// every listed unit's slot.  n_map: entries of the unit map (the keys are below it).
inline void unit_lists(int64_t n_map, const int32_t* slot_map, int32_t* keys, int32_t* ids, int64_t E, int32_t* keys_sorted,
                       int32_t* ids_sorted, int32_t* ranges, const Work& W, hipStream_t s) {
    // passes over the bits of the largest map index; one more over zero digits (the identity, the sort being stable) where
    // that makes their number odd: the result then lies in keys_sorted / ids_sorted.  (A fifth pass repeats the top byte:
    // the identity again.)
    int passes = radix_passes(n_map - 1);
    if (passes % 2 == 0) passes++;
    int32_t *ka = keys, *va = ids, *kb = keys_sorted, *vb = ids_sorted;
    radix_sort(ka, va, kb, vb, E, passes, W.sort, W.scr, s);
    hipLaunchKernelGGL(unit_ranges_kernel, dim3(blocks(E, 256)), dim3(256), 0, s, (const int32_t*)keys_sorted, E, slot_map, ranges);
}

}  // namespace
