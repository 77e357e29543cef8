// unionfind.h -- the lock-free union-find shared by cluster.hip (radius-graph clustering),
// meshclean.hip (mesh components and boundary loops, section 18) and meshfill.hip (the patches of the free vertices, sections
// 29 and 31): links always point to a smaller index, so every component's root is its smallest member, whatever the
// scheduling.  After the uniting part, its read-out: the initial forest, the root walk by plain loads, and the kernel that
// flattens the trees and counts their members.
//
// Everything sits in an unnamed namespace, as in cellhash.h: each translation unit compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// parent[x] <= x always, and parent[x] is a member of x's component (of the graph whose edges are united); x is a root iff parent[x] == x.
//
// Inside a uniting kernel workgroups on different CUs and XCDs talk through parent[] alone, so EVERY access to it there is an
// agent-scope relaxed atomic (loads and stores that bypass the CU's L1, compare-and-swaps executed at the memory side):
// no fence is needed per element.  What such a load returns is a value parent[x] held at SOME earlier time, not
// necessarily the latest.  That is harmless:
//   * every value parent[x] ever held is a member of x's component and is <= x, and < x once x has stopped being a root
//     (a root is only ever un-rooted by the compare-and-swap below, which a halving store never undoes: a store to
//     parent[x] is issued only after x was seen as a non-root, with a value that was parent[parent[x]] < parent[x] < x);
//   * so a walk along (possibly old) values strictly descends and ends, after finitely many steps, at an index that was a
//     root of x's component when it was read; links only point downwards: no interleaving can close a cycle;
//   * a halving store replaces the link x -> p by x -> g, g an earlier parent of p.  g < x is not below x in the tree (a
//     descendant has a larger index), so it lies in the part that stays connected to p: the trees never split, even when
//     the stored value is older (larger) than the one it overwrites.  That can only lengthen a later walk;
//   * a hook compare-and-swap(parent[a], a, b) with b < a succeeds only if a IS a root at that moment: two trees of one
//     component become one.  If a stale read made a look like a root, the swap fails: a retry, nothing else (unite).
// When the kernel ends every edge (i, j) has been seen with find(i) == find(j) or hooked, so the trees are exactly the
// components, and each tree's root, the smallest index on every downward path, is the component's smallest member.
__device__ __forceinline__ int32_t ld_parent(int32_t* parent, int32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x's tree, with path halving
__device__ __forceinline__ int32_t find_root(int32_t* parent, int32_t x) {
    int32_t p = ld_parent(parent, x);
    while (p != x) {
        const int32_t g = ld_parent(parent, p);
        if (g == p) return p;
        __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
        p = ld_parent(parent, x);
    }
    return x;
}

// joins the trees of a and b (both members of what must become one component); returns a root of the joined tree as seen
// by this thread (the caller's next starting point).  A failed swap returns the TRUE parent of a, strictly below a, and the
// walk goes on from there: max(a, b) falls with every failure, so the loop ends even if every load were stale.
__device__ __forceinline__ int32_t unite(int32_t* parent, int32_t a, int32_t b) {
    while (true) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return a;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t seen = atomicCAS(parent + a, a, b);         // the larger root under the smaller
        if (seen == a) return b;
        a = seen;
    }
}

// ----------------------------------------------------------------------------------------------------- read-out
// (kernels as templates: a file that includes this header and launches none of them gets none in its code object)
// every vertex its own tree, and the array that goes with it (sizes, flags) cleared
template <typename Z>
__global__ __launch_bounds__(256) void uf_init_kernel(int64_t n, int32_t* __restrict__ parent, Z* __restrict__ zero) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    parent[i] = (int32_t)i;
    zero[i] = 0;
}

// The root of v's tree in a kernel AFTER the uniting one: past the kernel boundary parent[] is read-only, so plain loads.
__device__ __forceinline__ int32_t walk_root(const int32_t* __restrict__ parent, int32_t v) {
    int32_t r = v;
    for (int32_t p = parent[r]; p != r; p = parent[r]) r = p;
    return r;
}

// root[v] = the root of v's tree (MASKED: -1 where mask[v] is 0), and size[root] counts its members: integer adds, one per
// distinct root among a wave's lanes.
template <bool MASKED>
__global__ __launch_bounds__(256) void flatten_kernel(const int32_t* __restrict__ parent, const uint8_t* __restrict__ mask, int64_t n,
                                                      int32_t* __restrict__ root, int32_t* __restrict__ size) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool pending = v < n && (!MASKED || mask[v]);
    const int32_t r = pending ? walk_root(parent, (int32_t)v) : -1;
    if (v < n) root[v] = r;
    while (true) {
        const unsigned long long todo = __ballot(pending);
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t r0 = __shfl(r, leader);
        const bool same = pending && r == r0;
        const unsigned long long group = __ballot(same);
        if (lane == leader) atomicAdd(&size[r0], __popcll(group));
        if (same) pending = false;
    }
}

}  // namespace
