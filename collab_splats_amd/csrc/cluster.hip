// cluster.hip -- connected components of the radius graph over the selected mesh vertices.
//
// Semantics: the reference's mesh_clustering restated (tests/meshquery_restatement.py is the oracle).  Vertices i != j with
// mask set are joined iff d2 < r2, d2 = ((dx dx + dy dy) + dz dz) and r2 = r r in fp32 (compiled with -ffp-contract=off:
// every expression is evaluated in the written order); clusters are the connected components with more than
// min_cluster_size members, numbered in ascending order of their smallest vertex index.
//
// Spatial index (csrc/cellhash.h): a hash of the occupied cells of edge h = r over the SELECTED vertices only, the
// vertices regrouped by cell.  Union: one thread per selected vertex, in cell order, over the cells its radius can reach,
// into a lock-free union-find whose links always point to a smaller index: every component's root is its smallest member,
// whatever the scheduling.  Flatten, count (integer atomics), rank the kept roots by a scan in vertex order.  Memory O(M);
// no float atomics; two runs are bitwise equal.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"
#include "internal.h"
#include "cellhash.h"
#include "unionfind.h"

namespace {

// ---------------------------------------------------------------------------------------------------------- union
// (the union-find itself, why stale reads are harmless in it, and its read-out -- the initial forest, the flatten kernel that
// gives an unselected vertex root -1: csrc/unionfind.h)

// kSub lanes per entry of the cell-ordered list (the selected vertices), each taking every kSub-th candidate of every cell:
// neighbouring lanes hold vertices of one cell and walk the same candidate lists.  (One lane per vertex left a 106 k-vertex
// mesh with two waves per CU, each lane a serial chain of some 500 dependent loads: DESIGN.md section 16.)
//
// Which cells hold a neighbour.  d2 < r2 implies |x_i - x_j| < r EXACTLY on every axis: rounding is monotone and the
// terms are non-negative, so fl(dx dx) <= d2 < fl(r r) gives |dx| < r, and dx = fl(x_i - x_j) with |dx| < r (r a float)
// gives |x_i - x_j| < r.  The cell of a coordinate is floorf(fl(x inv_h)), a non-decreasing function of x, the same for
// both ends.  It does NOT follow that the two cell indices differ by at most one: at |x| / r near 2^18 the product
// x inv_h is rounded to a grid of 2^-5, so two coordinates just under r apart can land 1 + 2^-5 apart and straddle two
// cell boundaries.  The box is therefore taken from the coordinates, as knn_kernel does: cells
// cell_of(x_i - t) .. cell_of(x_i + t) with t = r + margin.  The rounding errors of t and of the subtraction are together
// at most 2^-24 (|x_i| + 2 t) < margin / 2 with margin = 2^-22 (amax + r), so fl(x_i - t) <= x_i - r < x_j, and by
// monotonicity cell_of(fl(x_i - t)) <= cell_of(x_j); likewise above.  Away from the bound that is at most the 27 cells
// around the vertex's own (more only when the vertex lies within the margin of a cell face).
// A vertex outside the coordinate bound the host checks (or not finite) is left alone: its box would not be bounded.
constexpr int kSub = 8;

__global__ __launch_bounds__(256) void union_kernel(Index ix, int64_t cap, float r, float r2, float inv_h,
                                                    int32_t* __restrict__ parent) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t t = g / kSub;
    const int sub = (int)(g % kSub);
    if (t >= ix.starts[cap]) return;                              // the number of selected vertices
    const float4 q = ix.pts[t];
    const int32_t i = __float_as_int(q.w);
    const float amax = fmaxf(fmaxf(fabsf(q.x), fabsf(q.y)), fabsf(q.z));
    if (!(amax * inv_h < kCoordCells + 2.f)) return;
    const float reach = r + 2.3841858e-7f * (amax + r);
    const float p[3] = {q.x, q.y, q.z};
    int lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) { lo[a] = cell_of(p[a] - reach, inv_h); hi[a] = cell_of(p[a] + reach, inv_h); }
    int32_t root = i;                                             // a member of i's tree: where the next find starts
    for (int cz = lo[2]; cz <= hi[2]; cz++)
        for (int cy = lo[1]; cy <= hi[1]; cy++)
            for (int cx = lo[0]; cx <= hi[0]; cx++) {
                const int s = find_cell(ix.keys, ix.mask, cell_key(cx, cy, cz));
                if (s < 0) continue;
                const int e1 = ix.starts[s + 1];
                for (int e = ix.starts[s] + sub; e < e1; e += kSub) {
                    const float4 c = ix.pts[e];
                    const int32_t j = __float_as_int(c.w);
                    const float dx = q.x - c.x, dy = q.y - c.y, dz = q.z - c.z;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (j < i && d2 < r2) root = unite(parent, root, j);      // each edge once, from its larger end
                }
            }
}

// ----------------------------------------------------------------------------------------------------------- rank
__global__ __launch_bounds__(256) void keep_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size, int64_t M,
                                                   int32_t min_size, int32_t* __restrict__ keep) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= M) return;
    keep[v] = (root[v] == (int32_t)v && size[v] > min_size) ? 1 : 0;
}

// rank[v] = number of kept roots below v: the kept clusters in ascending order of their smallest member (= their root).
__global__ __launch_bounds__(256) void label_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                                    const int32_t* __restrict__ rank, int64_t M, int32_t min_size,
                                                    int32_t* __restrict__ labels, int32_t* __restrict__ sizes,
                                                    int32_t* __restrict__ n_clusters) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v == 0) *n_clusters = rank[M];
    if (v >= M) return;
    const int32_t r = root[v];
    const bool kept = r >= 0 && size[r] > min_size;
    labels[v] = kept ? rank[r] : -1;
    if (kept && r == (int32_t)v) sizes[rank[r]] = size[r];
}

// ------------------------------------------------------------------------------------------------------- workspace
struct Work {
    IndexBufs ix;
    int32_t *vslot, *scr, *parent, *size, *root, *keep, *rank;
};

inline Work carve(Carver& c, int64_t M) {
    Work W;
    W.ix = take_index(c, M);
    W.vslot = c.take<int32_t>(M);
    W.scr = take_scan(c, W.ix.cap > M ? W.ix.cap : M);              // the index's counts, then M keep flags
    W.parent = c.take<int32_t>(M);
    W.size = c.take<int32_t>(M);
    W.root = c.take<int32_t>(M);
    W.keep = c.take<int32_t>(M);
    W.rank = c.take<int32_t>(M + 1);
    return W;
}

inline bool sizes_ok(int64_t M) { return M >= 0 && M < (1ll << 30); }

}  // namespace

extern "C" int64_t misplat_cluster_workspace(int64_t n_vertices) {
    if (!sizes_ok(n_vertices)) return -1;
    Carver c{nullptr};
    carve(c, n_vertices);
    return c.o;
}

extern "C" int misplat_cluster_radius(const float* vertices, int64_t n_vertices, const uint8_t* mask, float radius,
                                      int32_t min_cluster_size, void* workspace, int64_t workspace_bytes, int32_t* labels,
                                      int32_t* sizes, int32_t* n_clusters, misplat_stream_t stream) {
    const int64_t M = n_vertices;
    const float inv_h = 1.f / radius;
    if (!sizes_ok(M) || !(radius > 0.f) || !(radius < 3.0e37f) || !(inv_h < 3.0e38f) || min_cluster_size < 0 || !workspace ||
        !n_clusters || (M > 0 && (!vertices || !mask || !labels || !sizes)))
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, M);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) {
        misplat_internal::fill_bytes(n_clusters, 4, 0u, s);
        return launched();
    }
    const unsigned nb = blocks(M, 256);
    const Index ix = build_index(vertices, M, mask, inv_h, W.ix, W.vslot, W.scr, s);
    hipLaunchKernelGGL(uf_init_kernel<int32_t>, dim3(nb), dim3(256), 0, s, M, W.parent, W.size);
    hipLaunchKernelGGL(union_kernel, dim3(blocks(M * kSub, 256)), dim3(256), 0, s, ix, W.ix.cap, radius, radius * radius, inv_h,
                       W.parent);
    hipLaunchKernelGGL(flatten_kernel<true>, dim3(nb), dim3(256), 0, s, (const int32_t*)W.parent, mask, M, W.root, W.size);
    hipLaunchKernelGGL(keep_kernel, dim3(nb), dim3(256), 0, s, (const int32_t*)W.root, (const int32_t*)W.size, M, min_cluster_size,
                       W.keep);
    scan(W.keep, M, W.rank, W.scr, s);
    hipLaunchKernelGGL(label_kernel, dim3(nb), dim3(256), 0, s, (const int32_t*)W.root, (const int32_t*)W.size,
                       (const int32_t*)W.rank, M, min_cluster_size, labels, sizes, n_clusters);
    return launched();
}
