// meshclean.hip -- mesh finishing: the edge table of a triangle mesh and what reads it (edge
// statistics, edge-connected components, boundary loops), the RANSAC plane fit (hypotheses, inlier counts, the fp64
// moments of the refit), and Laplacian smoothing over a sorted CSR of the directed edges.
//
// Semantics: tests/meshclean_restatement.py is the oracle.  Compiled with -ffp-contract=off: every fp32 expression is
// evaluated in the written order.  Integer atomics only; every fp64 sum runs in a fixed order; two runs are bitwise equal.
//
// Edge table: every undirected edge (lo, hi), lo < hi, of every triangle in an open-addressing hash, key lo << 32 | hi,
// capacity the power of two >= max(64, 6 T): facetable.h's.  A slot holds the number of (face, corner) incidences of its edge
// and the smallest incident face.  Which slot an edge takes depends on the insertion race; nothing that is read back does.  A corner
// repeated inside a triangle gives an edge (a, a): it is ignored everywhere.  Readers find an edge's slot by probing
// again: the table keeps no per-corner slot list (3 T int32 the less).
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

// ----------------------------------------------------------------------------------------------------- edge table
// (facetable.h's, taken without the largest face)

// counts: 0 edges, 1 boundary edges (one incidence), 2 non-manifold edges (more than two)
__global__ __launch_bounds__(256) void edge_count_kernel(EdgeTable E, int64_t cap, int32_t* __restrict__ counts) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = (s < cap && E.keys[s] != kEmpty) ? E.cnt[s] : 0;
    const unsigned long long any = __ballot(c > 0), one = __ballot(c == 1), many = __ballot(c > 2);
    if ((threadIdx.x & 63) == 0) {
        if (any) atomicAdd(&counts[0], __popcll(any));
        if (one) atomicAdd(&counts[1], __popcll(one));
        if (many) atomicAdd(&counts[2], __popcll(many));
    }
}

// ------------------------------------------------------------------------------------------------- fixed-order sums
// wgprims.h's: K doubles per thread through block_sums<K>, the workgroup partials through sum_final_kernel<K, 256>.
// Every undirected edge once, in an order the table has no part in: at the lowest corner of its smallest incident face.
__global__ __launch_bounds__(256) void edge_length_kernel(const float* __restrict__ V, const int32_t* __restrict__ tri, int64_t T,
                                                          EdgeTable E, double* __restrict__ part) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double len[1] = {0.0};
    if (h < 3 * T) {
        const int64_t f = h / 3;
        const int c = (int)(h - 3 * f);
        int32_t a, b;
        corner_edge(tri, f, c, a, b);
        if (a != b) {
            const unsigned long long key = edge_key(a, b);
            bool first = E.fmin[edge_find(E, key)] == (int32_t)f;
            for (int c0 = 0; c0 < c; c0++) {
                int32_t a0, b0;
                corner_edge(tri, f, c0, a0, b0);
                if (a0 != b0 && edge_key(a0, b0) == key) first = false;
            }
            if (first) len[0] = (double)edge_length(V, a, b);
        }
    }
    block_sums<1>(len, part + blockIdx.x);
}

__global__ void edge_mean_kernel(const double* __restrict__ sum, const int32_t* __restrict__ counts, double* __restrict__ mean) {
    *mean = counts[0] > 0 ? *sum / (double)counts[0] : 0.0;
}

// ------------------------------------------------------------------------------------------------------ components
// every face is united with the smallest face of each of its edges: the faces around one edge, a non-manifold one
// included, end in one tree
__global__ __launch_bounds__(256) void face_union_kernel(const int32_t* __restrict__ tri, int64_t T, EdgeTable E,
                                                         int32_t* __restrict__ parent) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= 3 * T) return;
    const int64_t f = h / 3;
    int32_t a, b;
    corner_edge(tri, f, (int)(h - 3 * f), a, b);
    if (a == b) return;
    const int32_t g = E.fmin[edge_find(E, edge_key(a, b))];
    if (g != (int32_t)f) (void)unite(parent, (int32_t)f, g);
}

__global__ __launch_bounds__(256) void is_root_kernel(const int32_t* __restrict__ root, int64_t n, int32_t* __restrict__ keep) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n) keep[v] = root[v] == (int32_t)v ? 1 : 0;
}

// rank[f] = the number of roots below f: the components in ascending order of their smallest face (= their root)
__global__ __launch_bounds__(256) void face_label_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                                         const int32_t* __restrict__ rank, int64_t T, int32_t* __restrict__ labels,
                                                         int32_t* __restrict__ sizes, int32_t* __restrict__ n_components) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f == 0) *n_components = rank[T];
    if (f >= T) return;
    const int32_t r = root[f];
    labels[f] = rank[r];
    if (r == (int32_t)f) sizes[rank[r]] = size[r];
}

// ----------------------------------------------------------------------------------------------------------- holes
__global__ __launch_bounds__(256) void boundary_flag_kernel(const int32_t* __restrict__ tri, int64_t T, EdgeTable E,
                                                            int32_t* __restrict__ flag) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= 3 * T) return;
    const int64_t f = h / 3;
    int32_t a, b;
    corner_edge(tri, f, (int)(h - 3 * f), a, b);
    flag[h] = (a != b && E.cnt[edge_find(E, edge_key(a, b))] == 1) ? 1 : 0;
}

// the boundary edges in ascending (face, corner) order, directed as their face runs; their ends are united
__global__ __launch_bounds__(256) void boundary_emit_kernel(const float* __restrict__ V, const int32_t* __restrict__ tri, int64_t T,
                                                            const int32_t* __restrict__ flag, const int32_t* __restrict__ pos,
                                                            int32_t* __restrict__ edges, float* __restrict__ length,
                                                            int32_t* __restrict__ vparent, int32_t* __restrict__ counts) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h == 0) counts[0] = pos[3 * T];
    if (h >= 3 * T || !flag[h]) return;
    const int64_t f = h / 3;
    int32_t a, b;
    corner_edge(tri, f, (int)(h - 3 * f), a, b);
    const int64_t e = pos[h];
    edges[2 * e] = a;
    edges[2 * e + 1] = b;
    length[e] = edge_length(V, a, b);
    (void)unite(vparent, a, b);
}

// eroot[e] = the smallest vertex of edge e's loop; on[v] = 1 for the vertices that are such a root (every writer stores 1)
__global__ __launch_bounds__(256) void loop_root_kernel(const int32_t* __restrict__ edges, const int32_t* __restrict__ n_boundary,
                                                        const int32_t* __restrict__ vparent, int32_t* __restrict__ eroot,
                                                        int32_t* __restrict__ on) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= *n_boundary) return;
    const int32_t r = walk_root(vparent, edges[2 * e]);
    eroot[e] = r;
    on[r] = 1;
}

__global__ __launch_bounds__(256) void loop_label_kernel(const int32_t* __restrict__ eroot, const int32_t* __restrict__ vrank,
                                                         int64_t M, int32_t* __restrict__ counts, int32_t* __restrict__ loop_of_edge) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e == 0) counts[1] = vrank[M];
    if (e >= counts[0]) return;
    loop_of_edge[e] = vrank[eroot[e]];
}

// out[l] = values[order[e]] summed in fp64 over e = offsets[l] .. offsets[l + 1) in that order: one thread per segment
__global__ __launch_bounds__(256) void segment_sum_kernel(const float* __restrict__ values, const int32_t* __restrict__ order,
                                                          const int32_t* __restrict__ offsets, int64_t L, double* __restrict__ out) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    double acc = 0.0;
    for (int32_t e = offsets[l]; e < offsets[l + 1]; e++) acc += (double)values[order[e]];
    out[l] = acc;
}

// ----------------------------------------------------------------------------------------------------------- planes
// Draw `draw` of hypothesis i under `seed`: a counter-based integer hash (two rounds of a 32-bit finaliser, hashmix.h),
// reduced to 0 .. N - 1 by the high half of a 64-bit product.  tests/meshclean_restatement.py holds the same arithmetic.
__device__ __forceinline__ uint32_t draw_index(uint32_t seed, uint32_t i, uint32_t draw, uint32_t N) {
    return (uint32_t)(((unsigned long long)mix32(seed, i, draw) * N) >> 32);
}

constexpr uint32_t kMaxDraws = 64;    // after so many draws a repeat is resolved by stepping to the next index (N >= 3)

// Three distinct indices (drawn, or given), then the plane through them in fp32: e1 = p1 - p0, e2 = p2 - p0, n = e1 x e2,
// |n| = sqrtf((nx nx + ny ny) + nz nz), the plane (n / |n|, -((nx' x0 + ny' y0) + nz' z0)).  A triple whose |n| is not > 0
// (collinear, repeated) gives four NaN: no point is ever within a threshold of it.
__global__ __launch_bounds__(256) void plane_build_kernel(const float* __restrict__ P, uint32_t N, const int32_t* __restrict__ given,
                                                          uint32_t seed, int32_t H, int32_t* __restrict__ triples,
                                                          float4* __restrict__ planes) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H) return;
    uint32_t id[3];
    if (given) {
        for (int j = 0; j < 3; j++) id[j] = (uint32_t)given[3 * i + j];
    } else {
        uint32_t draw = 0;
        for (int j = 0; j < 3; j++) {
            while (true) {
                uint32_t c = draw_index(seed, (uint32_t)i, draw, N);
                draw++;
                bool repeat = false;
                for (int q = 0; q < j; q++) repeat |= id[q] == c;
                if (repeat && draw > kMaxDraws) {
                    while (repeat) {
                        c = c + 1 == N ? 0 : c + 1;
                        repeat = false;
                        for (int q = 0; q < j; q++) repeat |= id[q] == c;
                    }
                }
                if (!repeat) { id[j] = c; break; }
            }
        }
        for (int j = 0; j < 3; j++) triples[3 * i + j] = (int32_t)id[j];
    }
    const float* p0 = P + 3 * (int64_t)id[0];
    const float* p1 = P + 3 * (int64_t)id[1];
    const float* p2 = P + 3 * (int64_t)id[2];
    const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
    const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
    float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const float norm = sqrtf((nx * nx + ny * ny) + nz * nz);
    const float nan = __int_as_float(0x7fc00000);
    float4 pl = make_float4(nan, nan, nan, nan);
    if (norm > 0.f) {
        nx = nx / norm; ny = ny / norm; nz = nz / norm;
        pl = make_float4(nx, ny, nz, -((nx * p0[0] + ny * p0[1]) + nz * p0[2]));
    }
    planes[i] = pl;
}

// The hot kernel: N x H (point, plane) pairs.  A workgroup owns a tile of KT hypotheses: their coefficients are the same
// for every lane (loaded through a workgroup-uniform index: scalar loads, scalar operands of the vector multiplies) and
// a stride of the points; each lane keeps one counter per hypothesis in a register while it walks its points, so a point is
// loaded once per KT planes.  The counters are summed across the wave by shuffles, across the four waves in LDS, and
// reach memory as one integer add per (workgroup, hypothesis).  inlier iff |((a x + b y) + c z) + d| < t, strict.
template <int KT>
__global__ __launch_bounds__(256) void plane_count_kernel(const float* __restrict__ P, int64_t N, const float4* __restrict__ planes,
                                                          int32_t H, float t, int32_t* __restrict__ counts) {
    __shared__ int32_t total[KT];
    const int32_t h0 = blockIdx.x * KT;
    float4 pl[KT];
    int32_t cnt[KT];
#pragma unroll
    for (int k = 0; k < KT; k++) {
        pl[k] = planes[h0 + k < H ? h0 + k : H - 1];
        cnt[k] = 0;
    }
    if (threadIdx.x < KT) total[threadIdx.x] = 0;
    const int64_t step = (int64_t)gridDim.y * 256;
    for (int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x; i < N; i += step) {
        const float x = P[3 * i], y = P[3 * i + 1], z = P[3 * i + 2];
#pragma unroll
        for (int k = 0; k < KT; k++) {
            const float v = ((pl[k].x * x + pl[k].y * y) + pl[k].z * z) + pl[k].w;
            cnt[k] += fabsf(v) < t ? 1 : 0;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KT; k++) {
        int32_t c = cnt[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&total[k], c);
    }
    __syncthreads();
    if (threadIdx.x < KT && h0 + (int)threadIdx.x < H && total[threadIdx.x]) atomicAdd(&counts[h0 + threadIdx.x], total[threadIdx.x]);
}

template <int KT>
void launch_plane_count(const float* P, int64_t N, const float* planes, int32_t H, float t, int32_t* counts, hipStream_t s) {
    const int64_t tiles = (H + KT - 1) / KT;
    // enough workgroups to fill the device (256 CUs, 8 of these workgroups each) however few the tiles, at most one per 256
    // points, and no more: every workgroup ends in KT integer adds to memory
    int64_t chunks = (4096 + tiles - 1) / tiles;
    const int64_t most = (N + 255) / 256;
    if (chunks > most) chunks = most;
    if (chunks > 65535) chunks = 65535;
    hipLaunchKernelGGL((plane_count_kernel<KT>), dim3((unsigned)tiles, (unsigned)chunks), dim3(256), 0, s, P, N, (const float4*)planes,
                       H, t, counts);
}

// The refit's moments of the inliers of ONE plane (on the device).  Pass 0 writes mask[i] and sums (n, x, y, z); pass 1 sums
// the six products of the coordinates minus the mean, (xx, xy, xz, yy, yz, zz).  fp64, 256 points per workgroup.
__device__ __forceinline__ bool plane_inlier(const float* __restrict__ P, int64_t i, const float4 pl, float t) {
    const float v = ((pl.x * P[3 * i] + pl.y * P[3 * i + 1]) + pl.z * P[3 * i + 2]) + pl.w;
    return fabsf(v) < t;
}

__global__ __launch_bounds__(256) void moment_mean_kernel(const float* __restrict__ P, int64_t N, const float4* __restrict__ plane,
                                                          float t, uint8_t* __restrict__ mask, double* __restrict__ part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    if (i < N) {
        const bool in = plane_inlier(P, i, *plane, t);
        mask[i] = in ? 1 : 0;
        if (in) { x[0] = 1.0; x[1] = (double)P[3 * i]; x[2] = (double)P[3 * i + 1]; x[3] = (double)P[3 * i + 2]; }
    }
    block_sums<4>(x, part + 4 * (int64_t)blockIdx.x);
}

__global__ __launch_bounds__(256) void moment_cov_kernel(const float* __restrict__ P, int64_t N, const uint8_t* __restrict__ mask,
                                                         const double* __restrict__ mom, double* __restrict__ part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < N && mask[i]) {
        const double dx = (double)P[3 * i] - mom[1] / mom[0], dy = (double)P[3 * i + 1] - mom[2] / mom[0],
                     dz = (double)P[3 * i + 2] - mom[3] / mom[0];
        x[0] = dx * dx; x[1] = dx * dy; x[2] = dx * dz; x[3] = dy * dy; x[4] = dy * dz; x[5] = dz * dz;
    }
    block_sums<6>(x, part + 6 * (int64_t)blockIdx.x);
}

// ------------------------------------------------------------------------------------------------------- smoothing
// Laplacian smoothing over the CSR of the sorted directed edges of all corners (meshadj.h).
__global__ __launch_bounds__(256) void smooth_edges_kernel(const int32_t* __restrict__ tri, int64_t T, int32_t* __restrict__ tgt,
                                                           int32_t* __restrict__ src) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= 3 * T) return;
    const int64_t f = h / 3;
    emit_corner_edges(tri, f, (int)(h - 3 * f), h, tgt, src);
}

// One lane per (vertex i, channel c) of values [M, D]: out = x + lam (sum_j w_ij x_j / sum_j w_ij - x) over the distinct
// neighbours j != i in ascending order, w_ij = 1 / (|p_i - p_j| + 1e-12) from the positions pos; fp64 throughout in this one
// order, stored fp32.  A repeated edge is met once (the row is sorted: a repeat follows its twin); no neighbour: unchanged.
__global__ __launch_bounds__(256) void smooth_gather_kernel(const float* __restrict__ pos, int64_t M, const int32_t* __restrict__ rows,
                                                            const int32_t* __restrict__ tgt, const float* __restrict__ values, int D,
                                                            double lam, float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * D) return;
    const int64_t i = idx / D;
    const int c = (int)(idx - i * D);
    const double px = (double)pos[3 * i], py = (double)pos[3 * i + 1], pz = (double)pos[3 * i + 2];
    double W = 0.0, S = 0.0;
    int32_t prev = -1;
    for (int32_t e = rows[2 * i]; e < rows[2 * i + 1]; e++) {
        const int32_t j = tgt[e];
        if (j == prev || j == (int32_t)i) continue;
        prev = j;
        const double dx = (double)pos[3 * (int64_t)j] - px, dy = (double)pos[3 * (int64_t)j + 1] - py,
                     dz = (double)pos[3 * (int64_t)j + 2] - pz;
        const double w = 1.0 / (sqrt((dx * dx + dy * dy) + dz * dz) + 1e-12);
        W += w;
        S += w * (double)values[(int64_t)j * D + c];
    }
    const double x = (double)values[idx];
    out[idx] = W > 0.0 ? (float)(x + lam * (S / W - x)) : values[idx];
}

// ------------------------------------------------------------------------------------------------------- workspace
enum { kKindStats = 0, kKindComponents = 1, kKindHoles = 2, kKindMoments = 3, kKindSmooth = 4 };

// what a kind does not use stays null
struct Work {
    EdgeTable edges;                  // (the smallest face only)
    int32_t* scr;
    double *part, *sum;
    int32_t *parent, *size, *root, *keep, *rank, *flag, *pos, *eroot;
    int32_t *ka, *va, *kb, *vb, *rows;    // smoothing: the two pairs of the sort over the 6 T directed edges, the CSR rows [2 M]
    SortBufs sort;
};

// M vertices, T triangles (mesh kinds) or N points (kKindMoments, passed as M)
inline Work carve(Carver& c, int64_t M, int64_t T, int kind) {
    Work W = {};
    if (kind == kKindMoments) {
        W.part = c.take<double>(6 * ((M + 255) / 256 + 1));
        return W;
    }
    if (kind == kKindSmooth) {                             // (no edge table: the sorted directed edges serve)
        const int64_t E = 6 * T;
        W.ka = c.take<int32_t>(E);
        W.va = c.take<int32_t>(E);
        W.kb = c.take<int32_t>(E);
        W.vb = c.take<int32_t>(E);
        W.rows = c.take<int32_t>(2 * M);
        W.scr = take_scan(c, 256 * ((E + kTile - 1) / kTile) + 1);
        W.sort = take_sort(c, E);
        return W;
    }
    W.edges = take_edge_table(c, T, false);
    W.scr = take_scan(c, 3 * T > M ? 3 * T : M);
    if (kind == kKindStats) {
        W.part = c.take<double>((3 * T + 255) / 256 + 1);
        W.sum = c.take<double>(1);
    }
    if (kind == kKindComponents) {
        W.parent = c.take<int32_t>(T);
        W.size = c.take<int32_t>(T);
        W.root = c.take<int32_t>(T);
        W.keep = c.take<int32_t>(T);
        W.rank = c.take<int32_t>(T + 1);
    }
    if (kind == kKindHoles) {
        W.flag = c.take<int32_t>(3 * T);
        W.pos = c.take<int32_t>(3 * T + 1);
        W.eroot = c.take<int32_t>(3 * T);
        W.parent = c.take<int32_t>(M);
        W.keep = c.take<int32_t>(M);
        W.rank = c.take<int32_t>(M + 1);
    }
    return W;
}

inline bool mesh_ok(int64_t M, int64_t T) { return M >= 0 && M < (1ll << 31) && T >= 0 && T < (1ll << 30); }
// the calls that number the 3 T corners (or the edges) in int32
inline bool corners_ok(int64_t T) { return 3 * T < (1ll << 31); }
inline bool cloud_ok(int64_t N) { return N >= 0 && N < (1ll << 30); }
// smoothing sorts the 6 T directed edges
inline bool smooth_ok(int64_t T) { return 6 * T < (1ll << 31) - kTile; }

}  // namespace

extern "C" int64_t misplat_meshclean_workspace(int64_t n_vertices, int64_t n_triangles, int32_t kind) {
    if (kind < kKindStats || kind > kKindSmooth) return -1;
    if (kind == kKindMoments ? !cloud_ok(n_vertices)
                             : !mesh_ok(n_vertices, n_triangles) || (kind != kKindComponents && !corners_ok(n_triangles)))
        return -1;
    if (kind == kKindSmooth && !smooth_ok(n_triangles)) return -1;
    Carver c{nullptr};
    carve(c, n_vertices, kind == kKindMoments ? 0 : n_triangles, kind);
    return c.o;
}

extern "C" int misplat_meshclean_edge_stats(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                            void* workspace, int64_t workspace_bytes, int32_t* counts, double* mean_length,
                                            misplat_stream_t stream) {
    const int64_t M = n_vertices, T = n_triangles;
    if (!mesh_ok(M, T) || !corners_ok(T) || !workspace || !counts || !mean_length || (T > 0 && (!vertices || !triangles)))
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, M, T, kKindStats);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const EdgeTable& E = W.edges;
    build_edge_table(triangles, T, E, s);
    misplat_internal::fill_bytes(counts, 12, 0u, s);
    const int64_t cap = (int64_t)E.mask + 1;
    hipLaunchKernelGGL(edge_count_kernel, dim3(blocks(cap, 256)), dim3(256), 0, s, E, cap, counts);
    const int64_t nb = (3 * T + 255) / 256;
    if (nb > 0) hipLaunchKernelGGL(edge_length_kernel, dim3((unsigned)nb), dim3(256), 0, s, vertices, triangles, T, E, W.part);
    hipLaunchKernelGGL((sum_final_kernel<1, 256>), dim3(1), dim3(256), 0, s, (const double*)W.part, nb, W.sum);
    hipLaunchKernelGGL(edge_mean_kernel, dim3(1), dim3(1), 0, s, (const double*)W.sum, (const int32_t*)counts, mean_length);
    return launched();
}

extern "C" int misplat_meshclean_components(const int32_t* triangles, int64_t n_vertices, int64_t n_triangles, void* workspace,
                                            int64_t workspace_bytes, int32_t* labels, int32_t* sizes, int32_t* n_components,
                                            misplat_stream_t stream) {
    const int64_t M = n_vertices, T = n_triangles;
    if (!mesh_ok(M, T) || !workspace || !n_components || (T > 0 && (!triangles || !labels || !sizes))) return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, M, T, kKindComponents);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (T == 0) {
        misplat_internal::fill_bytes(n_components, 4, 0u, s);
        return launched();
    }
    const EdgeTable& E = W.edges;
    build_edge_table(triangles, T, E, s);
    const unsigned nb = blocks(T, 256);
    hipLaunchKernelGGL(uf_init_kernel<int32_t>, dim3(nb), dim3(256), 0, s, T, W.parent, W.size);
    hipLaunchKernelGGL(face_union_kernel, dim3(blocks(3 * T, 256)), dim3(256), 0, s, triangles, T, E, W.parent);
    hipLaunchKernelGGL(flatten_kernel<false>, dim3(nb), dim3(256), 0, s, (const int32_t*)W.parent, (const uint8_t*)nullptr, T, W.root,
                       W.size);
    hipLaunchKernelGGL(is_root_kernel, dim3(nb), dim3(256), 0, s, (const int32_t*)W.root, T, W.keep);
    scan(W.keep, T, W.rank, W.scr, s);
    hipLaunchKernelGGL(face_label_kernel, dim3(nb), dim3(256), 0, s, (const int32_t*)W.root, (const int32_t*)W.size,
                       (const int32_t*)W.rank, T, labels, sizes, n_components);
    return launched();
}

extern "C" int misplat_meshclean_holes(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                       void* workspace, int64_t workspace_bytes, int32_t* edges, int32_t* loop_of_edge,
                                       float* length, int32_t* counts, misplat_stream_t stream) {
    const int64_t M = n_vertices, T = n_triangles;
    if (!mesh_ok(M, T) || !corners_ok(T) || !workspace || !counts ||
        (T > 0 && (M < 1 || !vertices || !triangles || !edges || !loop_of_edge || !length)))
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, M, T, kKindHoles);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (T == 0) {
        misplat_internal::fill_bytes(counts, 8, 0u, s);
        return launched();
    }
    const EdgeTable& E = W.edges;
    build_edge_table(triangles, T, E, s);
    int32_t *scr = W.scr, *flag = W.flag, *pos = W.pos, *eroot = W.eroot;
    int32_t *vparent = W.parent, *on = W.keep, *vrank = W.rank;     // (over the vertices here)
    const unsigned nh = blocks(3 * T, 256);
    hipLaunchKernelGGL(uf_init_kernel<int32_t>, dim3(blocks(M, 256)), dim3(256), 0, s, M, vparent, on);
    hipLaunchKernelGGL(boundary_flag_kernel, dim3(nh), dim3(256), 0, s, triangles, T, E, flag);
    scan(flag, 3 * T, pos, scr, s);
    hipLaunchKernelGGL(boundary_emit_kernel, dim3(nh), dim3(256), 0, s, vertices, triangles, T, (const int32_t*)flag,
                       (const int32_t*)pos, edges, length, vparent, counts);
    hipLaunchKernelGGL(loop_root_kernel, dim3(nh), dim3(256), 0, s, (const int32_t*)edges, (const int32_t*)counts,
                       (const int32_t*)vparent, eroot, on);
    scan(on, M, vrank, scr, s);
    hipLaunchKernelGGL(loop_label_kernel, dim3(nh), dim3(256), 0, s, (const int32_t*)eroot, (const int32_t*)vrank, M, counts,
                       loop_of_edge);
    return launched();
}

extern "C" int misplat_meshclean_segment_sum(const float* values, const int32_t* order, const int32_t* offsets, int64_t n_segments,
                                             double* out, misplat_stream_t stream) {
    if (n_segments < 0 || n_segments >= (1ll << 31) || !offsets || (n_segments > 0 && (!values || !order || !out)))
        return MISPLAT_EINVAL;
    if (n_segments == 0) return MISPLAT_OK;
    hipLaunchKernelGGL(segment_sum_kernel, dim3(blocks(n_segments, 256)), dim3(256), 0, (hipStream_t)stream, values, order, offsets,
                       n_segments, out);
    return launched();
}

extern "C" int misplat_meshclean_smooth(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                        const float* attributes, int32_t n_channels, int32_t iterations, double lam,
                                        void* workspace, int64_t workspace_bytes, float* vertices_out, float* attributes_out,
                                        float* vertices_tmp, float* attributes_tmp, misplat_stream_t stream) {
    const int64_t M = n_vertices, T = n_triangles, E = 6 * T;
    const int D = n_channels;
    if (!mesh_ok(M, T) || !corners_ok(T) || !smooth_ok(T) || M < 1 || T < 1 || D < 0 || D > 4096 || M * (D > 3 ? D : 3) >= (1ll << 39) ||
        iterations < 1 || !(lam == lam) || !vertices || !triangles || !workspace || !vertices_out ||
        (D > 0 && (!attributes || !attributes_out)) || (iterations > 1 && (!vertices_tmp || (D > 0 && !attributes_tmp))))
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, M, T, kKindSmooth);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int32_t *ka = W.ka, *va = W.va, *kb = W.kb, *vb = W.vb;
    hipLaunchKernelGGL(smooth_edges_kernel, dim3(blocks(3 * T, 256)), dim3(256), 0, s, triangles, T, ka, va);
    const int passes = radix_passes(M - 1);
    sort_directed(ka, va, kb, vb, E, passes, passes, W.sort, W.scr, s);        // va the sources, ka the targets
    misplat_internal::fill_bytes(W.rows, 8 * (size_t)M, 0u, s);
    hipLaunchKernelGGL(rows_kernel, dim3(blocks(E, 256)), dim3(256), 0, s, (const int32_t*)va, E, W.rows);
    const float *pos = vertices, *att = attributes;
    for (int it = 0; it < iterations; it++) {
        const bool last_parity = (iterations - 1 - it) % 2 == 0;        // the last iteration writes the outputs
        float* pos_to = last_parity ? vertices_out : vertices_tmp;
        float* att_to = last_parity ? attributes_out : attributes_tmp;
        hipLaunchKernelGGL(smooth_gather_kernel, dim3(blocks(M * 3, 256)), dim3(256), 0, s, pos, M, (const int32_t*)W.rows,
                           (const int32_t*)ka, pos, 3, lam, pos_to);
        if (D > 0)
            hipLaunchKernelGGL(smooth_gather_kernel, dim3(blocks(M * D, 256)), dim3(256), 0, s, pos, M, (const int32_t*)W.rows,
                               (const int32_t*)ka, att, D, lam, att_to);
        pos = pos_to;
        att = att_to;
    }
    return launched();
}

extern "C" int misplat_meshclean_plane_build(const float* points, int64_t n_points, const int32_t* triples_in, uint32_t seed,
                                             int32_t n_planes, int32_t* triples_out, float* planes, misplat_stream_t stream) {
    if (!cloud_ok(n_points) || n_points < 3 || n_planes < 0 || n_planes > (1 << 24) || !points ||
        (n_planes > 0 && (!planes || (!triples_in && !triples_out))))
        return MISPLAT_EINVAL;
    if (n_planes == 0) return MISPLAT_OK;
    hipLaunchKernelGGL(plane_build_kernel, dim3(blocks(n_planes, 256)), dim3(256), 0, (hipStream_t)stream, points, (uint32_t)n_points,
                       triples_in, seed, n_planes, triples_out, (float4*)planes);
    return launched();
}

extern "C" int misplat_meshclean_plane_count(const float* points, int64_t n_points, const float* planes, int32_t n_planes,
                                             float threshold, int32_t tile, int32_t* counts, misplat_stream_t stream) {
    if (!cloud_ok(n_points) || n_planes < 0 || n_planes > (1 << 24) || !(threshold > 0.f) || !(tile == 8 || tile == 16 || tile == 32) ||
        (n_points > 0 && !points) || (n_planes > 0 && (!planes || !counts)))
        return MISPLAT_EINVAL;
    if (n_planes == 0) return MISPLAT_OK;
    hipStream_t s = (hipStream_t)stream;
    misplat_internal::fill_bytes(counts, 4 * (size_t)n_planes, 0u, s);
    if (n_points > 0) {
        if (tile == 8) launch_plane_count<8>(points, n_points, planes, n_planes, threshold, counts, s);
        else if (tile == 16) launch_plane_count<16>(points, n_points, planes, n_planes, threshold, counts, s);
        else launch_plane_count<32>(points, n_points, planes, n_planes, threshold, counts, s);
    }
    return launched();
}

extern "C" int misplat_meshclean_plane_moments(const float* points, int64_t n_points, const float* plane, float threshold,
                                               void* workspace, int64_t workspace_bytes, uint8_t* mask, double* moments,
                                               misplat_stream_t stream) {
    const int64_t N = n_points;
    if (!cloud_ok(N) || N < 1 || !(threshold > 0.f) || !points || !plane || !workspace || !mask || !moments) return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    double* part = carve(c, N, 0, kKindMoments).part;
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = (N + 255) / 256;
    hipLaunchKernelGGL(moment_mean_kernel, dim3((unsigned)nb), dim3(256), 0, s, points, N, (const float4*)plane, threshold, mask, part);
    hipLaunchKernelGGL((sum_final_kernel<4, 256>), dim3(1), dim3(256), 0, s, (const double*)part, nb, moments);
    hipLaunchKernelGGL(moment_cov_kernel, dim3((unsigned)nb), dim3(256), 0, s, points, N, (const uint8_t*)mask,
                       (const double*)moments, part);
    hipLaunchKernelGGL((sum_final_kernel<6, 256>), dim3(1), dim3(256), 0, s, (const double*)part, nb, moments + 4);
    return launched();
}
