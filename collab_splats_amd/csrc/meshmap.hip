// meshmap.hip -- k-nearest-vertex mapping of per-point values onto mesh vertices.
//
// Semantics: the Gaussian-weighted kNN map of the reference's features2vertex / normals2vertex, restated in fp32
// (tests/meshmap_restatement.py is the oracle).  Compiled with -ffp-contract=off: every expression is evaluated in the
// written order, so the neighbour lists equal the restatement's bit for bit and two runs are bitwise equal.
//
// Spatial index (csrc/cellhash.h): a hash of the OCCUPIED cells of edge h = sdf_trunc (open addressing, capacity a power of two >= 2 M), and
// the vertices regrouped by cell (count, scan, fill): memory O(M) whatever the extent of the scene.
// Query: one thread per point; the cells within sdf_trunc first (no vertex there: invalid, done), then rings of cells until
// the k-th distance is below the distance to the unvisited space; beyond kMaxRings rings, a scan of every vertex.
// Aggregation: sigma (fp64, fixed order) -> row weights -> a stable LSD radix sort of the contributions by vertex (each list
// then in (i, j) order) -> per-chunk fp32 sums in list order -> per-vertex sum of the chunks in chunk order.  No float atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"
#include "internal.h"
#include "cellhash.h"
#include "radixsort.h"

namespace {

constexpr int kMaxRings = 6;          // rings beyond the sdf_trunc box before the query falls back to a scan of every vertex
constexpr int kChunk = 512;           // contributions per partial sum (longer lists are split, cdna guide Appendix B)

// ----------------------------------------------------------------------------------------------------------- query
// k best of (d2 bits, vertex index) as one 64-bit key (cellhash.h's KBest); unset slots hold kEmpty
template <int KC>
using Best = KBest<unsigned long long, KC>;

__device__ __forceinline__ unsigned long long cand_key(float px, float py, float pz, float4 q) {
    const float dx = px - q.x, dy = py - q.y, dz = pz - q.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    return ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)__float_as_int(q.w);
}

template <int KC>
__device__ __forceinline__ void visit(const Index& ix, int cx, int cy, int cz, float px, float py, float pz, Best<KC>& best) {
    const int s = find_cell(ix.keys, ix.mask, cell_key(cx, cy, cz));
    if (s < 0) return;
    const int e1 = ix.starts[s + 1];
    for (int e = ix.starts[s]; e < e1; e++) best.offer(cand_key(px, py, pz, ix.pts[e]));
}

// cells of the box lo..hi that are not in the box lo + 1 .. hi - 1 (all of them if `all`)
template <int KC>
__device__ __forceinline__ void visit_box(const Index& ix, const int (&lo)[3], const int (&hi)[3], bool all, float px, float py,
                                          float pz, Best<KC>& best) {
    for (int cz = lo[2]; cz <= hi[2]; cz++)
        for (int cy = lo[1]; cy <= hi[1]; cy++) {
            const bool inner = !all && cz > lo[2] && cz < hi[2] && cy > lo[1] && cy < hi[1];
            const int step = (inner && hi[0] > lo[0]) ? hi[0] - lo[0] : 1;
            for (int cx = lo[0]; cx <= hi[0]; cx += step) visit<KC>(ix, cx, cy, cz, px, py, pz, best);
        }
}

template <int KC>
__global__ __launch_bounds__(256) void knn_kernel(Index ix, int64_t M, const float* __restrict__ P, int64_t N, int k, float trunc,
                                                  float h, float inv_h, int32_t* __restrict__ idx, float* __restrict__ dist,
                                                  uint8_t* __restrict__ valid) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float px = P[3 * i], py = P[3 * i + 1], pz = P[3 * i + 2];
    const float amax = fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz));
    // Every vertex has |v| < 2^18 h: a point further out than 2^18 h + 2 h (or not finite) has none within h >= trunc.
    bool ok = amax * inv_h < kCoordCells + 2.f;
    Best<KC> best;
    best.reset(k);
    int lo[3], hi[3];
    // rounding of the cell assignment, of the distances and of the box faces: the box and the stop test are widened by this
    const float margin = 1e-5f * (amax + h * (float)(kMaxRings + 4));
    if (ok) {
        const float p[3] = {px, py, pz};
        const float tt = trunc + margin;
#pragma unroll
        for (int a = 0; a < 3; a++) { lo[a] = cell_of(p[a] - tt, inv_h); hi[a] = cell_of(p[a] + tt, inv_h); }
        visit_box<KC>(ix, lo, hi, true, px, py, pz, best);
        const unsigned long long b0 = best.nearest(k);
        ok = b0 != kEmpty && sqrtf(__uint_as_float((uint32_t)(b0 >> 32))) <= trunc;
    }
    if (!ok) {
        valid[i] = 0;
        for (int j = 0; j < k; j++) {
            idx[i * k + j] = -1;
            dist[i * k + j] = __int_as_float(0x7f800000);
        }
        return;
    }
    const float p[3] = {px, py, pz};
    for (int r = 0;; r++) {
        float gap = 3.4e38f;
#pragma unroll
        for (int a = 0; a < 3; a++) gap = fminf(gap, fminf(p[a] - (float)lo[a] * h, (float)(hi[a] + 1) * h - p[a]));
        const unsigned long long kth = best.b[KC - 1];
        if (kth != kEmpty && sqrtf(__uint_as_float((uint32_t)(kth >> 32))) < gap - margin) break;
        if (r == kMaxRings) {                               // far-flung neighbours: every vertex, once
            best.reset(k);
            for (int64_t e = 0; e < M; e++) best.offer(cand_key(px, py, pz, ix.pts[e]));
            break;
        }
#pragma unroll
        for (int a = 0; a < 3; a++) { lo[a] -= 1; hi[a] += 1; }
        visit_box<KC>(ix, lo, hi, false, px, py, pz, best);
    }
    valid[i] = 1;
#pragma unroll
    for (int j = 0; j < KC; j++) {
        if (j < KC - k) continue;
        idx[i * k + (j - (KC - k))] = (int32_t)(uint32_t)best.b[j];
        dist[i * k + (j - (KC - k))] = sqrtf(__uint_as_float((uint32_t)(best.b[j] >> 32)));
    }
}

// ---------------------------------------------------------------------------------------------------------- sigma
// stats[0] = sum of the distances of the valid rows (fp64), stats[1] = number of valid rows.  Rows are summed in j order,
// 256 rows per workgroup in a fixed tree, the workgroup sums in index order by one workgroup: the result does not depend on
// scheduling (wgprims.h: block_sums, then sum_final_kernel<2, 256>).
__global__ __launch_bounds__(256) void sigma_partial_kernel(const float* __restrict__ dist, const uint8_t* __restrict__ valid,
                                                            int64_t N, int k, double* __restrict__ part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double sc[2] = {0.0, 0.0};
    if (i < N && valid[i]) {
        for (int j = 0; j < k; j++) sc[0] += (double)dist[i * k + j];
        sc[1] = 1.0;
    }
    block_sums<2>(sc, part + 2 * blockIdx.x);
}

// --------------------------------------------------------------------------------------------------------- weights
// One thread per row.  w[i, j] = e_j / sum_j e_j with e_j = exp(-(d2_j - d2_0) / (2 sigma^2)) (e_0 = 1: never 0 / 0);
// sigma = 0: 1 / k.  Sort keys: the vertex of each valid contribution, M (after every vertex) for an invalid row; values:
// the contribution id i k + j.
__device__ __forceinline__ float row_exp(float dj, float d02, float c, bool flat) {
    const float delta = dj * dj - d02;
    return (flat || !(delta > 0.f)) ? 1.f : expf(-(delta * c));
}

__global__ __launch_bounds__(256) void weights_kernel(const int32_t* __restrict__ idx, const float* __restrict__ dist,
                                                      const uint8_t* __restrict__ valid, int64_t N, int k, int32_t M,
                                                      const double* __restrict__ stats, float* __restrict__ w,
                                                      int32_t* __restrict__ keys, int32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int64_t base = i * k;
    for (int j = 0; j < k; j++) vals[base + j] = (int32_t)(base + j);
    if (!valid[i]) {
        for (int j = 0; j < k; j++) keys[base + j] = M;
        return;
    }
    const double n_valid = stats[1];
    const double sigma = stats[0] / (n_valid * (double)k);
    const bool flat = !(sigma > 0.0);
    const float c = flat ? 0.f : (float)(1.0 / (2.0 * sigma * sigma));
    const float d0 = dist[base];
    const float d02 = d0 * d0;
    float sum = 0.f;
    for (int j = 0; j < k; j++) sum += row_exp(dist[base + j], d02, c, flat);
    for (int j = 0; j < k; j++) {
        w[base + j] = row_exp(dist[base + j], d02, c, flat) / sum;
        keys[base + j] = idx[base + j];
    }
}

// ----------------------------------------------------------------------------------------------------- radix sort
// csrc/radixsort.h (stable, by key): the values enter in contribution order, so every vertex's list leaves in (i, j) order.

// offs[v] = first sorted position whose key is >= v (a binary search), v = 0 .. M (offs[M]: number of valid contributions)
__global__ __launch_bounds__(256) void list_offsets_kernel(const int32_t* __restrict__ skeys, int64_t E, int32_t M,
                                                           int32_t* __restrict__ offs) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v > M) return;
    int64_t a = 0, b = E;
    while (a < b) {
        const int64_t m = (a + b) >> 1;
        if (skeys[m] < v) a = m + 1;
        else b = m;
    }
    offs[v] = (int32_t)a;
}

__global__ __launch_bounds__(256) void chunk_count_kernel(const int32_t* __restrict__ offs, int32_t M, int32_t* __restrict__ nch) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= M) return;
    nch[v] = (offs[v + 1] - offs[v] + kChunk - 1) / kChunk;
}

__global__ __launch_bounds__(256) void chunk_owner_kernel(const int32_t* __restrict__ choff, int32_t M, int32_t* __restrict__ owner) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= M) return;
    for (int32_t q = choff[v]; q < choff[v + 1]; q++) owner[q] = (int32_t)v;
}

// ------------------------------------------------------------------------------------------------------------- sums
// One thread per (chunk, channel); channel D is the weight sum.  fp32, in list order.
__global__ __launch_bounds__(256) void chunk_sum_kernel(const int32_t* __restrict__ owner, const int32_t* __restrict__ choff,
                                                        const int32_t* __restrict__ offs, int32_t M,
                                                        const int32_t* __restrict__ svals, const float* __restrict__ w,
                                                        const float* __restrict__ F, int D, int k, int64_t q_cap,
                                                        float* __restrict__ part) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t q = t / (D + 1);
    const int c = (int)(t - q * (D + 1));
    if (q >= q_cap || q >= choff[M]) return;
    const int32_t v = owner[q];
    const int32_t e0 = offs[v] + (int32_t)(q - choff[v]) * kChunk;
    const int32_t e1 = min(e0 + kChunk, offs[v + 1]);
    float acc = 0.f;
    if (c < D) {
        for (int32_t e = e0; e < e1; e++) {
            const int32_t id = svals[e];
            acc += w[id] * F[(int64_t)(id / k) * D + c];
        }
    } else {
        for (int32_t e = e0; e < e1; e++) acc += w[svals[e]];
    }
    part[q * (D + 1) + c] = acc;
}

// One thread per vertex: the chunk sums in chunk order, divided by the weight sum (0 without a contribution); channels
// 0 .. n_unit - 1 then divided by (their norm + 1e-8).
__global__ __launch_bounds__(256) void vertex_sum_kernel(const int32_t* __restrict__ choff, int32_t M, const float* __restrict__ part,
                                                         int D, int n_unit, float* __restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= M) return;
    const int32_t q0 = choff[v], q1 = choff[v + 1];
    float den = 0.f;
    for (int32_t q = q0; q < q1; q++) den += part[(int64_t)q * (D + 1) + D];
    float* o = out + v * D;
    for (int c = 0; c < D; c++) {
        float num = 0.f;
        for (int32_t q = q0; q < q1; q++) num += part[(int64_t)q * (D + 1) + c];
        o[c] = den > 0.f ? num / den : 0.f;
    }
    if (n_unit == 3) {
        const float x = o[0], y = o[1], z = o[2];
        const float nrm = sqrtf((x * x + y * y) + z * z) + 1e-8f;
        o[0] = x / nrm; o[1] = y / nrm; o[2] = z / nrm;
    }
}

// ------------------------------------------------------------------------------------------------------- workspace
// the query's part first: misplat_meshmap_knn asks for no more than `knn_bytes`
struct Work {
    IndexBufs ix;
    int32_t *vslot, *scr;
    double* sig;
    int64_t knn_bytes;
    float* w;
    int32_t *ka, *va, *kb, *vb;
    SortBufs sort;
    int32_t *offs, *nch, *choff, *owner;
    float* part;
    int64_t E, q_cap;
};

inline Work carve(Carver& c, int64_t M, int64_t N, int k, int D) {
    Work W;
    W.E = N * k;
    W.q_cap = M + W.E / kChunk + 1;
    const int64_t n_hist = 256 * ((W.E + kTile - 1) / kTile);
    int64_t scan_n = hash_capacity(M);                              // the index's counts, the sort's histograms, M chunk counts
    if (n_hist > scan_n) scan_n = n_hist;
    if (M + 1 > scan_n) scan_n = M + 1;
    W.ix = take_index(c, M);
    W.vslot = c.take<int32_t>(M);
    W.scr = take_scan(c, scan_n);
    W.sig = c.take<double>(2 * ((N + 255) / 256) + 2);
    W.knn_bytes = c.o;
    W.w = c.take<float>(W.E);
    W.ka = c.take<int32_t>(W.E);
    W.va = c.take<int32_t>(W.E);
    W.kb = c.take<int32_t>(W.E);
    W.vb = c.take<int32_t>(W.E);
    W.sort = take_sort(c, W.E);
    W.offs = c.take<int32_t>(M + 1);
    W.nch = c.take<int32_t>(M);
    W.choff = c.take<int32_t>(M + 1);
    W.owner = c.take<int32_t>(W.q_cap);
    W.part = c.take<float>(W.q_cap * (D + 1));
    return W;
}

inline bool sizes_ok(int64_t M, int64_t N, int k, int D) {
    return M >= k && M < (1ll << 30) && N >= 0 && k >= 1 && k <= 16 && N * k < (1ll << 31) - kTile && D >= 0 && D <= 4096;
}

template <int KC>
void launch_knn(const Index& ix, int64_t M, const float* P, int64_t N, int k, float trunc, float h, float inv_h, int32_t* idx,
                float* dist, uint8_t* valid, hipStream_t s) {
    hipLaunchKernelGGL(knn_kernel<KC>, dim3(blocks(N, 256)), dim3(256), 0, s, ix, M, P, N, k, trunc, h, inv_h, idx, dist, valid);
}

}  // namespace

extern "C" int64_t misplat_meshmap_workspace(int64_t n_vertices, int64_t n_points, int32_t k, int32_t n_channels) {
    if (!sizes_ok(n_vertices, n_points, k, n_channels)) return -1;
    Carver c{nullptr};
    carve(c, n_vertices, n_points, k, n_channels);
    return c.o;
}

extern "C" int misplat_meshmap_knn(const float* vertices, int64_t n_vertices, const float* points, int64_t n_points, int32_t k,
                                   float sdf_trunc, void* workspace, int64_t workspace_bytes, int32_t* idx, float* dist,
                                   uint8_t* valid, misplat_stream_t stream) {
    const int64_t M = n_vertices, N = n_points;
    if (!sizes_ok(M, N, k, 0) || !(sdf_trunc > 0.f) || !(sdf_trunc < 3.0e37f) || !vertices || !workspace ||
        (N > 0 && (!points || !idx || !dist || !valid)))
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, M, N, k, 0);
    if (workspace_bytes < W.knn_bytes) return MISPLAT_EWORKSPACE;
    if (N == 0) return MISPLAT_OK;
    hipStream_t s = (hipStream_t)stream;
    const float h = sdf_trunc, inv_h = 1.f / sdf_trunc;
    const Index ix = build_index(vertices, M, nullptr, inv_h, W.ix, W.vslot, W.scr, s);
    if (k <= 4) launch_knn<4>(ix, M, points, N, k, sdf_trunc, h, inv_h, idx, dist, valid, s);
    else if (k <= 8) launch_knn<8>(ix, M, points, N, k, sdf_trunc, h, inv_h, idx, dist, valid, s);
    else launch_knn<16>(ix, M, points, N, k, sdf_trunc, h, inv_h, idx, dist, valid, s);
    return launched();
}

extern "C" int misplat_meshmap_aggregate(int64_t n_vertices, int64_t n_points, int32_t k, const int32_t* idx, const float* dist,
                                         const uint8_t* valid, const float* values, int32_t n_channels, int32_t n_unit,
                                         void* workspace, int64_t workspace_bytes, float* out, misplat_stream_t stream) {
    const int64_t M = n_vertices, N = n_points;
    const int D = n_channels;
    if (!sizes_ok(M, N, k, D) || D < 1 || !(n_unit == 0 || (n_unit == 3 && D >= 3)) || !workspace || !out ||
        (N > 0 && (!idx || !dist || !valid || !values)))
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, M, N, k, D);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        misplat_internal::fill_bytes(out, 4 * M * D, 0u, s);
        return launched();
    }
    const int64_t nb_sig = (N + 255) / 256;
    hipLaunchKernelGGL(sigma_partial_kernel, dim3((unsigned)nb_sig), dim3(256), 0, s, dist, valid, N, (int)k, W.sig + 2);
    hipLaunchKernelGGL((sum_final_kernel<2, 256>), dim3(1), dim3(256), 0, s, (const double*)(W.sig + 2), nb_sig, W.sig);
    int32_t *ka = W.ka, *va = W.va, *kb = W.kb, *vb = W.vb;
    hipLaunchKernelGGL(weights_kernel, dim3(blocks(N, 256)), dim3(256), 0, s, idx, dist, valid, N, (int)k, (int32_t)M,
                       (const double*)W.sig, W.w, ka, va);
    radix_sort(ka, va, kb, vb, W.E, radix_passes(M), W.sort, W.scr, s);       // (the keys are 0 .. M)
    hipLaunchKernelGGL(list_offsets_kernel, dim3(blocks(M + 1, 256)), dim3(256), 0, s, (const int32_t*)ka, W.E, (int32_t)M, W.offs);
    hipLaunchKernelGGL(chunk_count_kernel, dim3(blocks(M, 256)), dim3(256), 0, s, (const int32_t*)W.offs, (int32_t)M, W.nch);
    scan(W.nch, M, W.choff, W.scr, s);
    hipLaunchKernelGGL(chunk_owner_kernel, dim3(blocks(M, 256)), dim3(256), 0, s, (const int32_t*)W.choff, (int32_t)M, W.owner);
    hipLaunchKernelGGL(chunk_sum_kernel, dim3(blocks(W.q_cap * (D + 1), 256)), dim3(256), 0, s, (const int32_t*)W.owner,
                       (const int32_t*)W.choff, (const int32_t*)W.offs, (int32_t)M, (const int32_t*)va, (const float*)W.w, values, D,
                       (int)k, W.q_cap, W.part);
    hipLaunchKernelGGL(vertex_sum_kernel, dim3(blocks(M, 256)), dim3(256), 0, s, (const int32_t*)W.choff, (int32_t)M,
                       (const float*)W.part, D, (int)n_unit, out);
    return launched();
}
