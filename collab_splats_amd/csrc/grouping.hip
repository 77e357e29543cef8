// grouping.hip -- Gaga-style Gaussian grouping on the device: per view, the front fraction by depth of
// the Gaussians that project into every (mask, patch) cell; across views, a bank of Gaussian sets per label.
//
// Semantics (tests/grouping_restatement.py is the oracle; everything compared is an integer).
//   project: valid = any(radii > 1); pixel = rintf(mean) (half to even) clamped to the image, NaN -> 0; flat = x + y W.
//   cells:   mask index m = the rank of the pixel's id among the positive ids present in the mask image; patch (py, px) =
//            (min(y / ceil(H / P), P - 1), min(x / ceil(W / P), P - 1)); cell = (m P + py) P + px.  A pixel has one id and one
//            patch, so a Gaussian has at most one cell.
//   front:   in a cell of n valid Gaussians keep k = max((int64)((double)fp (double)n), 1) of them, the k smallest by
//            (depth, id): two stable radix sorts, by the depth's order-preserving bits and then by cell.
//   bank:    per Gaussian the ascending list of the labels it belongs to (CSR: off [N + 1], lab []).  count[m, l] = the
//            Gaussians selected for mask m that carry label l; q = float(count / (n_m + count + 1e-8)) with the quotient in
//            double; a mask takes the lowest label of maximal q, or the next new label (numbered in mask order) when q <
//            float(threshold), compared in fp32.
// Integer atomics only and plain vector stores: two runs are bitwise equal.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"
#include "internal.h"
#include "wgprims.h"
#include "radixsort.h"

namespace {

constexpr int kIds = 65536;           // mask ids 0 .. 65535; 0 is background
constexpr int kMaxPatches = 128;
constexpr int64_t kMaxPairs = 1ll << 26;   // M L of the overlap table

inline bool gauss_ok(int64_t N) { return N >= 1 && N < (1ll << 31); }
inline bool image_ok(int64_t W, int64_t H) { return W >= 1 && H >= 1 && W * H < (1ll << 31); }

// ----------------------------------------------------------------------------------------------------------- project
__global__ __launch_bounds__(256) void project_kernel(const int32_t* __restrict__ radii, const float* __restrict__ means2d,
                                                      int64_t N, int W, int H, int32_t* __restrict__ flat,
                                                      uint8_t* __restrict__ valid) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= N) return;
    const int2 r = ((const int2*)radii)[g];
    const float2 m = ((const float2*)means2d)[g];
    const float rx = rintf(m.x), ry = rintf(m.y);                   // round half to even
    const int x = !(rx > 0.f) ? 0 : (rx >= (float)(W - 1) ? W - 1 : (int)rx);       // (NaN: 0)
    const int y = !(ry > 0.f) ? 0 : (ry >= (float)(H - 1) ? H - 1 : (int)ry);
    flat[g] = x + y * W;
    valid[g] = (r.x > 1 || r.y > 1) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------- mask ids
// present[id] = 1 for every positive id of the image (every writer stores the same value)
__global__ __launch_bounds__(256) void presence_kernel(const int32_t* __restrict__ mask, int64_t n_pixels,
                                                       int32_t* __restrict__ present) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_pixels; p += stride) {
        const int32_t id = mask[p];
        if (id > 0 && id < kIds && present[id] == 0) present[id] = 1;
    }
}

// rank[id] = the number of present ids below id (the exclusive scan of present); rank[kIds] = M
__global__ __launch_bounds__(256) void mask_ids_kernel(const int32_t* __restrict__ present, const int32_t* __restrict__ rank,
                                                       int32_t* __restrict__ mask_ids, int32_t* __restrict__ n_masks) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id < kIds && present[id]) mask_ids[rank[id]] = id;
    if (id == 0) n_masks[0] = rank[kIds];
}

// ------------------------------------------------------------------------------------------------------------- front
__device__ __forceinline__ int32_t depth_key(float d) {
    const uint32_t b = __float_as_uint(d);
    return (int32_t)((b >> 31) ? ~b : (b | 0x80000000u));
}

__global__ __launch_bounds__(256) void depth_keys_kernel(const float* __restrict__ depths, int64_t N, int32_t* __restrict__ keys,
                                                         int32_t* __restrict__ vals, int32_t* __restrict__ mask_of) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= N) return;
    keys[g] = depth_key(depths[g]);
    vals[g] = (int32_t)g;
    mask_of[g] = -1;
}

// the cell of the Gaussian at every position of the depth order; `none` (one past the last cell) for a Gaussian that is
// invalid or lands on background
__global__ __launch_bounds__(256) void cell_keys_kernel(const int32_t* __restrict__ order, int64_t N, const int32_t* __restrict__ flat,
                                                        const uint8_t* __restrict__ valid, const int32_t* __restrict__ mask,
                                                        const int32_t* __restrict__ rank, int W, int32_t n_pixels, int pw, int ph,
                                                        int P, int32_t none, int32_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int32_t g = order[i];
    int32_t cell = none;
    if (valid[g]) {
        const int32_t p = flat[g];
        const int32_t id = (p >= 0 && p < n_pixels) ? mask[p] : 0;
        if (id > 0 && id < kIds) {
            const int x = p % W, y = p / W;
            const int px = min(x / pw, P - 1), py = min(y / ph, P - 1);
            cell = (rank[id] * P + py) * P + px;
        }
    }
    keys[i] = cell;
}

// keys ascending by cell, inside a cell by (depth, id).  Every element finds its cell's extent by two binary searches.
__global__ __launch_bounds__(256) void select_kernel(const int32_t* __restrict__ keys, const int32_t* __restrict__ order, int64_t N,
                                                     int32_t none, int PP, double fp, int32_t* __restrict__ mask_of,
                                                     int32_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int32_t c = keys[i];
    if (c >= none) return;
    int64_t lo = 0, hi = i;                                         // the first position with keys >= c
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < c) lo = mid + 1; else hi = mid;
    }
    const int64_t start = lo;
    lo = i + 1; hi = N;                                             // the first position with keys > c
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] <= c) lo = mid + 1; else hi = mid;
    }
    const int64_t n = lo - start;
    int64_t k = (int64_t)(fp * (double)n);
    if (k < 1) k = 1;
    if (i - start < k) {
        const int32_t m = c / PP;
        mask_of[order[i]] = m;
        atomicAdd(&counts[m], 1);
    }
}

__global__ __launch_bounds__(256) void fill_i32_kernel(int32_t* __restrict__ dst, int64_t n, int32_t v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = v;
}

__global__ __launch_bounds__(256) void relabel_kernel(const int32_t* __restrict__ mask, int64_t n_pixels,
                                                      const int32_t* __restrict__ rank, const int64_t* __restrict__ labels,
                                                      int32_t* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pixels) return;
    const int32_t id = mask[p];
    out[p] = (id > 0 && id < kIds) ? (int32_t)labels[rank[id]] + 1 : 0;
}

// -------------------------------------------------------------------------------------------------------------- bank
__global__ __launch_bounds__(256) void overlap_kernel(const int32_t* __restrict__ mask_of, int64_t N, const int32_t* __restrict__ off,
                                                      const int32_t* __restrict__ lab, int M, int L, int32_t* __restrict__ count) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= N) return;
    const int32_t m = mask_of[g];
    if (m < 0 || m >= M) return;
    const int32_t e1 = off[g + 1];
    for (int32_t e = off[g]; e < e1; e++) {
        const int32_t l = lab[e];
        if (l >= 0 && l < L) atomicAdd(&count[(int64_t)m * L + l], 1);
    }
}

// One workgroup.  Mask after mask: the lowest label of maximal q; new labels are numbered in mask order.
__global__ __launch_bounds__(256) void assign_kernel(const int32_t* __restrict__ count, const int32_t* __restrict__ set_sizes, int M,
                                                     int L, float threshold, int64_t* __restrict__ labels,
                                                     int32_t* __restrict__ n_new) {
    __shared__ float sq[256];
    __shared__ int32_t sl[256];
    int32_t next = L;                                               // (thread 0's copy is the one that counts)
    for (int m = 0; m < M; m++) {
        if (L == 0) {                                               // the first view: labels = arange(M)
            if (threadIdx.x == 0) labels[m] = m;
            continue;
        }
        const double n = (double)set_sizes[m];
        float best = -1.f;
        int32_t best_l = 0x7fffffff;
        for (int l = threadIdx.x; l < L; l += 256) {
            const double inter = (double)count[(int64_t)m * L + l];
            const float q = (float)(inter / (n + inter + 1e-8));
            if (q > best) { best = q; best_l = l; }                 // ascending l: a later equal does not replace
        }
        sq[threadIdx.x] = best;
        sl[threadIdx.x] = best_l;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) {
                const float q = sq[threadIdx.x + s];
                const int32_t l = sl[threadIdx.x + s];
                if (q > sq[threadIdx.x] || (q == sq[threadIdx.x] && l < sl[threadIdx.x])) { sq[threadIdx.x] = q; sl[threadIdx.x] = l; }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) labels[m] = (sq[0] < threshold) ? next++ : sl[0];
        __syncthreads();
    }
    if (threadIdx.x == 0) n_new[0] = (L == 0) ? M : next - L;
}

// position of `label` in the ascending list lab[e0 .. e1): found, or where it would go
__device__ __forceinline__ int32_t list_find(const int32_t* __restrict__ lab, int32_t e0, int32_t e1, int32_t label, bool& found) {
    int32_t lo = e0, hi = e1;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (lab[mid] < label) lo = mid + 1; else hi = mid;
    }
    found = lo < e1 && lab[lo] == label;
    return lo;
}

__device__ __forceinline__ int32_t new_label(const int32_t* __restrict__ mask_of, const int64_t* __restrict__ labels, int M,
                                             int64_t g) {
    const int32_t m = mask_of[g];
    return (m < 0 || m >= M) ? -1 : (int32_t)labels[m];
}

__global__ __launch_bounds__(256) void merge_count_kernel(const int32_t* __restrict__ mask_of, int64_t N,
                                                          const int64_t* __restrict__ labels, int M, const int32_t* __restrict__ off,
                                                          const int32_t* __restrict__ lab, int32_t* __restrict__ cnt) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= N) return;
    const int32_t e0 = off[g], e1 = off[g + 1];
    const int32_t label = new_label(mask_of, labels, M, g);
    bool found = true;
    if (label >= 0) (void)list_find(lab, e0, e1, label, found);
    cnt[g] = (e1 - e0) + (found ? 0 : 1);
}

__global__ __launch_bounds__(256) void merge_copy_kernel(const int32_t* __restrict__ mask_of, int64_t N,
                                                         const int64_t* __restrict__ labels, int M, const int32_t* __restrict__ off,
                                                         const int32_t* __restrict__ lab, const int32_t* __restrict__ new_off,
                                                         int64_t new_cap, int32_t* __restrict__ new_lab, int32_t* __restrict__ sizes,
                                                         int L_new) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= N) return;
    const int32_t e0 = off[g], e1 = off[g + 1];
    const int32_t o0 = new_off[g], o1 = new_off[g + 1];
    if (o0 < 0 || o1 < o0 || (int64_t)o1 > new_cap || o1 - o0 < e1 - e0) return;      // (an inconsistent caller: write nothing)
    const int32_t label = new_label(mask_of, labels, M, g);
    bool found = true;
    int32_t at = e1;
    if (label >= 0) at = list_find(lab, e0, e1, label, found);
    const bool add = !found && o1 - o0 == e1 - e0 + 1;
    for (int32_t e = e0; e < e1; e++) new_lab[o0 + (e - e0) + ((add && e >= at) ? 1 : 0)] = lab[e];
    if (add) {
        new_lab[o0 + (at - e0)] = label;
        if (label < L_new) atomicAdd(&sizes[label], 1);
    }
}

__global__ __launch_bounds__(256) void members_kernel(const int32_t* __restrict__ off, const int32_t* __restrict__ lab, int64_t N,
                                                      int32_t label, uint8_t* __restrict__ flags) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= N) return;
    bool found;
    (void)list_find(lab, off[g], off[g + 1], label, found);
    flags[g] = found ? 1 : 0;
}

// --------------------------------------------------------------------------------------------------------- workspace
// the mask table (present, rank) and the scan's scratch come first: they are what misplat_grouping_mask_ids leaves for
// _front and _relabel.  _mask_ids and _relabel carve for N = 1 and ask for `table_bytes`: the table sits at the same offsets for every N,
// and the scan of kIds flags needs no more scratch than N = 1 gives
struct Work {
    int32_t *present, *rank, *scr;
    int64_t table_bytes;
    int32_t *ka, *va, *kb, *vb;
    SortBufs sort;
};

inline Work carve(Carver& c, int64_t N) {
    Work W;
    const int64_t n_hist = 256 * ((N + kTile - 1) / kTile);
    int64_t scan_n = N;                                             // the bank's merge scans N counts
    if (n_hist > scan_n) scan_n = n_hist;
    if (kIds > scan_n) scan_n = kIds;
    W.present = c.take<int32_t>(kIds);
    W.rank = c.take<int32_t>(kIds + 1);
    W.scr = take_scan(c, scan_n);
    W.table_bytes = c.o;
    W.ka = c.take<int32_t>(N);
    W.va = c.take<int32_t>(N);
    W.kb = c.take<int32_t>(N);
    W.vb = c.take<int32_t>(N);
    W.sort = take_sort(c, N);
    return W;
}

}  // namespace

extern "C" int64_t misplat_grouping_workspace(int64_t n_gauss) {
    if (!gauss_ok(n_gauss)) return -1;
    Carver c{nullptr};
    carve(c, n_gauss);
    return c.o;
}

extern "C" int misplat_grouping_project(const int32_t* radii, const float* means2d, int64_t n_gauss, int32_t width, int32_t height,
                                        int32_t* flat, uint8_t* valid, misplat_stream_t stream) {
    if (!gauss_ok(n_gauss) || !image_ok(width, height) || !radii || !means2d || !flat || !valid) return MISPLAT_EINVAL;
    hipLaunchKernelGGL(project_kernel, dim3(blocks(n_gauss, 256)), dim3(256), 0, (hipStream_t)stream, radii, means2d, n_gauss,
                       (int)width, (int)height, flat, valid);
    return launched();
}

extern "C" int misplat_grouping_mask_ids(const int32_t* mask, int64_t n_pixels, void* workspace, int64_t workspace_bytes,
                                         int32_t* mask_ids, int32_t* n_masks, misplat_stream_t stream) {
    if (n_pixels < 1 || n_pixels >= (1ll << 31) || !mask || !workspace || !mask_ids || !n_masks) return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, 1);
    if (workspace_bytes < W.table_bytes) return MISPLAT_EWORKSPACE;  // the table and the scan's scratch: what every N has
    hipStream_t s = (hipStream_t)stream;
    misplat_internal::fill_bytes(W.present, 4 * kIds, 0u, s);
    unsigned nb = blocks(n_pixels, 256);
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(presence_kernel, dim3(nb), dim3(256), 0, s, mask, n_pixels, W.present);
    scan(W.present, kIds, W.rank, W.scr, s);
    hipLaunchKernelGGL(mask_ids_kernel, dim3(kIds / 256), dim3(256), 0, s, (const int32_t*)W.present, (const int32_t*)W.rank,
                       mask_ids, n_masks);
    return launched();
}

extern "C" int misplat_grouping_front(const int32_t* flat, const uint8_t* valid, const float* depths, int64_t n_gauss,
                                      const int32_t* mask, int32_t width, int32_t height, int32_t num_patches, int32_t n_masks,
                                      double front_percentage, void* workspace, int64_t workspace_bytes, int32_t* mask_of,
                                      int32_t* counts, misplat_stream_t stream) {
    const int64_t N = n_gauss;
    const int P = num_patches, M = n_masks;
    if (!gauss_ok(N) || !image_ok(width, height) || P < 1 || P > kMaxPatches || M < 0 || M >= kIds ||
        !(front_percentage > 0.0) || !(front_percentage <= 1.0) || !flat || !valid || !depths || !mask || !workspace || !mask_of ||
        (M > 0 && !counts))
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, N);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const unsigned nb = blocks(N, 256);
    if (M == 0) {
        hipLaunchKernelGGL(fill_i32_kernel, dim3(nb), dim3(256), 0, s, mask_of, N, -1);
        return launched();
    }
    int32_t *ka = W.ka, *va = W.va, *kb = W.kb, *vb = W.vb;
    misplat_internal::fill_bytes(counts, 4 * (size_t)M, 0u, s);
    hipLaunchKernelGGL(depth_keys_kernel, dim3(nb), dim3(256), 0, s, depths, N, ka, va, mask_of);
    radix_sort(ka, va, kb, vb, N, 4, W.sort, W.scr, s);             // (the depth's bits: all 32)
    const int32_t none = M * P * P;                                 // 1 <= none < 2^30: 1 <= M < 2^16, 1 <= P <= 2^7
    const int pw = (width + P - 1) / P, ph = (height + P - 1) / P;
    hipLaunchKernelGGL(cell_keys_kernel, dim3(nb), dim3(256), 0, s, (const int32_t*)va, N, flat, valid, mask, (const int32_t*)W.rank,
                       (int)width, (int32_t)(width * height), pw, ph, P, none, ka);
    // the keys are 0 .. none.  none >= 1 here (M == 0 has returned above, P >= 1 is checked), so at least one pass runs
    radix_sort(ka, va, kb, vb, N, radix_passes(none), W.sort, W.scr, s);
    hipLaunchKernelGGL(select_kernel, dim3(nb), dim3(256), 0, s, (const int32_t*)ka, (const int32_t*)va, N, none, P * P, front_percentage,
                       mask_of, counts);
    return launched();
}

extern "C" int misplat_grouping_relabel(const int32_t* mask, int64_t n_pixels, const void* workspace, int64_t workspace_bytes,
                                        const int64_t* labels, int32_t* out, misplat_stream_t stream) {
    if (n_pixels < 1 || n_pixels >= (1ll << 31) || !mask || !workspace || !labels || !out) return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, 1);
    if (workspace_bytes < W.table_bytes) return MISPLAT_EWORKSPACE;
    hipLaunchKernelGGL(relabel_kernel, dim3(blocks(n_pixels, 256)), dim3(256), 0, (hipStream_t)stream, mask, n_pixels,
                       (const int32_t*)W.rank, labels, out);
    return launched();
}

extern "C" int misplat_grouping_overlap(const int32_t* mask_of, int64_t n_gauss, const int32_t* bank_off, const int32_t* bank_labels,
                                        int32_t n_masks, int32_t n_labels, int32_t* count, misplat_stream_t stream) {
    const int64_t ML = (int64_t)n_masks * n_labels;
    if (!gauss_ok(n_gauss) || n_masks < 1 || n_labels < 1 || ML > kMaxPairs || !mask_of || !bank_off || !bank_labels || !count)
        return MISPLAT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    misplat_internal::fill_bytes(count, 4 * (size_t)ML, 0u, s);
    hipLaunchKernelGGL(overlap_kernel, dim3(blocks(n_gauss, 256)), dim3(256), 0, s, mask_of, n_gauss, bank_off, bank_labels,
                       (int)n_masks, (int)n_labels, count);
    return launched();
}

extern "C" int misplat_grouping_assign(const int32_t* count, const int32_t* set_sizes, int32_t n_masks, int32_t n_labels,
                                       float iou_threshold, int64_t* labels, int32_t* n_new, misplat_stream_t stream) {
    if (n_masks < 0 || n_labels < 0 || (int64_t)n_masks * n_labels > kMaxPairs || (n_masks > 0 && n_labels > 0 && (!count || !set_sizes)) ||
        (n_masks > 0 && !labels) || !n_new)
        return MISPLAT_EINVAL;
    hipLaunchKernelGGL(assign_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, count, set_sizes, (int)n_masks, (int)n_labels,
                       iou_threshold, labels, n_new);
    return launched();
}

extern "C" int misplat_grouping_merge_count(const int32_t* mask_of, int64_t n_gauss, const int64_t* labels, int32_t n_masks,
                                            const int32_t* bank_off, const int32_t* bank_labels, void* workspace,
                                            int64_t workspace_bytes, int32_t* new_off, misplat_stream_t stream) {
    const int64_t N = n_gauss;
    if (!gauss_ok(N) || n_masks < 1 || !mask_of || !labels || !bank_off || !bank_labels || !workspace || !new_off) return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, N);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(merge_count_kernel, dim3(blocks(N, 256)), dim3(256), 0, s, mask_of, N, labels, (int)n_masks, bank_off, bank_labels,
                       W.ka);                                        // (the counts borrow the sort's first key buffer)
    scan(W.ka, N, new_off, W.scr, s);
    return launched();
}

extern "C" int misplat_grouping_merge_copy(const int32_t* mask_of, int64_t n_gauss, const int64_t* labels, int32_t n_masks,
                                           const int32_t* bank_off, const int32_t* bank_labels, const int32_t* new_off,
                                           int64_t new_capacity, int32_t* new_labels, int32_t* sizes, int32_t n_labels_new,
                                           misplat_stream_t stream) {
    if (!gauss_ok(n_gauss) || n_masks < 1 || new_capacity < 0 || n_labels_new < 1 || !mask_of || !labels || !bank_off || !bank_labels ||
        !new_off || (new_capacity > 0 && !new_labels) || !sizes)
        return MISPLAT_EINVAL;
    hipLaunchKernelGGL(merge_copy_kernel, dim3(blocks(n_gauss, 256)), dim3(256), 0, (hipStream_t)stream, mask_of, n_gauss, labels,
                       (int)n_masks, bank_off, bank_labels, new_off, new_capacity, new_labels, sizes, (int)n_labels_new);
    return launched();
}

extern "C" int misplat_grouping_members(const int32_t* bank_off, const int32_t* bank_labels, int64_t n_gauss, int32_t label,
                                        uint8_t* flags, misplat_stream_t stream) {
    if (!gauss_ok(n_gauss) || label < 0 || !bank_off || !bank_labels || !flags) return MISPLAT_EINVAL;
    hipLaunchKernelGGL(members_kernel, dim3(blocks(n_gauss, 256)), dim3(256), 0, (hipStream_t)stream, bank_off, bank_labels, n_gauss,
                       label, flags);
    return launched();
}
