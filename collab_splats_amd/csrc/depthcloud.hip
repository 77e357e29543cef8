// depthcloud.hip -- oriented point clouds from depth and normal maps: the depth-edge filter (inverse
// depth Laplacian, box dilation on a bit image), the candidate mask, a seeded uniform sample of S candidate pixels per frame
// (radix select of a hashed key), the back-projection of the sampled pixels with their normals and colours, and the mask
// filter of Gaussian centres.
//
// Semantics: tests/depthcloud_restatement.py is the oracle.  Compiled with -ffp-contract=off: every fp32 expression is
// evaluated in the written order.  Integer atomics only; two runs are bitwise equal.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"
#include "internal.h"
#include "wgprims.h"
#include "hashmix.h"

namespace {

// ------------------------------------------------------------------------------------------------------------ edges
// inv = 1 / (d + 1e-6) inside the image, 0 outside (the reference pads the inverse-depth image with zeros)
__device__ __forceinline__ float inv_depth(const float* __restrict__ D, int W, int H, int x, int y) {
    if (x < 0 || x >= W || y < 0 || y >= H) return 0.f;
    return 1.0f / (D[(int64_t)y * W + x] + 1e-6f);
}

// One lane per pixel, one wave per 64 pixels of a row: bit (x & 63) of bits[(v H + y) Wd + x / 64] = lap > threshold,
// lap = ((up + left) + (right + down)) - 4 inv.  Bits at x >= W are 0.
__global__ __launch_bounds__(256) void edge_bits_kernel(const float* __restrict__ depth, int64_t n_words, int H, int W, int Wd,
                                                        float threshold, unsigned long long* __restrict__ bits) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t word = gid >> 6;
    if (word >= n_words) return;                                     // (the whole wave leaves)
    const int lane = threadIdx.x & 63;
    const int wx = (int)(word % Wd);
    const int64_t row = word / Wd;
    const int y = (int)(row % H);
    const float* D = depth + (row / H) * ((int64_t)H * W);
    const int x = wx * 64 + lane;
    bool edge = false;
    if (x < W) {
        const float c = inv_depth(D, W, H, x, y);
        const float up = inv_depth(D, W, H, x, y - 1), left = inv_depth(D, W, H, x - 1, y);
        const float right = inv_depth(D, W, H, x + 1, y), down = inv_depth(D, W, H, x, y + 1);
        const float lap = ((up + left) + (right + down)) - 4.0f * c;
        edge = lap > threshold;
    }
    const unsigned long long b = __ballot(edge);
    if (lane == 0) bits[word] = b;
}

// The middle word of (L, C, R) dilated by r pixels to either side, 0 <= r <= 63: shifts and ORs that double the reach
// (after a step the word holds the OR of the shifts 0 .. a; the next step ORs in that shifted by s <= a + 1).
__device__ __forceinline__ unsigned long long dilate_row(unsigned long long L, unsigned long long C, unsigned long long R, int r) {
    unsigned long long up = C, lo = L, down = C, hi = R;           // up: towards larger x (left shifts), down: smaller x
    for (int a = 0; a < r;) {
        const int s = (a + 1 < r - a) ? a + 1 : r - a;
        up |= (up << s) | (lo >> (64 - s));
        lo |= lo << s;
        down |= (down >> s) | (hi << (64 - s));
        hi |= hi >> s;
        a += s;
    }
    return up | down;
}

// One wave per output word: lane l takes the rows y - r + l and y - r + l + 64 (2 r + 1 <= 127 rows), dilates each along
// the row, the wave ORs them together, and lane l writes pixel 64 wx + l.
__global__ __launch_bounds__(256) void edge_dilate_kernel(const unsigned long long* __restrict__ bits, int64_t n_words, int H, int W,
                                                          int Wd, int r, uint8_t* __restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t word = gid >> 6;
    if (word >= n_words) return;
    const int lane = threadIdx.x & 63;
    const int wx = (int)(word % Wd);
    const int64_t row = word / Wd;
    const int y = (int)(row % H);
    const unsigned long long* B = bits + (row - y) * Wd;            // the frame's first row
    unsigned long long acc = 0ull;
    for (int l = lane; l <= 2 * r; l += 64) {
        const int yy = y - r + l;
        if (yy < 0 || yy >= H) continue;
        const unsigned long long* rowp = B + (int64_t)yy * Wd;
        acc |= dilate_row(wx > 0 ? rowp[wx - 1] : 0ull, rowp[wx], wx + 1 < Wd ? rowp[wx + 1] : 0ull, r);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc |= __shfl_xor(acc, off);
    const int x = wx * 64 + lane;
    if (x < W) out[row * W + x] = (uint8_t)((acc >> lane) & 1ull);
}

// candidate iff depth > 0 and mask and valid and not edge (each of the three optional)
__global__ __launch_bounds__(256) void candidate_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ mask,
                                                        const uint8_t* __restrict__ valid, const uint8_t* __restrict__ edges,
                                                        int64_t n, uint8_t* __restrict__ cand) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool c = depth[i] > 0.f;
    if (mask) c = c && mask[i] != 0;
    if (valid) c = c && valid[i] != 0;
    if (edges) c = c && edges[i] == 0;
    cand[i] = c ? 1 : 0;
}

// --------------------------------------------------------------------------------------------------------- sampling
// A frame keeps the min(S, n) candidates with the smallest (key, pixel).  The pivot key T (the S-th smallest) comes from a
// radix select, 8 bits a pass: a histogram of the next digit over the candidates that match the prefix so far, then the
// digit in which the running count reaches k.  After four passes: every key < T is taken, and of the keys == T the first
// `k` in pixel order.  All frames of the call go through each launch (blockIdx.y = frame).
constexpr int kChunk = 2048;          // pixels per workgroup (8 per thread)

struct FrameState {
    uint32_t prefix;                  // the known high digits of T
    int32_t k;                        // how many of the keys that match the prefix are still to be taken
    int32_t take_all;                 // n <= S: every candidate is taken
    int32_t n;                        // candidates of the frame
};

__device__ __forceinline__ uint32_t key_of(const int32_t* __restrict__ keys, uint32_t seed, uint32_t frame, int64_t at, uint32_t pix) {
    return keys ? (uint32_t)keys[at] : mix32(seed, frame, pix);
}

__global__ __launch_bounds__(256) void key_hist_kernel(const uint8_t* __restrict__ cand, const int32_t* __restrict__ keys, int64_t P,
                                                       uint32_t seed, uint32_t frame_offset, int pass,
                                                       const FrameState* __restrict__ state, int32_t* __restrict__ hist) {
    __shared__ int32_t h[256];
    const int v = blockIdx.y;
    const FrameState st = state[v];
    if (pass > 0 && st.take_all) return;
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)v * P;
    const int64_t start = (int64_t)blockIdx.x * kChunk;
    for (int it = 0; it < kChunk / 256; it++) {
        const int64_t pix = start + it * 256 + threadIdx.x;
        if (pix < P && cand[base + pix]) {
            const uint32_t key = key_of(keys, seed, frame_offset + (uint32_t)v, base + pix, (uint32_t)pix);
            if (pass == 0 || (key >> (32 - 8 * pass)) == st.prefix) atomicAdd(&h[(key >> (24 - 8 * pass)) & 255u], 1);
        }
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[((int64_t)v * 4 + pass) * 256 + threadIdx.x], h[threadIdx.x]);
}

// One workgroup per frame: the digit d whose inclusive count first reaches k; pass 0 also settles n, take_all and counts.
__global__ __launch_bounds__(256) void key_pick_kernel(int pass, int32_t S, FrameState* __restrict__ state,
                                                       const int32_t* __restrict__ hist, int32_t* __restrict__ counts) {
    __shared__ int32_t wsum[4];
    const int v = blockIdx.x;
    const FrameState st = state[v];
    if (pass > 0 && st.take_all) return;
    const int32_t c = hist[((int64_t)v * 4 + pass) * 256 + threadIdx.x];
    int32_t total;
    const int32_t incl = block_scan_excl<int32_t, 4>(c, wsum, total) + c;
    int32_t k = st.k, n = st.n;
    if (pass == 0) {
        n = total;
        if (n <= S) {
            if (threadIdx.x == 0) { state[v] = FrameState{0u, 0, 1, n}; counts[v] = n; }
            return;
        }
        k = S;
        if (threadIdx.x == 0) counts[v] = S;
    }
    if (incl >= k && incl - c < k) state[v] = FrameState{(pass == 0 ? 0u : st.prefix << 8) | (uint32_t)threadIdx.x, k - (incl - c), 0, n};
}

// less: taken whatever its rank; equal: taken iff fewer than st.k equal keys precede it in the frame
__device__ __forceinline__ void classify(const uint8_t* __restrict__ cand, const int32_t* __restrict__ keys, int64_t P, uint32_t seed,
                                         uint32_t frame, int64_t base, int64_t pix, const FrameState& st, bool& less, bool& equal) {
    less = equal = false;
    if (pix >= P || !cand[base + pix]) return;
    if (st.take_all) { less = true; return; }
    const uint32_t key = key_of(keys, seed, frame, base + pix, (uint32_t)pix);
    less = key < st.prefix;
    equal = key == st.prefix;
}

// part[(0 V + v) nb + b] / part[(1 V + v) nb + b] = the less / equal pixels of chunk b of frame v
__global__ __launch_bounds__(256) void select_count_kernel(const uint8_t* __restrict__ cand, const int32_t* __restrict__ keys, int64_t P,
                                                           uint32_t seed, uint32_t frame_offset, const FrameState* __restrict__ state,
                                                           int32_t* __restrict__ part) {
    __shared__ int32_t wl[4], we[4];
    const int v = blockIdx.y, V = gridDim.y, nb = gridDim.x;
    const FrameState st = state[v];
    const int64_t base = (int64_t)v * P, start = (int64_t)blockIdx.x * kChunk;
    int32_t nl = 0, ne = 0;
    for (int it = 0; it < kChunk / 256; it++) {
        bool less, equal;
        classify(cand, keys, P, seed, frame_offset + (uint32_t)v, base, start + it * 256 + threadIdx.x, st, less, equal);
        nl += __popcll(__ballot(less));
        ne += __popcll(__ballot(equal));
    }
    if ((threadIdx.x & 63) == 0) { wl[threadIdx.x >> 6] = nl; we[threadIdx.x >> 6] = ne; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[((int64_t)v) * nb + blockIdx.x] = (wl[0] + wl[1]) + (wl[2] + wl[3]);
        part[((int64_t)V + v) * nb + blockIdx.x] = (we[0] + we[1]) + (we[2] + we[3]);
    }
}

// A taken pixel lands at frame_base[v] + (less before it) + min(equal before it, k): frames in order, pixels ascending.
__global__ __launch_bounds__(256) void select_emit_kernel(const uint8_t* __restrict__ cand, const int32_t* __restrict__ keys, int64_t P,
                                                          uint32_t seed, uint32_t frame_offset, const FrameState* __restrict__ state,
                                                          const int32_t* __restrict__ offs, const int32_t* __restrict__ frame_base,
                                                          int32_t* __restrict__ frame_ids, int32_t* __restrict__ pixel_ids) {
    __shared__ int32_t wl[4], we[4];
    const int v = blockIdx.y, V = gridDim.y, nb = gridDim.x;
    const FrameState st = state[v];
    const int64_t base = (int64_t)v * P, start = (int64_t)blockIdx.x * kChunk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int32_t nl = offs[(int64_t)v * nb + blockIdx.x], ne = offs[((int64_t)V + v) * nb + blockIdx.x];
    const int64_t out0 = frame_base[v];
    for (int it = 0; it < kChunk / 256; it++) {
        const int64_t pix = start + it * 256 + threadIdx.x;
        bool less, equal;
        classify(cand, keys, P, seed, frame_offset + (uint32_t)v, base, pix, st, less, equal);
        const unsigned long long bl = __ballot(less), be = __ballot(equal);
        __syncthreads();                                            // (the previous round's reads of wl / we are done)
        if (lane == 0) { wl[wave] = __popcll(bl); we[wave] = __popcll(be); }
        __syncthreads();
        int32_t pl = nl + __popcll(bl & below), pe = ne + __popcll(be & below);
#pragma unroll
        for (int w = 0; w < 4; w++) {
            pl += (w < wave) ? wl[w] : 0;
            pe += (w < wave) ? we[w] : 0;
            nl += wl[w];
            ne += we[w];
        }
        if (less || (equal && pe < st.k)) {
            const int64_t pos = out0 + pl + (pe < st.k ? pe : st.k);
            frame_ids[pos] = v;
            pixel_ids[pos] = (int32_t)pix;
        }
    }
}

// --------------------------------------------------------------------------------------------------- back-projection
struct Pose { float r[3][3], t[3]; };

// R = c2w[:3,:3] diag(1, -1, -1) (nerfstudio's OpenGL pose to the OpenCV camera the depth is measured in), t = c2w[:3,3]
__device__ __forceinline__ Pose load_pose(const float* __restrict__ c2w) {
    Pose p;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        p.r[i][0] = c2w[4 * i];
        p.r[i][1] = -c2w[4 * i + 1];
        p.r[i][2] = -c2w[4 * i + 2];
        p.t[i] = c2w[4 * i + 3];
    }
    return p;
}

// x = ((u + 0.5) - cx) d / fx, y likewise, p = ((R0 x + R1 y) + R2 d) + t; n = 2 m - 1, y and z flipped, divided by
// max(sqrt((nx nx + ny ny) + nz nz), 1e-12), rotated by R; colours gathered.
__global__ __launch_bounds__(256) void backproject_kernel(const float* __restrict__ depth, const float* __restrict__ rgb,
                                                          const float* __restrict__ normals, const float* __restrict__ c2w,
                                                          const float* __restrict__ intr, int64_t P, int W,
                                                          const int32_t* __restrict__ frame_ids, const int32_t* __restrict__ pixel_ids,
                                                          int64_t n, float* __restrict__ points, float* __restrict__ out_normals,
                                                          float* __restrict__ colors) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int v = frame_ids[i], pix = pixel_ids[i];
    const int64_t at = (int64_t)v * P + pix;
    const Pose q = load_pose(c2w + 12 * (int64_t)v);
    const float fx = intr[4 * v], fy = intr[4 * v + 1], cx = intr[4 * v + 2], cy = intr[4 * v + 3];
    const float d = depth[at];
    const float x = (((float)(pix % W) + 0.5f) - cx) * d / fx;
    const float y = (((float)(pix / W) + 0.5f) - cy) * d / fy;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        points[3 * i + a] = ((q.r[a][0] * x + q.r[a][1] * y) + q.r[a][2] * d) + q.t[a];
        colors[3 * i + a] = rgb[3 * at + a];
    }
    if (normals) {
        float nx = 2.0f * normals[3 * at] - 1.0f, ny = -(2.0f * normals[3 * at + 1] - 1.0f), nz = -(2.0f * normals[3 * at + 2] - 1.0f);
        const float len = fmaxf(sqrtf((nx * nx + ny * ny) + nz * nz), 1e-12f);
        nx = nx / len; ny = ny / len; nz = nz / len;
#pragma unroll
        for (int a = 0; a < 3; a++) out_normals[3 * i + a] = (q.r[a][0] * nx + q.r[a][1] * ny) + q.r[a][2] * nz;
    }
}

// ---------------------------------------------------------------------------------------------- Gaussian mask filter
// keep[g] = no view drops g.  Per view: c = (p - t) @ R in the order (d0 R0j + d1 R1j) + d2 R2j; a centre with z <= 0 is not
// tested; u = x fx / z + cx, iu = floor(u - 0.5) (v likewise); dropped iff 0 < iu < W, 0 < iv < H and the mask is 0 there.
__global__ __launch_bounds__(256) void gaussian_filter_kernel(const float* __restrict__ means, int64_t N, const float* __restrict__ c2w,
                                                              const float* __restrict__ intr, const uint8_t* __restrict__ masks, int V,
                                                              int H, int W, uint8_t* __restrict__ keep) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= N) return;
    const float px = means[3 * g], py = means[3 * g + 1], pz = means[3 * g + 2];
    bool kept = true;
    for (int v = 0; v < V && kept; v++) {
        const Pose q = load_pose(c2w + 12 * (int64_t)v);
        const float d0 = px - q.t[0], d1 = py - q.t[1], d2 = pz - q.t[2];
        const float z = (d0 * q.r[0][2] + d1 * q.r[1][2]) + d2 * q.r[2][2];
        if (!(z > 0.f)) continue;
        const float x = (d0 * q.r[0][0] + d1 * q.r[1][0]) + d2 * q.r[2][0];
        const float y = (d0 * q.r[0][1] + d1 * q.r[1][1]) + d2 * q.r[2][1];
        const float iu = floorf((x * intr[4 * v] / z + intr[4 * v + 2]) - 0.5f);
        const float iv = floorf((y * intr[4 * v + 1] / z + intr[4 * v + 3]) - 0.5f);
        if (iu > 0.f && iu < (float)W && iv > 0.f && iv < (float)H)
            kept = masks[((int64_t)v * H + (int)iv) * W + (int)iu] != 0;
    }
    keep[g] = kept ? 1 : 0;
}

// -------------------------------------------------------------------------------------------------------- workspace
enum { kKindEdges = 0, kKindSample = 1 };

inline bool maps_ok(int64_t V, int64_t H, int64_t W) {
    return V >= 1 && V <= 65535 && H >= 1 && W >= 1 && H < (1ll << 31) / W && V * H * W < (1ll << 40);
}

struct SampleLayout { int64_t nb, o_hist, o_state, o_part, o_offs, total; };

inline SampleLayout sample_layout(int64_t V, int64_t P) {
    SampleLayout L;
    int64_t o = 0;
    L.nb = (P + kChunk - 1) / kChunk;
    L.o_hist = o;  o += al(4 * V * 4 * 256);
    L.o_state = o; o += al((int64_t)sizeof(FrameState) * V);
    L.o_part = o;  o += al(4 * 2 * V * L.nb);
    L.o_offs = o;  o += al(4 * 2 * V * L.nb);
    L.total = o;
    return L;
}

}  // namespace

extern "C" int64_t misplat_depthcloud_workspace(int64_t n_views, int64_t height, int64_t width, int32_t kind) {
    if (!maps_ok(n_views, height, width)) return -1;
    if (kind == kKindEdges) return al(8 * n_views * height * ((width + 63) / 64));
    if (kind == kKindSample) return sample_layout(n_views, height * width).total;
    return -1;
}

extern "C" int misplat_depthcloud_edges(const float* depth, int32_t n_views, int32_t height, int32_t width, float threshold,
                                        int32_t dilation, void* workspace, int64_t workspace_bytes, uint8_t* edges,
                                        misplat_stream_t stream) {
    if (!maps_ok(n_views, height, width) || dilation < 0 || dilation > 63 || !depth || !workspace || !edges) return MISPLAT_EINVAL;
    const int Wd = (width + 63) / 64;
    const int64_t n_words = (int64_t)n_views * height * Wd;
    if (n_words >= (1ll << 31)) return MISPLAT_EINVAL;
    if (workspace_bytes < al(8 * n_words)) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* bits = (unsigned long long*)workspace;
    hipLaunchKernelGGL(edge_bits_kernel, dim3(blocks(n_words, 4)), dim3(256), 0, s, depth, n_words, height, width, Wd, threshold, bits);
    hipLaunchKernelGGL(edge_dilate_kernel, dim3(blocks(n_words, 4)), dim3(256), 0, s, (const unsigned long long*)bits, n_words, height,
                       width, Wd, dilation, edges);
    return launched();
}

extern "C" int misplat_depthcloud_candidates(const float* depth, const uint8_t* masks, const uint8_t* valid, const uint8_t* edges,
                                             int64_t n_pixels, uint8_t* candidates, misplat_stream_t stream) {
    if (n_pixels < 1 || n_pixels >= (1ll << 40) || !depth || !candidates) return MISPLAT_EINVAL;
    hipLaunchKernelGGL(candidate_kernel, dim3(blocks(n_pixels, 256)), dim3(256), 0, (hipStream_t)stream, depth, masks, valid, edges,
                       n_pixels, candidates);
    return launched();
}

extern "C" int misplat_depthcloud_sample(const uint8_t* candidates, const int32_t* keys, int32_t n_views, int32_t height, int32_t width,
                                         int32_t samples_per_frame, uint32_t seed, uint32_t frame_offset, void* workspace,
                                         int64_t workspace_bytes, int32_t* frame_ids, int32_t* pixel_ids, int32_t* counts,
                                         int32_t* frame_base, misplat_stream_t stream) {
    if (!maps_ok(n_views, height, width) || samples_per_frame < 1 || !candidates || !workspace || !frame_ids || !pixel_ids || !counts ||
        !frame_base)
        return MISPLAT_EINVAL;
    const int64_t V = n_views, P = (int64_t)height * width;
    const int64_t most = samples_per_frame < P ? samples_per_frame : P;
    if (V * most >= (1ll << 31)) return MISPLAT_EINVAL;
    const SampleLayout L = sample_layout(V, P);
    if (workspace_bytes < L.total) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int32_t* hist = (int32_t*)(ws + L.o_hist);
    FrameState* state = (FrameState*)(ws + L.o_state);
    int32_t* part = (int32_t*)(ws + L.o_part);
    int32_t* offs = (int32_t*)(ws + L.o_offs);
    misplat_internal::fill_bytes(ws + L.o_hist, (size_t)(L.o_part - L.o_hist), 0u, s);      // histograms and states
    const dim3 grid((unsigned)L.nb, (unsigned)V);
    for (int pass = 0; pass < 4; pass++) {
        hipLaunchKernelGGL(key_hist_kernel, grid, dim3(256), 0, s, candidates, keys, P, seed, frame_offset, pass,
                           (const FrameState*)state, hist);
        hipLaunchKernelGGL(key_pick_kernel, dim3((unsigned)V), dim3(256), 0, s, pass, samples_per_frame, state, (const int32_t*)hist,
                           counts);
    }
    hipLaunchKernelGGL((carry_scan_kernel<int32_t, int32_t>), dim3(1), dim3(kScanBlock), 0, s, (const int32_t*)counts, V, V, frame_base,
                       frame_base + V);
    hipLaunchKernelGGL(select_count_kernel, grid, dim3(256), 0, s, candidates, keys, P, seed, frame_offset, (const FrameState*)state, part);
    // every row of part [2 V, nb]: one workgroup a row
    hipLaunchKernelGGL((carry_scan_kernel<int32_t, int32_t>), dim3((unsigned)(2 * V)), dim3(kScanBlock), 0, s, (const int32_t*)part,
                       (int64_t)L.nb, (int64_t)L.nb, offs, (int32_t*)nullptr);
    hipLaunchKernelGGL(select_emit_kernel, grid, dim3(256), 0, s, candidates, keys, P, seed, frame_offset, (const FrameState*)state,
                       (const int32_t*)offs, (const int32_t*)frame_base, frame_ids, pixel_ids);
    return launched();
}

extern "C" int misplat_depthcloud_backproject(const float* depth, const float* rgb, const float* normals, const float* c2w,
                                              const float* intrinsics, int32_t n_views, int32_t height, int32_t width,
                                              const int32_t* frame_ids, const int32_t* pixel_ids, int64_t n_samples, float* points,
                                              float* out_normals, float* colors, misplat_stream_t stream) {
    if (!maps_ok(n_views, height, width) || n_samples < 0 || n_samples >= (1ll << 31) || !depth || !rgb || !c2w || !intrinsics ||
        (normals != nullptr) != (out_normals != nullptr) || (n_samples > 0 && (!frame_ids || !pixel_ids || !points || !colors)))
        return MISPLAT_EINVAL;
    if (n_samples == 0) return MISPLAT_OK;
    hipLaunchKernelGGL(backproject_kernel, dim3(blocks(n_samples, 256)), dim3(256), 0, (hipStream_t)stream, depth, rgb, normals, c2w,
                       intrinsics, (int64_t)height * width, width, frame_ids, pixel_ids, n_samples, points, out_normals, colors);
    return launched();
}

extern "C" int misplat_depthcloud_gaussian_filter(const float* means, int64_t n_gauss, const float* c2w, const float* intrinsics,
                                                  const uint8_t* masks, int32_t n_views, int32_t height, int32_t width, uint8_t* keep,
                                                  misplat_stream_t stream) {
    if (!maps_ok(n_views, height, width) || n_gauss < 0 || n_gauss >= (1ll << 31) || !c2w || !intrinsics || !masks ||
        (n_gauss > 0 && (!means || !keep)))
        return MISPLAT_EINVAL;
    if (n_gauss == 0) return MISPLAT_OK;
    hipLaunchKernelGGL(gaussian_filter_kernel, dim3(blocks(n_gauss, 256)), dim3(256), 0, (hipStream_t)stream, means, n_gauss, c2w,
                       intrinsics, masks, n_views, height, width, keep);
    return launched();
}
