// tsdf.hip -- TSDF fusion of depth maps into a scalable voxel volume and marching-cubes mesh extraction.
//
// Semantics: Open3D's legacy ScalableTSDFVolume, restated in fp32 (tests/tsdf_restatement.py is the oracle).  Compiled with
// -ffp-contract=off; every expression below is evaluated in the written order, so the voxel grids equal the restatement's
// bit for bit.
//
// Volume: unitgrid.h's (units of 16^3 voxels, a dense unit map of pool slots, 5 planes of 4096 fp32 per slot); for the batch
// being integrated the map also holds a 64-bit word per unit, with bit j set iff view j of the batch touches the unit.
//
// Pipeline per batch of <= 64 views: mark (words) -> alloc (slots, touched list; the host reads two counts) -> integrate.
// Extraction: order (allocated units in map order) -> classify + count + unit scan (the host reads two totals) -> emit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"

#define MC_QUAL static __constant__
#include "mc_tables.h"
#include "wgprims.h"
#include "unitgrid.h"

namespace {

struct Grid {                                           // UnitGrid's members and the two truncations
    float vs, trunc, dtrunc, ulen;
    int lo[3], dims[3];
};

__device__ __forceinline__ bool depth_ok(float d, float dtrunc) { return d > 0.f && !(d > dtrunc); }

__device__ __forceinline__ float read_depth(const float* __restrict__ depths, const uint8_t* __restrict__ masks, int64_t pix,
                                            float dtrunc) {
    const float d = depths[pix];
    if (masks && !masks[pix]) return 0.f;
    return depth_ok(d, dtrunc) ? d : 0.f;
}

__device__ __forceinline__ float to_u8(float x) {       // uint8(rgb * 255) with truncation (numpy's cast), clamped to [0, 255]
    float c = x * 255.f;
    c = c > 0.f ? c : 0.f;                              // (NaN -> 0)
    c = c < 255.f ? c : 255.f;
    return (float)(int)c;
}

// ---------------------------------------------------------------------------------------------------------------- mark
// One thread per sampled pixel (u, v multiples of 4) of each view: every unit overlapping the box p +- sdf_trunc around the
// back-projected sample gets the view's bit.  A lane whose box equals the previous lane's leaves the atomics to it.
__global__ __launch_bounds__(256) void tsdf_mark_kernel(Grid g, const float* __restrict__ depths, const uint8_t* __restrict__ masks,
                                                        int V, int H, int W, const float* __restrict__ viewmats,
                                                        const float* __restrict__ Ks, unsigned long long* __restrict__ words) {
    const int sw = (W + 3) / 4, sh = (H + 3) / 4;
    const int64_t per_view = (int64_t)sw * sh;
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int box[6] = {0, -1, 0, -1, 0, -1};                 // lo/hi per axis; empty
    int j = 0;
    if (s < per_view * V) {
        j = (int)(s / per_view);
        const int r = (int)(s - (int64_t)j * per_view);
        const int u = (r % sw) * 4, v = (r / sw) * 4;
        const int64_t pix = ((int64_t)j * H + v) * W + u;
        const float d = read_depth(depths, masks, pix, g.dtrunc);
        if (d > 0.f) {
            const float* M = viewmats + 16 * j;
            const float* K = Ks + 9 * j;
            const float fx = K[0], cx = K[2], fy = K[4], cy = K[5];
            const float xc = (((float)u - cx) * d) / fx, yc = (((float)v - cy) * d) / fy, zc = d;
            const float dx = xc - M[3], dy = yc - M[7], dz = zc - M[11];
            float p[3];
#pragma unroll
            for (int a = 0; a < 3; a++) p[a] = (M[a] * dx + M[4 + a] * dy) + M[8 + a] * dz;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                // (clamped before the conversion: a far or non-finite point must not overflow the int)
                int lo = (int)fminf(fmaxf(floorf((p[a] - g.trunc) / g.ulen), -1e6f), 1e6f);
                int hi = (int)fminf(fmaxf(floorf((p[a] + g.trunc) / g.ulen), -1e6f), 1e6f);
                clamp_units(g, a, lo, hi);
                box[2 * a] = lo; box[2 * a + 1] = hi;
            }
        }
    }
    bool same = (threadIdx.x & 63) != 0;
#pragma unroll
    for (int k = 0; k < 6; k++) same = (__shfl_up(box[k], 1) == box[k]) && same;
    same = (__shfl_up(j, 1) == j) && same;
    if (same) return;
    const unsigned long long bit = 1ull << j;
    for (int z = box[4]; z <= box[5]; z++)
        for (int y = box[2]; y <= box[3]; y++)
            for (int x = box[0]; x <= box[1]; x++) {
                // most samples of a view land in units the view has already marked: a plain load of the (L2-resident)
                // word spares the contended atomic; a stale copy only costs the atomic it would have issued anyway
                unsigned long long* w = &words[map_index(g, x, y, z)];
                if (!(__atomic_load_n(w, __ATOMIC_RELAXED) & bit)) atomicOr(w, bit);
            }
}

// --------------------------------------------------------------------------------------------------------------- alloc
// counters[0]: allocated slots so far (a new unit takes the next one); counters[1]: touched units of this batch (zeroed by
// the caller).  touched[2 t] = map index, touched[2 t + 1] = slot.  Slot and list order do not reach any result.
__global__ __launch_bounds__(256) void tsdf_alloc_kernel(int64_t n_map, const unsigned long long* __restrict__ words,
                                                         int32_t* __restrict__ slot_map, int32_t* __restrict__ counters,
                                                         int32_t* __restrict__ touched) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= n_map || words[m] == 0ull) return;
    int s = slot_map[m];
    if (s < 0) {
        s = atomicAdd(&counters[0], 1);
        slot_map[m] = s;
    }
    const int t = atomicAdd(&counters[1], 1);
    touched[2 * t] = (int32_t)m;
    touched[2 * t + 1] = s;
}

// ----------------------------------------------------------------------------------------------------------- integrate
// One workgroup of 1024 threads per touched unit; lane t holds the kVPL voxels i = (t % 256) + 256 (kVPL (t / 256) + k)
// (lx = t % 16, ly = t / 16 % 16, lz = kVPL (t / 256) + k) in registers across the batch's views, which it applies in view
// order.  The unit's view word makes the per-view branch uniform.  (16 voxels per lane in 256 threads: 236 VGPRs, 2 waves per
// SIMD and a unit's 64 views run serially on 4 waves -- 1.3 ms per batch when few units are touched; 4 per lane fits 128.)
constexpr int kVPL = 4;
__global__ __launch_bounds__(4096 / kVPL) void tsdf_integrate_kernel(Grid g, const int32_t* __restrict__ touched,
                                                             const unsigned long long* __restrict__ words,
                                                             const float* __restrict__ depths, const uint8_t* __restrict__ masks,
                                                             const float* __restrict__ rgbs, int V, int H, int W,
                                                             const float* __restrict__ viewmats, const float* __restrict__ Ks,
                                                             float* __restrict__ pool) {
    const int64_t m = touched[2 * blockIdx.x];
    const int64_t slot = touched[2 * blockIdx.x + 1];
    const unsigned long long word = words[m];
    int ux, uy, uz;
    unit_coords(g, m, ux, uy, uz);
    const int t = threadIdx.x & 255, z0 = kVPL * (threadIdx.x >> 8);
    float* base = pool + pool_index(slot, 0, 0) + 256 * z0 + t;
    float ts[kVPL], ws[kVPL], cr[kVPL], cg[kVPL], cb[kVPL];
#pragma unroll
    for (int k = 0; k < kVPL; k++) {
        ts[k] = base[0 * kUnitVoxels + 256 * k];
        ws[k] = base[1 * kUnitVoxels + 256 * k];
        cr[k] = base[2 * kUnitVoxels + 256 * k];
        cg[k] = base[3 * kUnitVoxels + 256 * k];
        cb[k] = base[4 * kUnitVoxels + 256 * k];
    }
    const float x = ((float)(ux * 16 + (t & 15)) + 0.5f) * g.vs;
    const float y = ((float)(uy * 16 + (t >> 4)) + 0.5f) * g.vs;
    const float fW = (float)W, fH = (float)H;
    for (int j = 0; j < V; j++) {
        if (!((word >> j) & 1ull)) continue;
        const float* M = viewmats + 16 * j;
        const float* K = Ks + 9 * j;
        const float fx = K[0], cx = K[2], fy = K[4], cy = K[5];
        const float r00 = M[0], r01 = M[1], r02 = M[2], t0 = M[3], r10 = M[4], r11 = M[5], r12 = M[6], t1 = M[7];
        const float r20 = M[8], r21 = M[9], r22 = M[10], t2 = M[11];
        const float* D = depths + (int64_t)j * H * W;
        const uint8_t* Mk = masks ? masks + (int64_t)j * H * W : nullptr;
        const float* C = rgbs ? rgbs + (int64_t)j * H * W * 3 : nullptr;
#pragma unroll
        for (int k = 0; k < kVPL; k++) {
            const float z = ((float)(uz * 16 + z0 + k) + 0.5f) * g.vs;
            const float zc = ((r20 * x + r21 * y) + r22 * z) + t2;
            if (!(zc > 0.f)) continue;
            const float xc = ((r00 * x + r01 * y) + r02 * z) + t0;
            const float yc = ((r10 * x + r11 * y) + r12 * z) + t1;
            const float uf = ((xc * fx) / zc + cx) + 0.5f;
            const float vf = ((yc * fy) / zc + cy) + 0.5f;
            if (!(uf >= 0.0001f && uf < fW && vf >= 0.0001f && vf < fH)) continue;
            const int u = (int)uf, v = (int)vf;
            const int64_t pix = (int64_t)v * W + u;
            const float d = read_depth(D, Mk, pix, g.dtrunc);
            if (d == 0.f) continue;
            const float a = ((float)u - cx) / fx, b = ((float)v - cy) / fy;
            const float sdf = (d - zc) * sqrtf((1.f + a * a) + b * b);
            if (!(sdf > -g.trunc)) continue;
            const float tn = fminf(1.f, sdf / g.trunc);
            const float w = ws[k], w1 = w + 1.f;
            float r = 0.f, gg = 0.f, bb = 0.f;
            if (C) { r = to_u8(C[3 * pix]); gg = to_u8(C[3 * pix + 1]); bb = to_u8(C[3 * pix + 2]); }
            ts[k] = (ts[k] * w + tn) / w1;
            cr[k] = (cr[k] * w + r) / w1;
            cg[k] = (cg[k] * w + gg) / w1;
            cb[k] = (cb[k] * w + bb) / w1;
            ws[k] = w1;
        }
    }
#pragma unroll
    for (int k = 0; k < kVPL; k++) {
        base[0 * kUnitVoxels + 256 * k] = ts[k];
        base[1 * kUnitVoxels + 256 * k] = ws[k];
        base[2 * kUnitVoxels + 256 * k] = cr[k];
        base[3 * kUnitVoxels + 256 * k] = cg[k];
        base[4 * kUnitVoxels + 256 * k] = cb[k];
    }
}

// ------------------------------------------------------------------------------------------------------ scan / order
// The scans of the block counts and of the per-unit counts are wgprims.h's carry_scan_kernel (one workgroup per array).
// allocated units of map block b (4096 map entries, 16 consecutive per lane): count (WRITE = false) or write their map
// indices, in map order, from offs[b] on (WRITE = true)
template <bool WRITE>
__global__ __launch_bounds__(256) void tsdf_order_kernel(int64_t n_map, const int32_t* __restrict__ slot_map,
                                                         int32_t* __restrict__ counts, const int32_t* __restrict__ offs,
                                                         int32_t* __restrict__ order) {
    __shared__ uint32_t wsum[4];
    const int64_t m0 = (int64_t)blockIdx.x * 4096 + 16 * threadIdx.x;
    uint32_t bits = 0u;
#pragma unroll
    for (int k = 0; k < 16; k++)
        if (m0 + k < n_map && slot_map[m0 + k] >= 0) bits |= 1u << k;
    uint32_t total;
    const uint32_t pre = block_scan_excl<uint32_t, 4>((uint32_t)__popc(bits), wsum, total);
    if (!WRITE) {
        if (threadIdx.x == 0) counts[blockIdx.x] = (int32_t)total;
        return;
    }
    int32_t pos = offs[blockIdx.x] + (int32_t)pre;
    while (bits) {
        const int k = __ffs((int)bits) - 1;
        order[pos++] = (int32_t)(m0 + k);
        bits &= bits - 1u;
    }
}

// ---------------------------------------------------------------------------------------------------- marching cubes
// classify: code[voxel] = 256 | cube index if the cell at the voxel is valid (all 8 corners allocated with w > 0), else 0
__global__ __launch_bounds__(256) void mc_classify_kernel(Grid g, const int32_t* __restrict__ slot_map,
                                                          const int32_t* __restrict__ order, const float* __restrict__ pool,
                                                          uint16_t* __restrict__ code) {
    const int64_t m = order[blockIdx.x];
    const int64_t slot = slot_map[m];
    int ux, uy, uz;
    unit_coords(g, m, ux, uy, uz);
    const int t = threadIdx.x;
    for (int k = 0; k < 16; k++) {
        const int i = t + 256 * k;
        const int gx = ux * 16 + (i & 15), gy = uy * 16 + ((i >> 4) & 15), gz = uz * 16 + (i >> 8);
        int cube = 0;
        bool valid = true;
        for (int c = 0; c < 8 && valid; c++) {
            const int64_t ref = voxel_ref(g, slot_map, gx + (c & 1), gy + ((c >> 1) & 1), gz + ((c >> 2) & 1));
            if (ref < 0 || !(plane(pool, ref, 1) > 0.f)) { valid = false; break; }
            if (plane(pool, ref, 0) < 0.f) cube |= 1 << c;
        }
        code[slot * kUnitVoxels + i] = valid ? (uint16_t)(256 | cube) : (uint16_t)0;
    }
}

__device__ __forceinline__ bool cell_valid(const Grid& g, const int32_t* __restrict__ slot_map, const uint16_t* __restrict__ code,
                                           int gx, int gy, int gz) {
    const int64_t ref = voxel_ref(g, slot_map, gx, gy, gz);
    return ref >= 0 && (code[ref] & 256);
}

// count: cnt[voxel] = vertex mask (bit a: the voxel's +a edge is crossed and belongs to a valid cell) | triangles << 3;
// unit_counts[k] / unit_counts[n_units + k] = vertices / triangles of unit k (map order)
__global__ __launch_bounds__(256) void mc_count_kernel(Grid g, const int32_t* __restrict__ slot_map,
                                                       const int32_t* __restrict__ order, int64_t n_units,
                                                       const float* __restrict__ pool, const uint16_t* __restrict__ code,
                                                       uint8_t* __restrict__ cnt, int32_t* __restrict__ unit_counts) {
    __shared__ uint32_t wsum[4];
    const int64_t m = order[blockIdx.x];
    const int64_t slot = slot_map[m];
    int ux, uy, uz;
    unit_coords(g, m, ux, uy, uz);
    const int t = threadIdx.x;
    uint32_t nv = 0u, nt = 0u;
    for (int k = 0; k < 16; k++) {
        const int i = t + 256 * k;
        const int gx = ux * 16 + (i & 15), gy = uy * 16 + ((i >> 4) & 15), gz = uz * 16 + (i >> 8);
        const int64_t me = slot * kUnitVoxels + i;
        const uint16_t c0 = code[me];
        const bool v000 = c0 & 256;
        const bool vx = cell_valid(g, slot_map, code, gx - 1, gy, gz), vy = cell_valid(g, slot_map, code, gx, gy - 1, gz);
        const bool vz = cell_valid(g, slot_map, code, gx, gy, gz - 1);
        const bool vxy = cell_valid(g, slot_map, code, gx - 1, gy - 1, gz), vxz = cell_valid(g, slot_map, code, gx - 1, gy, gz - 1);
        const bool vyz = cell_valid(g, slot_map, code, gx, gy - 1, gz - 1);
        const bool any[3] = {v000 || vy || vz || vyz, v000 || vx || vz || vxz, v000 || vx || vy || vxy};
        uint32_t mask = 0u;
        if (any[0] || any[1] || any[2]) {
            const bool n0 = plane(pool, me, 0) < 0.f;
            for (int a = 0; a < 3; a++) {
                if (!any[a]) continue;
                const int64_t o = voxel_ref(g, slot_map, gx + (a == 0), gy + (a == 1), gz + (a == 2));
                if (o >= 0 && (plane(pool, o, 0) < 0.f) != n0) mask |= 1u << a;     // (o >= 0: a valid cell holds it)
            }
        }
        const uint32_t tri = v000 ? (uint32_t)MC_NTRI[c0 & 255] : 0u;
        cnt[me] = (uint8_t)(mask | (tri << 3));
        nv += __popc(mask);
        nt += tri;
    }
    uint32_t tv, tt;
    (void)block_scan_excl<uint32_t, 4>(nv, wsum, tv);
    (void)block_scan_excl<uint32_t, 4>(nt, wsum, tt);
    if (t == 0) {
        unit_counts[blockIdx.x] = (int32_t)tv;
        unit_counts[n_units + blockIdx.x] = (int32_t)tt;
    }
}

// emit vertices: lane t owns voxels 16 t .. 16 t + 15 of unit k, so a workgroup scan gives the voxel-order offsets; each owned
// crossed edge (+x, +y, +z) gets the vertex p0 + |f0| / (|f0| + |f1|) * voxel_size along it.  vert_base[voxel] = index of the
// voxel's first vertex.
__global__ __launch_bounds__(256) void mc_vertices_kernel(Grid g, const int32_t* __restrict__ slot_map,
                                                          const int32_t* __restrict__ order, const float* __restrict__ pool,
                                                          const uint8_t* __restrict__ cnt, const int32_t* __restrict__ voffs,
                                                          int32_t* __restrict__ vert_base, float* __restrict__ vertices,
                                                          float* __restrict__ colors) {
    __shared__ uint32_t wsum[4];
    const int64_t m = order[blockIdx.x];
    const int64_t slot = slot_map[m];
    int ux, uy, uz;
    unit_coords(g, m, ux, uy, uz);
    const int t = threadIdx.x;
    const int64_t v0 = slot * kUnitVoxels + 16 * t;
    uint8_t c[16];
    uint32_t n = 0u;
#pragma unroll
    for (int k = 0; k < 16; k++) { c[k] = cnt[v0 + k]; n += __popc(c[k] & 7u); }
    uint32_t total;
    int32_t idx = voffs[blockIdx.x] + (int32_t)block_scan_excl<uint32_t, 4>(n, wsum, total);
    for (int k = 0; k < 16; k++) {
        const uint32_t mask = c[k] & 7u;
        if (!mask) continue;
        vert_base[v0 + k] = idx;
        const int i = 16 * t + k;
        const int gi[3] = {ux * 16 + (i & 15), uy * 16 + ((i >> 4) & 15), uz * 16 + (i >> 8)};
        const float f0 = plane(pool, v0 + k, 0);
        const float a0 = fabsf(f0);
        for (int a = 0; a < 3; a++) {
            if (!((mask >> a) & 1u)) continue;
            const int64_t o = voxel_ref(g, slot_map, gi[0] + (a == 0), gi[1] + (a == 1), gi[2] + (a == 2));
            if (o < 0) continue;                          // (never: mc_count set the bit only with the neighbour allocated)
            const float a1 = fabsf(plane(pool, o, 0));
            const float s = a0 + a1;
#pragma unroll
            for (int q = 0; q < 3; q++) {
                float p = ((float)gi[q] + 0.5f) * g.vs;
                if (q == a) p = p + (a0 / s) * g.vs;
                vertices[3 * (int64_t)idx + q] = p;
                colors[3 * (int64_t)idx + q] = ((a1 * plane(pool, v0 + k, 2 + q) + a0 * plane(pool, o, 2 + q)) / s) / 255.f;
            }
            idx++;
        }
    }
}

// emit triangles, in voxel order and table order; a triangle's corners are the vertices of the edges' owner voxels
__global__ __launch_bounds__(256) void mc_triangles_kernel(Grid g, const int32_t* __restrict__ slot_map,
                                                           const int32_t* __restrict__ order, const uint16_t* __restrict__ code,
                                                           const uint8_t* __restrict__ cnt, const int32_t* __restrict__ toffs,
                                                           const int32_t* __restrict__ vert_base, int32_t* __restrict__ triangles) {
    __shared__ uint32_t wsum[4];
    const int64_t m = order[blockIdx.x];
    const int64_t slot = slot_map[m];
    int ux, uy, uz;
    unit_coords(g, m, ux, uy, uz);
    const int t = threadIdx.x;
    const int64_t v0 = slot * kUnitVoxels + 16 * t;
    uint8_t c[16];
    uint32_t n = 0u;
#pragma unroll
    for (int k = 0; k < 16; k++) { c[k] = cnt[v0 + k]; n += c[k] >> 3; }
    uint32_t total;
    int64_t tri = toffs[blockIdx.x] + (int32_t)block_scan_excl<uint32_t, 4>(n, wsum, total);
    for (int k = 0; k < 16; k++) {
        const int nt = c[k] >> 3;
        if (!nt) continue;
        const int cube = code[v0 + k] & 255;
        const int i = 16 * t + k;
        const int gx = ux * 16 + (i & 15), gy = uy * 16 + ((i >> 4) & 15), gz = uz * 16 + (i >> 8);
        for (int q = 0; q < 3 * nt; q++) {
            const int e = MC_TRI[cube][q];
            const int c0 = MC_EDGE_CORNERS[e][0], a = e >> 2;
            const int64_t o = voxel_ref(g, slot_map, gx + (c0 & 1), gy + ((c0 >> 1) & 1), gz + ((c0 >> 2) & 1));
            // (o >= 0 always: the owner is a corner of this valid cell)
            triangles[3 * tri + q] = o < 0 ? -1 : vert_base[o] + __popc((uint32_t)(cnt[o] & 7u) & ((1u << a) - 1u));
        }
        tri += nt;
    }
}

bool make_grid(const misplat_tsdf_grid* p, Grid& g, int64_t& n_map) {
    if (!make_unit_grid(p, g, n_map) || !(p->sdf_trunc > 0.f) || !(p->depth_trunc > 0.f)) return false;
    g.trunc = p->sdf_trunc;
    g.dtrunc = p->depth_trunc;
    return true;
}

}  // namespace

extern "C" int misplat_tsdf_mark(const misplat_tsdf_grid* grid, const float* depths, const uint8_t* masks, int32_t n_views,
                                 int32_t height, int32_t width, const float* viewmats, const float* Ks, uint64_t* words,
                                 misplat_stream_t stream) {
    Grid g;
    int64_t n_map;
    if (!make_grid(grid, g, n_map) || n_views < 1 || n_views > MISPLAT_TSDF_MAX_VIEWS || height < 1 || width < 1 ||
        (int64_t)height * width > (1ll << 30) || !depths || !viewmats || !Ks || !words)
        return MISPLAT_EINVAL;
    const int64_t n = (int64_t)((width + 3) / 4) * ((height + 3) / 4) * n_views;
    hipLaunchKernelGGL(tsdf_mark_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, depths, masks,
                       (int)n_views, (int)height, (int)width, viewmats, Ks, (unsigned long long*)words);
    return launched();
}

extern "C" int misplat_tsdf_alloc(const misplat_tsdf_grid* grid, const uint64_t* words, int32_t* slot_map, int32_t* counters,
                                  int32_t* touched, misplat_stream_t stream) {
    Grid g;
    int64_t n_map;
    if (!make_grid(grid, g, n_map) || !words || !slot_map || !counters || !touched) return MISPLAT_EINVAL;
    hipLaunchKernelGGL(tsdf_alloc_kernel, dim3((unsigned)((n_map + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_map,
                       (const unsigned long long*)words, slot_map, counters, touched);
    return launched();
}

extern "C" int misplat_tsdf_integrate(const misplat_tsdf_grid* grid, const int32_t* touched, int32_t n_touched,
                                      const uint64_t* words, const float* depths, const uint8_t* masks, const float* rgbs,
                                      int32_t n_views, int32_t height, int32_t width, const float* viewmats, const float* Ks,
                                      float* pool, misplat_stream_t stream) {
    Grid g;
    int64_t n_map;
    if (!make_grid(grid, g, n_map) || n_touched < 0 || n_touched > n_map || n_views < 1 || n_views > MISPLAT_TSDF_MAX_VIEWS ||
        height < 1 || width < 1 || (int64_t)height * width > (1ll << 30) || !depths || !viewmats || !Ks || !pool ||
        (n_touched > 0 && (!touched || !words)))
        return MISPLAT_EINVAL;
    if (n_touched == 0) return MISPLAT_OK;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)n_touched), dim3(4096 / kVPL), 0, (hipStream_t)stream, g, touched,
                       (const unsigned long long*)words, depths, masks, rgbs, (int)n_views, (int)height, (int)width, viewmats, Ks,
                       pool);
    return launched();
}

extern "C" int misplat_tsdf_order(const misplat_tsdf_grid* grid, const int32_t* slot_map, int32_t* scratch, int32_t* order,
                                  misplat_stream_t stream) {
    Grid g;
    int64_t n_map;
    if (!make_grid(grid, g, n_map) || !slot_map || !scratch || !order) return MISPLAT_EINVAL;
    const int64_t nb = (n_map + 4095) / 4096;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tsdf_order_kernel<false>, dim3((unsigned)nb), dim3(256), 0, s, n_map, slot_map, scratch, nullptr, nullptr);
    hipLaunchKernelGGL((carry_scan_kernel<int32_t, int32_t>), dim3(1), dim3(kScanBlock), 0, s, (const int32_t*)scratch, nb, nb,
                       scratch + nb, scratch + 2 * nb);
    hipLaunchKernelGGL(tsdf_order_kernel<true>, dim3((unsigned)nb), dim3(256), 0, s, n_map, slot_map, nullptr, scratch + nb, order);
    return launched();
}

extern "C" int misplat_tsdf_mc_count(const misplat_tsdf_grid* grid, const int32_t* slot_map, const int32_t* order,
                                     int32_t n_units, const float* pool, uint16_t* code, uint8_t* cnt, int32_t* unit_counts,
                                     int32_t* unit_offs, int32_t* totals, misplat_stream_t stream) {
    Grid g;
    int64_t n_map;
    if (!make_grid(grid, g, n_map) || n_units < 1 || n_units > n_map || !slot_map || !order || !pool || !code || !cnt ||
        !unit_counts || !unit_offs || !totals)
        return MISPLAT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_classify_kernel, dim3((unsigned)n_units), dim3(256), 0, s, g, slot_map, order, pool, code);
    hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)n_units), dim3(256), 0, s, g, slot_map, order, (int64_t)n_units, pool,
                       (const uint16_t*)code, cnt, unit_counts);
    hipLaunchKernelGGL((carry_scan_kernel<int32_t, int32_t>), dim3(2), dim3(kScanBlock), 0, s, (const int32_t*)unit_counts,
                       (int64_t)n_units, (int64_t)n_units, unit_offs, totals);
    return launched();
}

extern "C" int misplat_tsdf_mc_emit(const misplat_tsdf_grid* grid, const int32_t* slot_map, const int32_t* order,
                                    int32_t n_units, const float* pool, const uint16_t* code, const uint8_t* cnt,
                                    const int32_t* unit_offs, int32_t* vert_base, float* vertices, float* colors,
                                    int32_t* triangles, misplat_stream_t stream) {
    Grid g;
    int64_t n_map;
    if (!make_grid(grid, g, n_map) || n_units < 1 || n_units > n_map || !slot_map || !order || !pool || !code || !cnt ||
        !unit_offs || !vert_base || (((uintptr_t)cnt) & 15))
        return MISPLAT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (vertices && colors)
        hipLaunchKernelGGL(mc_vertices_kernel, dim3((unsigned)n_units), dim3(256), 0, s, g, slot_map, order, pool, cnt, unit_offs,
                           vert_base, vertices, colors);
    if (triangles)
        hipLaunchKernelGGL(mc_triangles_kernel, dim3((unsigned)n_units), dim3(256), 0, s, g, slot_map, order, code, cnt,
                           unit_offs + n_units, (const int32_t*)vert_base, triangles);
    return launched();
}
