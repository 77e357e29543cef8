// unitgrid.h -- the sparse unit volume that tsdf.hip, density.hip, pointtsdf.hip and poisson.hip share.
//
// Units of 16^3 voxels; voxel g (global integer coordinate) has its centre at (g + 0.5) * voxel_size.  A DENSE unit map over the
// grid's bounds (lo, dims, x fastest) holds per unit the pool slot (int32, -1 = unallocated).  The pool holds per slot kPlanes
// planes of kUnitVoxels fp32 (tsdf, w, r, g, b), voxel index i = lx + 16 ly + 256 lz.
//
// In an unnamed namespace, as wgprims.h: each translation unit compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"

namespace {

constexpr int kUnitVoxels = 4096;
constexpr int kPlanes = 5;

// the kernels' form of a misplat_tsdf_grid.  tsdf.hip's own Grid carries its two truncations between vs and ulen (the layout
// of its kernel arguments, kept); the helpers below take either (G: any struct with these four members).
struct UnitGrid {
    float vs, ulen;
    int lo[3], dims[3];
};

// what every user of the volume requires of a grid; n_map = entries of the unit map
template <class G> inline bool make_unit_grid(const misplat_tsdf_grid* p, G& g, int64_t& n_map) {
    if (!p || !(p->voxel_size > 0.f)) return false;
    n_map = 1;
    for (int a = 0; a < 3; a++) {
        if (p->dims[a] < 1) return false;
        // global voxel coordinates (unit * 16 + 15 + 1) stay inside int32 and exact in fp32
        if (p->lo[a] < -(1 << 19) || (int64_t)p->lo[a] + p->dims[a] > (1 << 19)) return false;
        g.lo[a] = p->lo[a];
        g.dims[a] = p->dims[a];
        n_map *= p->dims[a];
    }
    if (n_map > MISPLAT_TSDF_MAX_UNITS) return false;
    g.vs = p->voxel_size;
    g.ulen = p->voxel_size * 16.f;
    return true;
}

// map index of unit (ux, uy, uz), or -1 outside the map
template <class G> __device__ __forceinline__ int64_t map_index(const G& g, int ux, int uy, int uz) {
    const int mx = ux - g.lo[0], my = uy - g.lo[1], mz = uz - g.lo[2];
    if (mx < 0 || my < 0 || mz < 0 || mx >= g.dims[0] || my >= g.dims[1] || mz >= g.dims[2]) return -1;
    return (int64_t)mx + (int64_t)g.dims[0] * ((int64_t)my + (int64_t)g.dims[1] * mz);
}

template <class G> __device__ __forceinline__ void unit_coords(const G& g, int64_t m, int& ux, int& uy, int& uz) {
    const int64_t nxy = (int64_t)g.dims[0] * g.dims[1];
    uz = (int)(m / nxy) + g.lo[2];
    const int64_t r = m % nxy;
    uy = (int)(r / g.dims[0]) + g.lo[1];
    ux = (int)(r % g.dims[0]) + g.lo[0];
}

// the inclusive unit range lo .. hi along axis a, clipped to the map (empty: lo > hi)
template <class G> __device__ __forceinline__ void clamp_units(const G& g, int a, int& lo, int& hi) {
    lo = lo > g.lo[a] ? lo : g.lo[a];
    hi = hi < g.lo[a] + g.dims[a] - 1 ? hi : g.lo[a] + g.dims[a] - 1;
}

// pool offset of voxel i of plane c of a slot
__device__ __forceinline__ int64_t pool_index(int64_t slot, int c, int64_t i) { return (slot * kPlanes + c) * kUnitVoxels + i; }

// voxel reference slot * 4096 + i of global voxel (gx, gy, gz), or -1 if its unit is not allocated
template <class G> __device__ __forceinline__ int64_t voxel_ref(const G& g, const int32_t* __restrict__ slot_map, int gx, int gy, int gz) {
    const int64_t m = map_index(g, gx >> 4, gy >> 4, gz >> 4);
    if (m < 0) return -1;
    const int s = slot_map[m];
    if (s < 0) return -1;
    return (int64_t)s * kUnitVoxels + ((gx & 15) | ((gy & 15) << 4) | ((gz & 15) << 8));
}

__device__ __forceinline__ float plane(const float* __restrict__ pool, int64_t ref, int c) {
    return pool[pool_index(ref >> 12, c, ref & 4095)];
}

}  // namespace
