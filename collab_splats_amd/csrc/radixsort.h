// radixsort.h -- the stable radix sort shared by meshmap.hip (contributions by vertex) and
// pointcloud.hip (points by voxel, section 17).  In an unnamed namespace, as cellhash.h: each translation unit that includes
// this header compiles its own copy of the kernels into its own code object.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

}  // namespace
