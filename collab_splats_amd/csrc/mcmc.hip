// mcmc.hip -- MCMC densification: "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et
// al. 2024), the fixed-budget alternative to the adaptive density control of strategy.py.  gsplat, whose MCMCStrategy the
// reference's models inherit through Splatfacto's `strategy` field, is not on this machine or in the reference tree: the three
// operations are restated from the published method and parity with gsplat's code is unpinned [UNVERIFIED-UPSTREAM].
//
//   noise       every step, in place on means [N, 3]:  o = sigmoid(logit), s = exp(log scale), R from the normalised wxyz
//               quaternion, g = 1 / (1 + exp(-100 ((1 - o) - 0.995))), z three standard normals,
//               d = R diag(s^2) R^T (z g scaler) rounded to fp32, means += d.  One launch, 44 B read and 12 B written per
//               Gaussian, no [N, 3, 3] covariance.  z comes from the counter-based hash of hashmix.h, so the same (seed, step)
//               gives the same bits on every rank, in every run and under any launch shape.
//   sample      M draws with replacement from N weights, exact integer work:  q_i = (uint32)(o_i 2^24) (0 at or below the alive
//               threshold), an int64 inclusive scan in three launches (block totals, one workgroup over the totals with a
//               carry, block scans), draw j = the first i with incl[i] > (u_j total) >> 64 by binary search, and how often
//               each row was drawn by integer atomics.  No limit of 2^24 categories.
//   relocation  the paper's Eq. 9 for M (opacity, scale, ratio) entries, the double sum in fp64 in the written order.
//
// The hash schedule (the restatement, tests/mcmc_restatement.py, holds the same uint32 arithmetic):
//   key_noise  = mix32(seed, step, 1);   word k of Gaussian i = mix32(key_noise, i, k), k = 0 .. 3
//   key_sample = mix32(seed, step, 2);   u_j = mix32(key_sample, j, 0) << 32 | mix32(key_sample, j, 1)
// A uniform in (0, 1] is ((w >> 8) + 1) 2^-24 and one in [0, 1) is (w >> 8) 2^-24, both exact in fp32: the logarithm never
// sees 0.  Box-Muller: r = sqrt(-2 log u), (z0, z1) = r0 (cos, sin)(2 pi v0), z2 = r1 cos(2 pi v1); the angle goes through
// sincospi, whose argument 2 v is exact.
//
// Contraction is OFF for this file (build.py): d is rounded to fp32 on its own and then added to the mean, so the update
// equals fl32(mean + d) bit for bit for the d that zero means return.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "misplat.h"
#include "hashmix.h"
#include "wgprims.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;                    // grid cap of the streaming kernels; the rest is a grid-stride loop
constexpr uint32_t kNoiseStream = 1u, kSampleStream = 2u;

inline unsigned capped_blocks(int64_t n) {
    const int64_t b = (n + kThreads - 1) / kThreads;
    return (unsigned)(b < kMaxBlocks ? b : kMaxBlocks);
}

// ------------------------------------------------------------------------------------------------------------- noise
__device__ __forceinline__ float unit_open_low(uint32_t w) { return (float)((w >> 8) + 1u) * 0x1p-24f; }     // (0, 1]
__device__ __forceinline__ float unit_open_high(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }           // [0, 1)

__global__ __launch_bounds__(kThreads) void mcmc_noise_kernel(int64_t n, float* __restrict__ means,
                                                              const float* __restrict__ opacities, const float* __restrict__ scales,
                                                              const float* __restrict__ quats, float scaler, uint32_t seed,
                                                              uint32_t step) {
    const uint32_t key = mix32(seed, step, kNoiseStream);
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        const float4 q4 = *reinterpret_cast<const float4*>(quats + 4 * i);
        const float l = opacities[i];
        const float s0 = expf(scales[3 * i]), s1 = expf(scales[3 * i + 1]), s2 = expf(scales[3 * i + 2]);
        const float o = 1.0f / (1.0f + expf(-l));
        const float g = 1.0f / (1.0f + expf(-100.0f * ((1.0f - o) - 0.995f)));
        const uint32_t ii = (uint32_t)i;
        const float r0 = sqrtf(-2.0f * logf(unit_open_low(mix32(key, ii, 0))));
        const float r1 = sqrtf(-2.0f * logf(unit_open_low(mix32(key, ii, 2))));
        float sn0, cs0, sn1, cs1;
        sincospif(2.0f * unit_open_high(mix32(key, ii, 1)), &sn0, &cs0);
        sincospif(2.0f * unit_open_high(mix32(key, ii, 3)), &sn1, &cs1);
        const float t = g * scaler;
        const float v0 = (r0 * cs0) * t, v1 = (r0 * sn0) * t, v2 = (r1 * cs1) * t;
        // R, the build_rotation convention (w first)
        const float inv = 1.0f / sqrtf(q4.x * q4.x + q4.y * q4.y + q4.z * q4.z + q4.w * q4.w);
        const float w = q4.x * inv, x = q4.y * inv, y = q4.z * inv, z = q4.w * inv;
        const float R00 = 1.0f - 2.0f * (y * y + z * z), R01 = 2.0f * (x * y - w * z), R02 = 2.0f * (x * z + w * y);
        const float R10 = 2.0f * (x * y + w * z), R11 = 1.0f - 2.0f * (x * x + z * z), R12 = 2.0f * (y * z - w * x);
        const float R20 = 2.0f * (x * z - w * y), R21 = 2.0f * (y * z + w * x), R22 = 1.0f - 2.0f * (x * x + y * y);
        // d = R (s^2 * (R^T v)): the covariance is never formed
        const float a0 = (s0 * s0) * ((R00 * v0 + R10 * v1) + R20 * v2);
        const float a1 = (s1 * s1) * ((R01 * v0 + R11 * v1) + R21 * v2);
        const float a2 = (s2 * s2) * ((R02 * v0 + R12 * v1) + R22 * v2);
        const float d0 = (R00 * a0 + R01 * a1) + R02 * a2;
        const float d1 = (R10 * a0 + R11 * a1) + R12 * a2;
        const float d2 = (R20 * a0 + R21 * a1) + R22 * a2;
        means[3 * i] += d0;
        means[3 * i + 1] += d1;
        means[3 * i + 2] += d2;
    }
}

// ------------------------------------------------------------------------------------------------------------ sample
// the integer weight of an activated opacity: floor(min(o, 1) 2^24), both steps exact in fp32; 0 for o <= 0, a NaN, and, with a
// threshold, o <= min_opacity
__device__ __forceinline__ int64_t weight_of(float o, int32_t has_min, float min_opacity) {
    if (!(o > 0.0f) || (has_min && o <= min_opacity)) return 0;
    return (int64_t)(uint32_t)((o < 1.0f ? o : 1.0f) * 16777216.0f);
}

__global__ __launch_bounds__(kScanBlock) void mcmc_weight_totals_kernel(const float* __restrict__ opacities, int64_t n, int32_t has_min,
                                                                        float min_opacity, int64_t* __restrict__ bsum) {
    __shared__ int64_t wsum[kScanBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kScanBlock + threadIdx.x;
    int64_t total;
    (void)block_scan_excl<int64_t, kScanBlock / 64>(i < n ? weight_of(opacities[i], has_min, min_opacity) : 0, wsum, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kScanBlock) void mcmc_weight_scan_kernel(const float* __restrict__ opacities, int64_t n, int32_t has_min,
                                                                      float min_opacity, const int64_t* __restrict__ boff,
                                                                      int64_t* __restrict__ incl) {
    __shared__ int64_t wsum[kScanBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kScanBlock + threadIdx.x;
    const int64_t q = i < n ? weight_of(opacities[i], has_min, min_opacity) : 0;
    int64_t total;
    const int64_t ex = block_scan_excl<int64_t, kScanBlock / 64>(q, wsum, total);
    if (i < n) incl[i] = boff[blockIdx.x] + ex + q;
}

__global__ __launch_bounds__(kThreads) void mcmc_draw_kernel(const int64_t* __restrict__ incl, int64_t n, const int64_t* __restrict__ total_p,
                                                             int64_t m, uint32_t seed, uint32_t step, int64_t* __restrict__ idx,
                                                             int32_t* __restrict__ counts, int32_t* __restrict__ status) {
    const uint64_t total = (uint64_t)*total_p;
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = total == 0 ? MISPLAT_MCMC_NOTHING : 0;
    const uint32_t key = mix32(seed, step, kSampleStream);
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < m; j += stride) {
        if (total == 0) { idx[j] = -1; continue; }
        const uint32_t jj = (uint32_t)j;
        const uint64_t u = ((uint64_t)mix32(key, jj, 0) << 32) | (uint64_t)mix32(key, jj, 1);
        const int64_t r = (int64_t)__umul64hi(u, total);                  // in [0, total)
        int64_t lo = 0, hi = n - 1;                                       // incl[n - 1] = total > r: the answer lies in [lo, hi]
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (incl[mid] > r) hi = mid; else lo = mid + 1;
        }
        idx[j] = lo;
        if (counts) atomicAdd(&counts[lo], 1);
    }
}

struct SampleWorkspace {
    int64_t *incl, *bsum, *boff, *total;
    int64_t bytes;
};

inline SampleWorkspace carve_sample(void* base, int64_t n) {
    Carver c{(char*)base};
    const int64_t nb = (n + kScanBlock - 1) / kScanBlock;
    SampleWorkspace w;
    w.incl = c.take<int64_t>(n);
    w.bsum = c.take<int64_t>(nb);
    w.boff = c.take<int64_t>(nb);
    w.total = c.take<int64_t>(1);
    w.bytes = c.o;
    return w;
}

// -------------------------------------------------------------------------------------------------------- relocation
__global__ __launch_bounds__(kThreads) void mcmc_relocation_kernel(int64_t m, const float* __restrict__ opacities,
                                                                   const float* __restrict__ scales, const int32_t* __restrict__ ratios,
                                                                   const double* __restrict__ binoms, int32_t n_max,
                                                                   float* __restrict__ new_opacities, float* __restrict__ new_scales) {
    __shared__ double coef[MISPLAT_MCMC_N_MAX * MISPLAT_MCMC_N_MAX];     // C(i, k) (-1)^k / sqrt(k + 1), row i = 0 .. n_max - 1
    for (int e = threadIdx.x; e < n_max * n_max; e += kThreads) {
        const int k = e % n_max;
        const double c = binoms[e] / sqrt((double)(k + 1));
        coef[e] = (k & 1) ? -c : c;
    }
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < m; j += stride) {
        const float of = opacities[j];
        int32_t n = ratios[j];
        n = n < 1 ? 1 : (n > n_max ? n_max : n);
        const double o = (double)of;
        // 1 - (1 - o)^(1 / n), written so that a small o does not cancel
        const double op = -expm1(log1p(-o) / (double)n);
        double D = 0.0;
        for (int i = 1; i <= n; i++) {
            const double* row = coef + (i - 1) * n_max;
            double p = op;
            for (int k = 0; k < i; k++) {
                D += row[k] * p;
                p *= op;
            }
        }
        const double f = of > 0.0f ? o / D : 1.0;                         // (o -> 0: D -> n o' -> o)
        new_opacities[j] = (float)op;
        new_scales[3 * j] = (float)(f * (double)scales[3 * j]);
        new_scales[3 * j + 1] = (float)(f * (double)scales[3 * j + 1]);
        new_scales[3 * j + 2] = (float)(f * (double)scales[3 * j + 2]);
    }
}

constexpr int64_t kMaxRows = (1ll << 31) - 1;       // the hash counter is 32 bits wide

}  // namespace

extern "C" int misplat_mcmc_noise(int64_t n, float* means, const float* opacities, const float* scales, const float* quats,
                                  float scaler, uint32_t seed, uint32_t step, misplat_stream_t stream) {
    if (n < 1 || n > kMaxRows || !means || !opacities || !scales || !quats || ((uintptr_t)quats & 15)) return MISPLAT_EINVAL;
    hipLaunchKernelGGL(mcmc_noise_kernel, dim3(capped_blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, n, means, opacities,
                       scales, quats, scaler, seed, step);
    return launched();
}

extern "C" int64_t misplat_mcmc_sample_workspace_bytes(int64_t n) {
    if (n < 1 || n > kMaxRows) return -1;
    return carve_sample(nullptr, n).bytes;
}

extern "C" int misplat_mcmc_sample(int64_t n, const float* opacities, int32_t has_min_opacity, float min_opacity, int64_t m,
                                   uint32_t seed, uint32_t step, void* workspace, int64_t workspace_bytes, int64_t* idx,
                                   int32_t* counts, int32_t* status, misplat_stream_t stream) {
    if (n < 1 || n > kMaxRows || m < 1 || m > kMaxRows || !opacities || !workspace || !idx || !status) return MISPLAT_EINVAL;
    if (((uintptr_t)workspace & 7)) return MISPLAT_EINVAL;
    const SampleWorkspace w = carve_sample(workspace, n);
    if (workspace_bytes < w.bytes) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = (n + kScanBlock - 1) / kScanBlock;
    if (counts && hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)n, s) != hipSuccess) return MISPLAT_ELAUNCH;
    hipLaunchKernelGGL(mcmc_weight_totals_kernel, dim3((unsigned)nb), dim3(kScanBlock), 0, s, opacities, n, has_min_opacity,
                       min_opacity, w.bsum);
    hipLaunchKernelGGL((carry_scan_kernel<int64_t, int64_t>), dim3(1), dim3(kScanBlock), 0, s, (const int64_t*)w.bsum, nb, nb, w.boff,
                       w.total);
    hipLaunchKernelGGL(mcmc_weight_scan_kernel, dim3((unsigned)nb), dim3(kScanBlock), 0, s, opacities, n, has_min_opacity, min_opacity,
                       (const int64_t*)w.boff, w.incl);
    hipLaunchKernelGGL(mcmc_draw_kernel, dim3(capped_blocks(m)), dim3(kThreads), 0, s, (const int64_t*)w.incl, n,
                       (const int64_t*)w.total, m, seed, step, idx, counts, status);
    return launched();
}

extern "C" int misplat_mcmc_relocation(int64_t m, const float* opacities, const float* scales, const int32_t* ratios,
                                       const double* binoms, int32_t n_max, float* new_opacities, float* new_scales,
                                       misplat_stream_t stream) {
    if (m < 1 || m > kMaxRows || n_max < 1 || n_max > MISPLAT_MCMC_N_MAX) return MISPLAT_EINVAL;
    if (!opacities || !scales || !ratios || !binoms || !new_opacities || !new_scales) return MISPLAT_EINVAL;
    hipLaunchKernelGGL(mcmc_relocation_kernel, dim3(capped_blocks(m)), dim3(kThreads), 0, (hipStream_t)stream, m, opacities, scales,
                       ratios, binoms, n_max, new_opacities, new_scales);
    return launched();
}
