// rowlinear.h -- the layer "lane = row, wave-uniform weight rows" of the loss-side files: a lane keeps
// its row of up to N values in registers, and a weight row comes through scalar loads and is contracted with it in two chains of
// multiply-adds.  Users: featloss.hip (section 21) and
// identity.hip (section 33).  In an unnamed namespace, as wgprims.h.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// the lane's row: n values (kFull: n == N, no guard), the registers past n are 0
template <int N, bool kFull>
__device__ __forceinline__ void load_row(float (&x)[N], const float* __restrict__ src, int n) {
#pragma unroll
    for (int d = 0; d < N; d++) x[d] = (kFull || d < n) ? src[d] : 0.f;
}

// bias + <wr, x> over n values: the even indices into one chain that starts at the bias, the odd ones into one that starts
// at 0, the two added at the end.  wr is wave-uniform.  N is even.
template <int N, bool kFull>
__device__ __forceinline__ float dot2(const float* __restrict__ wr, float bias, const float (&x)[N], int n) {
    float a0 = bias, a1 = 0.f;
#pragma unroll
    for (int d = 0; d + 1 < N; d += 2) {
        if (kFull || d < n) a0 = fmaf(wr[d], x[d], a0);
        if (kFull || d + 1 < n) a1 = fmaf(wr[d + 1], x[d + 1], a1);
    }
    return a0 + a1;
}

}  // namespace
