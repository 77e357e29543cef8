// bilinear.h -- the 4-tap resize rule shared by featloss.hip and textquery.hip (section 23):
// F.interpolate(mode="bilinear", align_corners=False), no antialiasing, the same rule whether it shrinks or enlarges, and its
// exact transpose (the gathers of featloss.hip's backward).  The restatements under tests/ hold the same rule.
#pragma once

namespace {

struct Taps { int i0, i1; float l0, l1; };

// source coordinate (dst + 0.5) * (n_in / n_out) - 0.5, clamped at 0, the upper tap clamped to the last index.  The
// coordinate is formed in fp64, the two weights are fp32.
__device__ __forceinline__ Taps taps(int dst, int n_in, double scale) {
    double src = ((double)dst + 0.5) * scale - 0.5;
    if (src < 0.0) src = 0.0;
    int i0 = (int)src;
    if (i0 > n_in - 1) i0 = n_in - 1;
    Taps t;
    t.i0 = i0;
    t.i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    t.l1 = (float)(src - (double)i0);
    t.l0 = 1.0f - t.l1;
    return t;
}

// the four taps blended, columns first: v[row tap][column tap]
__device__ __forceinline__ float bilerp(const Taps& ty, const Taps& tx, float v00, float v01, float v10, float v11) {
    return ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
}

// the destinations whose taps can touch source index i: source coordinate in (i - 1, i + 1), one more on each side for
// rounding; every candidate is then tested with taps() itself, so the gather is the exact transpose of the sampling
__device__ __forceinline__ void touching(int i, int n_out, double inv_scale, int* lo, int* hi) {
    const double a = ((double)i - 0.5) * inv_scale - 0.5, b = ((double)i + 1.5) * inv_scale - 0.5;
    const double l = floor(a) - 1.0, h = ceil(b) + 1.0, last = (double)(n_out - 1);
    *lo = (int)(l < 0.0 ? 0.0 : (l > last ? last : l));
    *hi = (int)(h > last ? last : (h < 0.0 ? 0.0 : h));
}

__device__ __forceinline__ float tap_weight(const Taps& t, int i) {
    return (t.i0 == i ? t.l0 : 0.f) + (t.i1 == i ? t.l1 : 0.f);
}

}  // namespace
