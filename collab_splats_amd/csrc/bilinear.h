// bilinear.h -- the 4-tap resize rule shared by featloss.hip and textquery.hip (section 23):
// F.interpolate(mode="bilinear", align_corners=False), no antialiasing, the same rule whether it shrinks or enlarges.  The
// restatements under tests/ hold the same rule.
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

}  // namespace
