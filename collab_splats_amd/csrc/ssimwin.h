// ssimwin.h -- what the SSIM kernels of the loss (ssim.hip) and of the evaluation metrics (evalmetrics.hip) share: the tile
// and window geometry, the window's weights and the two stabilising constants.  One definition, so that the training loss
// and the evaluation score are the same index.
#pragma once
#include <cmath>

namespace {

constexpr int kTile = 16;
constexpr int kWin = 11;
constexpr int kPatch = kTile + kWin - 1;        // 26

// the LDS layout of a tile's patch (channel-interleaved rows) and of the row pass's results
constexpr int kRow3 = 3 * kPatch;               // 78 floats of a patch row
constexpr int kRowS = kRow3 + 1;                // LDS row stride (odd: the stride-3 channel walk stays conflict-free)
constexpr int kHzS = 20;                        // row stride of the row-pass results: row quads 16 banks apart
constexpr int kQuads = kTile / 4;

// data_range = 1: C1 = (0.01)^2, C2 = (0.03)^2
constexpr float kSsimC1 = 0.01f * 0.01f;
constexpr float kSsimC2 = 0.03f * 0.03f;

struct Window { float w[kWin]; };

// pytorch_msssim._fspecial_gauss_1d(11, 1.5): float32 exp of -(c^2) / (2 sigma^2), normalised by the float32 sum
inline Window make_window() {
    Window W;
    float sum = 0.f;
    for (int i = 0; i < kWin; i++) {
        const float c = (float)(i - kWin / 2);
        W.w[i] = expf(-(c * c) / (2.0f * 1.5f * 1.5f));
        sum += W.w[i];
    }
    for (int i = 0; i < kWin; i++) W.w[i] /= sum;
    return W;
}

}  // namespace
