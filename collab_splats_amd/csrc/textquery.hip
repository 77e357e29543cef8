// textquery.hip -- text-query similarity of rendered views and of Gaussians (rade_features_model.py:493-539
// `get_outputs_for_camera`, :143-147 the per-Gaussian `similarity`; utils/features.py:237-325 `compute_similarity`) without
// the decoded features.  The text embeddings E [Q, C] meet a prediction p = w_out h + b_out only through E p, so
//   E p = (E w_out) h + E b_out = A h + c,   A [Q, Hd], c [Q]          (fold_kernel: once per query set, fp64 sums)
// and a pixel (or a Gaussian) is
//   x   = bilinear(features [H,W,L] -> (h, w))                          (bilinear.h; rows: the latent itself)
//   hid = relu(w_hidden x + b_hidden)
//   z_q = (A_q . hid + c_q) / T
//   "standard": softmax(z)[:n_pos].sum();  "pairwise": exp(p) / (n_neg exp(p) + sum_j exp(n_j)), p = mean positive z
// with the maximum subtracted before any exp and a NaN result (non-finite inputs only) written as 0.
//
// Layout: lane = pixel.  The pixel keeps x (<= 32 values) and its Q <= 64 logits in registers and walks the hidden units
// once: a unit's activation is formed and added into every logit, so no hidden vector is held and every Hd runs the same
// code.  w_hidden, b_hidden, A and c are wave-uniform (scalar loads).  Every sum runs in index order: two runs, and a
// strided and a contiguous view of the same features, give the same bits.  No LDS, no barrier, no atomics.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "bilinear.h"
#include "misplat.h"
#include "wgprims.h"

namespace {

constexpr int kMaxLatent = 32;
constexpr int kMaxHidden = 256;
constexpr int kMaxQuery = 64;
constexpr int kFewQueries = 8;                  // up to here the logits take 8 registers, beyond 64
constexpr int kMaxChannels = 1 << 20;
constexpr int64_t kMaxPixels = (int64_t)1 << 28;

struct Query {
    const float* wh;                            // [Hd, L]
    const float* bh;                            // [Hd]
    const float* A;                             // [Q, Hd]
    const float* c;                             // [Q]
    int L, Hd, Q, n_pos, pairwise;
    float T;
};

// ---- A [Q, Hd] and c [Q]: one thread per output, its sum over the C channels in index order in fp64 (the products of two
// floats are exact there), rounded once
__global__ __launch_bounds__(256) void fold_kernel(int Q, int C, int Hd, const float* __restrict__ E, const float* __restrict__ w_out,
                                                   const float* __restrict__ b_out, float* __restrict__ A, float* __restrict__ c) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Q * (Hd + 1)) return;
    const int q = e / (Hd + 1), j = e - q * (Hd + 1);
    const float* er = E + (size_t)q * C;
    double s = 0.0;
    if (j < Hd) {
        for (int k = 0; k < C; k++) s += (double)er[k] * (double)w_out[(size_t)k * Hd + j];
        A[q * Hd + j] = (float)s;
    } else {
        for (int k = 0; k < C; k++) s += (double)er[k] * (double)b_out[k];
        c[q] = (float)s;
    }
}

// The similarity of one pixel from its latent x (entries past L are unread).  kQ: the logits held in registers, 8 or 64
// (Q <= kQ); the loops over them are unrolled whole and guarded by the wave-uniform q < Q.
template <int kQ>
__device__ __forceinline__ float similarity(const Query& qy, const float (&x)[kMaxLatent]) {
    const int L = qy.L, Hd = qy.Hd, Q = qy.Q;
    float z[kQ];
#pragma unroll
    for (int q = 0; q < kQ; q++) z[q] = q < Q ? qy.c[q] : 0.f;
    for (int j = 0; j < Hd; j++) {
        const float* wr = qy.wh + j * L;
        float a = qy.bh[j];
#pragma unroll
        for (int l = 0; l < kMaxLatent; l++) {
            if (l < L) a = fmaf(wr[l], x[l], a);
        }
        a = a < 0.f ? 0.f : a;                                          // relu as torch's: a NaN stays one (and ends as 0 below)
        const float* Aj = qy.A + j;
#pragma unroll
        for (int q = 0; q < kQ; q++) {
            if (q < Q) z[q] = fmaf(Aj[q * Hd], a, z[q]);
        }
    }
    const int n_pos = qy.n_pos;
    float r;
    if (!qy.pairwise) {
        float m = -INFINITY;
#pragma unroll
        for (int q = 0; q < kQ; q++) {
            if (q < Q) {
                z[q] = z[q] / qy.T;
                m = fmaxf(m, z[q]);
            }
        }
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int q = 0; q < kQ; q++) {
            if (q < Q) den += expf(z[q] - m);
            if (q == n_pos - 1) num = den;                              // the positives come first: their sum is a prefix
        }
        r = num / den;
    } else {
        float p = 0.f, m = -INFINITY;
#pragma unroll
        for (int q = 0; q < kQ; q++) {
            if (q < Q) {
                z[q] = z[q] / qy.T;
                if (q < n_pos) p += z[q];
                else m = fmaxf(m, z[q]);
            }
        }
        p = p / (float)n_pos;
        m = fmaxf(m, p);
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < kQ; q++) {
            if (q >= n_pos && q < Q) s += expf(z[q] - m);
        }
        const float e = expf(p - m);
        r = e / ((float)(Q - n_pos) * e + s);
    }
    return r == r ? r : 0.f;
}

// ---- one thread per pixel of the working map (h, w); identity: (h, w) is the image's own size (and the row form, an
// image of one column): the latent is read as it is
template <int kQ>
__global__ __launch_bounds__(256) void similarity_kernel(Query qy, int H, int W, int pix_stride, const float* __restrict__ features,
                                                         int h, int w, int identity, float* __restrict__ out) {
    const size_t P = (size_t)h * w, m = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= P) return;
    const int L = qy.L;
    float x[kMaxLatent];
#pragma unroll
    for (int l = 0; l < kMaxLatent; l++) x[l] = 0.f;
    if (identity) {
        const float* f = features + m * pix_stride;
#pragma unroll
        for (int l = 0; l < kMaxLatent; l++) {
            if (l < L) x[l] = f[l];
        }
    } else {
        const Taps ty = taps((int)(m / w), H, (double)H / h), tx = taps((int)(m % w), W, (double)W / w);
        const float* f00 = features + ((size_t)ty.i0 * W + tx.i0) * pix_stride;
        const float* f01 = features + ((size_t)ty.i0 * W + tx.i1) * pix_stride;
        const float* f10 = features + ((size_t)ty.i1 * W + tx.i0) * pix_stride;
        const float* f11 = features + ((size_t)ty.i1 * W + tx.i1) * pix_stride;
#pragma unroll
        for (int l = 0; l < kMaxLatent; l++) {
            if (l < L) x[l] = bilerp(ty, tx, f00[l], f01[l], f10[l], f11[l]);
        }
    }
    out[m] = similarity<kQ>(qy, x);
}

// ---- the heat map [h, w] -> [H, W] by the same rule: one thread per output pixel
__global__ __launch_bounds__(256) void upsample_kernel(int h, int w, const float* __restrict__ in, int H, int W, float* __restrict__ out) {
    const size_t P = (size_t)H * W, m = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= P) return;
    const Taps ty = taps((int)(m / W), h, (double)h / H), tx = taps((int)(m % W), w, (double)w / W);
    const float v00 = in[(size_t)ty.i0 * w + tx.i0], v01 = in[(size_t)ty.i0 * w + tx.i1];
    const float v10 = in[(size_t)ty.i1 * w + tx.i0], v11 = in[(size_t)ty.i1 * w + tx.i1];
    out[m] = bilerp(ty, tx, v00, v01, v10, v11);
}

bool make_query(int32_t latent, int32_t hidden, const float* w_hidden, const float* b_hidden, int32_t n_queries, int32_t n_positive,
                const float* A, const float* c, int32_t method, float softmax_temp, Query* qy) {
    if (latent < 1 || latent > kMaxLatent || hidden < 1 || hidden > kMaxHidden || n_queries < 2 || n_queries > kMaxQuery ||
        n_positive < 1 || n_positive > n_queries - 1 || (method != 0 && method != 1) || !(softmax_temp > 0.f) ||
        !std::isfinite(softmax_temp) || !w_hidden || !b_hidden || !A || !c)
        return false;
    *qy = Query{w_hidden, b_hidden, A, c, latent, hidden, n_queries, n_positive, method, softmax_temp};
    return true;
}

int launch_similarity(const Query& qy, int H, int W, int pix_stride, const float* features, int h, int w, float* out, hipStream_t s) {
    const size_t P = (size_t)h * w;
    const dim3 grid((unsigned)((P + 255) / 256));
    const int identity = h == H && w == W;
    if (qy.Q <= kFewQueries) hipLaunchKernelGGL(similarity_kernel<kFewQueries>, grid, dim3(256), 0, s, qy, H, W, pix_stride, features, h, w, identity, out);
    else hipLaunchKernelGGL(similarity_kernel<kMaxQuery>, grid, dim3(256), 0, s, qy, H, W, pix_stride, features, h, w, identity, out);
    return launched();
}

}  // namespace

extern "C" int misplat_textquery_fold(int32_t n_queries, int32_t channels, int32_t hidden, const float* embeddings,
                                      const float* w_out, const float* b_out, float* A, float* c, misplat_stream_t stream) {
    if (n_queries < 2 || n_queries > kMaxQuery || channels < 1 || channels > kMaxChannels || hidden < 1 || hidden > kMaxHidden ||
        !embeddings || !w_out || !b_out || !A || !c)
        return MISPLAT_EINVAL;
    const int n = n_queries * (hidden + 1);
    hipLaunchKernelGGL(fold_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (int)n_queries, (int)channels, (int)hidden,
                       embeddings, w_out, b_out, A, c);
    return launched();
}

extern "C" int misplat_textquery_map(int32_t height, int32_t width, int32_t latent, int32_t pix_stride, const float* features,
                                     int32_t hidden, const float* w_hidden, const float* b_hidden, int32_t n_queries,
                                     int32_t n_positive, const float* A, const float* c, int32_t method, float softmax_temp,
                                     int32_t work_h, int32_t work_w, float* similarity, misplat_stream_t stream) {
    Query qy;
    if (!make_query(latent, hidden, w_hidden, b_hidden, n_queries, n_positive, A, c, method, softmax_temp, &qy)) return MISPLAT_EINVAL;
    if (height < 1 || width < 1 || (int64_t)height * width > kMaxPixels || pix_stride < latent || work_h < 1 || work_w < 1 ||
        (int64_t)work_h * work_w > kMaxPixels || !features || !similarity)
        return MISPLAT_EINVAL;
    return launch_similarity(qy, height, width, pix_stride, features, work_h, work_w, similarity, (hipStream_t)stream);
}

extern "C" int misplat_textquery_rows(int64_t n_rows, int32_t latent, int32_t row_stride, const float* latents, int32_t hidden,
                                      const float* w_hidden, const float* b_hidden, int32_t n_queries, int32_t n_positive,
                                      const float* A, const float* c, int32_t method, float softmax_temp, float* similarity,
                                      misplat_stream_t stream) {
    Query qy;
    if (!make_query(latent, hidden, w_hidden, b_hidden, n_queries, n_positive, A, c, method, softmax_temp, &qy)) return MISPLAT_EINVAL;
    if (n_rows < 0 || n_rows > kMaxPixels || row_stride < latent) return MISPLAT_EINVAL;
    if (n_rows == 0) return MISPLAT_OK;
    if (!latents || !similarity) return MISPLAT_EINVAL;
    return launch_similarity(qy, (int)n_rows, 1, row_stride, latents, (int)n_rows, 1, similarity, (hipStream_t)stream);
}

extern "C" int misplat_textquery_upsample(int32_t in_h, int32_t in_w, const float* in, int32_t out_h, int32_t out_w, float* out,
                                          misplat_stream_t stream) {
    if (in_h < 1 || in_w < 1 || (int64_t)in_h * in_w > kMaxPixels || out_h < 1 || out_w < 1 || (int64_t)out_h * out_w > kMaxPixels ||
        !in || !out)
        return MISPLAT_EINVAL;
    const size_t P = (size_t)out_h * out_w;
    hipLaunchKernelGGL(upsample_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)in_h, (int)in_w, in,
                       (int)out_h, (int)out_w, out);
    return launched();
}
