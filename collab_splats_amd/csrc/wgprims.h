// wgprims.h -- the workgroup primitives the kernel files share: fp64 sums in a fixed order, integer
// scans and the compaction that follows one, the wave-level helpers of the timed path, the claim loop of the open-addressing
// hashes, and the host helpers that go with them.  The order of the fp64 sums is a contract: the restatements under tests/
// (`_tree256` and its siblings) mirror it, and the results are compared bit for bit.
//
// Everything sits in an unnamed namespace on purpose: each translation unit that includes this header compiles its own
// copy into its own code object (the library is built without relocatable device code).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"

namespace {

// ------------------------------------------------------------------------------------------------- fixed-order sums
// 64 lanes by a shuffle-down tree (32, 16, ... 1): lane 0 holds the sum
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
    return x;
}

// sum over a workgroup of WAVES waves: wave_sum, then the waves in ascending order (((w0 + w1) + w2) + w3 for four).
// Every thread gets the sum; sh[WAVES] may be reused from one call to the next.
template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    __syncthreads();                                  // sh may still be read by a previous call
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh[0];
#pragma unroll
    for (int w = 1; w < WAVES; w++) s += sh[w];
    return s;
}

// K sums at once, in block_sum's order: thread k < K writes out[k].  Once per kernel (the LDS is not guarded for reuse).
template <int K, int WAVES = 4>
__device__ __forceinline__ void block_sums(double (&x)[K], double* out) {
    __shared__ double ws[K][WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; k++) {
        x[k] = wave_sum(x[k]);
        if (lane == 0) ws[k][wave] = x[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double s = ws[threadIdx.x][0];
#pragma unroll
        for (int w = 1; w < WAVES; w++) s += ws[threadIdx.x][w];
        out[threadIdx.x] = s;
    }
}

// The second level, one workgroup of B threads: out[k] = the sum over the nb workgroup partials part[b K + k]; thread t adds
// partials t, t + B, ... in ascending order, then the same tree.
template <int K, int B>
__global__ __launch_bounds__(B) void sum_final_kernel(const double* __restrict__ part, int64_t nb, double* __restrict__ out) {
    double x[K];
#pragma unroll
    for (int k = 0; k < K; k++) x[k] = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += B)
#pragma unroll
        for (int k = 0; k < K; k++) x[k] += part[b * K + k];
    block_sums<K, B / 64>(x, out);
}

// fp32, xor butterfly: every lane gets the sum
__device__ __forceinline__ float wave_sum_xor(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// the integer maximum of 64 lanes, xor butterfly: every lane gets it
__device__ __forceinline__ uint32_t wave_max(uint32_t m) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)m, off);
        m = o > m ? o : m;
    }
    return m;
}

// ------------------------------------------------------------------------------------------------------- wave scans
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_take(uint32_t ident, uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)ident, (int)x, CTRL, ROW_MASK, 0xF, false);
}
// inclusive wave scan: lane i ends with op(x_0 .. x_i); lane 63 holds the wave total
template <class Op>
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t x, uint32_t ident, Op op) {
    x = op(x, dpp_take<0x111, 0xF>(ident, x));      // row_shr:1
    x = op(x, dpp_take<0x112, 0xF>(ident, x));      // row_shr:2
    x = op(x, dpp_take<0x114, 0xF>(ident, x));      // row_shr:4
    x = op(x, dpp_take<0x118, 0xF>(ident, x));      // row_shr:8
    x = op(x, dpp_take<0x142, 0xA>(ident, x));      // row_bcast:15 -> rows 1, 3
    x = op(x, dpp_take<0x143, 0xC>(ident, x));      // row_bcast:31 -> rows 2, 3
    return x;
}

// ------------------------------------------------------------------------------------------------------------ scan
// exclusive scan of one value per thread over a workgroup of WAVES waves; `total` = the workgroup's sum (every thread gets
// it).  wsum[WAVES] may be reused from one call to the next.
template <typename T, int WAVES>
__device__ __forceinline__ T block_scan_excl(T x, T* wsum, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    __syncthreads();                                  // wsum may still be read by a previous call
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) { before += (w < wave) ? wsum[w] : (T)0; total += wsum[w]; }
    return before + incl - x;
}

constexpr int kScanBlock = 1024;

// Exclusive scan by ONE workgroup per row (blockIdx.x selects the row: `stride` elements apart in `in` and `out`, each n
// long), with a carry from one trip of kScanBlock elements to the next: a few thousand block counts.  total (or NULL):
// total[row] = the row's sum.
template <typename In, typename Out>
__global__ __launch_bounds__(kScanBlock) void carry_scan_kernel(const In* __restrict__ in, int64_t n, int64_t stride,
                                                                Out* __restrict__ out, Out* __restrict__ total) {
    __shared__ Out wsum[kScanBlock / 64];
    in += (int64_t)blockIdx.x * stride;
    out += (int64_t)blockIdx.x * stride;
    Out carry = 0;
    for (int64_t b0 = 0; b0 < n; b0 += kScanBlock) {
        const int64_t b = b0 + threadIdx.x;
        Out sum;
        const Out ex = block_scan_excl<Out, kScanBlock / 64>(b < n ? (Out)in[b] : (Out)0, wsum, sum);
        if (b < n) out[b] = carry + ex;
        carry += sum;
    }
    if (total && threadIdx.x == 0) total[blockIdx.x] = carry;
}

// Exclusive scan of n values in three launches: per-block sums, one workgroup over the block sums, per-block scans.
// out[n] = total.  scratch: scan_scratch_bytes(n).  (Templates, scan() included, as every kernel here: a file that includes
// this header and does not scan gets no scan kernel in its code object.)
template <typename T>
__global__ __launch_bounds__(kScanBlock) void scan_reduce_kernel(const T* __restrict__ in, int64_t n, T* __restrict__ bsum) {
    __shared__ T wsum[kScanBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kScanBlock + threadIdx.x;
    T total;
    (void)block_scan_excl<T, kScanBlock / 64>(i < n ? in[i] : (T)0, wsum, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

template <typename T>
__global__ __launch_bounds__(kScanBlock) void scan_down_kernel(const T* __restrict__ in, int64_t n, const T* __restrict__ boff,
                                                               int64_t nb, T* __restrict__ out) {
    __shared__ T wsum[kScanBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kScanBlock + threadIdx.x;
    T total;
    const T ex = block_scan_excl<T, kScanBlock / 64>(i < n ? in[i] : (T)0, wsum, total);
    if (i < n) out[i] = boff[blockIdx.x] + ex;
    if (i == 0) out[n] = boff[nb];
}

constexpr int64_t scan_scratch_bytes(int64_t n) { return 4 * (2 * ((n + kScanBlock - 1) / kScanBlock) + 2); }

template <typename T>
inline void scan(const T* in, int64_t n, T* out, T* scratch, hipStream_t s) {
    static_assert(sizeof(T) == 4, "scan_scratch_bytes counts 4-byte values");
    const int64_t nb = (n + kScanBlock - 1) / kScanBlock;
    if (nb > 0) hipLaunchKernelGGL(scan_reduce_kernel<T>, dim3((unsigned)nb), dim3(kScanBlock), 0, s, in, n, scratch);
    hipLaunchKernelGGL((carry_scan_kernel<T, T>), dim3(1), dim3(kScanBlock), 0, s, (const T*)scratch, nb, nb, scratch + nb,
                       scratch + 2 * nb);
    hipLaunchKernelGGL(scan_down_kernel<T>, dim3((unsigned)(nb > 0 ? nb : 1)), dim3(kScanBlock), 0, s, in, n,
                       (const T*)(scratch + nb), nb, out);
}

// Compaction after a scan: list[pos[i]] = i for the flagged i of 0 .. n - 1, pos the exclusive scan of the flags -- the flagged
// items in ascending order.  cap = the list's length: a caller's wrong count writes nothing beyond it.
template <typename T>
__global__ __launch_bounds__(256) void compact_kernel(const T* __restrict__ flag, const T* __restrict__ pos, int64_t n, int64_t cap,
                                                      T* __restrict__ list) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && flag[i] && pos[i] < cap) list[pos[i]] = (T)i;
}

// ------------------------------------------------------------------------------------------------------ hash claim
constexpr unsigned long long kEmpty = ~0ull;

// The slot of `key` in an open-addressing table (capacity mask + 1, a power of two; kEmpty marks a free slot): linear probing
// from `home`, the first free slot is claimed.  Which slot a key takes depends on the insertion race; the slot is the same
// for every thread that brings the key.
template <typename I>
__device__ __forceinline__ I claim_slot(unsigned long long* __restrict__ keys, I mask, I home, unsigned long long key) {
    I s = home;
    while (true) {
        const unsigned long long prev = atomicCAS(&keys[s], kEmpty, key);
        if (prev == kEmpty || prev == key) return s;
        s = (s + 1) & mask;
    }
}

// ------------------------------------------------------------------------------------------------------------- host
inline int64_t al(int64_t b) { return (b + 255) & ~(int64_t)255; }

// A scratch buffer handed out piece by piece, each piece 256-byte aligned.  A file describes its workspace ONCE, as a function
// that takes its pieces from a Carver: run over the caller's buffer it yields the pointers, run over a null base it yields
// null pointers and, in `o`, the bytes the buffer must have -- the *_workspace entry points return that.
struct Carver {
    char* base;
    int64_t o = 0;
    template <class T>
    T* take(int64_t n) {
        T* p = base ? (T*)(base + o) : nullptr;
        o += al((int64_t)sizeof(T) * n);
        return p;
    }
};

// the scratch of scan() over up to n values
inline int32_t* take_scan(Carver& c, int64_t n) { return c.take<int32_t>(scan_scratch_bytes(n) / 4); }

inline int launched() { return hipGetLastError() == hipSuccess ? MISPLAT_OK : MISPLAT_ELAUNCH; }

inline unsigned blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace
