// meshtri.hip -- minimum-area triangulation of hole loops and Delaunay-like edge flips: what
// fill_holes_nicely starts from in place of the fan, and what it interleaves with subdivision.
//
// Semantics: tests/meshtri_restatement.py is the oracle, bit for bit.  Compiled with -ffp-contract=off: every fp32 and fp64
// expression is evaluated in the written order.  Integer atomics only (the loop's vertex hash in LDS, the edge table, the 64-bit
// minimum that settles two flips wanting one new edge, the count of flips): two runs are bitwise equal.
//
// Triangulation.  order_kernel, one workgroup per loop: the loop's tails go into a hash in LDS, every head finds the edge it
// is the tail of (the successor map), one lane walks the cycle from the smallest vertex and writes the polygon q_0 = p_0, q_i =
// p_{n - i}; a loop that is no simple cycle, too short or too long gets its code and is left to the fan.  dp_kernel, one
// workgroup per loop: the table W[i][j], i < j, of the recurrence by diagonals with a barrier between them, in LDS for the
// loops that fit (two sizes of workgroup) and in the caller's slab for the others -- the same code over another pointer.
// The entry's weight is a template policy: the area sum (section 30), or Liepa's angle-and-area pair (section 31;
// tests/meshsmooth_restatement.py is its oracle), which also needs the rim faces' third corners from order_kernel<true>.
//
// Flips, one round (misplat_meshtri_flip_round): facetable.h's edge table; per corner the fp64 bits of the violation of a
// flippable edge; per face its first flippable edge, selected iff first in its other face too; the selected edges claim their
// new edge in a hash by the minimum of their own keys; the winners rewrite their two faces in place.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"
#include "internal.h"
#include "wgprims.h"
#include "radixsort.h"
#include "hashmix.h"
#include "meshedge.h"
#include "facetable.h"

namespace {

constexpr int kMaxLoop = MISPLAT_MESHTRI_MAX_LOOP;
constexpr int kLdsLoop = MISPLAT_MESHTRI_LDS_LOOP;
constexpr int kSmallLoop = MISPLAT_MESHTRI_SMALL_LOOP;      // loops up to here take a workgroup of 256 and 21 KB of LDS
constexpr int kHash = 2 * kMaxLoop;                         // the order kernel's hash: at most half full
static_assert((kHash & (kHash - 1)) == 0, "the hash is masked");
static_assert(kMaxLoop < 65536, "a split is kept in 16 bits");
static_assert(10 * (kLdsLoop * (kLdsLoop - 1) / 2) + 16 * kLdsLoop <= 160 * 1024, "the table of an LDS loop fits a workgroup's LDS");
constexpr int kAngleLdsLoop = MISPLAT_MESHTRI_ANGLE_LDS_LOOP;   // the angle-and-area weight: 12 B an entry, 28 B a polygon vertex
constexpr int kAngleSteps = MISPLAT_MESHTRI_ANGLE_STEPS;
static_assert(12 * (kAngleLdsLoop * (kAngleLdsLoop - 1) / 2) + 28 * kAngleLdsLoop <= 160 * 1024, "the angle table of an LDS loop fits");
static_assert(12 * ((kAngleLdsLoop + 1) * kAngleLdsLoop / 2) + 28 * (kAngleLdsLoop + 1) > 160 * 1024, "and it is the longest that does");
static_assert(kSmallLoop <= kAngleLdsLoop && kAngleSteps + 1 < 65536, "a badness is kept in 16 bits");

enum { kTriangulated = 0, kNotSimple = 1, kTooShort = 2, kTooLong = 3, kNotFilled = -1 };

// ------------------------------------------------------------------------------------------------------ cycle order
__device__ __forceinline__ uint32_t vertex_home(int32_t v) { return mix32((uint32_t)v, 0u, 0u) & (kHash - 1); }

// RIM: also rim[e0 + i] = o_i, the third corner of the one mesh face that holds the polygon's edge i = (q_i, q_{i+1}) (edge n - 1
// closes the polygon: (q_{n-1}, q_0)), found through the edge table E of the mesh; -1 where the table does not name such a face.
template <bool RIM>
__global__ __launch_bounds__(256) void order_kernel(const int32_t* __restrict__ edges, const int32_t* __restrict__ order,
                                                    const int32_t* __restrict__ offsets, const uint8_t* __restrict__ fill,
                                                    int64_t n_edges, int32_t* __restrict__ code, int32_t* __restrict__ polygon,
                                                    const int32_t* __restrict__ tri, int64_t T, EdgeTable E, int32_t* __restrict__ rim) {
    __shared__ int32_t hk[kHash], hv[kHash];
    __shared__ int32_t tl[kMaxLoop], hd[kMaxLoop], nx[kMaxLoop], seen[kMaxLoop];
    __shared__ int32_t bad, pmin;
    const int64_t l = blockIdx.x;
    const int32_t e0 = offsets[l], n = offsets[l + 1] - e0;
    int32_t c = kTriangulated;                                  // (everything up to the first barrier is uniform)
    if (!fill[l]) c = kNotFilled;
    else if (n < 3) c = kTooShort;
    else if (n > kMaxLoop) c = kTooLong;
    else if (e0 < 0 || (int64_t)e0 + n > n_edges) c = kNotSimple;   // (offsets that do not describe the list: nothing is read)
    if (c != kTriangulated) {
        if (threadIdx.x == 0) code[l] = c;
        return;
    }
    for (int i = threadIdx.x; i < kHash; i += 256) hk[i] = -1;
    for (int i = threadIdx.x; i < n; i += 256) seen[i] = 0;
    if (threadIdx.x == 0) { bad = 0; pmin = INT32_MAX; }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const int64_t e = order[e0 + i];
        const int32_t a = edges[2 * e], b = edges[2 * e + 1];
        tl[i] = a;
        hd[i] = b;
        atomicMin(&pmin, a);
        uint32_t s = vertex_home(a);
        while (true) {
            const int32_t prev = atomicCAS(&hk[s], -1, a);
            if (prev == -1) { hv[s] = i; break; }
            if (prev == a) { atomicOr(&bad, 1); break; }        // a tail twice: pinched
            s = (s + 1) & (kHash - 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const int32_t b = hd[i];
        uint32_t s = vertex_home(b);
        while (hk[s] != -1 && hk[s] != b) s = (s + 1) & (kHash - 1);
        int32_t to = 0;
        if (hk[s] == -1) atomicOr(&bad, 1);                     // a head that is no tail
        else {
            to = hv[s];
            if (atomicExch(&seen[to], 1)) atomicOr(&bad, 1);    // a head twice
        }
        nx[i] = to;
    }
    __syncthreads();
    if (threadIdx.x == 0 && !bad) {
        // tails and heads are the same n distinct vertices: a permutation, and the loop is connected: one cycle of n
        uint32_t s = vertex_home(pmin);
        while (hk[s] != pmin) s = (s + 1) & (kHash - 1);
        int32_t cur = hv[s];
        polygon[e0] = pmin;
        if constexpr (RIM) seen[cur] = n - 1;                   // (seen is free again: the edge p_0 -> p_1 closes the polygon)
        for (int i = 1; i < n; i++) {
            cur = nx[cur];
            polygon[e0 + (n - i)] = tl[cur];
            if constexpr (RIM) seen[cur] = n - 1 - i;           // the edge p_i -> p_{i+1} is (q_{n-i-1}, q_{n-i}) against its run
        }
        if (nx[cur] != hv[s]) bad = 1;                          // (it has not closed after n steps: not one cycle)
    }
    __syncthreads();
    if (threadIdx.x == 0) code[l] = bad ? kNotSimple : kTriangulated;
    if constexpr (RIM) {
        if (bad) return;                                        // (uniform)
        for (int i = threadIdx.x; i < n; i += 256) {
            const int32_t a = tl[i], b = hd[i];
            int32_t o = -1;
            if (a != b) {
                const u64 key = edge_key(a, b);
                u64 s = edge_home(key, E.mask);
                while (E.keys[s] != key && E.keys[s] != kEmpty) s = (s + 1) & E.mask;   // (the table is never full)
                if (E.keys[s] == key) {
                    const int64_t f = E.fmin[s];
                    if (f >= 0 && f < T)
                        for (int c = 0; c < 3; c++)
                            if (tri[3 * f + c] == a && tri[3 * f + (c + 1) % 3] == b) o = tri[3 * f + (c + 2) % 3];
                }
            }
            rim[e0 + seen[i]] = o;
        }
    }
}

// the fp64 vector helpers of the crease weight and of the flips
struct D3 {
    double x, y, z;
};
__device__ __forceinline__ D3 point(const float* __restrict__ V, int32_t v) {
    return D3{(double)V[3 * (int64_t)v], (double)V[3 * (int64_t)v + 1], (double)V[3 * (int64_t)v + 2]};
}
__device__ __forceinline__ D3 sub(const D3& p, const D3& q) { return D3{p.x - q.x, p.y - q.y, p.z - q.z}; }
__device__ __forceinline__ D3 cross(const D3& u, const D3& v) {
    return D3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}
__device__ __forceinline__ double dot(const D3& u, const D3& v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }

// --------------------------------------------------------------------------------------------------------------- DP
// Entry (i, j), i < j < n, of the triangular table, stored one diagonal after another (diagonal d = j - i holds its n - d
// entries by ascending i): the lanes of a diagonal's sweep have neighbouring i, and both entries a candidate reads, (i, k) and
// (k, j), then lie beside their neighbours' on the diagonals k - i and j - k.
__device__ __forceinline__ int tri_index(int n, int i, int j) {
    const int d = j - i;
    return (d - 1) * n - (d - 1) * d / 2 + i;
}

// the fp32 area of (q_i, q_k, q_j) in its written order
__device__ __forceinline__ float tri_area(const float* Q, int i, int k, int j) {
    const float e1x = Q[3 * k] - Q[3 * i], e1y = Q[3 * k + 1] - Q[3 * i + 1], e1z = Q[3 * k + 2] - Q[3 * i + 2];
    const float e2x = Q[3 * j] - Q[3 * i], e2y = Q[3 * j + 1] - Q[3 * i + 1], e2z = Q[3 * j + 2] - Q[3 * i + 2];
    const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    return 0.5f * sqrtf((cx * cx + cy * cy) + cz * cz);
}

// The weight of a table entry as a policy.  AreaWeight: the fp64 area sum alone (section 30).  AngleWeight (section 31): the pair
// (b, a), b the integer badness of the sharpest crease of the entry's faces among themselves and against the rim faces, a the
// same area sum, compared lexicographically; an entry is 8 + 2 + 2 bytes, so its LDS instance holds a shorter loop.
struct AreaWeight {
    static constexpr bool kAngle = false;
    static constexpr int kCap = kLdsLoop;
};
struct AngleWeight {
    static constexpr bool kAngle = true;
    static constexpr int kCap = kAngleLdsLoop;
};

__device__ __forceinline__ D3 lds_point(const float* Q, int i) { return D3{(double)Q[3 * i], (double)Q[3 * i + 1], (double)Q[3 * i + 2]}; }
// the unnormalised fp64 normal of the oriented face (a, b, c)
__device__ __forceinline__ D3 face_normal(const D3& a, const D3& b, const D3& c) { return cross(sub(b, a), sub(c, a)); }
// the badness of the crease between two oriented faces with these normals: 0 flat .. kAngleSteps folded over; a face without a
// normal (a squared length of 0, or a rim corner that is not there: NaN) poisons nothing
__device__ __forceinline__ int crease(const D3& n1, const D3& n2) {
    const double d1 = dot(n1, n1), d2 = dot(n2, n2);
    if (d1 == 0.0 || d2 == 0.0) return 0;
    const double c = dot(n1, n2) / sqrt(d1 * d2);
    const double x = floor((1.0 - c) * 0.5 * (double)kAngleSteps);
    if (!(x > 0.0)) return 0;
    return x > (double)kAngleSteps ? kAngleSteps : (int)x;
}

// One workgroup per loop with lo <= n <= hi.  CAP > 0: the table in LDS (n <= CAP); CAP = 0: in the slab at slab_off[l].
// Diagonal d has n - d entries of d - 1 candidates each: G lanes share an entry (G = 1 while the entries fill the workgroup,
// then the power of two that keeps it filled, at most a wave), each takes every G-th candidate in ascending k with a strict <,
// and a butterfly takes the smaller weight, on equal weights the smaller k: the first minimum in ascending k whatever G is.
template <class WEIGHT, int CAP, int THREADS>
__global__ __launch_bounds__(THREADS) void dp_kernel(const float* __restrict__ V, int64_t M, const int32_t* __restrict__ polygon,
                                                     const int32_t* __restrict__ rim, const int32_t* __restrict__ offsets,
                                                     const int32_t* __restrict__ code, int lo, int hi, double* slabW, uint16_t* slabS,
                                                     uint16_t* slabB, const int64_t* __restrict__ slab_off, int64_t n_entries,
                                                     const int32_t* __restrict__ face_base, int64_t n_faces,
                                                     const int32_t* __restrict__ area_slot, int64_t n_area, int32_t* __restrict__ faces,
                                                     double* __restrict__ area, int32_t* __restrict__ badness) {
    constexpr bool ANGLE = WEIGHT::kAngle;
    constexpr int NQ = CAP ? CAP : kMaxLoop;
    constexpr int NT = CAP ? CAP * (CAP - 1) / 2 : 1;
    __shared__ double Wl[NT];
    __shared__ float Q[3 * NQ];
    __shared__ float Rm[ANGLE ? 3 * NQ : 1];                    // the rim corners o_i
    __shared__ int32_t P[NQ];
    __shared__ uint16_t Sl[NT];
    __shared__ uint16_t Bl[ANGLE ? NT : 1];
    const int64_t l = blockIdx.x;
    if (code[l] != kTriangulated) return;                       // (every return here is uniform)
    const int32_t e0 = offsets[l];
    const int n = offsets[l + 1] - e0;
    if (n < lo || n > hi) return;
    const int64_t fb = face_base[l], as = area_slot[l];
    if (fb < 0 || fb + n - 2 > n_faces || as < 0 || as >= n_area) return;
    double* W;
    uint16_t *S, *B;
    if constexpr (CAP != 0) {
        W = Wl;
        S = Sl;
        B = Bl;
    } else {
        const int64_t off = slab_off[l];
        if (off < 0 || off + (int64_t)n * (n - 1) / 2 > n_entries) return;
        W = slabW + off;
        S = slabS + off;
        B = ANGLE ? slabB + off : nullptr;
    }
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += THREADS) {
        const int32_t v = polygon[e0 + i];
        P[i] = v;
        for (int c = 0; c < 3; c++) Q[3 * i + c] = V[3 * (int64_t)v + c];
        if constexpr (ANGLE) {
            const int32_t o = rim[e0 + i];
            for (int c = 0; c < 3; c++) Rm[3 * i + c] = o >= 0 && o < M ? V[3 * (int64_t)o + c] : __builtin_nanf("");
        }
    }
    for (int i = tid; i < n - 1; i += THREADS) {
        W[tri_index(n, i, i + 1)] = 0.0;
        if constexpr (ANGLE) {
            B[tri_index(n, i, i + 1)] = 0;
            S[tri_index(n, i, i + 1)] = 0;                      // (read beside a rim face's normal, never used)
        }
    }
    __syncthreads();
    for (int d = 2; d < n; d++) {                               // (the bounds are the loop's n: every barrier is uniform)
        const int E = n - d;
        int G = 1;
        while (G < 64 && 2 * G * E <= THREADS) G *= 2;
        const int groups = THREADS / G, g = tid & (G - 1);
        for (int base = 0; base < E; base += groups) {
            const int i = base + tid / G, j = i + d;
            double best = __builtin_huge_val();
            int bk = i + 1;
            int bb = kAngleSteps + 1;                           // (no candidate yet: above every badness)
            if (i < E)
                for (int k = i + 1 + g; k < j; k += G) {
                    const int ik = tri_index(n, i, k), kj = tri_index(n, k, j);
                    const double v = (W[ik] + W[kj]) + (double)tri_area(Q, i, k, j);
                    if constexpr (ANGLE) {
                        const D3 pi = lds_point(Q, i), pk = lds_point(Q, k), pj = lds_point(Q, j);
                        const D3 nt = face_normal(pi, pk, pj);
                        const D3 nl = k - i == 1 ? face_normal(pk, pi, lds_point(Rm, i)) : face_normal(pi, lds_point(Q, S[ik]), pk);
                        const D3 nr = j - k == 1 ? face_normal(pj, pk, lds_point(Rm, k)) : face_normal(pk, lds_point(Q, S[kj]), pj);
                        int b = B[ik] > B[kj] ? B[ik] : B[kj];
                        const int bl = crease(nt, nl), br = crease(nt, nr);
                        b = bl > b ? bl : b;
                        b = br > b ? br : b;
                        if (d == n - 1) {                       // the top entry: the rim face of the closing edge
                            const int bc = crease(nt, face_normal(pi, pj, lds_point(Rm, n - 1)));
                            b = bc > b ? bc : b;
                        }
                        if (b < bb || (b == bb && v < best)) { bb = b; best = v; bk = k; }
                    } else {
                        if (v < best) { best = v; bk = k; }
                    }
                }
            for (int off = G >> 1; off > 0; off >>= 1) {
                const double ov = __shfl_xor(best, off);
                const int ok = __shfl_xor(bk, off);
                if constexpr (ANGLE) {
                    const int ob = __shfl_xor(bb, off);
                    if (ob < bb || (ob == bb && (ov < best || (ov == best && ok < bk)))) { bb = ob; best = ov; bk = ok; }
                } else {
                    if (ov < best || (ov == best && ok < bk)) { best = ov; bk = ok; }
                }
            }
            if (i < E && g == 0) {
                W[tri_index(n, i, j)] = best;
                S[tri_index(n, i, j)] = (uint16_t)bk;
                if constexpr (ANGLE) B[tri_index(n, i, j)] = (uint16_t)bb;
            }
        }
        __syncthreads();
    }
    // apex k is the apex of exactly one face of the optimal tree: the node (i, j) whose split is k, found from the root
    for (int k = 1 + tid; k <= n - 2; k += THREADS) {
        int i = 0, j = n - 1;
        for (int step = 0; step < n; step++) {
            const int s = S[tri_index(n, i, j)];
            if (s == k || s <= i || s >= j) break;              // (a split outside its interval cannot be: no endless descent)
            if (k < s) j = s; else i = s;
        }
        int32_t* out = faces + 3 * (fb + k - 1);
        out[0] = P[i]; out[1] = P[k]; out[2] = P[j];
    }
    if (tid == 0) {
        area[as] = W[tri_index(n, 0, n - 1)];
        if constexpr (ANGLE) badness[as] = B[tri_index(n, 0, n - 1)];
    }
}

inline int64_t slab_bytes(int64_t n_entries) { return al(8 * n_entries) + al(2 * n_entries); }
inline int64_t angle_slab_bytes(int64_t n_entries) { return slab_bytes(n_entries) + al(2 * n_entries); }

// the three instances of one weight: the small workgroup, the LDS table, the table in the slab
template <class WEIGHT>
inline void launch_dp(int paths, int64_t L, hipStream_t s, const float* vertices, int64_t M, const int32_t* polygon, const int32_t* rim,
                      const int32_t* offsets, const int32_t* code, void* workspace, const int64_t* slab_offset, int64_t n_entries,
                      const int32_t* face_base, int64_t n_faces, const int32_t* area_slot, int64_t n_area, int32_t* faces, double* area,
                      int32_t* badness) {
    constexpr int CAP = WEIGHT::kCap;
    double* slabW = nullptr;
    uint16_t *slabS = nullptr, *slabB = nullptr;
    if (paths & 4) {
        slabW = (double*)workspace;
        slabS = (uint16_t*)((char*)workspace + al(8 * n_entries));
        slabB = (uint16_t*)((char*)workspace + slab_bytes(n_entries));      // (the angle weight's slab alone reaches this far)
    }
    if (paths & 1)
        hipLaunchKernelGGL((dp_kernel<WEIGHT, kSmallLoop, 256>), dim3((unsigned)L), dim3(256), 0, s, vertices, M, polygon, rim, offsets,
                           code, 3, kSmallLoop, nullptr, nullptr, nullptr, nullptr, 0, face_base, n_faces, area_slot, n_area, faces, area,
                           badness);
    if (paths & 2)
        hipLaunchKernelGGL((dp_kernel<WEIGHT, CAP, 1024>), dim3((unsigned)L), dim3(1024), 0, s, vertices, M, polygon, rim, offsets, code,
                           kSmallLoop + 1, CAP, nullptr, nullptr, nullptr, nullptr, 0, face_base, n_faces, area_slot, n_area, faces, area,
                           badness);
    if (paths & 4)
        hipLaunchKernelGGL((dp_kernel<WEIGHT, 0, 1024>), dim3((unsigned)L), dim3(1024), 0, s, vertices, M, polygon, rim, offsets, code,
                           CAP + 1, kMaxLoop, slabW, slabS, slabB, slab_offset, n_entries, face_base, n_faces, area_slot, n_area, faces,
                           area, badness);
}

// ------------------------------------------------------------------------------------------------------------ flips
struct Quad {
    int32_t a, b, c, d;                                         // f_min = (a, b, c) rotated, f_max holds b -> a and d
};

// the two faces of edge `key` as a quad; false where f_max does not run the edge the other way
__device__ __forceinline__ bool quad_of(const int32_t* __restrict__ tri, int32_t f0, int32_t f1, u64 key, Quad& q) {
    int c0 = -1;
    for (int c = 0; c < 3; c++) {
        int32_t x, y;
        corner_edge(tri, f0, c, x, y);
        if (c0 < 0 && x != y && edge_key(x, y) == key) c0 = c;
    }
    if (c0 < 0) return false;
    q.a = tri[3 * (int64_t)f0 + c0];
    q.b = tri[3 * (int64_t)f0 + (c0 + 1) % 3];
    q.c = tri[3 * (int64_t)f0 + (c0 + 2) % 3];
    for (int c = 0; c < 3; c++) {
        int32_t x, y;
        corner_edge(tri, f1, c, x, y);
        if (x == q.b && y == q.a) {
            q.d = tri[3 * (int64_t)f1 + (c + 2) % 3];
            return true;
        }
    }
    return false;
}

// the cotangent of the angle at p between p -> s and p -> t
__device__ __forceinline__ double cotangent(const D3& p, const D3& s, const D3& t) {
    const D3 u = sub(s, p), v = sub(t, p), n = cross(u, v);
    return dot(u, v) / sqrt(dot(n, n));
}

// the violation -(cot c + cot d) of the quad's edge if flipping it is allowed geometrically, else 0
__device__ __forceinline__ double violation(const float* __restrict__ V, const Quad& q, double min_violation) {
    const D3 pa = point(V, q.a), pb = point(V, q.b), pc = point(V, q.c), pd = point(V, q.d);
    const double sum = cotangent(pc, pa, pb) + cotangent(pd, pa, pb);
    if (!(sum < -min_violation)) return 0.0;
    const D3 n1 = cross(sub(pb, pa), sub(pc, pa)), n2 = cross(sub(pa, pb), sub(pd, pb));
    const D3 N{n1.x + n2.x, n1.y + n2.y, n1.z + n2.z};
    const D3 m1 = cross(sub(pd, pa), sub(pc, pa)), m2 = cross(sub(pb, pd), sub(pc, pd));    // the new faces (a, d, c), (d, b, c)
    if (!(dot(m1, N) > 0.0 && dot(m2, N) > 0.0)) return 0.0;
    return -sum;
}

// vbits[h] = the fp64 bits of the violation of corner h's edge if it is flippable, else 0
__global__ __launch_bounds__(256) void flippable_kernel(const float* __restrict__ V, const int32_t* __restrict__ tri, int64_t T,
                                                        const uint8_t* __restrict__ region, EdgeTable E, double min_violation,
                                                        u64* __restrict__ vbits) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= 3 * T) return;
    const int64_t f = h / 3;
    int32_t a, b;
    corner_edge(tri, f, (int)(h - 3 * f), a, b);
    u64 bits = 0;
    if (a != b) {
        const u64 key = edge_key(a, b);
        const int64_t s = edge_find(E, key);
        const int32_t n = E.cnt[s], f0 = E.fmin[s], f1 = E.fmax[s];
        Quad q;
        if (n == 2 && f0 != f1 && region[f0] && region[f1] && !repeated(tri, f0) && !repeated(tri, f1) && quad_of(tri, f0, f1, key, q) &&
            q.c != q.d && !edge_present(E, edge_key(q.c, q.d))) {
            const double v = violation(V, q, min_violation);
            if (v > 0.0) bits = (u64)__double_as_longlong(v);
        }
    }
    vbits[h] = bits;
}

// every selected edge (at the face that owns it) claims its new edge (c, d): the smallest key among the claimants stays
__global__ __launch_bounds__(256) void claim_kernel(const int32_t* __restrict__ tri, int64_t T, EdgeTable E,
                                                    const int32_t* __restrict__ owner, u64* __restrict__ ckeys, u64* __restrict__ cval,
                                                    u64 cmask) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= T || owner[f] < 0 || owner[f] / 3 != (int32_t)f) return;
    int32_t a, b;
    corner_edge(tri, f, owner[f] - 3 * (int32_t)f, a, b);
    const u64 key = edge_key(a, b);
    const int64_t s = edge_find(E, key);
    Quad q;
    if (!quad_of(tri, E.fmin[s], E.fmax[s], key, q)) return;
    const u64 nk = edge_key(q.c, q.d);
    const u64 slot = claim_slot(ckeys, cmask, edge_home(nk, cmask), nk);
    atomicMin(&cval[slot], key);
}

// the winners rewrite their two faces: f_min <- (a, d, c), f_max <- (d, b, c); counts[0] = their number
__global__ __launch_bounds__(256) void flip_kernel(int32_t* __restrict__ tri, int64_t T, EdgeTable E, const int32_t* __restrict__ owner,
                                                   const u64* __restrict__ ckeys, const u64* __restrict__ cval, u64 cmask,
                                                   int32_t* __restrict__ counts) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= T || owner[f] < 0 || owner[f] / 3 != (int32_t)f) return;
    int32_t a, b;
    corner_edge(tri, f, owner[f] - 3 * (int32_t)f, a, b);
    const u64 key = edge_key(a, b);
    const int64_t s = edge_find(E, key);
    const int32_t f0 = E.fmin[s], f1 = E.fmax[s];
    Quad q;
    if (!quad_of(tri, f0, f1, key, q)) return;
    const u64 nk = edge_key(q.c, q.d);
    u64 slot = edge_home(nk, cmask);
    while (ckeys[slot] != nk) {
        if (ckeys[slot] == kEmpty) return;                      // (never: the claim kernel put it there)
        slot = (slot + 1) & cmask;
    }
    if (cval[slot] != key) return;
    tri[3 * (int64_t)f0] = q.a; tri[3 * (int64_t)f0 + 1] = q.d; tri[3 * (int64_t)f0 + 2] = q.c;
    tri[3 * (int64_t)f1] = q.d; tri[3 * (int64_t)f1 + 1] = q.b; tri[3 * (int64_t)f1 + 2] = q.c;
    atomicAdd(&counts[0], 1);
}

struct FlipWork {
    EdgeTable edges;
    int64_t ccap;
    u64 *vbits, *ckeys, *cval;
    int32_t *best, *owner, *fsel, *flag;
};

inline FlipWork carve_flip(Carver& c, int64_t T) {
    FlipWork W = {};
    W.ccap = 64;
    while (W.ccap < 2 * T) W.ccap <<= 1;                        // (selected edges share no face: at most T / 2 claims)
    W.edges = take_edge_table(c, T);
    W.vbits = c.take<u64>(3 * T);
    W.best = c.take<int32_t>(T);
    W.owner = c.take<int32_t>(T);
    W.fsel = c.take<int32_t>(T);
    W.flag = c.take<int32_t>(3 * T);
    W.ckeys = c.take<u64>(W.ccap);
    W.cval = c.take<u64>(W.ccap);
    return W;
}

inline bool flip_ok(int64_t M, int64_t T) { return M >= 1 && M < (1ll << 31) && T >= 1 && 6 * T < (1ll << 31) - kTile; }

}  // namespace

extern "C" int misplat_meshtri_order(const int32_t* edges, const int32_t* order, const int32_t* offsets, const uint8_t* fill,
                                     int64_t n_edges, int64_t n_loops, int32_t* code, int32_t* polygon, misplat_stream_t stream) {
    if (n_edges < 1 || n_edges >= (1ll << 31) || n_loops < 1 || n_loops > n_edges || !edges || !order || !offsets || !fill || !code ||
        !polygon)
        return MISPLAT_EINVAL;
    hipLaunchKernelGGL(order_kernel<false>, dim3((unsigned)n_loops), dim3(256), 0, (hipStream_t)stream, edges, order, offsets, fill,
                       n_edges, code, polygon, (const int32_t*)nullptr, (int64_t)0, EdgeTable{}, (int32_t*)nullptr);
    return launched();
}

extern "C" int64_t misplat_meshtri_rim_workspace(int64_t n_triangles) {
    if (n_triangles < 1 || 6 * n_triangles >= (1ll << 31) - kTile) return -1;
    Carver c{nullptr};
    take_edge_table(c, n_triangles);
    return c.o;
}

extern "C" int misplat_meshtri_order_rim(const int32_t* edges, const int32_t* order, const int32_t* offsets, const uint8_t* fill,
                                         int64_t n_edges, int64_t n_loops, const int32_t* triangles, int64_t n_triangles,
                                         void* workspace, int64_t workspace_bytes, int32_t* code, int32_t* polygon, int32_t* rim,
                                         misplat_stream_t stream) {
    const int64_t T = n_triangles;
    if (n_edges < 1 || n_edges >= (1ll << 31) || n_loops < 1 || n_loops > n_edges || T < 1 || 6 * T >= (1ll << 31) - kTile || !edges ||
        !order || !offsets || !fill || !triangles || !workspace || !code || !polygon || !rim)
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const EdgeTable E = take_edge_table(c, T);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    build_edge_table(triangles, T, E, s);
    hipLaunchKernelGGL(order_kernel<true>, dim3((unsigned)n_loops), dim3(256), 0, s, edges, order, offsets, fill, n_edges, code, polygon,
                       triangles, T, E, rim);
    return launched();
}

extern "C" int64_t misplat_meshtri_workspace(int64_t n_entries) {
    if (n_entries < 0 || n_entries >= (1ll << 40)) return -1;
    return slab_bytes(n_entries);
}

extern "C" int misplat_meshtri_dp(const float* vertices, int64_t n_vertices, const int32_t* polygon, const int32_t* offsets,
                                  const int32_t* code, int64_t n_loops, int32_t paths, const int64_t* slab_offset, int64_t n_entries,
                                  void* workspace, int64_t workspace_bytes, const int32_t* face_base, int64_t n_faces,
                                  const int32_t* area_slot, int64_t n_area, int32_t* faces, double* area, misplat_stream_t stream) {
    const int64_t L = n_loops;
    if (n_vertices < 1 || n_vertices >= (1ll << 31) || L < 1 || L >= (1ll << 31) || paths < 1 || paths > 7 || n_entries < 0 ||
        n_entries >= (1ll << 40) || n_faces < 1 || n_area < 1 || !vertices || !polygon || !offsets || !code || !face_base || !area_slot ||
        !faces || !area || ((paths & 4) && (!slab_offset || !workspace)))
        return MISPLAT_EINVAL;
    if ((paths & 4) && workspace_bytes < slab_bytes(n_entries)) return MISPLAT_EWORKSPACE;
    launch_dp<AreaWeight>(paths, L, (hipStream_t)stream, vertices, n_vertices, polygon, nullptr, offsets, code, workspace, slab_offset,
                          n_entries, face_base, n_faces, area_slot, n_area, faces, area, nullptr);
    return launched();
}

extern "C" int64_t misplat_meshtri_angle_workspace(int64_t n_entries) {
    if (n_entries < 0 || n_entries >= (1ll << 40)) return -1;
    return angle_slab_bytes(n_entries);
}

extern "C" int misplat_meshtri_angle_dp(const float* vertices, int64_t n_vertices, const int32_t* polygon, const int32_t* rim,
                                        const int32_t* offsets, const int32_t* code, int64_t n_loops, int32_t paths,
                                        const int64_t* slab_offset, int64_t n_entries, void* workspace, int64_t workspace_bytes,
                                        const int32_t* face_base, int64_t n_faces, const int32_t* area_slot, int64_t n_area,
                                        int32_t* faces, double* area, int32_t* badness, misplat_stream_t stream) {
    const int64_t L = n_loops;
    if (n_vertices < 1 || n_vertices >= (1ll << 31) || L < 1 || L >= (1ll << 31) || paths < 1 || paths > 7 || n_entries < 0 ||
        n_entries >= (1ll << 40) || n_faces < 1 || n_area < 1 || !vertices || !polygon || !rim || !offsets || !code || !face_base ||
        !area_slot || !faces || !area || !badness || ((paths & 4) && (!slab_offset || !workspace)))
        return MISPLAT_EINVAL;
    if ((paths & 4) && workspace_bytes < angle_slab_bytes(n_entries)) return MISPLAT_EWORKSPACE;
    launch_dp<AngleWeight>(paths, L, (hipStream_t)stream, vertices, n_vertices, polygon, rim, offsets, code, workspace, slab_offset,
                           n_entries, face_base, n_faces, area_slot, n_area, faces, area, badness);
    return launched();
}

extern "C" int64_t misplat_meshtri_flip_workspace(int64_t n_vertices, int64_t n_triangles) {
    if (!flip_ok(n_vertices, n_triangles)) return -1;
    Carver c{nullptr};
    carve_flip(c, n_triangles);
    return c.o;
}

extern "C" int misplat_meshtri_flip_round(const float* vertices, int64_t n_vertices, int32_t* triangles, int64_t n_triangles,
                                          const uint8_t* region, double min_violation, void* workspace, int64_t workspace_bytes,
                                          int32_t* counts, misplat_stream_t stream) {
    const int64_t M = n_vertices, T = n_triangles;
    if (!flip_ok(M, T) || !(min_violation >= 0.0) || !vertices || !triangles || !region || !workspace || !counts) return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const FlipWork W = carve_flip(c, T);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const unsigned nh = blocks(3 * T, 256), nf = blocks(T, 256);
    const EdgeTable& E = W.edges;
    build_edge_table(triangles, T, E, s);
    hipLaunchKernelGGL(flippable_kernel, dim3(nh), dim3(256), 0, s, vertices, (const int32_t*)triangles, T, region, E, min_violation,
                       W.vbits);
    hipLaunchKernelGGL(face_best_kernel<u64>, dim3(nf), dim3(256), 0, s, (const int32_t*)triangles, T, (const u64*)W.vbits, W.best);
    hipLaunchKernelGGL(select_kernel, dim3(nf), dim3(256), 0, s, (const int32_t*)triangles, T, E, (const int32_t*)W.best, W.owner, W.fsel,
                       W.flag);
    misplat_internal::fill_bytes(W.ckeys, 8 * W.ccap, 0xffffffffu, s);
    misplat_internal::fill_bytes(W.cval, 8 * W.ccap, 0xffffffffu, s);
    misplat_internal::fill_bytes(counts, 4, 0u, s);
    const u64 cmask = (u64)(W.ccap - 1);
    hipLaunchKernelGGL(claim_kernel, dim3(nf), dim3(256), 0, s, (const int32_t*)triangles, T, E, (const int32_t*)W.owner, W.ckeys, W.cval,
                       cmask);
    hipLaunchKernelGGL(flip_kernel, dim3(nf), dim3(256), 0, s, triangles, T, E, (const int32_t*)W.owner, (const u64*)W.ckeys,
                       (const u64*)W.cval, cmask, counts);
    return launched();
}
