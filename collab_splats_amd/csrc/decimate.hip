// decimate.hip -- quadric-error mesh simplification: Garland-Heckbert edge collapses in rounds.  A round
// is a fixed sequence of ordinary kernels: list the live faces, build two CSRs by the stable radix sort (vertex -> corners in
// ascending corner index, vertex -> neighbours ascending, one entry per incident face), give every undirected edge its collapse
// target, cost and validity, take two levels of minima of the priority (cost bits, mixed edge key) over the vertices, select
// the edges that are the minimum around both their ends, and (a second call, after the host has read the counts) apply them.
// Selected edges have no end in each other's closed neighbourhood: what they read and write is disjoint.
//
// Semantics: tests/decimate_restatement.py is the oracle, bit for bit.  Compiled with -ffp-contract=off: every fp64 expression
// is evaluated in the written order.  Integer atomics only (minima and counts); every fp64 sum runs in a fixed order.  No
// kernel waits for another: every loop runs over a CSR row, a probe of two rows or a chain of strictly descending indices.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "misplat.h"
#include "internal.h"
#include "wgprims.h"
#include "radixsort.h"
#include "meshadj.h"

namespace {

typedef unsigned long long u64;
constexpr u64 kNone = ~0ull;                  // the priority of what is no valid edge; no valid cost has these bits
constexpr double kDetEps = 1e-10;

// ------------------------------------------------------------------------------------------------------- arithmetic
__device__ __forceinline__ double det3(double a, double b, double c, double d, double e, double f, double g, double h, double i) {
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g);
}

struct V3 { double x, y, z; };

__device__ __forceinline__ V3 load3(const float* __restrict__ P, int32_t v) {
    return V3{(double)P[3 * (int64_t)v], (double)P[3 * (int64_t)v + 1], (double)P[3 * (int64_t)v + 2]};
}
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ double norm(V3 a) { return sqrt(dot(a, a)); }

// acc += w (a, b, c, d)(a, b, c, d)^T, the ten distinct entries row by row
__device__ __forceinline__ void add_plane(double* acc, double a, double b, double c, double d, double w) {
    acc[0] += w * (a * a); acc[1] += w * (a * b); acc[2] += w * (a * c); acc[3] += w * (a * d); acc[4] += w * (b * b);
    acc[5] += w * (b * c); acc[6] += w * (b * d); acc[7] += w * (c * c); acc[8] += w * (c * d); acc[9] += w * (d * d);
}

// the unit normal of face f and |e1 x e2| (twice its area); false for a face without area
__device__ __forceinline__ bool face_plane(const float* __restrict__ P, const int32_t* __restrict__ tri, int64_t f, V3& n, double& len,
                                           V3& p0) {
    p0 = load3(P, tri[3 * f]);
    const V3 c = cross(sub(load3(P, tri[3 * f + 1]), p0), sub(load3(P, tri[3 * f + 2]), p0));
    len = norm(c);
    if (!(len > 0.0)) return false;
    n = V3{c.x / len, c.y / len, c.z / len};
    return true;
}

// v^T Q v of the fp32 point, clamped at 0
__device__ __forceinline__ double quadric_cost(const double* q, float fx, float fy, float fz) {
    const double x = (double)fx, y = (double)fy, z = (double)fz;
    const double t0 = (q[0] * x) * x, t1 = (q[4] * y) * y, t2 = (q[7] * z) * z;
    const double t3 = ((q[1] * x) * y + (q[2] * x) * z) + (q[5] * y) * z;
    const double t4 = (q[3] * x + q[6] * y) + q[8] * z;
    const double c = (((t0 + t1) + t2) + 2.0 * t3) + (2.0 * t4 + q[9]);
    return c > 0.0 ? c : 0.0;
}

// a bijection of the 64-bit edge keys (the finaliser of splitmix64): the tie-break among equal costs.  (Not hashmix.h's mix32,
// a 32-bit hash; and pair_key is not meshedge.h's edge_key, which orders its ends: (a, b) is taken as the entry holds it.)
__device__ __forceinline__ u64 mix_key(u64 k) {
    k ^= k >> 30; k *= 0xBF58476D1CE4E5B9ull;
    k ^= k >> 27; k *= 0x94D049BB133111EBull;
    return k ^ (k >> 31);
}
__device__ __forceinline__ u64 pair_key(int32_t a, int32_t b) { return ((u64)(uint32_t)a << 32) | (uint32_t)b; }

__device__ __forceinline__ bool has(const int32_t* __restrict__ t, int32_t v) { return t[0] == v || t[1] == v || t[2] == v; }

// ------------------------------------------------------------------------------------------------------------ tables
// What a round builds and the apply call reads again (both carve the same workspace).
struct Tables {
    const int32_t *crow, *ccorner;            // vertex v's corners ccorner[crow[2 v] .. crow[2 v + 1]), ascending corner index
    const int32_t *nrow, *nsrc, *ntgt;        // vertex v's neighbours ntgt[nrow[2 v] .. nrow[2 v + 1]), ascending, one per face
};

__global__ __launch_bounds__(256) void live_list_kernel(const int32_t* __restrict__ alive, const int32_t* __restrict__ pos, int64_t T,
                                                        int64_t n, int32_t* __restrict__ lf, int32_t* __restrict__ counts) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f == 0) { counts[0] = pos[T]; counts[1] = 0; counts[2] = 0; }
    if (f < T && alive[f] && pos[f] < n) lf[pos[f]] = (int32_t)f;
}

// the corners of the live faces as (key = vertex, value = corner index), and their directed edges (meshadj.h)
__global__ __launch_bounds__(256) void emit_kernel(const int32_t* __restrict__ tri, const int32_t* __restrict__ lf, int64_t n,
                                                   int32_t* __restrict__ ck, int32_t* __restrict__ cv, int32_t* __restrict__ tgt,
                                                   int32_t* __restrict__ src) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= 3 * n) return;
    const int64_t g = h / 3;
    const int c = (int)(h - 3 * g);
    const int64_t f = lf[g];
    ck[h] = tri[3 * f + c]; cv[h] = (int32_t)(3 * f + c);
    emit_corner_edges(tri, f, c, h, tgt, src);
}

// Per vertex: is it on the boundary (a neighbour met once), its minima reset, and in the first round its quadric: the face
// planes of its corners in ascending corner index, then the boundary planes in ascending neighbour index.
__global__ __launch_bounds__(256) void vertex_kernel(const float* __restrict__ P, int64_t M, const int32_t* __restrict__ tri, Tables tb,
                                                     int first, double* __restrict__ Q, int32_t* __restrict__ vbnd,
                                                     u64* __restrict__ l1c, u64* __restrict__ l1k) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= M) return;
    l1c[v] = kNone;
    l1k[v] = kNone;
    const int32_t c0 = tb.crow[2 * v], c1 = tb.crow[2 * v + 1], s = tb.nrow[2 * v], t = tb.nrow[2 * v + 1];
    double acc[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (first)
        for (int32_t i = c0; i < c1; i++) {
            V3 n, p0;
            double len;
            if (face_plane(P, tri, tb.ccorner[i] / 3, n, len, p0)) add_plane(acc, n.x, n.y, n.z, -dot(n, p0), 0.5 * len);
        }
    int bnd = 0;
    for (int32_t e = s; e < t; e++) {
        const int32_t j = tb.ntgt[e];
        if ((e > s && tb.ntgt[e - 1] == j) || (e + 1 < t && tb.ntgt[e + 1] == j)) continue;
        bnd = 1;
        if (!first) break;
        for (int32_t i = c0; i < c1; i++) {                 // the one face of the edge (v, j)
            const int64_t f = tb.ccorner[i] / 3;
            if (!has(tri + 3 * f, j)) continue;
            V3 n, p0;
            double len;
            if (face_plane(P, tri, f, n, len, p0)) {
                const int32_t lo = (int32_t)v < j ? (int32_t)v : j, hi = (int32_t)v < j ? j : (int32_t)v;
                const V3 pl = load3(P, lo);
                V3 m = cross(sub(load3(P, hi), pl), n);
                const double ml = norm(m);
                if (ml > 0.0) {
                    m = V3{m.x / ml, m.y / ml, m.z / ml};
                    add_plane(acc, m.x, m.y, m.z, -dot(m, pl), 0.5 * len);
                }
            }
            break;
        }
    }
    vbnd[v] = bnd;
    if (first)
        for (int k = 0; k < 10; k++) Q[10 * v + k] = acc[k];
}

// The surviving faces around end u (without the other end o) when u moves to `to`: false if one of them turns over (the dot
// product of its old and new unnormalised normals is not positive) or, with dup_row given (u = a, the row of b's corners), if
// one of them gets the vertex set of a surviving face around b.
__device__ bool end_ok(const float* __restrict__ P, const int32_t* __restrict__ tri, const Tables& tb, int32_t u, int32_t o, V3 to,
                       bool dup) {
    for (int32_t i = tb.crow[2 * (int64_t)u]; i < tb.crow[2 * (int64_t)u + 1]; i++) {
        const int32_t* t = tri + 3 * (int64_t)(tb.ccorner[i] / 3);
        if (has(t, o)) continue;
        V3 p[3], q[3];
        for (int k = 0; k < 3; k++) {
            p[k] = load3(P, t[k]);
            q[k] = t[k] == u ? to : p[k];
        }
        const V3 no = cross(sub(p[1], p[0]), sub(p[2], p[0])), nn = cross(sub(q[1], q[0]), sub(q[2], q[0]));
        if (!(dot(no, nn) > 0.0)) return false;
        if (!dup) continue;
        const int32_t x = t[0] == u ? t[1] : t[0], y = t[2] == u ? t[1] : t[2];          // the two other corners
        for (int32_t j = tb.crow[2 * (int64_t)o]; j < tb.crow[2 * (int64_t)o + 1]; j++) {
            const int32_t* r = tri + 3 * (int64_t)(tb.ccorner[j] / 3);
            if (!has(r, u) && has(r, x) && has(r, y)) return false;
        }
    }
    return true;
}

// One lane per directed entry; the entry that stands for the undirected edge (a, b), a < b, is the first of its run in a's row.
// Writes its incident faces, target and cost bits (kNone unless the edge is valid) and votes the cost into both ends.
__global__ __launch_bounds__(256) void edge_kernel(const float* __restrict__ P, const int32_t* __restrict__ tri, Tables tb, int64_t E,
                                                   const double* __restrict__ Q, const int32_t* __restrict__ vbnd,
                                                   u64* __restrict__ ebits, float* __restrict__ etgt, int32_t* __restrict__ efaces,
                                                   u64* __restrict__ l1c) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    ebits[e] = kNone;
    efaces[e] = 0;
    const int32_t a = tb.nsrc[e], b = tb.ntgt[e];
    const int32_t a0 = tb.nrow[2 * (int64_t)a], a1 = tb.nrow[2 * (int64_t)a + 1];
    if (b <= a || (e > a0 && tb.ntgt[e - 1] == b)) return;
    int32_t faces = 1;
    while (e + faces < a1 && tb.ntgt[e + faces] == b) faces++;
    efaces[e] = faces;
    if (faces > 2) return;                                                       // (1)
    if (faces == 2 && vbnd[a] && vbnd[b]) return;                                // (3)
    int32_t i = a0, j = tb.nrow[2 * (int64_t)b], common = 0;                     // (2) the distinct common neighbours
    const int32_t b1 = tb.nrow[2 * (int64_t)b + 1];
    while (i < a1 && j < b1) {
        const int32_t x = tb.ntgt[i], y = tb.ntgt[j];
        if (x < y) i++;
        else if (y < x) j++;
        else {
            common++;
            while (i < a1 && tb.ntgt[i] == x) i++;
            while (j < b1 && tb.ntgt[j] == x) j++;
        }
    }
    if (common != faces) return;
    double q[10];
    for (int k = 0; k < 10; k++) q[k] = Q[10 * (int64_t)a + k] + Q[10 * (int64_t)b + k];
    const double r0 = -q[3], r1 = -q[6], r2 = -q[8];
    const double det = det3(q[0], q[1], q[2], q[1], q[4], q[5], q[2], q[5], q[7]);
    float tx, ty, tz;
    if (fabs(det) > kDetEps) {
        tx = (float)(det3(r0, q[1], q[2], r1, q[4], q[5], r2, q[5], q[7]) / det);
        ty = (float)(det3(q[0], r0, q[2], q[1], r1, q[5], q[2], r2, q[7]) / det);
        tz = (float)(det3(q[0], q[1], r0, q[1], q[4], r1, q[2], q[5], r2) / det);
    } else {                                                                     // the cheapest of p_a, p_b, their midpoint
        const float* pa = P + 3 * (int64_t)a;
        const float* pb = P + 3 * (int64_t)b;
        const float mx = (float)(((double)pa[0] + (double)pb[0]) * 0.5), my = (float)(((double)pa[1] + (double)pb[1]) * 0.5),
                    mz = (float)(((double)pa[2] + (double)pb[2]) * 0.5);
        double best = quadric_cost(q, pa[0], pa[1], pa[2]);
        tx = pa[0]; ty = pa[1]; tz = pa[2];
        const double cb = quadric_cost(q, pb[0], pb[1], pb[2]);
        if (cb < best) { best = cb; tx = pb[0]; ty = pb[1]; tz = pb[2]; }
        const double cm = quadric_cost(q, mx, my, mz);
        if (cm < best) { best = cm; tx = mx; ty = my; tz = mz; }
    }
    etgt[3 * e] = tx; etgt[3 * e + 1] = ty; etgt[3 * e + 2] = tz;
    if (!(isfinite(tx) && isfinite(ty) && isfinite(tz))) return;
    const V3 to{(double)tx, (double)ty, (double)tz};
    if (!end_ok(P, tri, tb, a, b, to, true) || !end_ok(P, tri, tb, b, a, to, false)) return;     // (4), (5)
    const u64 bits = (u64)__double_as_longlong(quadric_cost(q, tx, ty, tz));
    ebits[e] = bits;
    atomicMin(&l1c[a], bits);
    atomicMin(&l1c[b], bits);
}

// level 1, second half: among the edges of a vertex's smallest cost, the smallest mixed key
__global__ __launch_bounds__(256) void vote_key_kernel(Tables tb, int64_t E, const u64* __restrict__ ebits, const u64* __restrict__ l1c,
                                                       u64* __restrict__ l1k) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E || ebits[e] == kNone) return;
    const int32_t a = tb.nsrc[e], b = tb.ntgt[e];
    const u64 tie = mix_key(pair_key(a, b));
    if (ebits[e] == l1c[a]) atomicMin(&l1k[a], tie);
    if (ebits[e] == l1c[b]) atomicMin(&l1k[b], tie);
}

// level 2: the lexicographic minimum of level 1 over a vertex and its neighbours
__global__ __launch_bounds__(256) void level2_kernel(int64_t M, Tables tb, const u64* __restrict__ l1c, const u64* __restrict__ l1k,
                                                     u64* __restrict__ l2c, u64* __restrict__ l2k) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= M) return;
    u64 c = l1c[v], k = l1k[v];
    for (int32_t e = tb.nrow[2 * v]; e < tb.nrow[2 * v + 1]; e++) {
        const int32_t j = tb.ntgt[e];
        const u64 cj = l1c[j], kj = l1k[j];
        if (cj < c || (cj == c && kj < k)) { c = cj; k = kj; }
    }
    l2c[v] = c;
    l2k[v] = k;
}

// sel[e] = the faces the collapse of a selected edge removes, 0 for every other entry; counts[1], counts[2]: edges, faces
__global__ __launch_bounds__(256) void select_kernel(Tables tb, int64_t E, const u64* __restrict__ ebits, const int32_t* __restrict__ efaces,
                                                     const u64* __restrict__ l2c, const u64* __restrict__ l2k, int32_t* __restrict__ sel,
                                                     int32_t* __restrict__ counts) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    int32_t s = 0;
    if (ebits[e] != kNone) {
        const int32_t a = tb.nsrc[e], b = tb.ntgt[e];
        const u64 bits = ebits[e], tie = mix_key(pair_key(a, b));
        if (bits == l2c[a] && tie == l2k[a] && bits == l2c[b] && tie == l2k[b]) s = efaces[e];
    }
    sel[e] = s;
    if (s) {
        atomicAdd(&counts[1], 1);
        atomicAdd(&counts[2], s);
    }
}

// ------------------------------------------------------------------------------------------------------------ landing
__global__ __launch_bounds__(256) void flag_kernel(const int32_t* __restrict__ sel, int64_t E, int32_t* __restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < E) flag[e] = sel[e] ? 1 : 0;
}

__global__ __launch_bounds__(256) void digit_kernel(const u64* __restrict__ ebits, const int32_t* __restrict__ list, int64_t S, int shift,
                                                    int32_t* __restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < S) key[i] = (int32_t)((ebits[list[i]] >> shift) & 0x1fffffull);
}

__global__ __launch_bounds__(256) void removed_kernel(const int32_t* __restrict__ sel, const int32_t* __restrict__ list, int64_t S,
                                                      int32_t* __restrict__ rem) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < S) rem[i] = sel[list[i]];
}

// ------------------------------------------------------------------------------------------------------------ apply
// One lane per entry (list null) or per listed entry with before[i] < need: vertex a takes the target, the mean attributes and
// the sum of the quadrics; b dies into a; b's corners are rewired to a, the faces that held both die.
__global__ __launch_bounds__(256) void apply_kernel(float* __restrict__ P, int32_t* __restrict__ tri, Tables tb, int64_t n,
                                                    const int32_t* __restrict__ sel, const float* __restrict__ etgt,
                                                    const int32_t* __restrict__ list, const int32_t* __restrict__ before, int64_t need,
                                                    float* __restrict__ att, int D, double* __restrict__ Q, int32_t* __restrict__ alive,
                                                    int32_t* __restrict__ into) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t e = list ? list[i] : i;
    if (!sel[e] || (list && (int64_t)before[i] >= need)) return;
    const int32_t a = tb.nsrc[e], b = tb.ntgt[e];
    for (int k = 0; k < 3; k++) P[3 * (int64_t)a + k] = etgt[3 * e + k];
    for (int k = 0; k < D; k++) att[(int64_t)a * D + k] = 0.5f * (att[(int64_t)a * D + k] + att[(int64_t)b * D + k]);
    for (int k = 0; k < 10; k++) Q[10 * (int64_t)a + k] = Q[10 * (int64_t)a + k] + Q[10 * (int64_t)b + k];
    into[b] = a;
    for (int32_t c = tb.crow[2 * (int64_t)b]; c < tb.crow[2 * (int64_t)b + 1]; c++) {
        const int32_t h = tb.ccorner[c];
        const int64_t f = h / 3;
        if (has(tri + 3 * f, a)) alive[f] = 0;
        else tri[h] = a;
    }
}

// into[] points from a dead vertex to the strictly smaller vertex it collapsed into (-1: alive): the chain ends
__global__ __launch_bounds__(256) void resolve_kernel(const int32_t* __restrict__ into, int64_t M, int32_t* __restrict__ root) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= M) return;
    int32_t r = (int32_t)v;
    for (int32_t p = into[r]; p >= 0 && p < r; p = into[r]) r = p;
    root[v] = r;
}

// ------------------------------------------------------------------------------------------------------- workspace
struct Work {
    int32_t *lpos, *lf;
    int32_t *ck, *cv, *ckb, *cvb, *crow;          // the corner sort's two pairs, the rows [2 M]
    int32_t *nk, *nv, *nkb, *nvb, *nrow;          // the neighbour sort's two pairs, the rows [2 M]
    int32_t* vbnd;
    u64 *l1c, *l1k, *l2c, *l2k, *ebits;
    float* etgt;
    int32_t *efaces, *sel, *spos;
    int32_t *sk, *sv, *skb, *svb, *rem, *before;  // the landing sort of the selected edges
    int32_t* scr;
    SortBufs sort;
};

inline int64_t max3(int64_t a, int64_t b, int64_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// M vertices, T face slots, n live faces
inline Work carve(Carver& c, int64_t M, int64_t T, int64_t n) {
    Work W = {};
    const int64_t E = 6 * n;
    W.lpos = c.take<int32_t>(T + 1);
    W.lf = c.take<int32_t>(n);
    W.ck = c.take<int32_t>(3 * n); W.cv = c.take<int32_t>(3 * n); W.ckb = c.take<int32_t>(3 * n); W.cvb = c.take<int32_t>(3 * n);
    W.crow = c.take<int32_t>(2 * M);
    W.nk = c.take<int32_t>(E); W.nv = c.take<int32_t>(E); W.nkb = c.take<int32_t>(E); W.nvb = c.take<int32_t>(E);
    W.nrow = c.take<int32_t>(2 * M);
    W.vbnd = c.take<int32_t>(M);
    W.l1c = c.take<u64>(M); W.l1k = c.take<u64>(M); W.l2c = c.take<u64>(M); W.l2k = c.take<u64>(M);
    W.ebits = c.take<u64>(E);
    W.etgt = c.take<float>(3 * E);
    W.efaces = c.take<int32_t>(E); W.sel = c.take<int32_t>(E); W.spos = c.take<int32_t>(E + 1);
    W.sk = c.take<int32_t>(n); W.sv = c.take<int32_t>(n); W.skb = c.take<int32_t>(n); W.svb = c.take<int32_t>(n);
    W.rem = c.take<int32_t>(n); W.before = c.take<int32_t>(n + 1);
    W.scr = take_scan(c, max3(T, E + 1, 256 * ((E + kTile - 1) / kTile) + 1));
    W.sort = take_sort(c, E);
    return W;
}

inline bool sizes_ok(int64_t M, int64_t T, int64_t n) {
    return M >= 1 && M < (1ll << 31) && T >= 1 && 6 * T < (1ll << 31) - kTile && n >= 1 && n <= T;
}

// the tables of a round: built when `build`, else only named (the apply call reads what the round call built)
inline Tables tables(const Work& W, int64_t M, int64_t n, const int32_t* tri, bool build, hipStream_t s) {
    const int passes = radix_passes(M - 1);
    const int64_t E = 6 * n;
    int32_t *ck = W.ck, *cv = W.cv, *ckb = W.ckb, *cvb = W.cvb, *nk = W.nk, *nv = W.nv, *nkb = W.nkb, *nvb = W.nvb;
    if (build) {
        hipLaunchKernelGGL(emit_kernel, dim3(blocks(3 * n, 256)), dim3(256), 0, s, tri, (const int32_t*)W.lf, n, ck, cv, nk, nv);
        radix_sort(ck, cv, ckb, cvb, 3 * n, passes, sort_for(W.sort, 3 * n), W.scr, s);  // corners by vertex
        sort_directed(nk, nv, nkb, nvb, E, passes, passes, W.sort, W.scr, s);            // nv the sources, nk the targets
        misplat_internal::fill_bytes(W.crow, 8 * (size_t)M, 0u, s);
        misplat_internal::fill_bytes(W.nrow, 8 * (size_t)M, 0u, s);
        hipLaunchKernelGGL(rows_kernel, dim3(blocks(3 * n, 256)), dim3(256), 0, s, (const int32_t*)ck, 3 * n, W.crow);
        hipLaunchKernelGGL(rows_kernel, dim3(blocks(E, 256)), dim3(256), 0, s, (const int32_t*)nv, E, W.nrow);
    } else {
        sorted_names(ck, cv, ckb, cvb, passes);
        sorted_directed_names(nk, nv, nkb, nvb, passes, passes);
    }
    return Tables{W.crow, cv, W.nrow, nv, nk};
}

}  // namespace

extern "C" int64_t misplat_decimate_workspace(int64_t n_vertices, int64_t n_triangles) {
    if (!sizes_ok(n_vertices, n_triangles, n_triangles)) return -1;
    Carver c{nullptr};
    carve(c, n_vertices, n_triangles, n_triangles);
    return c.o;
}

extern "C" int misplat_decimate_round(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                      const int32_t* alive, int64_t n_alive, double* quadrics, int32_t first, void* workspace,
                                      int64_t workspace_bytes, int32_t* counts, misplat_stream_t stream) {
    const int64_t M = n_vertices, T = n_triangles, n = n_alive, E = 6 * n;
    if (!sizes_ok(M, T, n) || !vertices || !triangles || !alive || !quadrics || !workspace || !counts) return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, M, T, n);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    scan(alive, T, W.lpos, W.scr, s);
    misplat_internal::fill_bytes(W.lf, 4 * (size_t)n, 0u, s);           // (a wrong n_alive reads face 0, never beyond the list)
    hipLaunchKernelGGL(live_list_kernel, dim3(blocks(T, 256)), dim3(256), 0, s, alive, (const int32_t*)W.lpos, T, n, W.lf, counts);
    const Tables tb = tables(W, M, n, triangles, true, s);
    hipLaunchKernelGGL(vertex_kernel, dim3(blocks(M, 256)), dim3(256), 0, s, vertices, M, triangles, tb, (int)(first != 0), quadrics,
                       W.vbnd, W.l1c, W.l1k);
    hipLaunchKernelGGL(edge_kernel, dim3(blocks(E, 256)), dim3(256), 0, s, vertices, triangles, tb, E, (const double*)quadrics,
                       (const int32_t*)W.vbnd, W.ebits, W.etgt, W.efaces, W.l1c);
    hipLaunchKernelGGL(vote_key_kernel, dim3(blocks(E, 256)), dim3(256), 0, s, tb, E, (const u64*)W.ebits, (const u64*)W.l1c, W.l1k);
    hipLaunchKernelGGL(level2_kernel, dim3(blocks(M, 256)), dim3(256), 0, s, M, tb, (const u64*)W.l1c, (const u64*)W.l1k, W.l2c, W.l2k);
    hipLaunchKernelGGL(select_kernel, dim3(blocks(E, 256)), dim3(256), 0, s, tb, E, (const u64*)W.ebits, (const int32_t*)W.efaces,
                       (const u64*)W.l2c, (const u64*)W.l2k, W.sel, counts);
    return launched();
}

extern "C" int misplat_decimate_apply(float* vertices, int64_t n_vertices, int32_t* triangles, int64_t n_triangles, int32_t* alive,
                                      int64_t n_alive, float* attributes, int32_t n_channels, double* quadrics, int32_t* into,
                                      int64_t n_selected, int64_t need, void* workspace, int64_t workspace_bytes,
                                      misplat_stream_t stream) {
    const int64_t M = n_vertices, T = n_triangles, n = n_alive, E = 6 * n, S = n_selected;
    const int D = n_channels;
    if (!sizes_ok(M, T, n) || S < 1 || S > n || D < 0 || D > 4096 || M * (int64_t)(D > 3 ? D : 3) >= (1ll << 39) || !vertices ||
        !triangles || !alive || (D > 0 && !attributes) || !quadrics || !into || !workspace)
        return MISPLAT_EINVAL;
    Carver c{(char*)workspace};
    const Work W = carve(c, M, T, n);
    if (workspace_bytes < c.o) return MISPLAT_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const Tables tb = tables(W, M, n, triangles, false, s);
    if (need < 0) {                                                     // every selected edge
        hipLaunchKernelGGL(apply_kernel, dim3(blocks(E, 256)), dim3(256), 0, s, vertices, triangles, tb, E, (const int32_t*)W.sel,
                           (const float*)W.etgt, (const int32_t*)nullptr, (const int32_t*)nullptr, need, attributes, D, quadrics, alive,
                           into);
        return launched();
    }
    // The shortest prefix in ascending (cost bits, edge key) whose removed faces reach `need`: the selected entries in key
    // order, sorted stably by the 63 cost bits in three digits of 21 bits (three 8-bit passes each).
    hipLaunchKernelGGL(flag_kernel, dim3(blocks(E, 256)), dim3(256), 0, s, (const int32_t*)W.sel, E, W.efaces);
    scan(W.efaces, E, W.spos, W.scr, s);
    int32_t *sk = W.sk, *sv = W.sv, *skb = W.skb, *svb = W.svb;
    misplat_internal::fill_bytes(sv, 4 * (size_t)S, 0u, s);             // (a wrong n_selected reads entry 0)
    hipLaunchKernelGGL(compact_kernel<int32_t>, dim3(blocks(E, 256)), dim3(256), 0, s, (const int32_t*)W.sel, (const int32_t*)W.spos, E, S,
                       sv);                                             // (in entry order, which is ascending edge key)
    const SortBufs sb = sort_for(W.sort, S);
    for (int digit = 0; digit < 3; digit++) {
        hipLaunchKernelGGL(digit_kernel, dim3(blocks(S, 256)), dim3(256), 0, s, (const u64*)W.ebits, (const int32_t*)sv, S, 21 * digit, sk);
        radix_sort(sk, sv, skb, svb, S, 3, sb, W.scr, s);
    }
    hipLaunchKernelGGL(removed_kernel, dim3(blocks(S, 256)), dim3(256), 0, s, (const int32_t*)W.sel, (const int32_t*)sv, S, W.rem);
    scan(W.rem, S, W.before, W.scr, s);
    hipLaunchKernelGGL(apply_kernel, dim3(blocks(S, 256)), dim3(256), 0, s, vertices, triangles, tb, S, (const int32_t*)W.sel,
                       (const float*)W.etgt, (const int32_t*)sv, (const int32_t*)W.before, need, attributes, D, quadrics, alive, into);
    return launched();
}

extern "C" int misplat_decimate_resolve(const int32_t* into, int64_t n_vertices, int32_t* root, misplat_stream_t stream) {
    if (n_vertices < 0 || n_vertices >= (1ll << 31) || (n_vertices > 0 && (!into || !root))) return MISPLAT_EINVAL;
    if (n_vertices == 0) return MISPLAT_OK;
    hipLaunchKernelGGL(resolve_kernel, dim3(blocks(n_vertices, 256)), dim3(256), 0, (hipStream_t)stream, into, n_vertices, root);
    return launched();
}
