"""The semantics of csrc/meshfill.hip and collab_splats_amd/meshfill.py restated in numpy, one thread: longest-edge bisection
in rounds (uint32 length bits and mixing, fp32 lengths and midpoints in the kernels' operation order) and membrane fairing
(fp64 neighbour sums in ascending order, fp32 iterates and displacements).  The oracle of tests/test_meshfill_gpu.py;
tests/test_meshfill_host.py checks its own invariants."""
from __future__ import annotations

import numpy as np

import meshclean_restatement as MC

F = np.float32
M32 = np.uint64(0xFFFFFFFF)


def mix32(seed, i, draw):
    """hashmix.h's mix32 on arrays, in uint64 masked to 32 bits after every step."""
    u = np.uint64
    seed, i, draw = (np.asarray(x).astype(u) for x in (seed, i, draw))
    with np.errstate(over="ignore"):                                # (a wrap at 2^64 leaves the low 32 bits what they are)
        x = (seed * u(0x9E3779B1) + i * u(0x85EBCA77) + draw * u(0xC2B2AE3D) + u(0x27D4EB2F)) & M32
    x ^= x >> u(16); x = (x * u(0x85EBCA6B)) & M32; x ^= x >> u(13); x = (x * u(0xC2B2AE35)) & M32; x ^= x >> u(16)
    x = (x + i) & M32
    x ^= x >> u(15); x = (x * u(0x2C1B3C6D)) & M32; x ^= x >> u(12); x = (x * u(0x297A2D39)) & M32; x ^= x >> u(15)
    return x


def edge_length(V, a, b):
    d = V[b] - V[a]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


# ------------------------------------------------------------------------------------------------------ subdivision
class Round:
    """The edges of the current mesh and what a round decides about them (before it is applied)."""

    def __init__(self, V, tri, region, max_len):
        T = len(tri)
        a, b = tri.reshape(-1), tri[:, [1, 2, 0]].reshape(-1)
        face = np.repeat(np.arange(T), 3)
        ok = a != b
        key = (np.minimum(a, b) << 32) | np.maximum(a, b)
        self.key, inv, self.cnt = np.unique(key[ok], return_inverse=True, return_counts=True)
        E = len(self.key)
        self.of_corner = np.full(3 * T, -1, np.int64)
        self.of_corner[ok] = inv
        self.fmin = np.full(E, T, np.int64)
        self.fmax = np.full(E, -1, np.int64)
        np.minimum.at(self.fmin, inv, face[ok])
        np.maximum.at(self.fmax, inv, face[ok])
        self.lo, self.hi = self.key >> 32, self.key & 0xFFFFFFFF
        rep = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])
        self.length = edge_length(V, self.lo, self.hi)
        faces_ok = (self.cnt == 1) | ((self.cnt == 2) & (self.fmin != self.fmax))
        self.splittable = (faces_ok & region[self.fmin] & region[self.fmax] & ~rep[self.fmin] & ~rep[self.fmax]
                           & (self.length > max_len))
        bits = self.length.view(np.uint32)
        mix = mix32(self.lo, self.hi, np.zeros(E, np.int64))
        order = np.lexsort((self.key, mix, ~bits))                  # larger bits, then smaller mix, then smaller key
        self.rank = np.empty(E, np.int64)
        self.rank[order] = np.arange(E)
        corner_rank = np.where((self.of_corner >= 0) & self.splittable[np.maximum(self.of_corner, 0)],
                               self.rank[np.maximum(self.of_corner, 0)], E).reshape(T, 3)
        self.best_corner = np.where(corner_rank.min(1) < E, corner_rank.argmin(1), -1)
        self.best_edge = np.where(self.best_corner >= 0, self.of_corner.reshape(T, 3)[np.arange(T), np.maximum(self.best_corner, 0)], -1)
        e = np.arange(E)
        self.selected = self.splittable & (self.best_edge[np.minimum(self.fmin, T - 1)] == e) & (self.best_edge[np.maximum(self.fmax, 0)] == e)

    def owner_slot(self, e):
        """The (face, corner) slot that numbers edge e: the lowest corner of its smallest face."""
        f = self.fmin[e]
        c = (self.of_corner.reshape(-1, 3)[f] == e[:, None]).argmax(1)
        return 3 * f + c


def subdivide(V, tri, max_edge_len, max_edge_splits=10000, region=None, attributes=(), max_rounds=256, on_round=None):
    """(vertices, triangles int64, attributes, origin int64, n_splits, rounds)."""
    V = np.asarray(V, F).copy()
    tri = np.asarray(tri, np.int64).reshape(-1, 3).copy()
    att = [np.asarray(x, F).copy() for x in attributes]
    region = np.ones(len(tri), bool) if region is None else np.asarray(region, bool).copy()
    origin = np.arange(len(tri), dtype=np.int64)
    max_len = F(max_edge_len)
    n_splits = rounds = 0
    while len(tri) and rounds < max_rounds and n_splits < max_edge_splits:
        R = Round(V, tri, region, max_len)
        sel = np.flatnonzero(R.selected)
        if len(sel) == 0:
            break
        rounds += 1
        left = max_edge_splits - n_splits
        cut = len(sel) > left
        if cut:
            sel = sel[np.argsort(R.rank[sel])][:left]               # the first in priority
        if on_round is not None:
            on_round(R, sel)
        sel = sel[np.argsort(R.owner_slot(sel))]                    # numbered over the (face, corner) slots
        M, T = len(V), len(tri)
        number = np.full(len(R.key), -1, np.int64)
        number[sel] = np.arange(len(sel))
        V = np.concatenate([V, F(0.5) * (V[R.lo[sel]] + V[R.hi[sel]])])
        att = [np.concatenate([x, F(0.5) * (x[R.lo[sel]] + x[R.hi[sel]])]) for x in att]
        split = np.flatnonzero((R.best_edge >= 0) & (number[np.maximum(R.best_edge, 0)] >= 0))      # ascending face index
        c = R.best_corner[split]
        a, b, d = tri[split, c], tri[split, (c + 1) % 3], tri[split, (c + 2) % 3]
        m = M + number[R.best_edge[split]]
        tri[split] = np.stack([a, m, d], 1)
        tri = np.concatenate([tri, np.stack([m, b, d], 1)])
        region = np.concatenate([region, region[split]])
        origin = np.concatenate([origin, origin[split]])
        n_splits += len(sel)
        if cut:
            break
    return V, tri, tuple(att), origin, n_splits, rounds


def splittable_lengths(V, tri, max_edge_len, region=None):
    """The lengths of the edges of (V, tri) that are still splittable (empty when subdivision ran to its end)."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    R = Round(np.asarray(V, F), tri, np.ones(len(tri), bool) if region is None else np.asarray(region, bool), F(max_edge_len))
    return R.length[R.splittable]


# ---------------------------------------------------------------------------------------------------------- fairing
def free_rows(tri, free):
    """(fl [n] the free vertices ascending, nb [n, K] their distinct neighbours ascending (padded with 0), deg [n], patch [n]:
    the patch of every free vertex, patches numbered by smallest vertex)."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    free = np.asarray(free, bool)
    M = len(free)
    fl = np.flatnonzero(free)
    a = np.concatenate([tri.reshape(-1), tri[:, [1, 2, 0]].reshape(-1)])
    b = np.concatenate([tri[:, [1, 2, 0]].reshape(-1), tri.reshape(-1)])
    keep = (a != b) & free[a]
    pairs = np.unique(a[keep] * M + b[keep])                        # by source, then target, every pair once
    src, tgt = pairs // M, pairs % M
    fidx = np.cumsum(free) - 1
    deg = np.bincount(fidx[src], minlength=len(fl))
    start = np.concatenate([[0], np.cumsum(deg)])
    nb = np.zeros((len(fl), int(deg.max()) if len(deg) and len(src) else 0), np.int64)
    nb[fidx[src], np.arange(len(src)) - start[fidx[src]]] = tgt
    uf = MC._UnionFind(len(fl))
    for s, t in zip(fidx[src[free[tgt]]], fidx[tgt[free[tgt]]]):
        uf.unite(int(s), int(t))
    roots = np.array([uf.find(k) for k in range(len(fl))], np.int64)
    patch = np.unique(roots, return_inverse=True)[1] if len(fl) else np.zeros(0, np.int64)
    return fl, nb, deg, patch.astype(np.int64)


def _membrane(X, fl, nb, deg):
    """fp32(sum_j (double) x_j / |N(i)|) per free vertex and channel, the sum in ascending neighbour order; no neighbour:
    unchanged."""
    S = np.zeros((len(fl), X.shape[1]), np.float64)
    for col in range(nb.shape[1]):
        S = np.where((col < deg)[:, None], S + X[nb[:, col]].astype(np.float64), S)
    with np.errstate(all="ignore"):
        Y = (S / deg.astype(np.float64)[:, None]).astype(F)
    return np.where((deg > 0)[:, None], Y, X[fl])


def fair(V, tri, free, tolerance, max_iterations=10000, attributes=()):
    """(vertices, attributes, iterations [P] int32)."""
    X = np.asarray(V, F).copy()
    fl, nb, deg, patch = free_rows(tri, free)
    P = int(patch.max()) + 1 if len(fl) else 0
    iterations = np.zeros(P, np.int32)
    tol_bits = np.array([tolerance], F).view(np.uint32)[0]
    running = np.ones(P, bool)
    n = 0
    while n < max_iterations and running.any():
        n += 1
        Y = _membrane(X, fl, nb, deg)
        move = running[patch]
        with np.errstate(all="ignore"):
            disp = np.abs(Y - X[fl]).view(np.uint32).max(1)
        worst = np.zeros(P, np.uint32)
        np.maximum.at(worst, patch[move], disp[move])
        X[fl[move]] = Y[move]
        stop = running & (worst < tol_bits)
        iterations[stop] = n
        running &= ~stop
    iterations[running] = n
    out = []
    for A in attributes:
        A = np.asarray(A, F).copy()
        for n in range(1, int(iterations.max()) + 1 if P else 1):
            move = n <= iterations[patch]
            A[fl[move]] = _membrane(A, fl, nb, deg)[move]
        out.append(A)
    return X, tuple(out), iterations


def fair_displacements(V, tri, free, n_iterations):
    """[n_iterations, P] uint32: the displacement bits of every patch in iterations 1 .. n_iterations when no patch ever stops.
    Patches share no edge, so up to its stop a patch's column is what fair() compares with the tolerance: a test picks a
    tolerance from it that stops a patch at a chosen count."""
    X = np.asarray(V, F).copy()
    fl, nb, deg, patch = free_rows(tri, free)
    out = np.zeros((n_iterations, int(patch.max()) + 1 if len(fl) else 0), np.uint32)
    for row in out:
        Y = _membrane(X, fl, nb, deg)
        with np.errstate(all="ignore"):
            np.maximum.at(row, patch, np.abs(Y - X[fl]).view(np.uint32).max(1))
        X[fl] = Y
    return out


# --------------------------------------------------------------------------------------------------------- the fill
def fans(V, tri, max_hole_size=3.0, attributes=()):
    """meshclean_restatement.fill_holes with attributes: (vertices, triangles, attributes, n_filled)."""
    V = np.asarray(V, F)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    V2, T2, n_filled = MC.fill_holes(V, tri, max_hole_size)
    if n_filled == 0:
        return V2, T2, tuple(np.asarray(x, F) for x in attributes), 0
    loop, edges, _, perimeter = MC.mesh_holes(V, tri)
    out = []
    for A in attributes:
        A = np.asarray(A, F)
        new = [A[np.unique(edges[loop == l].astype(np.int64))].astype(np.float64).mean(0).astype(F)
               for l in np.flatnonzero(perimeter < max_hole_size)]
        out.append(np.concatenate([A, np.stack(new)]))
    return V2, T2, tuple(out), n_filled


def default_tolerance(max_edge_len):
    return F(1e-3 * float(F(max_edge_len)))


def fill_holes_nicely(V, tri, max_hole_size=3.0, max_edge_len=None, max_edge_splits=10000, tolerance=None, max_iterations=10000,
                      attributes=()):
    """(vertices, triangles, attributes, n_filled, info)."""
    V = np.asarray(V, F)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    M, T = len(V), len(tri)
    V2, T2, A2, n_filled = fans(V, tri, max_hole_size, attributes)
    info = {"n_splits": 0, "rounds": 0, "iterations": np.zeros(0, np.int32), "n_new_vertices": 0}
    if n_filled == 0:
        return V2, T2, A2, 0, info
    if max_edge_len is None:
        max_edge_len = MC.mesh_edge_stats(V, tri)["mean_edge_length"]
    max_edge_len = F(max_edge_len)
    tolerance = default_tolerance(max_edge_len) if tolerance is None else F(tolerance)
    V3, T3, A3, _, n_splits, rounds = subdivide(V2, T2, max_edge_len, max_edge_splits * n_filled, np.arange(len(T2)) >= T, A2)
    V4, A4, iterations = fair(V3, T3, np.arange(len(V3)) >= M, tolerance, max_iterations, A3)
    info.update(n_splits=n_splits, rounds=rounds, iterations=iterations, n_new_vertices=len(V4) - M)
    return V4, T3, A4, n_filled, info
