"""The semantics of DESIGN.md section 31 restated in numpy, one thread.  The angle-and-area weight of csrc/meshtri.hip
(``triangulate_holes(metric="angle_area")``): Liepa's recurrence over pairs (b, a), b the quantised badness of the sharpest
crease, a the fp64 area sum of tests/meshtri_restatement.py, the table filled one diagonal at a time.  The curvature fairing
of csrc/meshfill.hip (``fair_vertices_curvature``): the patches, three independent conjugate-gradient solves per patch on the
thin-plate system of the umbrella operator with every sum in the kernel's order, and beside it a dense assembly of the same
system for ``numpy.linalg.solve``.  The fill that uses both.  The oracle of tests/test_meshsmooth_gpu.py;
tests/test_meshsmooth_host.py checks its own invariants."""
from __future__ import annotations

import numpy as np

import meshclean_restatement as MC
import meshtri_restatement as MT

F = np.float32
ANGLE_STEPS = 1024                      # MISPLAT_MESHTRI_ANGLE_STEPS (tests/test_meshsmooth_host.py keeps the mirrors equal)
ANGLE_LDS_LOOP = 163                    # MISPLAT_MESHTRI_ANGLE_LDS_LOOP
SMALL_LOOP = 64                         # MISPLAT_MESHTRI_SMALL_LOOP


# ------------------------------------------------------------------------------------------------------------ creases
def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def face_normal(a, b, c):
    """The unnormalised fp64 normal of the oriented face (a, b, c): the cross product of b - a and c - a."""
    a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
    return _cross(b - a, c - a)


def crease(n1, n2):
    """The integer badness of the crease between two oriented faces with these normals: 0 flat .. ANGLE_STEPS folded over; 0
    where a face has no normal (a squared length of 0) or the value is not a number."""
    with np.errstate(all="ignore"):
        d1, d2 = _dot(n1, n1), _dot(n2, n2)
        c = _dot(n1, n2) / np.sqrt(d1 * d2)
        x = np.floor((1.0 - c) * 0.5 * float(ANGLE_STEPS))
        x = np.where(x > 0.0, np.minimum(x, float(ANGLE_STEPS)), 0.0)
    return np.where((d1 == 0.0) | (d2 == 0.0), 0.0, x).astype(np.int64)


def rim_corners(tri, q):
    """o_i for the polygon q of a loop: the third corner of the one face of ``tri`` that holds the boundary edge q_{i+1} -> q_i
    (i = n - 1: q_0 -> q_{n-1}); -1 where no face runs that way."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    third = {}
    for c in range(3):
        for a, b, o in zip(tri[:, c].tolist(), tri[:, (c + 1) % 3].tolist(), tri[:, (c + 2) % 3].tolist()):
            third.setdefault((a, b), o)
    n = len(q)
    return np.array([third.get((int(q[(i + 1) % n]), int(q[i])), -1) for i in range(n)], np.int64)


# -------------------------------------------------------------------------------------------------------- the table
def angle_area_table(Q, R):
    """(B [n,n] int64, W [n,n] fp64, S [n,n] int64) of the recurrence over the polygon Q [n,3] fp32 with rim corners R [n,3]
    fp32 (NaN rows: no corner).  Candidate k of (i, j): a = (W[i][k] + W[k][j]) + (double) A(i,k,j); b = max(B[i][k], B[k][j],
    crease(T, left), crease(T, right)), for (0, n - 1) also crease(T, (q_0, q_{n-1}, o_{n-1})); the first minimum of (b, a) in
    ascending k."""
    Q, R = np.asarray(Q, F), np.asarray(R, F)
    n = len(Q)
    B = np.zeros((n, n), np.int64)
    W = np.zeros((n, n), np.float64)
    S = np.zeros((n, n), np.int64)
    for d in range(2, n):
        i = np.arange(n - d)[:, None]
        j = i + d
        k = i + 1 + np.arange(d - 1)[None, :]
        i2, j2 = np.broadcast_to(i, k.shape), np.broadcast_to(j, k.shape)
        with np.errstate(all="ignore"):
            a = (W[i, k] + W[k, j]) + MT.area(Q, i2, k, j2).astype(np.float64)
            nt = face_normal(Q[i2], Q[k], Q[j2])
            nl = np.where((k - i2 == 1)[..., None], face_normal(Q[k], Q[i2], R[i2]), face_normal(Q[i2], Q[S[i, k]], Q[k]))
            nr = np.where((j2 - k == 1)[..., None], face_normal(Q[j2], Q[k], R[k]), face_normal(Q[k], Q[S[k, j]], Q[j2]))
        b = np.maximum(np.maximum(B[i, k], B[k, j]), np.maximum(crease(nt, nl), crease(nt, nr)))
        if d == n - 1:
            b = np.maximum(b, crease(nt, face_normal(Q[i2], Q[j2], np.broadcast_to(R[n - 1], Q[i2].shape))))
        # the first (b, a) below everything before it, strictly: the smallest b; among those the first smallest a that is
        # below +inf, and the first of them where no a is
        low = b == b.min(1, keepdims=True)
        a_low = np.where(low & (a < np.inf), a, np.inf)
        at = np.where(a_low.min(1) < np.inf, a_low.argmin(1), low.argmax(1))
        rows = np.arange(n - d)
        B[i[:, 0], j[:, 0]] = b[rows, at]
        W[i[:, 0], j[:, 0]] = np.where(a[rows, at] < np.inf, a[rows, at], np.inf)
        S[i[:, 0], j[:, 0]] = i[:, 0] + 1 + at
    return B, W, S


def triangulation_badness(V, tri, faces):
    """The sharpest crease of a patch (``faces`` [m,3], oriented, vertex indices) among its own faces and against the faces of
    ``tri`` across its rim: what a triangulation's top entry holds, computed from the finished faces."""
    V = np.asarray(V, F)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    every = np.concatenate([tri, faces])
    against = {}
    for f, (a, b, c) in enumerate(every.tolist()):
        for x, y in ((a, b), (b, c), (c, a)):
            against[(x, y)] = f
    worst = 0
    for f in range(len(tri), len(every)):
        a, b, c = every[f].tolist()
        for x, y in ((a, b), (b, c), (c, a)):
            g = against.get((y, x))
            if g is not None:
                worst = max(worst, int(crease(face_normal(*V[every[f]]), face_normal(*V[every[g]]))))
    return worst


def triangulate_holes(V, tri, max_hole_size=3.0, attributes=(), metric="area"):
    """(vertices, triangles int64, attributes, n_filled, info); ``metric="area"`` is tests/meshtri_restatement.py's."""
    if metric == "area":
        return MT.triangulate_holes(V, tri, max_hole_size, attributes)
    assert metric == "angle_area"
    V = np.asarray(V, F)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    att = [np.asarray(x, F) for x in attributes]
    info = {"n_triangulated": 0, "n_fans": 0, "area": np.zeros(0, np.float64), "fallback": np.zeros(0, np.int32),
            "badness": np.zeros(0, np.int32)}
    if len(tri) == 0:
        return V, tri, tuple(att), 0, info
    loop, edges, _, perimeter = MC.mesh_holes(V, tri)
    new_v, new_a, new_t, areas, codes, bads = [], [[] for _ in att], [], [], [], []
    for l in np.flatnonzero(perimeter < max_hole_size):
        mine = edges[loop == l].astype(np.int64)
        code, q = MT.loop_polygon(mine)
        codes.append(code)
        if code == MT.TRIANGULATED:
            o = rim_corners(tri, q)
            R = np.where((o >= 0)[:, None], V[np.maximum(o, 0)], F(np.nan)).astype(F)
            B, W, S = angle_area_table(V[q], R)
            new_t += [tuple(q[list(f)]) for f in MT.polygon_faces(S, len(q))]
            areas.append(W[0, len(q) - 1])
            bads.append(B[0, len(q) - 1])
        else:                                                       # fill_holes's fan
            c = len(V) + len(new_v)
            members = np.unique(mine)
            new_v.append(V[members].astype(np.float64).mean(0).astype(F))
            for x, rows in zip(att, new_a):
                rows.append(x[members].astype(np.float64).mean(0).astype(F))
            new_t += [(b, a, c) for a, b in mine]
    if not codes:
        return V, tri, tuple(att), 0, info
    if new_v:
        V = np.concatenate([V, np.stack(new_v)])
        att = [np.concatenate([x, np.stack(rows)]) for x, rows in zip(att, new_a)]
    codes = np.array(codes, np.int32)
    info = {"n_triangulated": int((codes == 0).sum()), "n_fans": int((codes != 0).sum()), "area": np.array(areas, np.float64),
            "fallback": codes, "badness": np.array(bads, np.int32)}
    return V, np.concatenate([tri, np.array(new_t, np.int64).reshape(-1, 3)]), tuple(att), len(codes), info


# ================================================================================================ curvature fairing
CG_VERTICES = 65536                     # MISPLAT_MESHFILL_CG_VERTICES
CG_THREADS = 1024                       # the workgroup of the solve: thread t adds the elements t, t + 1024, ...


def block_dot(a, b):
    """sum a_k b_k in the kernel's order: thread t of 1024 adds its products t, t + 1024, ... in ascending order from 0.0, a
    shuffle-down tree (32, 16, .. 1) inside each wave of 64, then the 16 waves in ascending order."""
    prod = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    rows = -(-len(prod) // CG_THREADS)
    padded = np.zeros(rows * CG_THREADS, np.float64)                # (an added +0.0 changes no bit of a sum that started at +0.0)
    padded[:len(prod)] = prod
    acc = np.zeros(CG_THREADS, np.float64)
    for row in padded.reshape(rows, CG_THREADS):
        acc = acc + row
    x = acc.reshape(CG_THREADS // 64, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):
        x[:, :off] = x[:, :off] + x[:, off:2 * off]
    s = x[0, 0]
    for w in range(1, CG_THREADS // 64):
        s = s + x[w, 0]
    return s


def neighbours(tri, m):
    """N(i) for every vertex: the distinct edge-neighbours in ascending order."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    a = np.concatenate([tri[:, [0, 1, 2]].reshape(-1), tri[:, [1, 2, 0]].reshape(-1)])
    b = np.concatenate([tri[:, [1, 2, 0]].reshape(-1), tri[:, [0, 1, 2]].reshape(-1)])
    keep = a != b
    key = np.unique(a[keep] * m + b[keep])
    src, tgt = key // m, key % m
    start = np.searchsorted(src, np.arange(m + 1))
    return [tgt[start[i]:start[i + 1]] for i in range(m)]


def curvature_patches(tri, free):
    """(N, patches): patches is a list of (F_p, R_p), index arrays in ascending order, numbered by the smallest free vertex.
    Free vertices are connected when they are adjacent or share a neighbour in R (the fixed vertices with a free neighbour)."""
    free = np.asarray(free, bool)
    m = len(free)
    N = neighbours(tri, m)
    parent = np.arange(m)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    in_r = np.zeros(m, bool)
    for i in range(m):
        nf = [j for j in N[i] if free[j]]
        if not nf:
            continue
        if not free[i]:
            in_r[i] = True
        for j in nf:                                                # a row of S and its free neighbours: one patch
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    root = np.array([find(i) for i in range(m)])
    groups = {}
    for i in np.flatnonzero(free):                                  # ascending: a patch is met at its smallest free vertex
        groups.setdefault(root[i], ([], []))[0].append(i)
    for i in np.flatnonzero(in_r):
        groups[root[i]][1].append(i)
    return N, [(np.array(f, np.int64), np.array(r, np.int64)) for f, r in groups.values()]


def _rows(N, rows):
    """The neighbours of `rows` as a padded matrix and its mask, columns in ascending neighbour order."""
    width = max(len(N[i]) for i in rows)
    idx, ok = np.zeros((len(rows), width), np.int64), np.zeros((len(rows), width), bool)
    for a, i in enumerate(rows):
        idx[a, :len(N[i])] = N[i]
        ok[a, :len(N[i])] = True
    return idx, ok


def _gather(idx, ok, val):
    """Per row the sum of val over its neighbours in ascending order, from 0.0 (a masked entry adds +0.0, which changes no bit
    of a sum that started at +0.0)."""
    s = np.zeros((len(idx), 3))
    for d in range(idx.shape[1]):
        s = s + np.where(ok[:, d, None], val[idx[:, d]], 0.0)
    return s


class _Patch:
    """The rows of one patch: S = F then R, with the padded neighbour matrices of S and of F."""

    def __init__(self, N, deg, Fp, Rp, free):
        self.F, self.S = Fp, np.concatenate([Fp, Rp])
        self.idx, self.ok = _rows(N, self.S)
        self.okF = self.ok & free[self.idx]                         # the neighbours that are free
        self.n = deg[self.S].astype(np.float64)[:, None]
        self.free_row = free[self.S][:, None]
        self.m = len(free)

    def umbrella_t(self, val, only_free):
        """(t, t / n) over S as [M,3] arrays: t_i = (sum_j val_j) / n_i - val_i, the sum over the free neighbours only and the
        own value only at free rows when `only_free` (val is then a direction, zero off F)."""
        s = _gather(self.idx, self.okF if only_free else self.ok, val)
        own = np.where(self.free_row, val[self.S], 0.0) if only_free else val[self.S]
        t, tn = np.zeros((self.m, 3)), np.zeros((self.m, 3))
        t[self.S] = s / self.n - own
        tn[self.S] = t[self.S] / self.n
        return t, tn

    def transpose(self, t, tn):
        """q over F: q_i = (sum_j t_j / n_j) - t_i."""
        nf = len(self.F)
        q = np.zeros((self.m, 3))
        q[self.F] = _gather(self.idx[:nf], self.ok[:nf], tn) - t[self.F]
        return q


def fair_curvature(V, tri, free, rtol=1e-6, max_iterations=None):
    """(vertices fp32, info) of fair_vertices_curvature: per patch three independent CGs with one stop, every sum in the
    kernel's order."""
    V = np.asarray(V, F)
    free = np.asarray(free, bool)
    m = len(V)
    N, patches = curvature_patches(tri, free)
    deg = np.array([len(x) for x in N])
    out = V.copy()
    X0 = V.astype(np.float64)
    iters, conv, resid, codes = [], [], [], []
    for Fp, Rp in patches:
        code = 1 if deg[Fp].max() == 0 else 2 if len(Rp) == 0 else 3 if len(Fp) > CG_VERTICES else 0
        codes.append(code)
        if code:
            iters.append(0), conv.append(False), resid.append(0.0)
            continue
        limit = len(Fp) if max_iterations is None else max_iterations
        P = _Patch(N, deg, Fp, Rp, free)
        r = -P.transpose(*P.umbrella_t(X0, False))                  # r0 = -L^T U(x0): the umbrella from every neighbour's position
        x, p = X0.copy(), r.copy()
        rr = np.array([block_dot(r[Fp, c], r[Fp, c]) for c in range(3)])
        rr0 = (rr[0] + rr[1]) + rr[2]
        stop, ratio, it = rr0 == 0.0, 0.0, 0
        while it < limit and not stop:
            q = P.transpose(*P.umbrella_t(p, True))
            pq = np.array([block_dot(p[Fp, c], q[Fp, c]) for c in range(3)])
            with np.errstate(all="ignore"):
                alpha = np.where(pq == 0.0, 0.0, rr / np.where(pq == 0.0, 1.0, pq))
                x[Fp] = x[Fp] + alpha * p[Fp]
                r[Fp] = r[Fp] - alpha * q[Fp]
                new = np.array([block_dot(r[Fp, c], r[Fp, c]) for c in range(3)])
                beta = np.where(pq == 0.0, 0.0, new / np.where(pq == 0.0, 1.0, rr))
                p[Fp] = r[Fp] + beta * p[Fp]
            rr = new
            now = (rr[0] + rr[1]) + rr[2]
            ratio, stop = now / rr0, now <= (rtol * rtol) * rr0
            it += 1
        if it > 0:
            out[Fp] = x[Fp].astype(F)
        iters.append(it), conv.append(bool(stop)), resid.append(float(np.sqrt(ratio)))
    return out, {"iterations": np.array(iters, np.int32), "converged": np.array(conv, bool), "residual": np.array(resid, np.float64),
                 "code": np.array(codes, np.int32)}


def curvature_system(V, tri, Fp, Rp):
    """(A [f,f], b [f,3]) of one patch (every coordinate has the same matrix), assembled densely in fp64: L the rows of S
    and all columns of the umbrella operator, A = L_F^T L_F, b = -L_F^T L_X x_X."""
    V = np.asarray(V, np.float64)
    m = len(V)
    N = neighbours(tri, m)
    Sp = np.concatenate([Fp, Rp])
    L = np.zeros((len(Sp), m))
    for a, i in enumerate(Sp):
        L[a, N[i]] = 1.0 / len(N[i])
        L[a, i] -= 1.0
    LF = L[:, Fp]
    fixed = np.ones(m, bool)
    fixed[Fp] = False
    return LF.T @ LF, -LF.T @ (L[:, fixed] @ V[fixed])


def direct_curvature(V, tri, free):
    """The minimiser by numpy.linalg.solve, per patch with code 0 (fp64 [M,3]; other vertices as they came)."""
    V = np.asarray(V, F)
    out = V.astype(np.float64)
    N, patches = curvature_patches(tri, np.asarray(free, bool))
    deg = np.array([len(x) for x in N])
    for Fp, Rp in patches:
        if deg[Fp].max() == 0 or len(Rp) == 0 or len(Fp) > CG_VERTICES:
            continue
        A, b = curvature_system(V, tri, Fp, Rp)
        out[Fp] = np.linalg.solve(A, b)
    return out


# --------------------------------------------------------------------------------------------------------- the fill
def fill_holes_nicely(V, tri, max_hole_size=3.0, max_edge_len=None, max_edge_splits=10000, tolerance=None, max_iterations=10000,
                      attributes=(), triangulation="fan", flip=False, max_passes=4, metric="area", fairing="membrane"):
    """(vertices, triangles, attributes, n_filled, info): tests/meshtri_restatement.py's fill with the triangulation under
    ``metric`` and, for ``fairing="curvature"``, fair_curvature over the created vertices after the membrane."""
    import meshfill_restatement as MF
    V = np.asarray(V, F)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    M, T = len(V), len(tri)
    info = {"n_splits": 0, "rounds": 0, "iterations": np.zeros(0, np.int32), "n_new_vertices": 0, "n_flips": 0, "flip_rounds": 0,
            "passes": 0, "n_triangulated": 0, "n_fans": 0}
    if fairing == "curvature":
        info.update(curvature_iterations=np.zeros(0, np.int32), curvature_converged=np.zeros(0, bool),
                    curvature_code=np.zeros(0, np.int32))
    n_triangulated = 0
    if triangulation == "min_area":
        V3, T3, A3, n_filled, tinfo = triangulate_holes(V, tri, max_hole_size, attributes, metric)
        n_triangulated = tinfo["n_triangulated"]
    else:
        V3, T3, A3, n_filled = MF.fans(V, tri, max_hole_size, attributes)
    if n_filled == 0:
        return V3, T3, A3, 0, info
    if max_edge_len is None:
        max_edge_len = MC.mesh_edge_stats(V, tri)["mean_edge_length"]
    max_edge_len = F(max_edge_len)
    tolerance = MF.default_tolerance(max_edge_len) if tolerance is None else F(tolerance)
    region = np.arange(len(T3)) >= T
    budget = max_edge_splits * n_filled
    n_splits = rounds = n_flips = flip_rounds = passes = 0
    while True:
        passes += 1
        V3, T3, A3, origin, k, r = MF.subdivide(V3, T3, max_edge_len, budget - n_splits, region, A3)
        n_splits, rounds = n_splits + k, rounds + r
        if not flip:
            break
        region = region[origin]
        T3, k, r = MT.flip_edges(V3, T3, region)
        n_flips, flip_rounds = n_flips + k, flip_rounds + r
        if k == 0 or n_splits >= budget or passes >= max_passes:
            break
    free = np.arange(len(V3)) >= M
    V4, A4, iterations = MF.fair(V3, T3, free, tolerance, max_iterations, A3)
    info.update(n_splits=n_splits, rounds=rounds, iterations=iterations, n_new_vertices=len(V4) - M, n_flips=n_flips,
                flip_rounds=flip_rounds, passes=passes, n_triangulated=n_triangulated, n_fans=n_filled - n_triangulated)
    if fairing == "curvature":
        V4, cinfo = fair_curvature(V4, T3, free)
        info.update(curvature_iterations=cinfo["iterations"], curvature_converged=cinfo["converged"], curvature_code=cinfo["code"])
    return V4, T3, A4, n_filled, info
