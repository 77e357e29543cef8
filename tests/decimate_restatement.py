"""Numpy restatement of csrc/decimate.hip: round-based quadric-error edge collapse.

It is the oracle of tests/test_decimate_gpu.py: positions, triangles, vertex_map, attributes and the number of rounds are
compared for equality.  Everything a kernel computes in fp64 is computed here in fp64 by the same expressions in the same
order (elementwise numpy: one IEEE operation per operator, no contraction), fp32 where the device rounds; every ordered sum is
an explicit loop over "the k-th term of every row".  ``simplify_greedy`` is the plain sequential Garland-Heckbert order (one
collapse at a time, the global minimum) over the same cost and validity functions: the quality yardstick of the host tests.
"""
from __future__ import annotations

import numpy as np

F = np.float32
D = np.float64
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)           # the priority of an invalid edge; no valid cost has these bits
DET_EPS = 1e-10


# ------------------------------------------------------------------------------------------------------- arithmetic
def _det3(a, b, c, d, e, f, g, h, i):
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g)


def _cross(ax, ay, az, bx, by, bz):
    return ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx


def _norm(x, y, z):
    return np.sqrt((x * x + y * y) + z * z)


def _plane_quadric(a, b, c, d, w):
    return np.stack([w * (a * a), w * (a * b), w * (a * c), w * (a * d), w * (b * b), w * (b * c), w * (b * d), w * (c * c),
                     w * (c * d), w * (d * d)], 1)


def _cost(q, v):
    """v^T Q v of the fp32 point v, clamped at 0 (a NaN gives 0)."""
    x, y, z = (v[:, i].astype(D) for i in range(3))
    t0 = (q[:, 0] * x) * x
    t1 = (q[:, 4] * y) * y
    t2 = (q[:, 7] * z) * z
    t3 = ((q[:, 1] * x) * y + (q[:, 2] * x) * z) + (q[:, 5] * y) * z
    t4 = (q[:, 3] * x + q[:, 6] * y) + q[:, 8] * z
    c = (((t0 + t1) + t2) + 2.0 * t3) + (2.0 * t4 + q[:, 9])
    return np.where(c > 0, c, 0.0)


def _mix(k):
    """A bijection of the 64-bit edge keys (the finaliser of splitmix64): the tie-break among equal costs."""
    k = k ^ (k >> np.uint64(30))
    k = k * np.uint64(0xBF58476D1CE4E5B9)
    k = k ^ (k >> np.uint64(27))
    k = k * np.uint64(0x94D049BB133111EB)
    return k ^ (k >> np.uint64(31))


def _expand(start, end):
    """(owner, index): for every i the indices start[i] .. end[i] - 1, i ascending."""
    n = (end - start).astype(np.int64)
    owner = np.repeat(np.arange(len(n)), n)
    first = np.cumsum(n) - n
    return owner, start[owner] + (np.arange(int(n.sum())) - first[owner])


def _ordered_add(Q, rows, values):
    """Q[rows[i]] += values[i] in the order of i inside every row (rows ascending)."""
    if len(rows) == 0:
        return
    first = np.searchsorted(rows, rows)                      # the first entry of each entry's row
    rank = np.arange(len(rows)) - first
    for k in range(int(rank.max()) + 1):
        m = rank == k
        Q[rows[m]] = Q[rows[m]] + values[m]


# ------------------------------------------------------------------------------------------------------------ state
class State:
    def __init__(self, vertices, triangles, attributes=()):
        self.pos = np.ascontiguousarray(vertices, F).copy()
        self.M = len(self.pos)
        self.tri = np.asarray(triangles).astype(np.int64).reshape(-1, 3).copy()
        t = self.tri
        self.alive = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
        self.att = [np.ascontiguousarray(a, F).copy() for a in attributes]
        self.into = np.full(self.M, -1, np.int64)
        self.Q = None

    def n_alive(self):
        return int(self.alive.sum())


class Tables:
    """The two CSRs of a round: corners by vertex (ascending corner index), directed edges by (source, target)."""

    def __init__(self, st):
        M = st.M
        self.lf = np.nonzero(st.alive)[0]
        self.t = t = st.tri[self.lf]
        vert = t.reshape(-1)
        self.corder = np.argsort(vert, kind="stable")           # local corner index 3 g + c, g the position in lf
        self.cvert = vert[self.corder]
        self.crow = np.searchsorted(self.cvert, np.arange(M + 1))
        a, b = vert, t[:, [1, 2, 0]].reshape(-1)
        src, tgt = np.stack([a, b], 1).reshape(-1), np.stack([b, a], 1).reshape(-1)
        face = np.repeat(np.arange(len(t)), 6)
        key = src * M + tgt
        o = np.argsort(key, kind="stable")
        self.ukey, first, self.cnt = np.unique(key[o], return_index=True, return_counts=True)
        self.us, self.ut = self.ukey // M, self.ukey % M
        self.uface = face[o][first]                              # a face of the pair (THE face where cnt == 1)
        self.urow = np.searchsorted(self.us, np.arange(M + 1))
        self.vbnd = np.zeros(M, bool)
        self.vbnd[self.us[self.cnt == 1]] = True


def vertex_quadrics(st, tb):
    P = st.pos.astype(D)
    t = tb.t
    p0, p1, p2 = P[t[:, 0]], P[t[:, 1]], P[t[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    with np.errstate(all="ignore"):
        nx, ny, nz = _cross(e1[:, 0], e1[:, 1], e1[:, 2], e2[:, 0], e2[:, 1], e2[:, 2])
        ln = _norm(nx, ny, nz)
        ok = ln > 0
        a, b, c = nx / ln, ny / ln, nz / ln
        d = -((a * p0[:, 0] + b * p0[:, 1]) + c * p0[:, 2])
        K = np.where(ok[:, None], _plane_quadric(a, b, c, d, 0.5 * ln), 0.0)
        Q = np.zeros((st.M, 10), D)
        _ordered_add(Q, tb.cvert, K[tb.corder // 3])
        # boundary planes: through the edge, perpendicular to its one face, weighted by that face's area
        m = tb.cnt == 1
        v, j, g = tb.us[m], tb.ut[m], tb.uface[m]
        lo, hi = np.minimum(v, j), np.maximum(v, j)
        e = P[hi] - P[lo]
        mx, my, mz = _cross(e[:, 0], e[:, 1], e[:, 2], a[g], b[g], c[g])
        ml = _norm(mx, my, mz)
        ok2 = ok[g] & (ml > 0)
        mx, my, mz = mx / ml, my / ml, mz / ml
        md = -((mx * P[lo, 0] + my * P[lo, 1]) + mz * P[lo, 2])
        B = np.where(ok2[:, None], _plane_quadric(mx, my, mz, md, 0.5 * ln[g]), 0.0)
        _ordered_add(Q, v, B)
    return Q


# ------------------------------------------------------------------------------------------------------- evaluation
class Edges:
    pass


def evaluate(st, tb):
    """Every undirected edge of the live faces in key order: ends, incident faces, target, cost bits, validity."""
    M = st.M
    ev = Edges()
    em = tb.us < tb.ut
    ea, eb, ec = tb.us[em], tb.ut[em], tb.cnt[em]
    ev.a, ev.b, ev.faces = ea, eb, ec
    E = len(ea)
    # (2) link condition: distinct common neighbours == incident faces
    owner, idx = _expand(tb.urow[ea], tb.urow[ea + 1])
    q = eb[owner] * M + tb.ut[idx]
    p = np.minimum(np.searchsorted(tb.ukey, q), max(len(tb.ukey) - 1, 0))
    common = np.bincount(owner[tb.ukey[p] == q], minlength=E) if E else np.zeros(0, np.int64)
    few, link, free = ec <= 2, common == ec, ~((ec == 2) & tb.vbnd[ea] & tb.vbnd[eb])
    valid = few & link & free
    # target and cost
    with np.errstate(all="ignore"):
        Qs = st.Q[ea] + st.Q[eb]
        q0, q1, q2, q3, q4, q5, q6, q7, q8 = (Qs[:, i] for i in range(9))
        r0, r1, r2 = -q3, -q6, -q8
        det = _det3(q0, q1, q2, q1, q4, q5, q2, q5, q7)
        sx = _det3(r0, q1, q2, r1, q4, q5, r2, q5, q7) / det
        sy = _det3(q0, r0, q2, q1, r1, q5, q2, r2, q7) / det
        sz = _det3(q0, q1, r0, q1, q4, r1, q2, q5, r2) / det
        solved = np.abs(det) > DET_EPS
        tsol = np.stack([sx, sy, sz], 1).astype(F)
        pa, pb = st.pos[ea], st.pos[eb]
        pm = ((pa.astype(D) + pb.astype(D)) * 0.5).astype(F)
        ca, cb, cm = _cost(Qs, pa), _cost(Qs, pb), _cost(Qs, pm)
        best, bc = pa.copy(), ca.copy()
        m = cb < bc
        best[m], bc[m] = pb[m], cb[m]
        m = cm < bc
        best[m], bc[m] = pm[m], cm[m]
        target = np.where(solved[:, None], tsol, best)
        cost = _cost(Qs, target)
    finite = np.isfinite(target).all(1)
    valid &= finite
    # (4) no surviving face around an end turns over; (5) no two surviving faces end with the same vertex set
    P = st.pos.astype(D)
    T64 = target.astype(D)
    sets = []
    upright, distinct = np.ones(E, bool), np.ones(E, bool)
    for u, o in ((ea, eb), (eb, ea)):
        owner, idx = _expand(tb.crow[u], tb.crow[u + 1])
        g = tb.corder[idx] // 3
        tv = tb.t[g]
        keep = ~(tv == o[owner][:, None]).any(1)
        owner, tv = owner[keep], tv[keep]
        X = P[tv]                                                   # [k, 3 corners, 3]
        Y = np.where((tv == u[owner][:, None])[:, :, None], T64[owner][:, None, :], X)
        dots = []
        for Z in (X, Y):
            e1, e2 = Z[:, 1] - Z[:, 0], Z[:, 2] - Z[:, 0]
            dots.append(_cross(e1[:, 0], e1[:, 1], e1[:, 2], e2[:, 0], e2[:, 1], e2[:, 2]))
        (ox, oy, oz), (nx, ny, nz) = dots
        dot = (ox * nx + oy * ny) + oz * nz
        upright[owner[~(dot > 0)]] = False
        rest = np.sort(np.where(tv == u[owner][:, None], -1, tv), 1)[:, 1:]      # the two other corners, ascending
        sets.append((owner, (owner * M + rest[:, 0]) * M + rest[:, 1]))
    (oa, ka), (_, kb) = sets
    distinct[oa[np.isin(ka, kb)]] = False
    valid &= upright & distinct
    ev.valid, ev.target = valid, target
    # for the host tests' account of the refusals: rules (1), (2), (3), a finite target, (4), (5), and the target's branch
    ev.rules, ev.solved = (few, link, free, finite, upright, distinct), solved
    ev.bits = np.where(valid, cost.view(np.uint64), NONE)
    ev.key = (ea.astype(np.uint64) << np.uint64(32)) | eb.astype(np.uint64)
    ev.tie = np.where(valid, _mix(ev.key), NONE)
    return ev


def select(st, tb, ev):
    """Two levels of minima of the priority (cost bits, mixed key): the edges that are the minimum around both their ends."""
    M = st.M
    l1c = np.full(M, NONE)
    np.minimum.at(l1c, ev.a, ev.bits)
    np.minimum.at(l1c, ev.b, ev.bits)
    l1k = np.full(M, NONE)
    for end in (ev.a, ev.b):
        m = ev.valid & (ev.bits == l1c[end])
        np.minimum.at(l1k, end[m], ev.tie[m])
    l2c = l1c.copy()
    np.minimum.at(l2c, tb.us, l1c[tb.ut])
    l2k = np.where(l1c == l2c, l1k, NONE)
    m = l1c[tb.ut] == l2c[tb.us]
    np.minimum.at(l2k, tb.us[m], l1k[tb.ut[m]])
    return (ev.valid & (ev.bits == l2c[ev.a]) & (ev.tie == l2k[ev.a]) & (ev.bits == l2c[ev.b]) & (ev.tie == l2k[ev.b]))


def apply(st, tb, ev, chosen):
    a, b = ev.a[chosen], ev.b[chosen]
    st.pos[a] = ev.target[chosen]
    for x in st.att:
        x[a] = F(0.5) * (x[a] + x[b])
    st.Q[a] = st.Q[a] + st.Q[b]
    st.into[b] = a
    rep = np.arange(st.M)
    rep[b] = a
    t = rep[tb.t]
    dead = (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])
    st.tri[tb.lf] = t
    st.alive[tb.lf[dead]] = False


def finish(st, index_dtype=np.int64):
    root = np.arange(st.M)
    while True:
        nxt = st.into[root]
        if not (nxt >= 0).any():
            break
        root = np.where(nxt >= 0, nxt, root)
    t = st.tri[st.alive]
    used = np.zeros(st.M, bool)
    used[t.reshape(-1)] = True
    new = np.cumsum(used) - 1
    vmap = np.where(used[root], new[root], -1).astype(np.int64)
    return st.pos[used], new[t].astype(index_dtype), tuple(x[used] for x in st.att), vmap


# ------------------------------------------------------------------------------------------------------------ drivers
def simplify(vertices, triangles, target_triangles, attributes=(), max_rounds=256, on_round=None):
    """(vertices, triangles, attributes, vertex_map, rounds) of the round-based simplifier.  ``on_round(st, tb, ev, selected,
    applied)`` sees every round before it is applied (a round's selection and what the landing keeps of it); it changes no
    result."""
    st = State(vertices, triangles, attributes)
    rounds = 0
    while rounds < max_rounds:
        n = st.n_alive()
        need = n - target_triangles
        if need <= 0 or n == 0:
            break
        tb = Tables(st)
        if st.Q is None:
            st.Q = vertex_quadrics(st, tb)
        ev = evaluate(st, tb)
        sel = select(st, tb, ev)
        if not sel.any():
            break
        rounds += 1
        selected = sel
        if int(ev.faces[sel].sum()) > need:                         # the last round: the shortest prefix in ascending priority
            ids = np.nonzero(sel)[0]
            ids = ids[np.lexsort((ev.key[ids], ev.bits[ids]))]
            before = np.cumsum(ev.faces[ids]) - ev.faces[ids]
            sel = np.zeros_like(sel)
            sel[ids[before < need]] = True
        if on_round is not None:
            on_round(st, tb, ev, selected, sel)
        apply(st, tb, ev, sel)
    return finish(st, np.asarray(triangles).dtype if np.asarray(triangles).size else np.int64) + (rounds,)


def simplify_greedy(vertices, triangles, target_triangles):
    """Plain Garland-Heckbert: one collapse at a time, the valid edge of the globally smallest priority; the same cost,
    target and validity as ``simplify``.  (vertices, triangles)."""
    st = State(vertices, triangles)
    while st.n_alive() > target_triangles:
        tb = Tables(st)
        if st.Q is None:
            st.Q = vertex_quadrics(st, tb)
        ev = evaluate(st, tb)
        if not ev.valid.any():
            break
        ids = np.nonzero(ev.valid)[0]
        best = ids[np.lexsort((ev.key[ids], ev.bits[ids]))[0]]
        sel = np.zeros(len(ev.a), bool)
        sel[best] = True
        apply(st, tb, ev, sel)
    out = finish(st)
    return out[0], out[1]
