"""Synthetic voxel fields for the marching-cubes tests, and fp64 checks of a mesh that share no code with the restatement
(tests/tsdf_restatement.py) or the kernels: the vertex and colour rule of DESIGN.md section 14.1 per lattice edge, the
directed-edge rule (closed and consistently oriented) and the winding number at voxel centres.  numpy only."""
from __future__ import annotations

import numpy as np

UNIT = 16
NVOX = UNIT ** 3


def block(lo, n):
    """Unit coordinates of the fully allocated n[0] x n[1] x n[2] block starting at lo."""
    return [(lo[0] + x, lo[1] + y, lo[2] + z) for z in range(n[2]) for y in range(n[1]) for x in range(n[0])]


def random_field(units, seed=0, p_neg=0.5, w0=0.0, zeros=0.0, closed=False):
    """{(ux, uy, uz): float32 [5, 4096]} (tsdf, w, r, g, b; voxel i = lx + 16 ly + 256 lz): tsdf = +-uniform[0.05, 1] with
    P(negative) = p_neg; a share ``zeros`` of the voxels is exactly +0.0 and as many are -0.0; a share ``w0`` has weight 0
    (the others an integer weight 1..9); colours are integers 0..255.  closed: the outermost voxel layer of the set's
    bounding box is made positive (magnitudes kept; a zero there gets 0.05), which closes the surface of a full block."""
    units = [tuple(int(c) for c in u) for u in units]
    rng = np.random.default_rng(seed)
    U = np.asarray(units, np.int64)
    glo, ghi = U.min(0) * UNIT, U.max(0) * UNIT + UNIT - 1
    i = np.arange(NVOX)
    local = np.stack([i & 15, (i >> 4) & 15, i >> 8], 1)
    field = {}
    for u in units:
        t = rng.uniform(0.05, 1.0, NVOX).astype(np.float32)
        t = np.where(rng.random(NVOX) < p_neg, -t, t)
        z = rng.random(NVOX)
        t = np.where(z < zeros, np.float32(0.0), np.where(z < 2 * zeros, np.float32(-0.0), t)).astype(np.float32)
        w = rng.integers(1, 10, NVOX).astype(np.float32)
        w[rng.random(NVOX) < w0] = 0.0
        c = rng.integers(0, 256, (3, NVOX)).astype(np.float32)
        if closed:
            g = np.asarray(u, np.int64) * UNIT + local
            shell = np.any((g == glo) | (g == ghi), 1)
            t = np.where(shell, np.maximum(np.abs(t), np.float32(0.05)), t).astype(np.float32)
        field[u] = np.concatenate([t[None], w[None], c]).astype(np.float32)
    return field


class Dense:
    """The field laid out over its bounding box, indexed [x, y, z] (voxel g at g - org)."""

    def __init__(self, field):
        U = np.asarray(sorted(field), np.int64)
        self.org = U.min(0) * UNIT
        shape = tuple((U.max(0) - U.min(0) + 1) * UNIT)
        self.tsdf = np.zeros(shape, np.float32)
        self.w = np.zeros(shape, np.float32)
        self.rgb = np.zeros(shape + (3,), np.float32)
        self.alloc = np.zeros(shape, bool)
        for u, d in field.items():
            o = np.asarray(u, np.int64) * UNIT - self.org
            sl = tuple(slice(int(o[k]), int(o[k]) + UNIT) for k in range(3))
            cube = np.asarray(d, np.float32).reshape(5, UNIT, UNIT, UNIT).transpose(0, 3, 2, 1)      # [plane, x, y, z]
            self.tsdf[sl], self.w[sl], self.alloc[sl] = cube[0], cube[1], True
            self.rgb[sl] = np.moveaxis(cube[2:5], 0, -1)
        self.neg = self.tsdf < 0
        good = self.alloc & (self.w > 0)
        n = [s - 1 for s in shape]
        v = np.ones(tuple(n), bool)
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    v &= good[dx:dx + n[0], dy:dy + n[1], dz:dz + n[2]]
        self.valid = np.zeros(shape, bool)                # cell at voxel g: corners g .. g + 1
        self.valid[:n[0], :n[1], :n[2]] = v

    def cubes(self):
        """Cube index (bit dx + 2 dy + 4 dz set iff that corner has tsdf < 0) of every valid cell."""
        s = self.tsdf.shape
        cube = np.zeros(s, np.int32)
        for c in range(8):
            d = (c & 1, (c >> 1) & 1, (c >> 2) & 1)
            sh = np.zeros(s, bool)
            sh[:s[0] - d[0], :s[1] - d[1], :s[2] - d[2]] = self.neg[d[0]:, d[1]:, d[2]:]
            cube |= sh.astype(np.int32) << c
        return cube[self.valid]

    def edge_held(self, a):
        """[x, y, z] bool: the lattice edge from voxel g to g + e_a lies in a valid cell (one of the up to 4 around it)."""
        b1, b2 = [k for k in range(3) if k != a]
        held = self.valid.copy()
        for s1, s2 in ((1, 0), (0, 1), (1, 1)):
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            if s1:
                src[b1], dst[b1] = slice(0, -1), slice(1, None)
            if s2:
                src[b2], dst[b2] = slice(0, -1), slice(1, None)
            held[tuple(dst)] |= self.valid[tuple(src)]
        return held


def configurations(field):
    """Number of valid cells per cube index, [256]."""
    return np.bincount(Dense(field).cubes(), minlength=256)


def zeros_next_to_negatives(field):
    """(n_plus, n_minus): voxels with w > 0 holding +0.0 / -0.0 whose cell-valid edge leads to a voxel with tsdf < 0."""
    D = Dense(field)
    out = [0, 0]
    zero = D.tsdf == 0
    sign = np.signbit(D.tsdf)
    for a in range(3):
        held = D.edge_held(a)
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        for z, n in ((lo, hi), (hi, lo)):                  # the zero at the edge's first / second voxel
            hit = held[lo] & zero[z] & D.neg[n]
            out[0] += int((hit & ~sign[z]).sum())
            out[1] += int((hit & sign[z]).sum())
    return tuple(out)


def expected_vertices(field, vs):
    """fp64 (positions [M,3], colours [M,3]) of the rule: one vertex per lattice edge that a valid cell holds and whose two
    voxels differ in tsdf < 0, at (g + 0.5) vs + |f0| / (|f0| + |f1|) vs along the edge (vs = float32(vs)); colour
    ((|f1| c0 + |f0| c1) / (|f0| + |f1|)) / 255.  Order: units by (z, y, x), voxels x fastest, edges +x, +y, +z."""
    vs = float(np.float32(vs))
    D = Dense(field)
    f = np.abs(D.tsdf.astype(np.float64))
    rgb = D.rgb.astype(np.float64)
    rows = []
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        has = D.edge_held(a)[lo] & (D.neg[lo] != D.neg[hi])
        g = np.argwhere(has)
        f0, f1 = f[lo][has], f[hi][has]
        p = (g + D.org[None] + 0.5) * vs
        p[:, a] += f0 / (f0 + f1) * vs
        c = (f1[:, None] * rgb[lo][has] + f0[:, None] * rgb[hi][has]) / (f0 + f1)[:, None] / 255.0
        rows.append((g + D.org[None], np.full(len(g), a), p, c))
    G = np.concatenate([r[0] for r in rows])
    A = np.concatenate([r[1] for r in rows])
    P = np.concatenate([r[2] for r in rows])
    Cc = np.concatenate([r[3] for r in rows])
    u, l = G >> 4, G & 15
    order = np.lexsort((A, l[:, 0], l[:, 1], l[:, 2], u[:, 0], u[:, 1], u[:, 2]))
    return P[order], Cc[order]


def check_vertices(field, vs, v, c):
    """Vertices within 4 * 2^-24 * (|p| + vs) of the fp64 rule (four fp32 roundings: the product, the sum s, the quotient,
    the final add), colours within 8 * 2^-24."""
    P, Cc = expected_vertices(field, vs)
    v, c = np.asarray(v), np.asarray(c)
    assert v.dtype == np.float32 and c.dtype == np.float32
    assert v.shape == P.shape and c.shape == Cc.shape, f"{len(v)} vertices, the rule gives {len(P)}"
    if len(P) == 0:
        return 0
    tol = 4 * 2.0 ** -24 * (np.abs(P) + float(np.float32(vs)))
    err = np.abs(v.astype(np.float64) - P)
    assert np.all(err <= tol), f"vertex off the rule by {float((err / tol).max()):.2f} x the bound at {int(np.argmax((err / tol).max(1)))}"
    cerr = np.abs(c.astype(np.float64) - Cc)
    assert np.all(cerr <= 8 * 2.0 ** -24), f"colour off the rule by {float(cerr.max()):.3g}"
    return len(P)


def check_directed_edges(f, n_vertices):
    """Every directed triangle edge occurs exactly once and its reverse exactly once: closed and consistently oriented."""
    f = np.asarray(f).astype(np.int64)
    assert f.ndim == 2 and f.shape[1] == 3 and len(f) > 0
    assert f.min() >= 0 and f.max() < n_vertices
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    assert np.all(a != b), "degenerate triangle"
    fwd, cnt = np.unique(a * n_vertices + b, return_counts=True)
    assert np.all(cnt == 1), f"{int((cnt > 1).sum())} directed edges occur more than once"
    assert np.array_equal(fwd, np.unique(b * n_vertices + a)), "a directed edge has no reverse"
    assert len(np.unique(f)) == n_vertices, "unreferenced vertices"


def winding_numbers(v, f, q):
    """fp64 winding number of the mesh about every point of q [n,3]: the triangles' signed solid angles (Van Oosterom and
    Strackee) summed, over 4 pi."""
    from concurrent.futures import ThreadPoolExecutor
    vt = np.ascontiguousarray(np.asarray(v, np.float64).T)                       # [3, Nv]
    f0, f1, f2 = (np.ascontiguousarray(np.asarray(f)[:, k].astype(np.int64)) for k in range(3))

    def one(p):
        d = vt - np.asarray(p, np.float64)[:, None]                              # vertex - point, once per vertex
        ln = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        a, b, c = d[:, f0], d[:, f1], d[:, f2]
        la, lb, lc = ln[f0], ln[f1], ln[f2]
        num = (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2])
               + a[2] * (b[0] * c[1] - b[1] * c[0]))
        den = la * lb * lc + (a * b).sum(0) * lc + (b * c).sum(0) * la + (c * a).sum(0) * lb
        return 2.0 * np.arctan2(num, den).sum() / (4.0 * np.pi)

    with ThreadPoolExecutor(4) as pool:
        return np.array(list(pool.map(one, np.asarray(q, np.float64))))


def check_winding(field, vs, v, f, n=600, seed=0):
    """The winding number at n randomly drawn voxel centres is 1 where tsdf < 0 and 0 elsewhere, to 1e-9."""
    vs = float(np.float32(vs))
    D = Dense(field)
    rng = np.random.default_rng(seed)
    g = np.stack([rng.integers(0, s, n) for s in D.tsdf.shape], 1)
    inside = D.neg[g[:, 0], g[:, 1], g[:, 2]]
    assert inside.any() and not inside.all()
    wn = winding_numbers(v, f, (g + D.org[None] + 0.5) * vs)
    err = np.abs(wn - inside)
    assert err.max() <= 1e-9, f"winding number off by {float(err.max()):.3g} at voxel {(g[np.argmax(err)] + D.org).tolist()}"
    return float(err.max())


def triangle_total(field, ntri_table):
    """Sum of the table's triangle count over the valid cells."""
    return int(np.asarray(ntri_table, np.int64)[Dense(field).cubes()].sum())


def check_closed_mesh(field, vs, v, f, c, n_winding=600):
    """Every independent check of a closed field's mesh."""
    check_vertices(field, vs, v, c)
    check_directed_edges(f, len(v))
    return check_winding(field, vs, v, f, n_winding)
