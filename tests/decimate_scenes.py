"""Meshes for the decimation tests and scripts/decimate_bench.py (numpy; vertices fp32, triangles int64), and the checks of a
result that need no device: counts of boundary and non-manifold edges, components, boundary loops, area.  CASES names the
irregular, defective and workload-sized runs that the host tests account for round by round (round_account) and the GPU tests
compare with the restatement (reference: computed once per process for both)."""
from __future__ import annotations

import numpy as np

from meshclean_scenes import F, THREE_HOLES, icosphere, merge, sheet, strip, tetra_pair  # noqa: F401  (re-exported)


def fan(n=300):
    """A hub of valence n: vertex 0 at the apex of a shallow cone over a regular n-gon, n triangles."""
    ang = 2 * np.pi * np.arange(n) / n
    V = np.concatenate([[[0.0, 0.0, 0.25]], np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], 1)]).astype(F)
    i = np.arange(n)
    return V, np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], 1).astype(np.int64)


def colour_ramp(V):
    """[M,3] fp32 in [0,1]: a ramp along each axis of the bounding box."""
    lo, hi = V.min(0), V.max(0)
    return ((V - lo) / np.maximum(hi - lo, F(1e-6))).astype(F)


# ------------------------------------------------------------------------------------------- irregular and defective scenes
def jitter_sheet(n, holes=(), seed=0):
    """sheet(n, holes) off its lattice: N(0,1) 0.25 / n on every z, uniform +- 0.4 / n on the x and y of the vertices strictly
    inside the unit square (the outline stays on the square, no quad can fold: 0.8 / n < 1 / n)."""
    V, T = sheet(n, holes)
    rng = np.random.default_rng(seed)
    V = V.astype(np.float64)
    inner = ((V[:, :2] > 0) & (V[:, :2] < 1)).all(1)
    V[:, 2] += rng.standard_normal(len(V)) * 0.25 / n
    V[:, :2] += np.where(inner[:, None], rng.uniform(-0.4 / n, 0.4 / n, (len(V), 2)), 0.0)
    return V.astype(F), T


def noisy_icosphere(level, seed=0):
    """icosphere(level) with every radius times 1 + 0.05 N(0,1), then the axes scaled by (1, 0.3, 2.5): closed, irregular,
    anisotropic."""
    V, T = icosphere(level)
    rng = np.random.default_rng(seed)
    V = V.astype(np.float64) * (1.0 + 0.05 * rng.standard_normal(len(V)))[:, None] * np.array([1.0, 0.3, 2.5])
    return V.astype(F), T


def high_indices(form, M=70001, seed=0):
    """icosphere(2) at vertex indices of three key bytes (>= 2^16: the CSR sorts take three passes).  "behind": after 65 836
    unreferenced vertices, every index >= 2^16.  "scattered": over sorted random slots of M, the last slot used."""
    V, T = icosphere(2)
    if form == "behind":
        pad = 65836
        return np.concatenate([np.full((pad, 3), 7.0, F), V]), T + pad
    rng = np.random.default_rng(seed)
    slots = np.sort(rng.choice(M - 1, len(V) - 1, replace=False))
    slots = np.concatenate([slots, [M - 1]])
    out = np.full((M, 3), 7.0, F)
    out[slots] = V
    return out, slots[T]


def defects():
    """sheet(12) with a face listed twice, a face listed again with its winding reversed, two coincident vertices (zero-area
    faces with distinct corners), and a NaN, an Inf and a 3e38 coordinate."""
    V, T = sheet(12)
    T = np.concatenate([T, T[10:11], T[40:41, ::-1]])
    V = V.copy()
    V[50] = V[51]
    V[80] = [np.nan, 0.5, 0.0]
    V[100] = [np.inf, 0.2, 0.0]
    V[120, 0] = 3e38
    return V, T


def bowtie():
    """Two icosphere(1), the second centred at (2, 0, 0), welded at the one vertex they share, (1, 0, 0)."""
    A, TA = icosphere(1)
    B, TB = icosphere(1, 1.0, (2.0, 0.0, 0.0))
    one = np.array([1.0, 0.0, 0.0], F)
    ia, ib = np.nonzero((A == one).all(1))[0], np.nonzero((B == one).all(1))[0]
    assert len(ia) == 1 and len(ib) == 1
    ia, ib = int(ia[0]), int(ib[0])
    new = np.arange(len(B)) + len(A) - (np.arange(len(B)) > ib)
    new[ib] = ia
    return np.concatenate([A, np.delete(B, ib, 0)]).astype(F), np.concatenate([TA, new[TB]])


def tube(rings=13, radius=0.01, seed=0):
    """An open, thin, crooked tube of triangular cross-section: rings of three vertices one unit apart along z, their centres
    off the axis by N(0,1) 0.3.  The two ends of a ring edge have the ring's third vertex as a common neighbour that is on
    neither of the edge's faces, and nothing else about the edge is wrong: the cheapest edges of this mesh are refused by the
    link condition (2) alone (without it the tube is pinched into edges with four faces)."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(3) / 3
    V = np.zeros((rings, 3, 3))
    V[:, :, 0] = radius * np.cos(ang)[None, :] + 0.3 * rng.standard_normal((rings, 1))
    V[:, :, 1] = radius * np.sin(ang)[None, :] + 0.3 * rng.standard_normal((rings, 1))
    V[:, :, 2] = np.arange(rings)[:, None]
    i, j = (x.reshape(-1) for x in np.meshgrid(np.arange(rings - 1), np.arange(3), indexing="ij"))
    a, b, c, d = 3 * i + j, 3 * i + (j + 1) % 3, 3 * (i + 1) + j, 3 * (i + 1) + (j + 1) % 3
    return V.reshape(-1, 3).astype(F), np.stack([np.stack([a, b, d], 1), np.stack([a, d, c], 1)], 1).reshape(-1, 3).astype(np.int64)


def inf_vertex():
    """noisy_icosphere(1, 0) with one coordinate at +Inf.  Around that vertex some collapse targets are not finite while every
    surviving face keeps a positive (infinite) dot product of its old and new normals: the refusal of a target that is not
    finite decides alone."""
    V, T = noisy_icosphere(1, 0)
    V[13, 2] = np.inf
    return V, T


def wide_attributes(V):
    """[M,515] fp32 normal-random, and the colour ramp: 518 channels."""
    return np.random.default_rng(11).standard_normal((len(V), 515)).astype(F), colour_ramp(V)


def _scaled(s):
    V, T = icosphere(2)
    return (V.astype(np.float64) * s).astype(F), T


def _with(mesh, attributes):
    return mesh[0], mesh[1], attributes(mesh[0])


# name -> (mesh or mesh and attributes, target_triangles, max_rounds).  What each case is for, and the conditions it was chosen
# to meet, are asserted on the restatement in test_decimate_host.py.
CASES = {
    "jitter24": (lambda: jitter_sheet(24, [(8, 14, 8, 14)], 5), 200, 256),
    "noisy3->100": (lambda: _with(noisy_icosphere(3, 1), lambda V: (colour_ramp(V),)), 100, 256),
    "noisy3->0": (lambda: _with(noisy_icosphere(3, 1), lambda V: (colour_ramp(V),)), 0, 256),
    "scale1e-3": (lambda: _scaled(1e-3), 80, 256),
    "scale1e-2": (lambda: _scaled(1e-2), 80, 256),
    "scale30": (lambda: _scaled(30.0), 80, 256),
    "scale1e4": (lambda: _scaled(1e4), 80, 256),
    "high_behind": (lambda: high_indices("behind"), 80, 256),
    "high_scattered": (lambda: high_indices("scattered"), 80, 256),
    "defects": (defects, 100, 256),
    "inf_vertex": (inf_vertex, 26, 256),
    "tube": (tube, 24, 256),
    "bowtie": (bowtie, 20, 256),
    "strip400": (lambda: strip(400), 50, 256),
    "wide": (lambda: _with(icosphere(2), wide_attributes), 80, 256),
    "jitter272 landing": (lambda: jitter_sheet(272, (), 5), 138918, 256),
    "jitter272 3 rounds": (lambda: jitter_sheet(272, (), 5), 0, 3),
}
SMALL = tuple(k for k in CASES if not k.startswith("jitter272"))
_MESHES, _REFERENCES = {}, {}


def case(name):
    """(V, T, attributes, target_triangles, max_rounds) of CASES[name]; the arrays are shared: do not write to them."""
    make, target, max_rounds = CASES[name]
    key = name.split(" ")[0]
    if key not in _MESHES:
        got = make()
        _MESHES[key] = (got[0], got[1], tuple(got[2]) if len(got) > 2 else ())
    return _MESHES[key] + (target, max_rounds)


def round_account(st, tb, ev, selected, applied):
    """What the restatement did in one round, before it is applied: the refusals in the order the kernel tests them, the two
    target branches, and the violations of the independence the apply step rests on."""
    few, link, free, finite, upright, distinct = ev.rules
    r1 = ~few
    r3 = few & ~free
    r2 = few & free & ~link
    passed = few & free & link
    nonfinite = passed & ~finite
    flip = passed & finite & ~(upright & distinct)
    assert np.array_equal(ev.valid, passed & finite & upright & distinct)
    assert not (selected & ~ev.valid).any() and not (applied & ~selected).any()
    alone = {}                                                              # refused by this rule and by no other
    for k, name in enumerate(("few", "link", "free", "finite", "upright", "distinct")):
        others = np.ones(len(ev.a), bool)
        for j, rule in enumerate(ev.rules):
            if j != k:
                others &= rule
        alone["only_" + name] = int((others & ~ev.rules[k]).sum())
    a, b = ev.a[selected], ev.b[selected]
    ends = np.concatenate([a, b])
    edge_of = np.full(st.M, -1, np.int64)
    edge_of[a] = np.arange(len(a))
    edge_of[b] = np.arange(len(b))
    both = (edge_of[tb.us] >= 0) & (edge_of[tb.ut] >= 0)
    return dict(M=st.M, faces=len(tb.lf), entries=6 * len(tb.lf), edges=len(ev.a), selected=int(selected.sum()),
                applied=int(applied.sum()), selected_faces=int(ev.faces[selected].sum()), removed=int(ev.faces[applied].sum()),
                r1=int(r1.sum()), r2=int(r2.sum()), r3=int(r3.sum()), nonfinite=int(nonfinite.sum()), flip_or_pillow=int(flip.sum()),
                cramer=int((passed & ev.solved).sum()), fallback=int((passed & ~ev.solved).sum()),
                shared_ends=len(ends) - len(np.unique(ends)),
                adjacent_ends=int((edge_of[tb.us][both] != edge_of[tb.ut][both]).sum()),
                top_digits=len(np.unique(ev.bits[selected] >> np.uint64(42))),
                middle_digits=len(np.unique((ev.bits[selected] >> np.uint64(21)) & np.uint64(0x1fffff))), **alone)


def reference(name):
    """(the restatement's result for CASES[name], one round_account per round), computed once for the host and the GPU tests."""
    if name not in _REFERENCES:
        import decimate_restatement as R
        V, T, att, target, max_rounds = case(name)
        rounds = []
        with np.errstate(all="ignore"):                             # (defects() has NaN and Inf coordinates)
            result = R.simplify(V, T, target, att, max_rounds, on_round=lambda *a: rounds.append(round_account(*a)))
        _REFERENCES[name] = (result, rounds)
    return _REFERENCES[name]


def total(rounds, key):
    return sum(r[key] for r in rounds)


def edge_counts(tri):
    """(n_edges, n_boundary, n_nonmanifold) of the undirected edges."""
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    _, cnt = np.unique(e[:, 0] * (t.max() + 1 if len(t) else 1) + e[:, 1], return_counts=True)
    return len(cnt), int((cnt == 1).sum()), int((cnt > 2).sum())


def _roots(parent):
    while True:
        nxt = parent[parent]
        if (nxt == parent).all():
            return parent
        parent = nxt


def _components(n, a, b):
    """labels [n] of the graph with edges (a, b): the smallest member of each component."""
    parent = np.arange(n)
    while True:
        r = _roots(parent)
        lo = np.minimum(r[a], r[b])
        new = r.copy()
        np.minimum.at(new, r[a], lo)
        np.minimum.at(new, r[b], lo)
        if (new == r).all():
            return r
        parent = new


def n_components(tri):
    """Components of the faces under "share a vertex" (equal to edge-connected for the manifold meshes tested)."""
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    lab = _components(int(t.max()) + 1, np.concatenate([t[:, 0], t[:, 1]]), np.concatenate([t[:, 1], t[:, 2]]))
    return len(np.unique(lab[t[:, 0]]))


def n_boundary_loops(tri):
    """Boundary edges connected through shared vertices (mesh_holes's definition)."""
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    e = np.sort(d, 1)
    m = int(t.max()) + 1
    _, inv, cnt = np.unique(e[:, 0] * m + e[:, 1], return_inverse=True, return_counts=True)
    b = d[cnt[inv] == 1]
    if len(b) == 0:
        return 0
    lab = _components(m, b[:, 0], b[:, 1])
    return len(np.unique(lab[b[:, 0]]))


def total_area(V, tri):
    P = np.asarray(V, np.float64)
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    return float(0.5 * np.linalg.norm(np.cross(P[t[:, 1]] - P[t[:, 0]], P[t[:, 2]] - P[t[:, 0]]), axis=1).sum())
