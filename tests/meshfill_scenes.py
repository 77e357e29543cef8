"""Meshes for the subdivision, fairing and hole-fill tests and scripts/meshfill_bench.py (numpy; vertices fp32, triangles
int64), with the arguments each case runs under.  SUBDIVIDE, FAIR and FILL name the cases; the host tests assert on the
restatement what each case was chosen for, the GPU tests compare with it (reference: computed once per process for both)."""
from __future__ import annotations

import numpy as np

from meshclean_scenes import F, icosphere, merge, sheet, strip, tetra_pair  # noqa: F401  (re-exported)

LDS_MAX_VERTICES = 4096                 # MISPLAT_MESHFILL_LDS_VERTICES (tests/test_meshfill_host.py keeps the three equal)


def one_triangle():
    """Legs 4 and 1: one edge (the hypotenuse, sqrt(17)) is the longest by far."""
    return np.array([[0, 0, 0], [4, 0, 0], [0, 1, 0]], F), np.array([[0, 1, 2]], np.int64)


def two_triangles():
    """The unit square cut along the diagonal 0 - 2."""
    return np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F), np.array([[0, 1, 2], [0, 2, 3]], np.int64)


def equal_spoke_fan():
    """A fan over the twelve lattice points of the circle x^2 + y^2 = 25: every spoke is 5.0 to the bit (no regular polygon
    beyond the square has bit-equal spokes in fp32), every rim edge sqrt(10) or sqrt(2)."""
    rim = [(5, 0), (4, 3), (3, 4), (0, 5), (-3, 4), (-4, 3), (-5, 0), (-4, -3), (-3, -4), (0, -5), (3, -4), (4, -3)]
    V = np.array([(0, 0, 0)] + [(x, y, 0) for x, y in rim], F)
    i = np.arange(12)
    return V, np.stack([np.zeros(12, np.int64), 1 + i, 1 + (i + 1) % 12], 1)


def grid(nx, ny, step=1.0):
    """nx x ny quads at z = 0, vertex j (nx + 1) + i at (i, j) step; two triangles per quad."""
    X, Y = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    V = (np.stack([X.reshape(-1), Y.reshape(-1), np.zeros((nx + 1) * (ny + 1))], 1) * step).astype(F)
    i, j = (x.reshape(-1) for x in np.meshgrid(np.arange(nx), np.arange(ny)))
    a = j * (nx + 1) + i
    b, c, d = a + 1, a + nx + 2, a + nx + 1
    return V, np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3).astype(np.int64)


def defective():
    """tetra_pair(2) (its shared edge 0 - 1 has four faces) and a face with a repeated corner, (2, 6, 6), to a far vertex: the
    edge 2 - 6 has two incidences, both of that one face."""
    V, T = tetra_pair(2)
    return np.concatenate([V, [[9, 9, 9]]]).astype(F), np.concatenate([T, [[2, len(V), len(V)]]]).astype(np.int64)


def colour_ramp(V):
    lo, hi = V.min(0), V.max(0)
    return ((V - lo) / np.maximum(hi - lo, F(1e-6))).astype(F)


def _strip_half():
    V, T = strip(8, step=1.0)
    return V, T, np.arange(len(T)) < len(T) // 2


# name -> (mesh and optional region, max_edge_len, max_edge_splits, with attributes)
SUBDIVIDE = {
    "one_triangle": (one_triangle, 2.0, 1, False),
    "two_triangles": (two_triangles, 1.2, 10000, False),
    "equal_spokes": (equal_spoke_fan, 4.0, 10000, True),
    "strip_half": (_strip_half, 0.7, 10000, True),
    "budget": (lambda: sheet(8), 0.05, 10, True),
    "icosahedron": (lambda: icosphere(0), 0.3, 10000, False),
    "grid37x41": (lambda: grid(37, 41), 0.8, 10000, True),
    "defective": (defective, 0.7, 10000, False),
}
_MESHES, _REFERENCES = {}, {}


def subdivide_case(name):
    """(V, T, region or None, attributes, max_edge_len, max_edge_splits); the arrays are shared: do not write to them."""
    make, max_len, budget, with_att = SUBDIVIDE[name]
    if name not in _MESHES:
        got = make()
        _MESHES[name] = (got[0], got[1], got[2] if len(got) > 2 else None, (colour_ramp(got[0]),) if with_att else ())
    return _MESHES[name] + (max_len, budget)


def subdivide_reference(name):
    """(the restatement's result, per round (selected in all, applied)) of SUBDIVIDE[name]."""
    key = ("subdivide", name)
    if key not in _REFERENCES:
        import meshfill_restatement as R
        V, T, region, att, max_len, budget = subdivide_case(name)
        rounds = []
        res = R.subdivide(V, T, max_len, budget, region, att, on_round=lambda rd, sel: rounds.append((int(rd.selected.sum()), len(sel))))
        _REFERENCES[key] = (res, rounds)
    return _REFERENCES[key]


# ---------------------------------------------------------------------------------------------------------- fairing
def _block(n, i0, i1, j0, j1):
    """The vertices (i, j), i0 <= i < i1, j0 <= j < j1, of sheet(n)."""
    i, j = np.meshgrid(np.arange(i0, i1), np.arange(j0, j1))
    return (j * (n + 1) + i).reshape(-1)


def single_fan():
    """equal_spoke_fan with its centre lifted and free."""
    V, T = equal_spoke_fan()
    V = V.copy()
    V[0] = [0.5, -0.25, 2.0]
    free = np.zeros(len(V), bool)
    free[0] = True
    return V, T, free


def two_patches(seed=3):
    """sheet(32) with a 3 x 3 and a 9 x 9 block of free vertices, all lifted off the plane by noise; vertex 5 of a second,
    unreferenced list of 8 vertices is free too (no neighbour)."""
    V, T = sheet(32)
    rng = np.random.default_rng(seed)
    free = np.zeros(len(V) + 8, bool)
    free[_block(32, 3, 6, 3, 6)] = True
    free[_block(32, 12, 21, 14, 23)] = True
    V = np.concatenate([V, np.full((8, 3), 2.0, F)])
    V[free, 2] += (0.05 * rng.standard_normal(int(free.sum()))).astype(F)
    free[len(V) - 3] = True
    return V, T, free


def cutoff_patches(seed=4):
    """Two sheet(80) side by side: a 64 x 64 block of free vertices in the first (LDS_MAX_VERTICES: the largest patch one
    workgroup takes), the same block and one more vertex beside it in the second (one too many)."""
    A, TA = sheet(80)
    V, T = merge((A, TA), (A + np.array([2, 0, 0], F), TA))
    rng = np.random.default_rng(seed)
    free = np.zeros(len(V), bool)
    block = _block(80, 8, 72, 8, 72)
    assert len(block) == LDS_MAX_VERTICES
    free[block] = True
    free[len(A) + block] = True
    free[len(A) + 8 * 81 + 72] = True
    V = V.copy()
    V[free, 2] += (0.01 * rng.standard_normal(int(free.sum()))).astype(F)
    return V, T, free


# name -> (mesh and free, tolerance, max_iterations)
FAIR = {
    "single_fan": (single_fan, 1e-3, 10000),
    "single_fan_once": (single_fan, 1e-3, 1),
    "two_patches": (two_patches, 1e-4, 10000),
    "cutoff": (cutoff_patches, 2e-4, 10000),
}


def fair_case(name):
    """(V, T, free, attributes, tolerance, max_iterations)."""
    make, tol, max_it = FAIR[name]
    key = ("fair", make.__name__)
    if key not in _MESHES:
        V, T, free = make()
        _MESHES[key] = (V, T, free, (colour_ramp(V),))
    return _MESHES[key] + (tol, max_it)


def fair_reference(name):
    key = ("fair", name)
    if key not in _REFERENCES:
        import meshfill_restatement as R
        V, T, free, att, tol, max_it = fair_case(name)
        _REFERENCES[key] = R.fair(V, T, free, tol, max_it, att)
    return _REFERENCES[key]


# --------------------------------------------------------------------------------------------------------- the fill
def open_cube(k=4, side=0.5):
    """A cube of the given side, k x k quads a face, welded, without its top face: one square hole of perimeter 4 side."""
    frames = [((0, 0, 0), (0, 1, 0), (1, 0, 0)), ((0, 0, 0), (1, 0, 0), (0, 0, 1)), ((1, 0, 0), (0, 1, 0), (0, 0, 1)),
              ((1, 1, 0), (-1, 0, 0), (0, 0, 1)), ((0, 1, 0), (0, -1, 0), (0, 0, 1))]      # (origin, u, v), u x v outward
    P, Q = [], []
    for o, u, v in frames:
        i, j = (x.reshape(-1) for x in np.meshgrid(np.arange(k + 1), np.arange(k + 1)))
        base = len(P) * (k + 1) ** 2
        P.append(np.array(o)[None] * k + i[:, None] * np.array(u)[None] + j[:, None] * np.array(v)[None])
        qi, qj = (x.reshape(-1) for x in np.meshgrid(np.arange(k), np.arange(k)))
        a = base + qj * (k + 1) + qi
        Q.append(np.stack([np.stack([a, a + 1, a + k + 2], 1), np.stack([a, a + k + 2, a + k + 1], 1)], 1).reshape(-1, 3))
    P = np.concatenate(P)
    uniq, inv = np.unique(P, axis=0, return_inverse=True)
    return (uniq * (side / k)).astype(F), inv.reshape(-1)[np.concatenate(Q)].astype(np.int64)


def holed_sheet():
    """sheet(32) without a 4 x 4-quad hole (perimeter 0.5) and a 16 x 16-quad hole (perimeter 2); its outline has perimeter 4."""
    return sheet(32, [(4, 8, 4, 8), (12, 28, 12, 28)])


# name -> (mesh, max_hole_size, max_edge_len)
FILL = {
    "open_cube": (open_cube, 3.0, 0.14),
    "holed_sheet": (holed_sheet, 1.0, 1.0 / 32),
}


def fill_case(name):
    """(V, T, attributes, max_hole_size, max_edge_len)."""
    make, size, max_len = FILL[name]
    key = ("fill", name)
    if key not in _MESHES:
        V, T = make()
        _MESHES[key] = (V, T, (colour_ramp(V),))
    return _MESHES[key] + (size, max_len)


def fill_reference(name):
    key = ("fill", name)
    if key not in _REFERENCES:
        import meshfill_restatement as R
        V, T, att, size, max_len = fill_case(name)
        _REFERENCES[key] = R.fill_holes_nicely(V, T, size, max_len, attributes=att)
    return _REFERENCES[key]


def edge_counts(tri):
    """(n_edges, n_boundary, n_nonmanifold) of the undirected edges with two distinct ends."""
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    e = e[e[:, 0] != e[:, 1]]
    _, cnt = np.unique(e[:, 0] * (t.max() + 1 if len(t) else 1) + e[:, 1], return_counts=True)
    return len(cnt), int((cnt == 1).sum()), int((cnt > 2).sum())


def boundary_edges(tri):
    """The sorted keys lo << 32 | hi of the edges with exactly one incident face."""
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    key, cnt = np.unique((e[:, 0] << 32) | e[:, 1], return_counts=True)
    return key[cnt == 1]


def total_area(V, tri):
    P = np.asarray(V, np.float64)
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    return float(0.5 * np.linalg.norm(np.cross(P[t[:, 1]] - P[t[:, 0]], P[t[:, 2]] - P[t[:, 0]]), axis=1).sum())


def face_normals(V, tri):
    P = np.asarray(V, np.float64)
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    return np.cross(P[t[:, 1]] - P[t[:, 0]], P[t[:, 2]] - P[t[:, 0]])
