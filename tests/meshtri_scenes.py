"""Meshes for the hole-triangulation and edge-flip tests and scripts/meshtri_bench.py (numpy; vertices fp32, triangles int64),
with the arguments each case runs under.  TRIANGULATE, FLIP and FILL name the cases; the host tests assert on the restatement
what each case was chosen for, the GPU tests compare with it (reference: computed once per process for both)."""
from __future__ import annotations

import numpy as np

from meshclean_scenes import BOW_TIE, F, icosphere, merge, sheet, tetra_pair  # noqa: F401  (re-exported)
from meshfill_scenes import (boundary_edges, colour_ramp, defective, edge_counts, face_normals, grid, holed_sheet,  # noqa: F401
                             open_cube, total_area)

LDS_LOOP = 176                          # MISPLAT_MESHTRI_LDS_LOOP (tests/test_meshtri_host.py keeps the three equal)
MAX_LOOP = 1024                         # MISPLAT_MESHTRI_MAX_LOOP


# ---------------------------------------------------------------------------------------------------- triangulation
def annulus(P, scale=2.0):
    """A ring of 2 n faces around the polygon P [n,3] (counter-clockwise seen from +z): vertex i is P_i, vertex n + i is P_i
    scaled about the polygon's mean.  The hole's rim is the loop 0 .. n - 1, a patch face (i, k, j), i < k < j, faces +z; the
    outer loop has `scale` times the rim's perimeter.  Only the ring's connectivity matters to a triangulation of the hole."""
    P = np.asarray(P, np.float64)
    n = len(P)
    c = P.mean(0)
    V = np.concatenate([P, c + scale * (P - c)]).astype(F)
    i = np.arange(n)
    j = (i + 1) % n
    T = np.stack([np.stack([i, n + i, n + j], 1), np.stack([i, n + j, j], 1)], 1).reshape(-1, 3)
    return V, T.astype(np.int64)


def circle(n, radius=0.1, lift=0.0, seed=0):
    """n points on a circle, counter-clockwise, each lifted off the plane by `lift` times a normal deviate."""
    a = 2 * np.pi * np.arange(n) / n
    z = lift * np.random.default_rng(seed).standard_normal(n)
    return np.stack([radius * np.cos(a), radius * np.sin(a), z], 1)


def convex_polygon():
    """Seven dyadic points in convex position, no three on a line."""
    return np.array([(0, 0), (2, -0.5), (3.5, 0.5), (4, 2), (3, 3.5), (1, 3.75), (-0.5, 2)], np.float64) @ np.eye(2, 3)


def c_polygon():
    """A C that opens to the right, eight dyadic points, no three on a line: the mean of its vertices, (2.375, 2), lies in the
    notch, outside the polygon."""
    return np.array([(0, 0), (4.5, 0), (4, 1), (1, 1), (1, 3), (4, 3), (4.5, 4), (0, 4)], np.float64) @ np.eye(2, 3)


def polygon_area(P):
    x, y = np.asarray(P, np.float64)[:, 0], np.asarray(P, np.float64)[:, 1]
    return float(0.5 * (x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def _bent_quad():
    """A square with one corner lifted: the diagonal 1 - 3 leaves a flat triangle and has the smaller area."""
    return annulus(np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0.75), (0, 1, 0)], np.float64))


def _three_loops():
    """Rims of 5, 9 and 14 edges; the last (radius 0.3) is above the limit of 1.0, as are all three outer loops."""
    return merge(annulus(circle(5, 0.1, 0.02, 1)), annulus(circle(9, 0.1, 0.02, 2) + [1, 0, 0]), annulus(circle(14, 0.3, 0.02, 3) + [3, 0, 0]))


def _cutoff():
    """A rim of LDS_LOOP edges (the longest whose table a workgroup's LDS holds) and one of an edge more."""
    return merge(annulus(circle(LDS_LOOP, 0.1, 0.002, 4)), annulus(circle(LDS_LOOP + 1, 0.1, 0.002, 5) + [1, 0, 0]))


def two_edge_loop():
    """tetra_pair(2), whose shared edge 0 - 1 has four faces, and a fifth face (0, 1, 6) on that edge: its other two edges are
    the mesh's only boundary edges, a loop of two."""
    V, T = tetra_pair(2)
    return np.concatenate([V, [[0.5, 0.5, 0.5]]]).astype(F), np.concatenate([T, [[0, 1, len(V)]]]).astype(np.int64)


def _fallbacks():
    """A pinched loop (two holes of sheet(64) that share a vertex), a loop of two edges and a rim of MAX_LOOP + 1 edges."""
    return merge(sheet(64, BOW_TIE), two_edge_loop(), annulus(circle(MAX_LOOP + 1, 0.1, 0.0005, 6) + [3, 0, 0]))


# name -> (mesh, max_hole_size)
TRIANGULATE = {
    "triangle": (lambda: annulus(circle(3, 0.1)), 1.0),
    "bent_quad": (_bent_quad, 5.0),
    "pentagon": (lambda: annulus(circle(5, 0.1, 0.02, 7)), 1.0),
    "square_tie": (lambda: annulus(np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], np.float64)), 5.0),
    "convex": (lambda: annulus(convex_polygon()), 16.0),
    "c_shape": (lambda: annulus(c_polygon()), 24.0),
    "three_loops": (_three_loops, 1.0),
    "cutoff": (_cutoff, 1.0),
    "fallbacks": (_fallbacks, 3.0),
    "closed": (lambda: icosphere(1), 3.0),
}
_MESHES, _REFERENCES = {}, {}


def triangulate_case(name):
    """(V, T, attributes, max_hole_size); the arrays are shared: do not write to them."""
    make, size = TRIANGULATE[name]
    if name not in _MESHES:
        V, T = make()
        _MESHES[name] = (V, T, (colour_ramp(V),))
    return _MESHES[name] + (size,)


def triangulate_reference(name):
    key = ("triangulate", name)
    if key not in _REFERENCES:
        import meshtri_restatement as R
        V, T, att, size = triangulate_case(name)
        _REFERENCES[key] = R.triangulate_holes(V, T, size, att)
    return _REFERENCES[key]


# ------------------------------------------------------------------------------------------------------------ flips
def kite(half_width):
    """Two triangles over the diagonal 0 - 2 of length 4; the other diagonal, 1 - 3, has length 2 half_width."""
    V = np.array([(-2, 0, 0), (0, -half_width, 0), (2, 0, 0), (0, half_width, 0)], F)
    return V, np.array([[0, 1, 2], [0, 2, 3]], np.int64)


def unit_square():
    """Four points on one circle: cot + cot = 0."""
    return np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], F), np.array([[0, 1, 2], [0, 2, 3]], np.int64)


def shifted_octahedron(t=0.6, h=0.3):
    """An octahedron over the unit diamond whose poles 4, 5 = (t, 0, +-h) are shifted towards vertex 0 = (1, 0, 0): the two
    equator edges at vertex 0 are mirror images, both see the poles under obtuse angles and both want the new edge 4 - 5."""
    V = np.array([(1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (t, 0, h), (t, 0, -h)], F)
    T = [(i, (i + 1) % 4, 4) for i in range(4)] + [((i + 1) % 4, i, 5) for i in range(4)]
    return V, np.array(T, np.int64)


def valence_three():
    """Vertex 3 has the neighbours 0, 1, 2 only: flipping an edge at it would create an edge of the triangle 0 1 2, which
    exists.  The edge 0 - 3 sees 1 and 2 under obtuse angles (3 lies beyond the edge 1 - 2 as seen from 0)."""
    V = np.array([(0, 0, 0), (0.5, 1, 0), (-0.5, 1, 0), (0, 2, 0)], F)
    return V, np.array([[0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64)


def sheared_grid(nx, ny, shear=1):
    """grid(nx, ny) sheared by x += shear y: every quad is a parallelogram cut along its long diagonal; the lattice is still
    the integer lattice, so from a shear of 2 on a round of flips leaves diagonals that the next round flips again."""
    V, T = grid(nx, ny)
    V = V.copy()
    V[:, 0] += shear * V[:, 1]
    return V, T


def _half_region():
    V, T = sheared_grid(8, 2)
    return V, T, np.arange(len(T)) < len(T) // 2


# name -> mesh and optional region
FLIP = {
    "bad_diagonal": lambda: kite(0.5),
    "delaunay_pair": lambda: kite(4.0),
    "cocircular": unit_square,
    "octahedron": shifted_octahedron,
    "valence_three": valence_three,
    "region_border": _half_region,
    "grid37x41": lambda: sheared_grid(37, 41, 3),
    "defective": defective,
}


def flip_case(name):
    """(V, T, region or None)."""
    key = ("flip", name)
    if key not in _MESHES:
        got = FLIP[name]()
        _MESHES[key] = (got[0], got[1], got[2] if len(got) > 2 else None)
    return _MESHES[key]


def flip_reference(name):
    """(the restatement's result, per round (selected, flipped))."""
    key = ("flip", name)
    if key not in _REFERENCES:
        import meshtri_restatement as R
        V, T, region = flip_case(name)
        rounds = []
        res = R.flip_edges(V, T, region, on_round=lambda rd: rounds.append((int(rd.selected.sum()), len(rd.flips))))
        _REFERENCES[key] = (res, rounds)
    return _REFERENCES[key]


# --------------------------------------------------------------------------------------------------------- the fill
def c_sheet():
    """sheet(16) without a C of quads that opens to the right (perimeter 2.75; the outline's is 4)."""
    return sheet(16, [(4, 12, 4, 6), (4, 6, 6, 10), (4, 12, 10, 12)])


# name -> (mesh, max_hole_size, max_edge_len)
FILL = {
    "c_sheet": (c_sheet, 3.0, 1.0 / 16),
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


def fill_reference(name, triangulation="min_area", flip=True):
    key = ("fill", name, triangulation, flip)
    if key not in _REFERENCES:
        import meshtri_restatement as R
        V, T, att, size, max_len = fill_case(name)
        _REFERENCES[key] = R.fill_holes_nicely(V, T, size, max_len, attributes=att, triangulation=triangulation, flip=flip)
    return _REFERENCES[key]
