"""Meshes for the tests of the angle-and-area hole triangulation and the curvature fairing and
scripts/meshsmooth_bench.py (numpy; vertices fp32, triangles int64), with the arguments each case runs under.  TRIANGULATE, FAIR
and FILL name the cases; the host tests assert on the restatement what each case was chosen for, the GPU tests compare with it
(reference: computed once per process)."""
from __future__ import annotations

import numpy as np

from meshfill_scenes import grid, holed_sheet  # noqa: F401
from meshtri_scenes import (BOW_TIE, F, LDS_LOOP, MAX_LOOP, annulus, boundary_edges, c_polygon, circle, colour_ramp,  # noqa: F401
                            convex_polygon, edge_counts, face_normals, icosphere, merge, polygon_area, sheet, two_edge_loop)

ANGLE_LDS_LOOP = 163                    # MISPLAT_MESHTRI_ANGLE_LDS_LOOP (tests/test_meshsmooth_host.py keeps the mirrors equal)
SMALL_LOOP = 64                         # MISPLAT_MESHTRI_SMALL_LOOP


def ridge_quad():
    """A four-edge hole whose smaller-area diagonal makes the sharper crease.  The rim is tests/meshtri_scenes.py's bent quad
    with a gentler lift, q = (0,0,0), (1,0,0), (1,1,1/4), (0,1,0): the diagonal 1 - 3 leaves the flat triangle (0, 1, 3) and has
    the smaller area.  The rim faces are chosen, through the ring's outer vertices, so that the surface is a ridge along the
    diagonal 0 - 2: the faces at the edges 1 - 2 and 2 - 3 lie in the planes of (0, 1, 2) and (0, 2, 3), the faces at the edges
    0 - 1 and 3 - 0 fall away at 45 degrees (z = y below the edge y = 0, z = x left of the edge x = 0).  The flat triangle then
    meets both falling faces at 45 degrees (bucket 149), while the triangles of the diagonal 0 - 2 meet them at 45 - atan(1/4) =
    31 degrees (the sharpest: bucket 72) and each other at acos(16/17) = 19.7 degrees (bucket 30).  All coordinates are dyadic."""
    P = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0.25), (0, 1, 0)], np.float64)
    V, T = annulus(P)
    V = V.copy()
    # the outer vertex 4 + j is the third corner of the rim face of the edge (j - 1, j)
    V[4:] = np.array([(-1, -0.5, -1), (1.5, -1, -1), (2, 1.5, 0.375), (0.5, 2, 0.125)], F)
    return V, T


def planar_ring(P, s=0.25):
    """annulus(P)'s connectivity around the planar counter-clockwise polygon P, the outer vertex of q_j at q_j + s (n_prev +
    n_next), n the outward unit normals of its two edges: for a small s every face of the ring faces +z whatever the polygon's
    shape (annulus scales about the mean, which folds the ring of a polygon that is not star-shaped).  The rim keeps P's
    coordinates; the outer vertices are in the plane too, which is all a crease asks of them."""
    P = np.asarray(P, np.float64)
    V, T = annulus(P)
    d = np.roll(P, -1, 0) - P                                       # edge j: q_j -> q_{j+1}
    nrm = np.stack([d[:, 1], -d[:, 0], np.zeros(len(P))], 1) / np.linalg.norm(d, axis=1)[:, None]
    V = V.copy()
    V[len(P):] = (P + s * (nrm + np.roll(nrm, 1, 0))).astype(F)
    return V, T


def collinear_loop():
    """A planar five-edge rim with three vertices on one line: (q_1, q_2, q_3) is a candidate of area 0, which has no normal
    and so no crease (badness 0), and must not be chosen for having none."""
    return annulus(np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (1.5, 2, 0)], np.float64))


def dome(n, radius=0.1, height=0.05, seed=0, lift=0.002):
    """n rim points on a circle (each lifted off its plane by `lift` times a normal deviate) whose ring of faces falls away
    below it: a rim that is not flat against its faces."""
    P = circle(n, radius, lift, seed)
    V, T = annulus(P)
    V = V.copy()
    V[n:, 2] -= F(height)
    return V, T


def _three_loops():
    """Rims of 5, 9 and 14 edges on domes; the last (radius 0.3) is above the limit of 1.0, as are all three outer loops."""
    a, b, c = dome(5, 0.1, 0.05, 1), dome(9, 0.1, 0.05, 2), dome(14, 0.3, 0.05, 3)
    return merge(a, (b[0] + F([1, 0, 0]), b[1]), (c[0] + F([3, 0, 0]), c[1]))


def _small_cutoff():
    """Rims of SMALL_LOOP and SMALL_LOOP + 1 edges: the workgroup of 256 and the one of 1024."""
    a, b = dome(SMALL_LOOP, 0.1, 0.05, 4), dome(SMALL_LOOP + 1, 0.1, 0.05, 5)
    return merge(a, (b[0] + F([1, 0, 0]), b[1]))


def _lds_cutoff():
    """Rims of ANGLE_LDS_LOOP edges (the longest whose table a workgroup's LDS holds) and of an edge more (the workspace)."""
    a, b = dome(ANGLE_LDS_LOOP, 0.1, 0.05, 6), dome(ANGLE_LDS_LOOP + 1, 0.1, 0.05, 7)
    return merge(a, (b[0] + F([1, 0, 0]), b[1]))


def _fallbacks():
    """A pinched loop (two holes of sheet(64) that share a vertex), a loop of two edges and a rim of MAX_LOOP + 1 edges."""
    c = annulus(circle(MAX_LOOP + 1, 0.1, 0.0005, 6))
    return merge(sheet(64, BOW_TIE), two_edge_loop(), (c[0] + F([3, 0, 0]), c[1]))


# name -> (mesh, max_hole_size)
TRIANGULATE = {
    "triangle": (lambda: dome(3, 0.1, 0.05), 1.0),
    "ridge_quad": (ridge_quad, 5.0),
    "pentagon": (lambda: dome(5, 0.1, 0.05, 7), 1.0),
    "square_tie": (lambda: annulus(np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], np.float64)), 5.0),
    "convex": (lambda: annulus(convex_polygon()), 16.0),
    "c_shape": (lambda: planar_ring(c_polygon()), 24.0),
    "collinear": (collinear_loop, 12.0),
    "three_loops": (_three_loops, 1.0),
    "small_cutoff": (_small_cutoff, 1.0),
    "lds_cutoff": (_lds_cutoff, 1.0),
    "fallbacks": (_fallbacks, 3.0),
    "closed": (lambda: icosphere(1), 3.0),
}
_MESHES, _REFERENCES = {}, {}


def triangulate_case(name):
    """(V, T, attributes, max_hole_size); the arrays are shared: do not write to them."""
    make, size = TRIANGULATE[name]
    if name not in _MESHES:
        V, T = make()
        _MESHES[name] = (np.ascontiguousarray(V, F), np.ascontiguousarray(T, np.int64), (colour_ramp(V),))
    return _MESHES[name] + (size,)


def triangulate_reference(name, metric="angle_area"):
    key = ("triangulate", name, metric)
    if key not in _REFERENCES:
        import meshsmooth_restatement as R
        V, T, att, size = triangulate_case(name)
        _REFERENCES[key] = R.triangulate_holes(V, T, size, att, metric)
    return _REFERENCES[key]


# ---------------------------------------------------------------------------------------------------------- fairing
def bumpy_grid(nx, ny, blocks, seed=0, lone=False):
    """grid(nx, ny) with smooth bumps in z and a little noise on everything; `blocks` = [(i0, i1, j0, j1)] free the vertices i0 <=
    i < i1, j0 <= j < j1 (keep them off the outline).  lone: one more vertex that no face uses, free."""
    V, T = grid(nx, ny)
    V = V.astype(np.float64)
    rng = np.random.default_rng(seed)
    V[:, 2] = 1.5 * np.sin(0.37 * V[:, 0]) * np.cos(0.23 * V[:, 1]) + 0.05 * rng.standard_normal(len(V))
    V[:, :2] += 0.1 * rng.uniform(-1, 1, (len(V), 2))
    free = np.zeros(len(V) + bool(lone), bool)
    for i0, i1, j0, j1 in blocks:
        j, i = np.meshgrid(np.arange(j0, j1), np.arange(i0, i1))
        free[(j * (nx + 1) + i).reshape(-1)] = True
    if lone:
        V = np.concatenate([V, [[-3.0, -3.0, 0.5]]])
        free[-1] = True
    return V.astype(F), T, free


def planar_fan():
    """The ring around the convex polygon at z = 1/2, closed by a fan whose centre, off the polygon's middle, is free: it moves
    in x and y and keeps the bits of its z (every umbrella's z is an exact 0)."""
    P = convex_polygon()
    V, T = annulus(P)
    n = len(P)
    V = np.concatenate([V, [[1.0, 1.25, 0.0]]]).astype(F)
    V[:, 2] = F(0.5)
    i = np.arange(n)
    T = np.concatenate([T, np.stack([i, (i + 1) % n, np.full(n, 2 * n)], 1)])
    free = np.zeros(len(V), bool)
    free[2 * n] = True
    return V, T, free


def sphere_cap(level=3, cut=0.8):
    """icosphere(level) with the vertices of the cap y > cut freed and flattened onto the plane y = cut: what a filled hole
    looks like before it is faired.  (V, T, free); the unit sphere about the origin is the surface to come back to."""
    V, T = icosphere(level)
    V = V.astype(np.float64)
    free = V[:, 1] > cut
    V[free, 1] = cut
    return V.astype(F), T, free


def radial_error(V, free):
    """The largest | |x| - 1 | over the free vertices."""
    return float(np.abs(np.linalg.norm(np.asarray(V, np.float64)[free], axis=1) - 1.0).max())


def mean_edge_length(V, T):
    V = np.asarray(V, np.float64)
    e = np.unique(np.sort(np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]]), 1), axis=0)
    return float(np.linalg.norm(V[e[:, 0]] - V[e[:, 1]], axis=1).mean())


def shared_rim_vertex():
    """grid(4, 4) with the vertices (1, 1) and (3, 3) free: not adjacent, and (2, 2) is a neighbour of both (the quads are cut
    along (i, j) - (i + 1, j + 1)): one patch of two vertices."""
    V, T, free = bumpy_grid(4, 4, [(1, 2, 1, 2), (3, 4, 3, 4)], 11)
    return V, T, free


def closed_free():
    V, T = icosphere(1)
    return V, T, np.ones(len(V), bool)


# name -> (mesh and free set, keyword arguments); the block of nx x ny free vertices of "block_nx_ny" has nx ny of them
FAIR = {
    "one_vertex": (lambda: bumpy_grid(4, 4, [(2, 3, 2, 3)], 1), {}),
    "planar_fan": (planar_fan, {}),
    "sphere_cap": (sphere_cap, {}),
    "block_1023": (lambda: bumpy_grid(34, 32, [(1, 34, 1, 32)], 2), {}),
    "block_1024": (lambda: bumpy_grid(33, 33, [(1, 33, 1, 33)], 3), {}),
    "block_1025": (lambda: bumpy_grid(42, 26, [(1, 42, 1, 26)], 4), {}),
    "two_patches": (lambda: bumpy_grid(24, 12, [(1, 9, 1, 11), (12, 17, 2, 6), (20, 21, 8, 9)], 5, lone=True), {}),
    "shared_rim": (shared_rim_vertex, {}),
    "closed": (closed_free, {}),
    "too_large": (lambda: bumpy_grid(258, 258, [(1, 258, 1, 258)], 6), {}),
    "capped": (lambda: bumpy_grid(33, 33, [(1, 33, 1, 33)], 3), {"max_iterations": 3}),
}


def fair_case(name):
    """(V, T, free, kwargs)."""
    key = ("fair", name)
    if key not in _MESHES:
        V, T, free = FAIR[name][0]()
        _MESHES[key] = (np.ascontiguousarray(V, F), np.ascontiguousarray(T, np.int64), free)
    return _MESHES[key] + (FAIR[name][1],)


def fair_reference(name):
    key = ("fair", name)
    if key not in _REFERENCES:
        import meshsmooth_restatement as R
        V, T, free, kw = fair_case(name)
        _REFERENCES[key] = R.fair_curvature(V, T, free, **kw)
    return _REFERENCES[key]


# --------------------------------------------------------------------------------------------------------- the fill
def cut_sphere(level=3, cut=0.8):
    """icosphere(level) without the faces that touch a vertex of the cap y > cut: one hole.  The unit sphere about the origin
    is the surface a patch should continue."""
    V, T = icosphere(level)
    return V, T[~np.isin(T, np.flatnonzero(V[:, 1] > cut)).any(1)]


# name -> (mesh, max_hole_size, max_edge_len or None for the mesh's mean edge length)
FILL = {
    "cut_sphere": (cut_sphere, 6.0, None),
    "holed_sheet": (holed_sheet, 1.0, 1.0 / 32),
}
SMOOTH = dict(triangulation="min_area", metric="angle_area", flip=True, fairing="curvature")


def fill_case(name):
    """(V, T, attributes, max_hole_size, max_edge_len)."""
    make, size, max_len = FILL[name]
    key = ("fill", name)
    if key not in _MESHES:
        V, T = make()
        _MESHES[key] = (np.ascontiguousarray(V, F), np.ascontiguousarray(T, np.int64), (colour_ramp(V),))
    return _MESHES[key] + (size, max_len)


def fill_reference(name, **how):
    key = ("fill", name, tuple(sorted(how.items())))
    if key not in _REFERENCES:
        import meshsmooth_restatement as R
        V, T, att, size, max_len = fill_case(name)
        _REFERENCES[key] = R.fill_holes_nicely(V, T, size, max_len, attributes=att, **how)
    return _REFERENCES[key]
