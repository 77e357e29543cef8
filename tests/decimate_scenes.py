"""Meshes for the decimation tests and scripts/decimate_bench.py (numpy; vertices fp32, triangles int64), and the checks of a
result that need no device: counts of boundary and non-manifold edges, components, boundary loops, area."""
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
