"""Meshes and clouds for the mesh-finishing tests and scripts/meshclean_bench.py (numpy; vertices fp32, triangles int64)."""
from __future__ import annotations

import numpy as np

F = np.float32

TETRA = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int64)


def tetra_pair(shared):
    """Two tetrahedra sharing `shared` (1: a vertex, 2: an edge) of their vertices.  (V [8 - shared, 3], tri [8,3])."""
    a = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    b = np.array([[0, 0, 0], [1, 0, 0], [0, -1, 0], [0, 0, -1]], F)
    if shared == 1:
        b[1] = [-1, 0, 0]
    V = np.concatenate([a, b[shared:]])
    second = np.concatenate([np.arange(shared), 4 + np.arange(4 - shared)])
    return V, np.concatenate([TETRA, second[TETRA]])


def strip(n, y0=0.0, step=0.001):
    """A 1 x n-quad strip along x: 2 (n + 1) vertices, 2 n triangles in order along the strip."""
    x = (np.arange(n + 1) * step).astype(F)
    V = np.concatenate([np.stack([x, np.full_like(x, y0), np.zeros_like(x)], 1),
                        np.stack([x, np.full_like(x, y0 + step), np.zeros_like(x)], 1)]).astype(F)
    i = np.arange(n)
    lo, hi = i, i + n + 1
    tri = np.stack([np.stack([lo, lo + 1, hi + 1], 1), np.stack([lo, hi + 1, hi], 1)], 1).reshape(-1, 3)
    return V, tri.astype(np.int64)


def icosphere(level, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """A welded icosphere: 20 4^level faces, closed, every edge with two faces."""
    p = (1 + 5 ** 0.5) / 2
    V = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    V = [np.array(v, np.float64) / np.linalg.norm(v) for v in V]
    tri = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
           (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, out = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                v = V[a] + V[b]
                V.append(v / np.linalg.norm(v))
                mid[k] = len(V) - 1
            return mid[k]

        for a, b, c in tri:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        tri = out
    return (np.asarray(V) * radius + np.asarray(centre, np.float64)).astype(F), np.asarray(tri, np.int64)


def merge(*meshes):
    """Meshes side by side in one vertex and one face list (no welding)."""
    Vs, Ts, base = [], [], 0
    for V, T in meshes:
        Vs.append(V)
        Ts.append(T + base)
        base += len(V)
    return np.concatenate(Vs).astype(F), np.concatenate(Ts)


def aabb_scene():
    """A large icosphere and three small ones: inside its bounding box, touching the box's +x face at exact fp32 equality,
    straddling that face.  Returns (V, tri, faces per part)."""
    big = icosphere(3)
    hi_x = big[0][:, 0].max()
    inside = icosphere(1, 0.05, (0.9, 0.9, 0.9))                    # outside the sphere, inside its box
    touch = icosphere(1, 0.05, (0.9, -0.9, 0.9))
    touch[0][np.argmax(touch[0][:, 0]), 0] = hi_x                   # one vertex exactly on the face, the others inside
    straddle = icosphere(1, 0.05, (float(hi_x), 0.9, -0.9))
    V, T = merge(big, inside, touch, straddle)
    assert touch[0][:, 0].max() == hi_x and straddle[0][:, 0].max() > hi_x
    return V, T, [len(m[1]) for m in (big, inside, touch, straddle)]


def sheet(n=64, holes=()):
    """An n x n-quad sheet over [0,1]^2 at z = 0 (vertex j (n + 1) + i at (i / n, j / n): exact in fp32 for n a power of two)
    without the quads of `holes` = [(i0, i1, j0, j1)] (quads i0 <= i < i1, j0 <= j < j1).  Every grid vertex stays in the list,
    the ones inside a hole unreferenced."""
    g = np.arange(n + 1, dtype=np.float64) / n
    X, Y = np.meshgrid(g, g)
    V = np.stack([X.reshape(-1), Y.reshape(-1), np.zeros((n + 1) ** 2)], 1).astype(F)
    keep = np.ones((n, n), bool)                                    # [j, i]
    for i0, i1, j0, j1 in holes:
        keep[j0:j1, i0:i1] = False
    j, i = np.nonzero(keep)
    a = j * (n + 1) + i
    b, c, d = a + 1, a + n + 2, a + n + 1
    tri = np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3)
    return V, tri.astype(np.int64)


THREE_HOLES = [(8, 16, 8, 20), (30, 34, 40, 50), (50, 60, 10, 14)]
BOW_TIE = [(10, 14, 10, 14), (14, 18, 14, 18)]                      # two holes that share the grid vertex (14, 14)


def planted_plane(n=20000, frac=0.6, normal=(0.3, -0.2, 0.9), offset=0.4, t=0.02, seed=0, clutter_gap=0.0):
    """n points: frac of them on the plane n . x = offset (|n| = 1 after normalising) with uniform noise of +- t / 4 along
    the normal, spread over a 2 x 2 patch; the rest clutter: uniform in the cube [-1.5, 1.5]^3 (clutter_gap 0), or between
    clutter_gap and clutter_gap + 1 above the plane along the normal's upward side.  Shuffled.  Returns (P fp32, unit normal)."""
    rng = np.random.default_rng(seed)
    nrm = np.asarray(normal, np.float64)
    nrm = nrm / np.linalg.norm(nrm)
    u = np.cross(nrm, [1.0, 0.0, 0.0] if abs(nrm[0]) < 0.9 else [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    w = np.cross(nrm, u)
    k = int(n * frac)
    st = rng.uniform(-1, 1, (k, 2))
    on = offset * nrm + st[:, :1] * u + st[:, 1:] * w + rng.uniform(-t / 4, t / 4, (k, 1)) * nrm
    if clutter_gap > 0:
        up = nrm if nrm[2] >= 0 else -nrm
        st = rng.uniform(-1, 1, (n - k, 2))
        off = offset * nrm + st[:, :1] * u + st[:, 1:] * w + rng.uniform(clutter_gap, clutter_gap + 1, (n - k, 1)) * up
    else:
        off = rng.uniform(-1.5, 1.5, (n - k, 3))
    P = np.concatenate([on, off])
    return P[rng.permutation(n)].astype(F), nrm
