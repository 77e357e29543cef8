"""Oriented point clouds for the Poisson tests (host and GPU): a seeded sphere, its open cap, a sparse sampling and the splat's
edge cases.  Everything is float32 numpy; every scene is small enough for the numpy restatement to solve in well under a second."""
from __future__ import annotations

import numpy as np

CENTRE = np.array([0.1, -0.2, 0.3])
RADIUS = 0.5


def _dirs(n, seed):
    d = np.random.default_rng(seed).standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _colour(d):
    return (0.5 + 0.5 * d).astype(np.float32)              # a smooth colour field on the sphere, in [0, 1]


def sphere(n=20000, seed=0, noise=0.0):
    """(points, normals, colours): n seeded uniform directions on the sphere, normals = directions."""
    d = _dirs(n, seed)
    p = CENTRE + RADIUS * d
    if noise:
        p = p + noise * np.random.default_rng(seed + 1).standard_normal((n, 3))
    return p.astype(np.float32), d.astype(np.float32), _colour(d)


def cap(n=20000, seed=0, cut=-0.3):
    """The sphere's directions with n_z > cut: an open surface."""
    p, d, c = sphere(n, seed)
    keep = d[:, 2] > cut
    return p[keep], d[keep], c[keep]


# scene name -> (builder, depth); the sizes and depths of the issue
SCENES = {
    "sphere5": (lambda: sphere(20000), 5),
    "sphere6": (lambda: sphere(50000, seed=1), 6),
    "cap5": (lambda: cap(20000), 5),
    "sparse5": (lambda: sphere(2000, seed=2), 5),
}


def scene(name):
    build, depth = SCENES[name]
    p, n, c = build()
    return p, n, c, depth


def splat_edge_cases(depth=5, scale=1.1):
    """name -> (points, normals, colours or None, scale): what the splat must get exactly right.  The cell-centre case is built
    against the grid of its own bounding box at scale 1 (two anchor points pin lo and hi; they sit on the grid's corners, so their
    outer cells are clamped)."""
    rng = np.random.default_rng(7)
    out = {}
    p, n, c = sphere(500, seed=3)
    out["no_colours"] = (p, n, None, scale)
    out["duplicates"] = (np.concatenate([p[:100]] * 4), np.concatenate([n[:100]] * 4), np.concatenate([c[:100]] * 4), scale)
    nz = n.copy()
    nz[::7] = 0.0
    out["zero_normal"] = (p, nz, c, scale)
    # the extremes of the bounding box: its eight corners and face centres, normals pointing outward
    box = np.array([[x, y, z] for x in (-1.0, 0.0, 1.0) for y in (-0.5, 0.0, 0.5) for z in (-0.25, 0.0, 0.25)], np.float32)
    bn = box / np.maximum(np.linalg.norm(box, axis=1, keepdims=True), 1e-6)
    out["extremes"] = (box, bn.astype(np.float32), np.abs(bn).astype(np.float32), scale)
    # points exactly on cell centres: lo = 0, hi = G h0 with h0 a power of two makes s = G h0, h = h0 and o = 0 exact at scale 1
    G = 1 << depth
    h0 = np.float32(2.0 ** -4)
    pc = ((rng.integers(0, G, size=(300, 3)).astype(np.float32) + np.float32(0.5)) * h0).astype(np.float32)
    pc[0], pc[1] = 0.0, np.float32(G) * h0                  # the anchors of the bounding box
    out["cell_centres"] = (pc, _dirs(300, 9).astype(np.float32), rng.random((300, 3)).astype(np.float32), 1.0)
    return out
