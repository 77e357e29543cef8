"""Oriented point clouds for the Poisson tests (host and GPU): a seeded sphere, its open cap, a sparse sampling and the splat's
edge cases.  Everything is float32 numpy; every scene of SCENES is small enough for the numpy restatement to solve in a second or
so.  LARGE holds the spheres of the depth-7 and depth-8 solver tests (a few iterations of them on the host), and the dense random
system, the mean's values and the sampler's queries are the inputs of the bit-for-bit kernel tests."""
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


# Scenes of the bit-for-bit solver tests that the numpy solve cannot finish in test time (a few iterations of them it can): the
# grid depths at which the second-level sums make more than one trip.  name -> (builder, depth); kept out of SCENES, whose every
# entry is solved to the end on the host.
LARGE = {
    "sphere7": (lambda: sphere(200000, seed=3), 7),        # 2 048 partials: two trips per thread
    "sphere8": (lambda: sphere(500000, seed=4), 8),        # 16 384 partials: 16 trips, the unrolled body twice
}
SMALL = {"sphere4": (lambda: sphere(5000, seed=5), 4)}     # the smallest grid: 4 partials


def any_scene(name):
    build, depth = {**SCENES, **LARGE, **SMALL}[name]
    p, n, c = build()
    return p, n, c, depth


def dense_random_system(depth, seed=11):
    """(b, D) fp32 [G,G,G] with no zero anywhere: b normal deviates in every cell, border cells included, D = the in-grid neighbour
    count + U(0, 2).  Every face, edge and corner of the stencil then changes the result."""
    G = 1 << depth
    rng = np.random.default_rng(seed + depth)
    b = rng.standard_normal((G, G, G)).astype(np.float32)
    nn = np.zeros((G, G, G), np.float32)
    for ax in range(3):
        idx = np.arange(G).reshape([G if a == ax else 1 for a in range(3)])
        nn = nn + (idx > 0) + (idx < G - 1)
    D = (nn.astype(np.float32) + rng.uniform(0.0, 2.0, (G, G, G)).astype(np.float32)).astype(np.float32)
    return b, D


def mean_values(n, wide=False, seed=13):
    """n fp32 values for the fp64 mean.  Default: normal deviates around a large common offset (1000).  These share one exponent,
    so they are multiples of 2^-14 and ANY order sums them exactly in fp64 (below 2^39 of them): they test the count, the ragged
    last block and the division, not the order.  wide: normal deviates scaled over 60 binades; their exact sum does not fit 53
    bits, so the order shows in the low bits of the mean."""
    rng = np.random.default_rng(seed + n % 1009)
    x = rng.standard_normal(n).astype(np.float32)
    if wide:
        return (x * np.exp2(rng.uniform(-30.0, 30.0, n)).astype(np.float32)).astype(np.float32)
    return (np.float32(1000.0) + x).astype(np.float32)


def sampler_queries(o, h, G, seed=17):
    """[n, 3] fp32 queries for the trilinear sampler on the grid (o, h, G): uniform in the cube; exactly on cell centres; on the
    cube's faces and corners; up to 3 h outside on every side; one at o + (G - 0.5) h on each axis (the last cell's centre)."""
    rng = np.random.default_rng(seed + G)
    o = np.asarray(o, np.float32)
    h = np.float32(h)
    s = np.float32(G) * h
    inside = o + rng.random((2000, 3)).astype(np.float32) * s
    centres = o + (rng.integers(0, G, (500, 3)).astype(np.float32) + np.float32(0.5)) * h
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    faces = rng.random((600, 3)).astype(np.float32)
    faces[np.arange(600), np.arange(600) % 3] = (np.arange(600) // 3 % 2).astype(np.float32)      # one coordinate on a face
    outside = o + (rng.random((1500, 3)).astype(np.float32) * (np.float32(G) + np.float32(6)) - np.float32(3)) * h
    last = np.full((3, 3), 0.37, np.float32) * s + o
    last[np.arange(3), np.arange(3)] = o[np.arange(3)] + (np.float32(G) - np.float32(0.5)) * h
    return np.concatenate([inside, centres, o + corners * s, o + faces * s, outside, last]).astype(np.float32)


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
