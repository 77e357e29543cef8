"""Inputs of the mesh-query tests (numpy only): point sets with a similarity field or a mask."""
from __future__ import annotations

import numpy as np


def sphere_blobs(n, seed, radius=0.3, n_blobs=12, width=0.15, noise=0.05):
    """n random points on a sphere and a similarity field of Gaussian blobs around n_blobs centres plus noise: (V fp32 [n,3],
    sim fp32 [n])."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = rng.standard_normal((n_blobs, 3))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    sim = np.exp(-((d[:, None, :] - c[None]) ** 2).sum(-1) / (2 * width ** 2)).max(1) + noise * rng.standard_normal(n)
    return (d * radius).astype(np.float32), sim.astype(np.float32)


def strict_grid(n=6):
    """n^3 points spaced 2^-5 exactly: nearest neighbours at d2 == r2 in fp32 for r = 2^-5."""
    g = np.arange(n, dtype=np.float32) * np.float32(2.0 ** -5)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def ten_and_eleven(r=0.03):
    """Two straight chains spaced 0.5 r, of 10 and of 11 points, 1 m apart, indices interleaved: (V, sizes by first index)."""
    a = np.stack([np.arange(10) * 0.5 * r, np.zeros(10), np.zeros(10)], 1)
    b = np.stack([np.arange(11) * 0.5 * r, np.ones(11), np.zeros(11)], 1)
    V = np.zeros((21, 3))
    V[0:20:2], V[1:20:2], V[20] = a, b[:10], b[10]
    return V.astype(np.float32)


def chains(n=50000, r=0.01, seed=0):
    """A chain of n points spaced 0.9 r along a helix and a second one of n // 2 points 1.5 r beside it, indices shuffled:
    (V, chain id per vertex)."""
    rng = np.random.default_rng(seed)
    R = 0.5                                                    # helix radius; pitch 4 r per turn keeps turns > r apart

    def helix(m, offset):
        s = np.arange(m) * 0.9 * r                             # arc length
        turn = np.sqrt((2 * np.pi * R) ** 2 + (4 * r) ** 2)
        t = s / turn
        return np.stack([(R + offset) * np.cos(2 * np.pi * t), (R + offset) * np.sin(2 * np.pi * t), 4 * r * t], 1)

    V = np.concatenate([helix(n, 0.0), helix(n // 2, 1.5 * r)])
    ids = np.concatenate([np.zeros(n, np.int64), np.ones(n // 2, np.int64)])
    p = rng.permutation(len(V))
    return V[p].astype(np.float32), ids[p]
