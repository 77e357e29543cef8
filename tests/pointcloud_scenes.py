"""Inputs of the point-cloud tests (numpy only)."""
from __future__ import annotations

import numpy as np


def shell(n, seed, radius=0.3, noise=0.002, outliers=0.01):
    """n points on a sphere shell of the given radius with Gaussian radial noise; a fraction ``outliers`` of them (random
    rows) replaced by uniform samples of [-1.5, 1.5]^3.  fp32 [n,3]."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    P = d * (radius + noise * rng.standard_normal((n, 1)))
    m = int(round(outliers * n))
    if m:
        P[rng.choice(n, m, replace=False)] = rng.uniform(-1.5, 1.5, (m, 3))
    return P.astype(np.float32)


def uniform(n, seed, extent=0.4):
    return (np.random.default_rng(seed).random((n, 3)) * extent).astype(np.float32)


def duplicates(n_sites, copies, seed, extent=0.25):
    """n_sites positions, each ``copies`` times, shuffled: fp32 [n_sites copies, 3]."""
    rng = np.random.default_rng(seed)
    base = (rng.random((n_sites, 3)) * extent).astype(np.float32)
    return np.concatenate([base] * copies)[rng.permutation(n_sites * copies)]


def clustered(n, n_clusters, seed, spread=0.004, extent=0.5):
    """Tight Gaussian clusters far apart relative to their size (empty space between them) plus every 50th point repeated."""
    rng = np.random.default_rng(seed)
    c = rng.random((n_clusters, 3)) * extent
    P = (c[rng.integers(0, n_clusters, n)] + spread * rng.standard_normal((n, 3))).astype(np.float32)
    P[1::50] = P[0::50][:len(P[1::50])]
    return P


def far(n, seed):
    """A shell with outliers translated to (2000, -1500, 2500): one float step is 2.4e-4 there."""
    return (shell(n, seed).astype(np.float64) + np.array([2000.0, -1500.0, 2500.0])).astype(np.float32)
