"""Restatement of the kNN vertex map: the oracle of csrc/meshmap.hip.

``knn``: an fp32 brute force in numpy, in chunks of points: d2 = ((dx dx + dy dy) + dz dz) in fp32, neighbours ordered by
(d2, vertex index), d = sqrt(d2) (correctly rounded), valid iff d[0] <= float32(sdf_trunc).
``aggregate``: the map of steps 1-7 in fp64 from given neighbours, with the build's two divergences from the reference: the
row-shifted weights (a row whose exps all underflow stays finite) and weights 1/k when sigma = 0.
"""
from __future__ import annotations

import numpy as np


def knn(vertices, points, k, sdf_trunc, chunk=None):
    """(idx [N,k] int64, d [N,k] fp32, d2 [N,k] fp32, valid [N] bool) for every point, valid or not."""
    V = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    P = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    M, N = len(V), len(P)
    if chunk is None:
        chunk = max(1, min(N, (1 << 24) // max(M, 1)))
    idx = np.empty((N, k), np.int64)
    d2 = np.empty((N, k), np.float32)
    vid = np.arange(M, dtype=np.uint64)
    for a in range(0, N, chunk):
        p = P[a:a + chunk]
        dx = p[:, None, 0] - V[None, :, 0]
        dy = p[:, None, 1] - V[None, :, 1]
        dz = p[:, None, 2] - V[None, :, 2]
        q = (dx * dx + dy * dy) + dz * dz                                     # fp32, in this order
        key = (q.view(np.uint32).astype(np.uint64) << np.uint64(32)) | vid[None, :]
        part = np.argpartition(key, k - 1, axis=1)[:, :k] if k < M else np.broadcast_to(np.arange(M), key.shape)
        kk = np.take_along_axis(key, part, 1)
        order = np.argsort(kk, axis=1)
        kk = np.take_along_axis(kk, order, 1)
        idx[a:a + chunk] = (kk & np.uint64(0xFFFFFFFF)).astype(np.int64)
        d2[a:a + chunk] = (kk >> np.uint64(32)).astype(np.uint32).view(np.float32)
    d = np.sqrt(d2)
    valid = d[:, 0] <= np.float32(sdf_trunc)
    return idx, d, d2, valid


def weights(d, valid):
    """Row weights [N,k] fp64 (0 on invalid rows) and sigma."""
    d = np.asarray(d, np.float64)
    w = np.zeros_like(d)
    if not valid.any():
        return w, 0.0
    k = d.shape[1]
    dv = d[valid]
    sigma = float(dv.sum() / (len(dv) * k))
    if sigma == 0.0:
        w[valid] = 1.0 / k
        return w, sigma
    e = np.exp(-(dv * dv - dv[:, :1] * dv[:, :1]) / (2.0 * sigma * sigma))
    w[valid] = e / e.sum(1, keepdims=True)
    return w, sigma


def aggregate(n_vertices, idx, d, valid, values, normalise=False):
    """[M,D] fp64: sum w F / sum w per vertex over the valid (i, j); 0 without a contribution; with ``normalise`` the
    result divided by (its norm + 1e-8) (normals2vertex)."""
    F = np.asarray(values, np.float64)
    valid = np.asarray(valid, bool)
    M, D = n_vertices, F.shape[1]
    w, _ = weights(d, valid)
    num = np.zeros((M, D))
    den = np.zeros(M)
    if valid.any():
        iv = np.nonzero(valid)[0]
        vi = np.asarray(idx)[iv].reshape(-1)
        wi = w[iv].reshape(-1)
        np.add.at(num, vi, wi[:, None] * np.repeat(F[iv], idx.shape[1], axis=0))
        np.add.at(den, vi, wi)
    out = np.where(den[:, None] > 0, num / np.where(den > 0, den, 1.0)[:, None], 0.0)
    if normalise:
        out = out / (np.linalg.norm(out, axis=1, keepdims=True) + 1e-8)
    return out


def map_values(vertices, points, values, k=5, sdf_trunc=0.03, normalise=False):
    idx, d, _, valid = knn(vertices, points, k, sdf_trunc)
    return aggregate(len(np.asarray(vertices).reshape(-1, 3)), idx, d, valid, values, normalise)
