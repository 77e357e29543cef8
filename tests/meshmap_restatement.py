"""Restatement of the kNN vertex map: the oracle of csrc/meshmap.hip.

``knn``: an fp32 brute force in numpy, in chunks of points: d2 = ((dx dx + dy dy) + dz dz) in fp32, neighbours ordered by
(d2, vertex index), d = sqrt(d2) (correctly rounded), valid iff d[0] <= float32(sdf_trunc).
``aggregate``: the map of steps 1-7 in fp64 from given neighbours, with the build's two divergences from the reference: the
row-shifted weights (a row whose exps all underflow stays finite) and weights 1/k when sigma = 0.
``aggregate_ordered``: the same map in fp32, in the kernel's written order and chunking: the yardstick of the rounding that
the fp64 form is blind to, and bit for bit the kernel's output where no exp is involved (k = 1, sigma = 0).
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


def row_weights_fp32(d, valid):
    """Row weights [N,k] fp32 (0 on invalid rows) in the kernel's written order: sigma in fp64 from the fp32 distances,
    c = float32(1 / (2 sigma^2)), delta = dj dj - d0 d0 in fp32, e = 1 when flat or delta <= 0 else exp(-(delta c)), the row
    sum in j order, w = e / sum."""
    d = np.ascontiguousarray(d, np.float32)
    valid = np.asarray(valid, bool)
    w = np.zeros(d.shape, np.float32)
    if not valid.any():
        return w
    k = d.shape[1]
    dv = d[valid]
    sigma = float(dv.astype(np.float64).sum() / (len(dv) * k))
    flat = not sigma > 0.0
    c = np.float32(0.0 if flat else 1.0 / (2.0 * sigma * sigma))
    delta = dv * dv - (dv[:, :1] * dv[:, :1])
    with np.errstate(under="ignore"):
        e = np.where(flat | ~(delta > 0), np.float32(1), np.exp(-(np.where(delta > 0, delta, np.float32(0)) * c)))
    e = e.astype(np.float32)
    s = np.zeros(len(dv), np.float32)
    for j in range(k):
        s = s + e[:, j]
    w[valid] = e / s[:, None]
    return w


def aggregate_ordered(n_vertices, idx, d, valid, values, normalise=False, chunk=512):
    """[M,D] fp32: the map in the kernel's arithmetic and order.  The weights of ``row_weights_fp32``; per vertex the
    contributions w F in (i, j) order, summed in fp32 from 0 in chunks of ``chunk``, the chunk sums in chunk order from 0, the
    division by the weight sum (summed the same way; 0 unless it is positive); with ``normalise`` the first three channels
    divided by (sqrt((x x + y y) + z z) + float32(1e-8)).  With k = 1 (w = 1) and with sigma = 0 (w = float32(1) / float32(k))
    no exp is involved and the kernel's output is this one bit for bit."""
    F = np.ascontiguousarray(values, np.float32)
    idx = np.asarray(idx)
    valid = np.asarray(valid, bool)
    M, D = n_vertices, F.shape[1]
    k = idx.shape[1]
    out = np.zeros((M, D), np.float32)
    w = row_weights_fp32(d, valid)
    iv = np.nonzero(valid)[0]
    if len(iv):
        vert = idx[iv].reshape(-1)
        order = np.argsort(vert, kind="stable")                           # each list in (i, j) order
        rows = np.repeat(iv, k)[order]
        ws = w[iv].reshape(-1)[order]
        terms = np.concatenate([ws[:, None] * F[rows], ws[:, None]], axis=1)      # fp32 products; column D: the weight
        offs = np.searchsorted(vert[order], np.arange(M + 1))
        zero = np.zeros((1, D + 1), np.float32)
        for v in np.nonzero(offs[1:] > offs[:-1])[0]:
            parts = [zero]
            for e0 in range(offs[v], offs[v + 1], chunk):
                e1 = min(e0 + chunk, offs[v + 1])
                parts.append(np.add.accumulate(np.concatenate([zero, terms[e0:e1]]), axis=0)[-1:])
            tot = np.add.accumulate(np.concatenate(parts), axis=0)[-1]
            if tot[D] > 0:
                out[v] = tot[:D] / tot[D]
    if normalise:
        x, y, z = out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()
        nrm = np.sqrt((x * x + y * y) + z * z) + np.float32(1e-8)
        out[:, 0], out[:, 1], out[:, 2] = x / nrm, y / nrm, z / nrm
    return out


def map_values(vertices, points, values, k=5, sdf_trunc=0.03, normalise=False):
    idx, d, _, valid = knn(vertices, points, k, sdf_trunc)
    return aggregate(len(np.asarray(vertices).reshape(-1, 3)), idx, d, valid, values, normalise)
