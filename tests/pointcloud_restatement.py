"""Restatement of the point-cloud cleaning: the oracle of csrc/pointcloud.hip.  numpy, with scipy's
cKDTree only as a source of CANDIDATES that are then re-ranked by the fp32 rule.

``d2``: ((dx dx + dy dy) + dz dz) in fp32, in this order.  ``knn_mean_distance``: the k smallest d2 per query (a multiset: no
tie rule), mean = the fp32 sum of sqrt(d2) in ascending order / float32(k), nearest = sqrt of the smallest.
``statistical_outlier``: Open3D's rule with mu and sigma in fp64 in the device's reduction order (``fixed_sum``).
``radius_count``: d2 < r2, r2 = r r in fp32, the point itself included.  ``voxel_down_sample``: Open3D's rule in fp64, voxels
in ascending order of their smallest member.
"""
from __future__ import annotations

import numpy as np

from meshquery_restatement import candidate_pairs


def d2(q, p):
    """fp32 squared distance between rows of two broadcastable [..., 3] fp32 arrays."""
    q, p = np.asarray(q, np.float32), np.asarray(p, np.float32)
    dx, dy, dz = q[..., 0] - p[..., 0], q[..., 1] - p[..., 1], q[..., 2] - p[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def knn_d2(points, k, queries=None, extra=8, chunk=1 << 15):
    """[Nq, k_eff] fp32: the k_eff = min(k, N) smallest fp32 d2 of every query, ascending.  The candidates are the k_eff +
    extra nearest in fp64; a row whose last candidate is not clearly beyond its k-th fp32 distance is redone over all points."""
    from scipy.spatial import cKDTree
    P = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    Q = P if queries is None else np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    n, k_eff = len(P), min(k, len(P))
    out = np.empty((len(Q), k_eff), np.float32)
    if len(Q) == 0:
        return out
    kc = min(n, k_eff + extra)
    tree = cKDTree(P.astype(np.float64))
    for s in range(0, len(Q), chunk):
        q = Q[s:s + chunk]
        dist, idx = tree.query(q.astype(np.float64), k=kc)
        dist, idx = dist.reshape(len(q), kc), idx.reshape(len(q), kc)
        cand = np.sort(d2(q[:, None, :], P[idx]), axis=1)
        out[s:s + chunk] = cand[:, :k_eff]
        if kc < n:
            unsure = np.nonzero(~(dist[:, -1] * (1 - 1e-5) > np.sqrt(cand[:, k_eff - 1].astype(np.float64))))[0]
            for i in unsure:
                out[s + i] = np.sort(d2(q[i][None, :], P))[:k_eff]
    return out


def knn_mean_distance(points, k, queries=None):
    """(mean [Nq] fp32, nearest [Nq] fp32)."""
    best = knn_d2(points, k, queries)
    if best.shape[1] == 0:                                         # an empty cloud (and then no query either)
        return np.zeros(len(best), np.float32), np.zeros(len(best), np.float32)
    d = np.sqrt(best)                                            # fp32, correctly rounded
    s = np.zeros(len(d), np.float32)
    for j in range(d.shape[1]):                                    # ascending order, one fp32 add at a time
        s = s + d[:, j]
    return s / np.float32(d.shape[1]), d[:, 0].copy()


def _tree256(x):
    """The device's sum of 256 fp64 values: four waves, each a halving tree over 64 lanes, then ((w0 + w1) + w2) + w3."""
    w = np.array(x, np.float64).reshape(*x.shape[:-1], 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        w[..., :off] = w[..., :off] + w[..., off:2 * off]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def fixed_sum(values):
    """The device's fixed-order fp64 sum: 256 values per workgroup (``_tree256``), the workgroup sums strided over 256 threads,
    each adding its own in ascending order, and those through the same tree."""
    v = np.asarray(values, np.float64).reshape(-1)
    nb = (len(v) + 255) // 256
    part = _tree256(np.concatenate([v, np.zeros(nb * 256 - len(v))]).reshape(nb, 256)) if nb else np.zeros(0)
    rounds = (nb + 255) // 256
    part = np.concatenate([part, np.zeros(rounds * 256 - nb)]).reshape(rounds, 256)
    s = np.zeros(256)
    for r in range(rounds):
        s = s + part[r]
    return float(_tree256(s))


def outlier_threshold(avg, std_ratio=2.0):
    """(threshold fp64 or +inf, n_valid)."""
    avg = np.asarray(avg, np.float32)
    valid = avg > 0
    a = np.where(valid, avg.astype(np.float64), 0.0)
    n = fixed_sum(valid.astype(np.float64))
    if not n > 1:
        return np.inf, int(n)
    mu = fixed_sum(a) / n
    dev = np.where(valid, avg.astype(np.float64) - mu, 0.0)
    return mu + float(std_ratio) * np.sqrt(fixed_sum(dev * dev) / (n - 1.0)), int(n)


def statistical_outlier(points, nb_neighbors=20, std_ratio=2.0):
    """(keep [N] bool, avg [N] fp32)."""
    avg, _ = knn_mean_distance(points, nb_neighbors)
    thr, _ = outlier_threshold(avg, std_ratio)
    return (avg > 0) & (avg.astype(np.float64) < thr), avg


def radius_count(points, radius, queries=None):
    """[Nq] int32: points with d2 < r2 (fp32, strict), the point itself included when the points query themselves."""
    P = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    r = np.float32(radius)
    r2 = r * r
    if queries is None:
        cnt = (d2(P, P) < r2).astype(np.int64)                     # the point itself: d2 = 0
        for a, b in candidate_pairs(P, float(r)):
            near = d2(P[a], P[b]) < r2
            cnt += np.bincount(a[near], minlength=len(P)) + np.bincount(b[near], minlength=len(P))
        return cnt.astype(np.int32)
    from scipy.spatial import cKDTree
    Q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    if len(P) == 0:
        return np.zeros(len(Q), np.int32)
    lists = cKDTree(P.astype(np.float64)).query_ball_point(Q.astype(np.float64), float(r) * (1 + 1e-5))
    return np.array([int((d2(Q[i][None, :], P[np.asarray(l, np.int64)]) < r2).sum()) for i, l in enumerate(lists)], np.int32)


def density_filter(points, radius=0.03, percentile=10):
    """ind int64 ascending."""
    cnt = radius_count(points, radius)
    if len(cnt) == 0:
        return np.zeros(0, np.int64)
    return np.nonzero(cnt >= np.percentile(cnt, percentile))[0]


def voxel_down_sample(points, voxel_size, attributes=(), min_bound=None):
    """(points [V,3] fp32, [attributes [V,D] fp32], first_index [V] int64, counts [V] int32)."""
    P = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    if len(P) == 0:
        return P, [np.zeros((0, np.asarray(a).shape[1]), np.float32) for a in attributes], np.zeros(0, np.int64), np.zeros(0, np.int32)
    P64 = P.astype(np.float64)
    mb = P64.min(0) if min_bound is None else np.asarray(min_bound, np.float64)
    origin = mb - float(voxel_size) / 2
    cell = np.floor((P64 - origin) / float(voxel_size)).astype(np.int64)
    _, first, inverse = np.unique(cell, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))                # voxels in ascending order of their smallest member
    vid = rank[inverse]
    counts = np.bincount(vid, minlength=len(first))

    def mean(x):
        x = np.asarray(x, np.float32).astype(np.float64)
        acc = np.zeros((len(first), x.shape[1]))
        np.add.at(acc, vid, x)                                     # unbuffered: one add per point, in ascending point index
        return (acc / counts[:, None].astype(np.float64)).astype(np.float32)

    return mean(P), [mean(a) for a in attributes], np.sort(first).astype(np.int64), counts.astype(np.int32)
