"""Restatement of the mesh queries: the oracle of csrc/cluster.hip and of meshquery.query_similarity.
numpy only.

``edges``: the fp32 edge rule -- selected vertices i < j are joined iff d2 < r2, d2 = ((dx dx + dy dy) + dz dz) and r2 = r r in
fp32 -- evaluated over the candidate pairs of a sort-by-cell join (cells of edge slightly above r in fp64: a superset of the
pairs within r).  ``components``: union-find with the invariant parent <= index (hook the larger root under the smaller,
pointer jumping), so a component's root is its smallest member.  ``labelling``: the canonical output (what scipy's
connected_components labelling yields in the reference): kept clusters numbered in ascending order of their smallest member.
``similarity``: the reference's compute_similarity in fp64, written as the reference writes it.
"""
from __future__ import annotations

import numpy as np

_HALF = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) >= (0, 0, 0)]   # 14 of 27


def candidate_pairs(points, radius, chunk=1 << 22):
    """Yield (a, b) index arrays (into points, a != b, every unordered pair at most once) covering every pair closer than
    radius on each axis: the pairs of points in the same or in adjacent cells of edge 1.0001 radius."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    n = len(P)
    if n == 0:
        return
    h = float(radius) * 1.0001
    cell = np.floor(P / h).astype(np.int64)
    cell -= cell.min(0)
    span = cell.max(0) + 3                                     # room for the +-1 offsets
    key = ((cell[:, 2] + 1) * span[1] + (cell[:, 1] + 1)) * span[0] + (cell[:, 0] + 1)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    for dx, dy, dz in _HALF:
        other = key + (dz * span[1] + dy) * span[0] + dx
        lo = np.searchsorted(skey, other, "left")
        hi = np.searchsorted(skey, other, "right")
        cnt = hi - lo
        for s in range(0, n, max(1, chunk // max(1, int(cnt.max())))):
            e = min(n, s + max(1, chunk // max(1, int(cnt.max()))))
            c = cnt[s:e]
            tot = int(c.sum())
            if tot == 0:
                continue
            a = np.repeat(np.arange(s, e), c)
            within = np.arange(tot) - np.repeat(np.cumsum(c) - c, c)
            b = order[np.repeat(lo[s:e], c) + within]
            keep = (a < b) if (dx, dy, dz) == (0, 0, 0) else np.ones(tot, bool)
            yield a[keep], b[keep]


def edge_rule(va, vb, radius):
    """The fp32 edge rule for rows of two [n,3] fp32 arrays."""
    va, vb = np.asarray(va, np.float32), np.asarray(vb, np.float32)
    r = np.float32(radius)
    r2 = r * r
    dx, dy, dz = va[:, 0] - vb[:, 0], va[:, 1] - vb[:, 1], va[:, 2] - vb[:, 2]
    d2 = (dx * dx + dy * dy) + dz * dz                                          # fp32, in this order
    return d2 < r2


def edges(vertices, mask, radius):
    """(sel, ea, eb): the selected vertex indices (ascending) and the edges as positions into sel, each unordered pair once."""
    V = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    sel = np.nonzero(np.asarray(mask).reshape(-1))[0]
    Vs = V[sel]
    ea, eb = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for a, b in candidate_pairs(Vs, radius):
        k = edge_rule(Vs[a], Vs[b], radius)
        ea.append(a[k])
        eb.append(b[k])
    return sel, np.concatenate(ea), np.concatenate(eb)


def components(n, ea, eb):
    """root [n]: the smallest member of each node's connected component."""
    parent = np.arange(n, dtype=np.int64)
    while True:
        while True:                                            # pointer jumping: every node to its root
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
        ra, rb = parent[ea], parent[eb]
        d = ra != rb
        if not d.any():
            return parent
        np.minimum.at(parent, np.maximum(ra, rb)[d], np.minimum(ra, rb)[d])    # the larger root under a smaller one


def labelling(n_vertices, sel, root, min_cluster_size=10):
    """(labels [M] int32, sizes [n_clusters] int32) from the roots (positions into sel) of the selected vertices."""
    labels = np.full(n_vertices, -1, np.int32)
    if len(sel) == 0:
        return labels, np.zeros(0, np.int32)
    size = np.bincount(root, minlength=len(sel))
    kept = size > min_cluster_size                            # only a root has a size: ascending root = ascending smallest member
    rank = np.cumsum(kept) - 1
    ok = kept[root]
    labels[sel[ok]] = rank[root[ok]].astype(np.int32)
    return labels, size[kept].astype(np.int32)


def cluster_labels(vertices, mask, radius, min_cluster_size=10):
    V = np.asarray(vertices).reshape(-1, 3)
    sel, ea, eb = edges(V, mask, radius)
    return labelling(len(V), sel, components(len(sel), ea, eb), min_cluster_size)


def cluster_lists(labels, sizes):
    """One ascending int64 array of vertex indices per cluster."""
    return [np.nonzero(labels == c)[0].astype(np.int64) for c in range(len(sizes))]


def mesh_clustering(vertices, similarity_values, similarity_threshold=0.8, spatial_radius=0.03, min_cluster_size=10):
    sim = np.asarray(similarity_values, np.float32).reshape(-1)
    labels, sizes = cluster_labels(vertices, sim > np.float32(similarity_threshold), spatial_radius, min_cluster_size)
    return cluster_lists(labels, sizes)


def _softmax(x, axis):
    x = x - x.max(axis=axis, keepdims=True)
    e = np.exp(x)
    return e / e.sum(axis=axis, keepdims=True)


def similarity(features, text_embeddings, n_positive, method="pairwise", softmax_temp=0.05, decoder=None):
    """[M] fp64.  decoder: (w_hidden, b_hidden, w_out, b_out) or None."""
    x = np.asarray(features, np.float64)
    if decoder is not None:
        w_h, b_h, w_o, b_o = (np.asarray(t, np.float64) for t in decoder)
        x = np.maximum(x @ w_h.T + b_h, 0.0) @ w_o.T + b_o
    raw = x @ np.asarray(text_embeddings, np.float64).T                          # [M,Q]
    if method == "standard":
        return _softmax(raw / softmax_temp, 1)[:, :n_positive].sum(1)
    if method != "pairwise":
        raise ValueError(method)
    pos, neg = raw[:, :n_positive], raw[:, n_positive:]
    paired = np.concatenate([np.repeat(pos.mean(1, keepdims=True), neg.shape[1], 1), neg], 1)
    with np.errstate(invalid="ignore"):
        probs = _softmax(paired / softmax_temp, 1)
    out = probs[:, :neg.shape[1]].min(1)
    return np.where(np.isnan(out), 0.0, out)
