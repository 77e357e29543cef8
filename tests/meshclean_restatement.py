"""The semantics of csrc/meshclean.hip and collab_splats_amd/meshclean.py restated in numpy, one thread, with the kernels'
fp32 operation order (every fp32 expression below is evaluated step by step on np.float32 arrays: no fused multiply-add).
The oracle of tests/test_meshclean_gpu.py; tests/test_meshclean_host.py checks it against independent scipy forms."""
from __future__ import annotations

import math

import numpy as np

F = np.float32


# ------------------------------------------------------------------------------------------------------- edge table
def corner_edges(tri):
    """The 3 T directed edges in (face, corner) order: a [3T], b [3T], face [3T]; valid = a != b."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    a = tri.reshape(-1)
    b = tri[:, [1, 2, 0]].reshape(-1)
    face = np.repeat(np.arange(len(tri)), 3)
    return a, b, face, a != b


def edge_table(tri):
    """Undirected edges in first-seen order: (key [E] = lo << 32 | hi, count [E] of (face, corner) incidences, index of the
    edge of every corner [3T], -1 for a repeated corner, first corner of every edge [E])."""
    a, b, face, ok = corner_edges(tri)
    key = (np.minimum(a, b) << 32) | np.maximum(a, b)
    uniq, first, inv, cnt = np.unique(key[ok], return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first, kind="stable")                        # first-seen order
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    of_corner = np.full(len(a), -1, np.int64)
    of_corner[ok] = rank[inv]
    return uniq[order], cnt[order], of_corner, np.flatnonzero(ok)[first[order]]


def edge_length(V, a, b):
    V = np.asarray(V, F)
    d = V[b] - V[a]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def mesh_edge_stats(V, tri):
    a, b, _, _ = corner_edges(tri)
    _, cnt, _, first = edge_table(tri)
    length = edge_length(V, a[first], b[first]).astype(np.float64)
    return {"n_edges": len(cnt), "n_boundary": int((cnt == 1).sum()), "n_nonmanifold": int((cnt > 2).sum()),
            "mean_edge_length": float(length.sum() / len(cnt)) if len(cnt) else 0.0}


class _UnionFind:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, x):
        p = self.p
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def unite(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.p[max(a, b)] = min(a, b)                           # the root is the smallest member


def _number_by_smallest(roots):
    """Labels 0.. in ascending order of the root (= smallest member) and the label of every entry."""
    uniq, inv = np.unique(roots, return_inverse=True)
    return inv.astype(np.int32), uniq


def mesh_components(V, tri):
    """(face_labels [T] int32, sizes [C] int32): faces joined through shared undirected edges."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    T = len(tri)
    _, _, of_corner, _ = edge_table(tri)
    uf = _UnionFind(T)
    owner = {}
    for h in range(3 * T):
        e = of_corner[h]
        if e < 0:
            continue
        f = h // 3
        if e in owner:
            uf.unite(f, owner[e])
        else:
            owner[e] = f
    roots = np.array([uf.find(f) for f in range(T)], np.int64)
    labels, _ = _number_by_smallest(roots)
    return labels, np.bincount(labels, minlength=0).astype(np.int32)


def filter_mesh_components(V, tri, use_largest=False):
    """(vertices, triangles, vertex_index int64, n_removed)."""
    V = np.asarray(V, F)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    if len(tri) == 0:
        return V[:0], tri, np.zeros(0, np.int64), 0
    labels, sizes = mesh_components(V, tri)
    largest = int(np.argmax(sizes))                                 # numpy: the first maximum
    keep = np.zeros(len(sizes), bool)
    keep[largest] = True
    if not use_largest:
        lo = np.stack([V[tri[labels == c]].reshape(-1, 3).min(0) for c in range(len(sizes))])
        hi = np.stack([V[tri[labels == c]].reshape(-1, 3).max(0) for c in range(len(sizes))])
        keep |= ((lo >= lo[largest]) & (hi <= hi[largest])).all(1)
    kept = tri[keep[labels]]
    index = np.unique(kept)
    remap = np.full(len(V), -1, np.int64)
    remap[index] = np.arange(len(index))
    return V[index], remap[kept], index, int((~keep).sum())


# ------------------------------------------------------------------------------------------------------------ holes
def mesh_holes(V, tri):
    """(loop_of_edge [B] int32, edges [B,2] int32, n_edges [L] int32, perimeter [L] float64)."""
    a, b, _, _ = corner_edges(tri)
    _, cnt, of_corner, _ = edge_table(tri)
    on = np.flatnonzero((of_corner >= 0) & (cnt[np.maximum(of_corner, 0)] == 1))
    edges = np.stack([a[on], b[on]], 1).astype(np.int32).reshape(-1, 2)
    uf = _UnionFind(len(np.asarray(V).reshape(-1, 3)))
    for x, y in edges:
        uf.unite(int(x), int(y))
    roots = np.array([uf.find(int(x)) for x in edges[:, 0]], np.int64)
    loop, uniq = _number_by_smallest(roots)
    length = edge_length(V, edges[:, 0], edges[:, 1])
    n_edges = np.bincount(loop, minlength=len(uniq)).astype(np.int32)
    perimeter = np.array([length[loop == l].astype(np.float64).sum() for l in range(len(uniq))], np.float64)
    return loop, edges, n_edges, perimeter


def fill_holes(V, tri, max_hole_size=3.0):
    """(vertices, triangles int64, n_filled)."""
    V = np.asarray(V, F)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    loop, edges, _, perimeter = mesh_holes(V, tri)
    new_v, new_t = [], []
    for l in np.flatnonzero(perimeter < max_hole_size):
        mine = edges[loop == l].astype(np.int64)
        c = len(V) + len(new_v)
        new_v.append(V[np.unique(mine)].astype(np.float64).mean(0).astype(F))
        new_t += [(b, a, c) for a, b in mine]
    if not new_v:
        return V, tri, 0
    return np.concatenate([V, np.stack(new_v)]), np.concatenate([tri, np.array(new_t, np.int64)]), len(new_v)


# ------------------------------------------------------------------------------------------------------------ plane
M32 = 0xFFFFFFFF
MAX_DRAWS = 64


def draw_index(seed, i, draw, n):
    x = (seed * 0x9E3779B1 + i * 0x85EBCA77 + draw * 0xC2B2AE3D + 0x27D4EB2F) & M32
    x ^= x >> 16; x = (x * 0x85EBCA6B) & M32; x ^= x >> 13; x = (x * 0xC2B2AE35) & M32; x ^= x >> 16
    x = (x + i) & M32
    x ^= x >> 15; x = (x * 0x2C1B3C6D) & M32; x ^= x >> 12; x = (x * 0x297A2D39) & M32; x ^= x >> 15
    return (x * n) >> 32


def ransac_triples(n, num, seed):
    out = np.zeros((num, 3), np.int32)
    for i in range(num):
        ids, draw = [], 0
        while len(ids) < 3:
            c = draw_index(seed, i, draw, n)
            draw += 1
            if c in ids and draw > MAX_DRAWS:
                while c in ids:
                    c = 0 if c + 1 == n else c + 1
            if c not in ids:
                ids.append(c)
        out[i] = ids
    return out


def planes_from_triples(P, triples):
    P = np.asarray(P, F)
    t = np.asarray(triples, np.int64)
    p0, p1, p2 = P[t[:, 0]], P[t[:, 1]], P[t[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    norm = np.sqrt((nx * nx + ny * ny) + nz * nz)
    with np.errstate(divide="ignore", invalid="ignore"):
        nx, ny, nz = nx / norm, ny / norm, nz / norm
        d = -((nx * p0[:, 0] + ny * p0[:, 1]) + nz * p0[:, 2])
    planes = np.stack([nx, ny, nz, d], 1).astype(F)
    planes[~(norm > 0)] = np.nan
    return planes


def plane_residual(P, plane):
    P = np.asarray(P, F)
    a, b, c, d = (F(x) for x in plane)
    return np.abs(((a * P[:, 0] + b * P[:, 1]) + c * P[:, 2]) + d)


def plane_inlier_counts(P, planes, t):
    t = F(t)
    with np.errstate(invalid="ignore"):
        return np.array([int((plane_residual(P, pl) < t).sum()) for pl in np.asarray(planes, F)], np.int32)


def segment_plane(P, t=0.02, num=1000, seed=0, triples=None):
    """(plane [4] float64, inliers int64, winning index)."""
    P = np.asarray(P, F)
    triples = ransac_triples(len(P), num, seed) if triples is None else np.asarray(triples)
    planes = planes_from_triples(P, triples)
    counts = plane_inlier_counts(P, planes, t)
    best = int(np.argmax(counts))                                   # the first maximum: the lowest index
    with np.errstate(invalid="ignore"):
        inl = np.flatnonzero(plane_residual(P, planes[best]) < F(t))
    Q = P[inl].astype(np.float64)
    mean = Q.mean(0)
    cov = (Q - mean).T @ (Q - mean) / len(Q)
    normal = np.linalg.eigh(cov)[1][:, 0]
    if normal @ planes[best, :3].astype(np.float64) < 0:
        normal = -normal
    return np.concatenate([normal, [-(normal @ mean)]]), inl, best


# -------------------------------------------------------------------------------------------------------- alignment
def floor_rotation(plane):
    a, b, c, d = (float(x) for x in plane)
    n = np.array([a, b, c]) / math.sqrt(a * a + b * b + c * c)
    if n[2] < 0:
        n, d = -n, -d
    axis = np.cross(n, [0.0, 0.0, 1.0])
    s = np.linalg.norm(axis)
    if s < 1e-6:
        return np.eye(3), d
    k = axis / s
    ang = math.acos(min(1.0, max(-1.0, n[2])))
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K), d


def rotate(P, R):
    P = np.asarray(P, F).astype(np.float64)
    return np.stack([(R[i, 0] * P[:, 0] + R[i, 1] * P[:, 1]) + R[i, 2] * P[:, 2] for i in range(3)], 1).astype(F)


def align_floor_cloud(P, t=0.02, num=1000, seed=0):
    """(aligned [N,3] fp32, R, translation) for a point cloud."""
    plane, _, _ = segment_plane(P, t, num, seed)
    R, _ = floor_rotation(plane)
    rot = rotate(P, R)
    plane2, _, _ = segment_plane(rot, t, num, seed)
    tr = np.array([0.0, 0.0, -(plane2[3] if plane2[2] < 0 else -plane2[3])])       # d for the downward normal
    return (rot.astype(np.float64) + tr).astype(F), R, tr
