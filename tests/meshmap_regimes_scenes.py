"""Scenes of the kNN vertex map's regime tests (tests/test_meshmap_regimes_host.py, tests/test_meshmap_regimes_gpu.py): the
inputs and, computed once and shared, their restatements (tests/meshmap_restatement.py) and the per-vertex bar, whose
derivation is the docstring of tests/test_meshmap_regimes_gpu.py.  Everything is numpy; nothing here touches the GPU."""
import functools
import os
import re

import numpy as np

import meshmap_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "collab_splats_amd", "csrc")
U = 2.0 ** -24                                   # fp32 unit roundoff
EXP_ULPS = 3                                     # see the derivation: the device's expf documents 1, numpy's fp32 exp under 3
K_CLASSES = (1, 4, 5, 8, 9, 16)                  # both ends of knn_kernel<4>, <8> and <16>, and k = 1


def _constant(header: str, name: str) -> int:
    text = open(os.path.join(CSRC, header)).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))


def chunk() -> int:
    """Contributions per partial sum of the aggregation (meshmap.hip)."""
    return _constant("meshmap.hip", "kChunk")


def coord_cells() -> float:
    text = open(os.path.join(CSRC, "cellhash.h")).read()
    return float(re.search(r"constexpr float kCoordCells = (\d+)\.f;", text).group(1))


def cloud(kind, n_v, n_p, seed):
    """tests/test_meshmap_gpu.py's ``_cloud`` (the host test holds the two equal)."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        V = rng.random((n_v, 3)) * 0.4
        P = rng.random((n_p, 3)) * 0.44 - 0.02
    else:
        c = rng.random((20, 3)) * 0.5
        V = c[rng.integers(0, 20, n_v)] + 0.01 * rng.standard_normal((n_v, 3))
        P = c[rng.integers(0, 20, n_p)] + 0.02 * rng.standard_normal((n_p, 3))
    return V.astype(np.float32), P.astype(np.float32)


def _f32(*arrays):
    return tuple(np.ascontiguousarray(a, np.float32) for a in arrays)


def _dirs(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------------------------ scenes
def _uniform():
    V, P = cloud("uniform", 3000, 8000, seed=101)
    return dict(V=V, P=P, trunc=0.03)


def _duplicated():
    """Every vertex position three times (equal distances are ordered by index), 500 points exactly on a position."""
    rng = np.random.default_rng(102)
    base = (rng.random((1500, 3)) * 0.2).astype(np.float32)
    V = np.concatenate([base, base, base])[rng.permutation(4500)]
    P = base[rng.integers(0, 1500, 3000)] + np.float32(0.003) * rng.standard_normal((3000, 3)).astype(np.float32)
    P[:500] = base[:500]
    return dict(V=V, P=P, trunc=0.02)


def _sparse_grid():
    """Vertices on a grid of spacing 2.5 sdf_trunc: a valid point's second and later neighbours lie rings out."""
    rng = np.random.default_rng(103)
    tr = 0.01
    g = np.arange(8) * 2.5 * tr
    V = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + 1e-4 * rng.standard_normal((512, 3))
    P = V[rng.integers(0, len(V), 4000)] + 0.004 * rng.standard_normal((4000, 3))
    V, P = _f32(V, P)
    return dict(V=V, P=P, trunc=tr)


FAR_SHIFT = (2000.0, -1500.0, 2500.0)


def _far():
    """The clustered cloud translated in fp64, then rounded to fp32 (a grid of 2.4e-4 at these coordinates)."""
    V, P = cloud("clustered", 3000, 8000, seed=104)
    V, P = _f32(V.astype(np.float64) + FAR_SHIFT, P.astype(np.float64) + FAR_SHIFT)
    F = np.random.default_rng(1040).standard_normal((len(P), 4)).astype(np.float32)
    return dict(V=V, P=P, F=F, trunc=0.03)


def cell_of(x, h):
    """The kernel's cell of a coordinate: floorf(x * inv_h) in fp32, inv_h = 1.f / h."""
    return np.floor(np.asarray(x, np.float32) * (np.float32(1) / np.float32(h))).astype(np.int64)


def first_box_stop(p, kth_d, h, margin):
    """The kernel's stop test after the first box, restated in fp32 with a given margin: (whether the search stops with the
    k-th distance ``kth_d``, lo [3], hi [3])."""
    p, h, margin = np.asarray(p, np.float32), np.float32(h), np.float32(margin)
    tt = h + margin
    lo, hi = cell_of(p - tt, h), cell_of(p + tt, h)
    gap = min(np.min(p - lo.astype(np.float32) * h), np.min((hi + 1).astype(np.float32) * h - p))
    return bool(np.float32(kth_d) < gap - margin), lo, hi


def _margin_traps():
    """Near x = 2500 at h = 0.03 the cell of a coordinate (floorf(x * inv_h)) and the face the stop test measures to
    (float(cell) * h) disagree by a float or two: a vertex ``star`` one float below the face of cell C is indexed in C.
    Each trap has a point 1.4 h below that face (cells C - 3 .. C - 1 are its first box when the margin is small), a vertex
    0.3 h from it (the row is valid), ``star``, and a vertex ``decoy`` in the box a hair further than ``star`` but nearer than
    the face: with k = 2 a stop test whose margin does not grow with the coordinates stops on the decoy.  Traps are 20
    cells apart in y (near -1500)."""
    h = np.float32(0.03)
    f32 = np.float32
    V, P, traps = [], [], []
    for C in range(83200, 83600):
        face = f32(C) * h
        star = np.nextafter(face, f32(0))
        if cell_of(star, h) != C:
            continue
        i = len(traps)
        py, pz = f32((-50000 + 20 * i + 0.5) * 0.03), f32(83333.5 * 0.03)
        px = f32(star - f32(0.042))
        d_star = f32(star - px)
        decoy = np.array([f32(px - d_star), py + 10 * np.spacing(py), pz], f32)
        if f32(px - decoy[0]) != d_star:
            continue
        V += [[px + f32(0.009), py, pz], [star, py, pz], decoy]
        P.append([px, py, pz])
        traps.append(C)
        if len(traps) == 40:
            break
    V, P = _f32(np.array(V), np.array(P))
    return dict(V=V, P=P, trunc=0.03, cells=np.array(traps))


def host_limit(trunc):
    """The largest fp32 coordinate the wrapper accepts for a vertex: |v| * float32(1 / trunc) < kCoordCells in fp32."""
    inv = np.float32(1.0 / trunc)
    x = np.float32(coord_cells() * trunc * 1.001)
    while not x * inv < np.float32(coord_cells()):
        x = np.nextafter(x, np.float32(0))
    return x


def out_of_range(P, trunc):
    """The kernel's range rule: rows it calls invalid without a search."""
    P = np.asarray(P, np.float32)
    inv_h = np.float32(1) / np.float32(trunc)
    with np.errstate(invalid="ignore"):
        return ~(np.fmax.reduce(np.abs(P), axis=1) * inv_h < np.float32(coord_cells() + 2))     # (fmaxf skips a NaN)


def _limit():
    """Vertices in a box whose +x and -y faces are the last coordinate the wrapper accepts; points among them, in the two
    cells beyond 2^18 h (in range: some have a vertex within sdf_trunc), beyond those (out of range) and at 1e6."""
    rng = np.random.default_rng(105)
    tr = 0.03
    top = float(host_limit(tr))
    lim = coord_cells() * tr
    V = np.stack([top - 0.3 * rng.random(1500), -top + 0.3 * rng.random(1500), 0.3 * rng.random(1500)], 1)
    V[0, 0], V[1, 1] = top, -top
    V[2:200, 0] = top - 0.01 * rng.random(198)                   # a dense layer under each face
    V[200:400, 1] = -top + 0.01 * rng.random(200)
    among = V[rng.integers(0, len(V), 800)] + 0.01 * rng.standard_normal((800, 3))
    yz = lambda n: np.stack([-top + 0.3 * rng.random(n), 0.3 * rng.random(n)], 1)
    xz = lambda n: np.stack([top - 0.3 * rng.random(n), 0.3 * rng.random(n)], 1)
    a, b = yz(300), xz(300)
    band = np.concatenate([np.column_stack([lim + 0.002 + 0.05 * rng.random(300), a]),       # lim .. lim + 2 h = + 0.06
                           np.column_stack([b[:, 0], -(lim + 0.002 + 0.05 * rng.random(300)), b[:, 1]])])
    a, b = yz(200), xz(200)
    beyond = np.concatenate([np.column_stack([lim + 0.08 + 0.2 * rng.random(200), a]),
                             np.column_stack([b[:, 0], -(lim + 0.08 + 0.2 * rng.random(200)), b[:, 1]])])
    huge = np.array([[1e6, 0, 0], [0, -1e6, 0], [top, -top, 1e6], [-1e6, 1e6, -1e6]])
    kinds = np.repeat(np.arange(4), [len(among), len(band), len(beyond), len(huge)])
    P = np.concatenate([among, band, beyond, huge])
    perm = rng.permutation(len(P))
    V, P = _f32(V, P[perm])
    return dict(V=V, P=P, trunc=tr, kinds=kinds[perm], top=np.float32(top))


STEP = 2.0 ** -5


def inclusive_truncs():
    """(sdf_trunc, whether a distance of exactly 2^-5 is valid under it)."""
    s = np.float32(STEP)
    return ((float(s), True), (float(np.nextafter(s, np.float32(0))), False), (float(np.nextafter(s, np.float32(1))), True))


def _inclusive():
    """An 8^3 lattice of spacing 2^-5; from every vertex of a face a point exactly 2^-5 outward (its nearest vertex, alone at
    that distance: ``n_at`` rows), ``n_on`` points exactly on vertices, 100 points 2^-4 outward."""
    rng = np.random.default_rng(106)
    g = np.arange(8) * STEP
    V = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    at, out2 = [], []
    for a in range(3):
        for side, sign in ((0.0, -1.0), (7 * STEP, 1.0)):
            face = V[V[:, a] == side]
            e = np.zeros(3)
            e[a] = sign * STEP
            at.append(face + e)
            out2.append(face[:17] + 2 * e)
    at, out2 = np.concatenate(at), np.concatenate(out2)[:100]
    on = V[rng.integers(0, len(V), 100)]
    kinds = np.repeat(np.arange(3), [len(at), len(on), len(out2)])
    P = np.concatenate([at, on, out2])
    perm = rng.permutation(len(P))
    V, P = _f32(V[rng.permutation(len(V))], P[perm])
    return dict(V=V, P=P, trunc=STEP, kinds=kinds[perm], n_at=len(at), n_on=len(on))


def _trunc_large():
    V, P = cloud("uniform", 3000, 2000, seed=107)
    F = np.random.default_rng(1070).standard_normal((len(P), 4)).astype(np.float32)
    return dict(V=V, P=P, F=F, trunc=50.0)


def _trunc_small():
    """A tenth of the points 3e-5 (per axis) off a vertex, the others uniform: valid against sdf_trunc = 1e-4 or not."""
    rng = np.random.default_rng(108)
    V, P = cloud("uniform", 3000, 2000, seed=108)
    near = rng.choice(len(P), len(P) // 10, replace=False)
    P = P.astype(np.float64)
    P[near] = V[rng.choice(len(V), len(near), replace=False)] + 3e-5 * rng.standard_normal((len(near), 3))
    (P,) = _f32(P)
    F = rng.standard_normal((len(P), 4)).astype(np.float32)
    return dict(V=V, P=P, F=F, trunc=1e-4)


def chunk_lengths():
    """List lengths at, one below and one above one, two and (above only) four chunks, and a single contribution."""
    c = chunk()
    return (1, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 4 * c + 1)


def _chunks(coincident):
    """Site s (a metre apart) receives exactly chunk_lengths()[s] points, shuffled among each other, and 5 far points
    bring the invalid key.  One vertex per site and jittered points (run with k = 1), or three coincident vertices per site
    and the points exactly on it (k = 3: sigma = 0)."""
    rng = np.random.default_rng(109)
    L = chunk_lengths()
    sites = np.stack([np.arange(len(L)) * 1.0, 0.25 * np.arange(len(L)), np.zeros(len(L))], 1)
    site_of = rng.permutation(np.repeat(np.arange(len(L)), L))
    P = sites[site_of]
    if coincident:
        V = np.repeat(sites, 3, 0)[rng.permutation(3 * len(L))]
    else:
        V = sites
        P = P + 0.004 * rng.standard_normal(P.shape)
    far = rng.choice(len(P) + 5, 5, replace=False)
    keep = np.ones(len(P) + 5, bool)
    keep[far] = False
    Q = np.empty((len(P) + 5, 3))
    Q[keep], Q[far] = P, sites[:5] + [0.0, 0.0, 7.0]
    V, Q = _f32(V, Q)
    F = rng.standard_normal((len(Q), 5)).astype(np.float32)
    return dict(V=V, P=Q, F=F, trunc=0.03, k=3 if coincident else 1)


def _channels(D, n_v, n_p, seed):
    V, P = cloud("uniform", n_v, n_p, seed)
    P = (V[np.random.default_rng(seed).integers(0, n_v, n_p)].astype(np.float64) + (P - 0.2) * 0.05).astype(np.float32)
    F = np.random.default_rng(seed + 1).standard_normal((n_p, D)).astype(np.float32)
    return dict(V=V, P=P, F=F, trunc=0.03)


BAD_ROWS = np.array([[np.nan, 0.1, 0.2], [0.1, np.nan, 0.2], [0.1, 0.2, np.nan], [np.nan, np.nan, np.nan],
                     [np.inf, 0.1, 0.2], [0.1, -np.inf, 0.2], [0.1, 0.2, np.inf], [-np.inf, np.inf, 0.1]], np.float32)


def _nonfinite():
    """A valid cloud (``P_clean``) and the same with BAD_ROWS mixed in (``P``), the first and the last row among them."""
    rng = np.random.default_rng(110)
    V, Pc = cloud("uniform", 1000, 2000, seed=110)
    Fc = rng.standard_normal((len(Pc), 3)).astype(np.float32)
    n = len(Pc) + len(BAD_ROWS)
    bad = np.sort(np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), len(BAD_ROWS) - 2, replace=False)]))
    keep = np.ones(n, bool)
    keep[bad] = False
    P, F = np.empty((n, 3), np.float32), np.full((n, 3), np.nan, np.float32)
    P[keep], P[bad], F[keep] = Pc, BAD_ROWS, Fc
    return dict(V=V, P=P, F=F, P_clean=Pc, F_clean=Fc, keep=keep, trunc=0.05)


MIXED_BLOBS, MIXED_PER_BLOB, MIXED_FAR_ONLY = 20, 100, (3, 8, 13, 18)


def _mixed():
    """Twenty tight blobs of 100 vertices, 0.2 apart; blob b carries magnitude 10^(b % 7 - 3) (1e-3 .. 1e3; blobs 3, 10 and 17
    are the unit ones).  Nine points in ten lie within 1e-4 of a vertex, one in ten 0.3 .. 0.9 sdf_trunc off one; the blobs
    of MIXED_FAR_ONLY (the unit blob 3 among them) receive points of the second kind only."""
    rng = np.random.default_rng(111)
    tr, n_p = 0.03, 4000
    cen = np.stack(np.meshgrid(*[np.arange(3) * 0.2] * 3, indexing="ij"), -1).reshape(-1, 3)[:MIXED_BLOBS]
    blob_v = np.repeat(np.arange(MIXED_BLOBS), MIXED_PER_BLOB)
    V = cen[blob_v] + 4e-4 * rng.standard_normal((len(blob_v), 3))
    far = np.arange(n_p) % 10 == 0
    near_ok = np.nonzero(~np.isin(blob_v, MIXED_FAR_ONLY))[0]
    src = np.where(far, rng.integers(0, len(V), n_p), near_ok[rng.integers(0, len(near_ok), n_p)])
    r = np.where(far, tr * (0.3 + 0.6 * rng.random(n_p)), 1e-4 * rng.random(n_p))
    P = V[src] + r[:, None] * _dirs(rng, n_p)
    mag = 10.0 ** (np.arange(MIXED_BLOBS) % 7 - 3)
    blob_p = blob_v[src]
    F = mag[blob_p, None] * rng.standard_normal((n_p, 6))
    N3 = mag[blob_p, None] * (0.2 * _dirs(rng, n_p) + [0.0, 0.0, 1.0])
    V, P, F, N3 = _f32(V, P, F, N3)
    return dict(V=V, P=P, F=F, N3=N3, trunc=tr, far=far, blob_v=blob_v, blob_p=blob_p, mag=mag)


_SCENES = {
    "uniform": _uniform, "duplicated": _duplicated, "sparse_grid": _sparse_grid, "far": _far, "limit": _limit,
    "inclusive": _inclusive, "trunc_large": _trunc_large, "trunc_small": _trunc_small,
    "chunks_k1": lambda: _chunks(False), "chunks_sigma0": lambda: _chunks(True),
    "d1": lambda: _channels(1, 500, 1500, 112), "d4096": lambda: _channels(4096, 257, 300, 113),
    "d7": lambda: _channels(7, 500, 1500, 114), "d13": lambda: _channels(13, 500, 1500, 115),
    "nonfinite": _nonfinite, "mixed": _mixed, "margin_traps": _margin_traps,
}

# (scene, k, values, normals): every use of the per-vertex bar
BAR_CASES = [("far", 5, "F", False), ("far", 16, "F", False), ("trunc_large", 5, "F", False), ("trunc_small", 5, "F", False),
             ("d1", 5, "F", False), ("d4096", 5, "F", False), ("mixed", 5, "F", False), ("mixed", 16, "F", False),
             ("mixed", 5, "N3", True), ("mixed", 16, "N3", True)]


@functools.lru_cache(maxsize=None)
def scene(name):
    s = _SCENES[name]()
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def restated_knn(name, k, trunc=None):
    """(idx, d, d2, valid) of the brute force; ``trunc``: the scene's own unless given."""
    s = scene(name)
    out = R.knn(s["V"], s["P"], k, s["trunc"] if trunc is None else trunc)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------- the per-vertex bar
def vertex_bound(n_vertices, idx, d, valid, values, ref64, chunk_len, normalise=False, ref64_pre=None):
    """bound [M,D] of |out - ref64| for the fp32 map in the kernel's order, from the neighbour lists alone (derivation:
    tests/test_meshmap_regimes_gpu.py); ``covered`` [M].  With ``normalise`` (three channels) ``ref64_pre`` is the fp64 map
    before the unit step."""
    F = np.asarray(values, np.float64)
    valid = np.asarray(valid, bool)
    M, k = n_vertices, idx.shape[1]
    iv = np.nonzero(valid)[0]
    covered = np.zeros(M, bool)
    if not len(iv):
        return np.zeros((M, F.shape[1])), covered
    dv = np.asarray(d, np.float64)[iv]
    w, sigma = R.weights(d, valid)
    w = w[iv]
    if sigma > 0:
        c = 1.0 / (2.0 * sigma * sigma)
        x = (dv * dv - dv[:, :1] * dv[:, :1]) * c
        s = (dv * dv + dv[:, :1] * dv[:, :1]) * c
        assert x.max() < 80.0, "a weight of this scene underflows in fp32: the bar does not cover it"
        ee = np.where(dv == dv[:, :1], 0.0, np.exp(U * (s + 4.0 * x)) * (1.0 + 2 * EXP_ULPS * U) - 1.0)
    else:
        ee = np.zeros_like(dv)
    eta = np.sum(w * ((1.0 + ee) * (1.0 + U) ** (k - 1) - 1.0), axis=1, keepdims=True)
    eps = (1.0 + ee) * (1.0 + U) / (1.0 - eta) - 1.0
    vert = np.asarray(idx)[iv].reshape(-1)
    covered[vert] = True
    eps_v = np.zeros(M)
    np.maximum.at(eps_v, vert, eps.reshape(-1))
    L = np.bincount(vert, minlength=M)
    n_l = np.maximum(np.minimum(L, chunk_len) - 1 + (L + chunk_len - 1) // chunk_len - 1, 0)
    g_num = ((1.0 + U) ** (n_l + 1) - 1.0)[:, None]
    g_den = ((1.0 + U) ** n_l - 1.0)[:, None]
    pre = ref64_pre if normalise else ref64
    wf = w.reshape(-1)
    Fe = np.repeat(F[iv], k, axis=0)
    A, B, den = np.zeros((M, F.shape[1])), np.zeros((M, F.shape[1])), np.zeros(M)
    np.add.at(A, vert, wf[:, None] * np.abs(Fe))
    np.add.at(B, vert, wf[:, None] * np.abs(Fe - pre[vert]))
    np.add.at(den, vert, wf)
    A, B = A / np.where(den > 0, den, 1.0)[:, None], B / np.where(den > 0, den, 1.0)[:, None]
    ev = eps_v[:, None]
    weight_term = ev / (1.0 - ev) * B
    sum_term = (g_num * A + g_den * (np.abs(pre) + weight_term)) * (1.0 + ev) / ((1.0 - ev) * (1.0 - g_den))
    bound = (weight_term + sum_term) * (1.0 + U) + 2.0 * U * np.abs(pre)
    if normalise:
        nrm = np.linalg.norm(pre, axis=1) + 1e-8
        b = (2.0 * np.linalg.norm(bound, axis=1) + abs(float(np.float32(1e-8)) - 1e-8)) / nrm + 4.0 * U * (1.0 + 4.0 * U)
        bound = np.repeat(b[:, None], 3, axis=1)
    bound[~covered] = 0.0
    return bound, covered


@functools.lru_cache(maxsize=None)
def bar(name, k, values="F", normals=False):
    """(ref64, bound, covered, ordered): the fp64 map, the per-vertex bar and the fp32 yardstick of a BAR_CASES entry."""
    s = scene(name)
    idx, d, _, valid = restated_knn(name, k)
    F, M = s[values], len(s["V"])
    ref = R.aggregate(M, idx, d, valid, F, normalise=normals)
    pre = R.aggregate(M, idx, d, valid, F) if normals else None
    bound, covered = vertex_bound(M, idx, d, valid, F, ref, chunk(), normalise=normals, ref64_pre=pre)
    ordered = R.aggregate_ordered(M, idx, d, valid, F, normalise=normals, chunk=chunk())
    return ref, bound, covered, ordered
