"""The level-set search along rays (csrc/density.hip's density_raycast) and the Laplacian smoothing
(csrc/meshclean.hip's smooth kernels) restated on the CPU in fp64: test infrastructure, never imported by the package.

The search, for a ray o + t v over [t0, t1] and a level l, with d(.) any density (density_restatement.Oracle's here):
  coarse pass   step = (t1 - t0) / 63, t_k = t0 + k step, D_k = d(o + t_k v), k = 0 .. 63 (shared by the levels);
  bracket       k* = the smallest k in 0 .. 62 with D_k < l <= D_{k+1}; none: a miss (hit 0, t 0);
  fine pass     a = t_k*, b = t_{k*+1}, fstep = (b - a) / 63, u_j = a + j fstep and F_j = d(o + u_j v) for j = 1 .. 62,
                u_0 = a, F_0 = D_k*, u_63 = b, F_63 = D_{k*+1} (reused, so a fine crossing exists);
                j* = the smallest j with F_j < l <= F_{j+1};
  result        t = u_j* + (u_{j*+1} - u_j*) ((l - F_j*) / (F_{j*+1} - F_j*)).
A ray with a non-finite o, v, t0 or t1, or with t1 <= t0, misses every level."""
import numpy as np

N = 64


def oracle_density(oracle, restated=None, chunk=8192):
    """points [P,3] -> d [P] fp64 over all the oracle's Gaussians; with `restated` (density_restatement.Restated: the unit map)
    0 outside the map, as the field's density is defined: the point's voxel floor(p / h) must lie in one of the map's units.
    (Inside the map an unallocated unit needs no rule: the lists are conservative, the oracle is 0 there to rounding.)"""
    def d(points):
        p = np.asarray(points, np.float64).reshape(-1, 3)
        out = np.zeros(p.shape[0])
        if len(oracle.ids) == 0:
            return out
        for c0 in range(0, p.shape[0], chunk):
            out[c0:c0 + chunk] = oracle.terms(p[c0:c0 + chunk])[0].sum(1)
        if restated is not None:
            with np.errstate(all="ignore"):
                unit = np.floor(np.floor(p / float(restated.h)) / 16.0)
                inside = ((unit >= restated.lo[None, :]) & (unit < (restated.lo + restated.dims)[None, :])).all(1)
            out = np.where(inside, out, 0.0)
        return out
    return d


def search(density, origins, dirs, t0, t1, levels):
    """dict: t, hit [L,M]; k [L,M] (the coarse bracket, -1 for a miss); tk, D [M,64] (the coarse pass); u, F [L,M,64] (the fine
    pass; zeros for a miss), all fp64."""
    o, v = np.asarray(origins, np.float64).reshape(-1, 3), np.asarray(dirs, np.float64).reshape(-1, 3)
    t0, t1 = np.asarray(t0, np.float64).reshape(-1), np.asarray(t1, np.float64).reshape(-1)
    M, L = o.shape[0], len(levels)
    with np.errstate(all="ignore"):
        valid = np.isfinite(o).all(1) & np.isfinite(v).all(1) & np.isfinite(t0) & np.isfinite(t1) & (t1 > t0)
    o, v = np.where(valid[:, None], o, 0.0), np.where(valid[:, None], v, 0.0)
    t0, t1 = np.where(valid, t0, 0.0), np.where(valid, t1, 1.0)
    j = np.arange(N, dtype=np.float64)
    step = (t1 - t0) / 63.0
    tk = t0[:, None] + j[None, :] * step[:, None]
    D = density((o[:, None, :] + tk[:, :, None] * v[:, None, :]).reshape(-1, 3)).reshape(M, N)
    out = dict(t=np.zeros((L, M)), hit=np.zeros((L, M), bool), k=np.full((L, M), -1, np.int64), tk=tk, D=D,
               u=np.zeros((L, M, N)), F=np.zeros((L, M, N)))
    for li, lev in enumerate(levels):
        cross = (D[:, :-1] < lev) & (lev <= D[:, 1:]) & valid[:, None]
        rays = np.nonzero(cross.any(1))[0]
        if len(rays) == 0:
            continue
        k = cross[rays].argmax(1)
        a, b = tk[rays, k], tk[rays, k + 1]
        fstep = (b - a) / 63.0
        u = a[:, None] + j[None, :] * fstep[:, None]
        u[:, 0], u[:, N - 1] = a, b
        F = density((o[rays, None, :] + u[:, :, None] * v[rays, None, :]).reshape(-1, 3)).reshape(-1, N)
        F[:, 0], F[:, N - 1] = D[rays, k], D[rays, k + 1]
        fine = (F[:, :-1] < lev) & (lev <= F[:, 1:])
        assert fine.any(1).all()                                           # F_0 < l <= F_63
        js = fine.argmax(1)
        r = np.arange(len(rays))
        uj, un, Fj, Fn = u[r, js], u[r, js + 1], F[r, js], F[r, js + 1]
        out["t"][li, rays] = uj + (un - uj) * ((lev - Fj) / (Fn - Fj))
        out["hit"][li, rays] = True
        out["k"][li, rays] = k
        out["u"][li, rays], out["F"][li, rays] = u, F
    return out


# --------------------------------------------------------------------------------------------------------- smoothing
def smooth_laplacian(vertices, triangles, iterations=1, lam=0.5, attributes=()):
    """Open3D's filter_smooth_laplacian restated: per iteration, from the previous iteration's positions, with N(i) the distinct
    vertices j != i sharing an edge with i in ascending order and w_ij = 1 / (|x_i - x_j| + 1e-12):
    x_i' = x_i + lam (sum_j w_ij x_j / sum_j w_ij - x_i); attributes take the same weights; no neighbour: unchanged.  fp64 from
    fp32 inputs, each iteration's result rounded to fp32 (what the kernel stores).  Returns (vertices', [attributes'])."""
    v = np.asarray(vertices, np.float32)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    att = [np.asarray(a, np.float32) for a in attributes]
    nbrs = [set() for _ in range(v.shape[0])]
    for a, b, c in tri:
        for p, q in ((a, b), (b, c), (c, a)):
            if p != q:
                nbrs[p].add(int(q))
                nbrs[q].add(int(p))
    nbrs = [np.array(sorted(s), np.int64) for s in nbrs]
    for _ in range(iterations):
        p64 = v.astype(np.float64)
        rows = [p64] + [a.astype(np.float64) for a in att]
        new = [r.copy() for r in rows]
        for i, nb in enumerate(nbrs):
            if len(nb) == 0:
                continue
            d = p64[nb] - p64[i]
            w = 1.0 / (np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + 1e-12)
            W = 0.0
            S = [np.zeros(r.shape[1]) for r in rows]
            for n, j in enumerate(nb):                                     # (ascending j: the kernel's order)
                W = W + w[n]
                for s, r in zip(S, rows):
                    s += w[n] * r[j]
            for s, r, out in zip(S, rows, new):
                out[i] = r[i] + lam * (s / W - r[i])
        v = new[0].astype(np.float32)
        att = [a.astype(np.float32) for a in new[1:]]
    return v, att
