"""numpy restatement of the dense-grid screened Poisson reconstruction: the oracle of csrc/poisson.hip.

The grid, the splat, the system and the sampler are evaluated in the kernels' order with float32 operands, so the int64 grids, b
and D are bit-identical to the GPU's.  The conjugate gradients come twice: ``cg`` is the recurrence in fp32 or fp64 with its sums
in numpy's order (chi is compared with it through residuals), ``cg_exact`` is the kernels' recurrence with every sum in the
device's written order (x, r, z, p and the solver state are compared with it bit for bit, iteration by iteration); ``mean_exact``
is the iso value's mean in the same order.  Extraction reuses the TSDF restatement's marching cubes on chi - iso.  Neither
Kazhdan's octree solver nor Open3D is pinned.
"""
from __future__ import annotations

import numpy as np

from tsdf_restatement import LOCAL, RestatedTSDF

F = np.float32
FIX = F(2.0 ** 30)
INV_FIX = F(2.0 ** -30)


# ------------------------------------------------------------------------------------------------------------------ grid
def grid(points, depth=8, scale=1.1):
    """(origin [3] fp32, h fp32, G): c = (lo + hi) / 2, s = scale max(hi - lo), h = s / G, o = c - s / 2, all fp32."""
    p = np.asarray(points, np.float32)
    if not np.isfinite(p).all():
        raise ValueError("points must be finite")
    G = 1 << depth
    lo, hi = p.min(0), p.max(0)
    c = (lo + hi) / F(2)
    s = F(scale) * (hi - lo).max()
    if not s > 0:
        raise ValueError("degenerate extent")
    h = F(s / F(G))
    o = (c - s / F(2)).astype(np.float32)
    return o, h, G


def _cells(points, o, h, G):
    g = (np.asarray(points, np.float32) - o) / h - F(0.5)
    fl = np.floor(g)
    return fl.astype(np.int64), (g - fl).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------- splat
def splat(points, normals, colors, o, h, G):
    """(Wq [G,G,G], Vq [3,G,G,G], Cq [3,G,G,G] or None) int64, indexed [z, y, x]."""
    i0, f = _cells(points, o, h, G)
    n = np.asarray(normals, np.float32)
    col = None if colors is None else np.asarray(colors, np.float32)
    Wq = np.zeros(G ** 3, np.int64)
    Vq = np.zeros((3, G ** 3), np.int64)
    Cq = None if col is None else np.zeros((3, G ** 3), np.int64)
    for c in range(8):
        d = np.array([c & 1, (c >> 1) & 1, c >> 2])
        wa = np.where(d[None, :] == 1, f, F(1) - f).astype(np.float32)
        w = ((wa[:, 0] * wa[:, 1]) * wa[:, 2]).astype(np.float32)
        idx = np.clip(i0 + d[None, :], 0, G - 1)
        cell = idx[:, 0] + G * (idx[:, 1] + G * idx[:, 2])
        np.add.at(Wq, cell, np.rint(w * FIX).astype(np.int64))
        for a in range(3):
            np.add.at(Vq[a], cell, np.rint((w * n[:, a]).astype(np.float32) * FIX).astype(np.int64))
            if col is not None:
                np.add.at(Cq[a], cell, np.rint((w * col[:, a]).astype(np.float32) * FIX).astype(np.int64))
    return Wq.reshape(G, G, G), Vq.reshape(3, G, G, G), None if Cq is None else Cq.reshape(3, G, G, G)


def to_float(q):
    return (q.astype(np.float32) * INV_FIX).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- system
def _shift(a, axis, step, fill=0):
    """a[i + step e_axis] with `fill` outside (axis 0 = x = the LAST array axis)."""
    ax = a.ndim - 1 - axis
    out = np.full_like(a, fill)
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    if step > 0:
        src[ax], dst[ax] = slice(step, None), slice(None, -step)
    else:
        src[ax], dst[ax] = slice(None, step), slice(-step, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def neighbours(G):
    n = np.zeros((G, G, G), np.float32)
    one = np.ones((G, G, G), np.float32)
    for a in range(3):
        n += _shift(one, a, 1) + _shift(one, a, -1)
    return n


def system(Wq, Vq, point_weight=1.0):
    """(W, b, D) fp32 [G,G,G] in the kernel's order."""
    G = Wq.shape[0]
    W = to_float(Wq)
    V = to_float(Vq)
    dv = [(_shift(V[a], a, 1, F(0)) - _shift(V[a], a, -1, F(0))).astype(np.float32) for a in range(3)]
    b = (F(-0.5) * ((dv[0] + dv[1]) + dv[2])).astype(np.float32)
    cnt = int((Wq > 0).sum())
    D = neighbours(G)
    if cnt > 0:
        wbar = F((float(int(Wq.sum())) * 2.0 ** -30) / float(cnt))
        D = (D + (F(point_weight) * W) / wbar).astype(np.float32)
    return W, b, D


def apply_A(D, x):
    """(A x)(i) = D(i) x(i) - the in-grid neighbours of x, in x's precision."""
    s = np.zeros_like(x)
    for a in range(3):
        s = s + _shift(x, a, -1) + _shift(x, a, 1)
    return D.astype(x.dtype) * x - s


# ----------------------------------------------------------------------------------------------------------------- solve
def cg(b, D, tol=1e-5, max_iters=None, dtype=np.float32):
    """Jacobi-preconditioned CG from 0: (x, iterations, recurrence residual |r| / |b|, converged)."""
    T = dtype
    G = b.shape[0]
    max_iters = 8 * G if max_iters is None else int(max_iters)
    b, D = b.astype(T), D.astype(T)
    x = np.zeros_like(b)
    r = b.copy()
    z = r / D
    p = z.copy()
    rz = T(np.vdot(r, z))
    bb = float(np.vdot(b.astype(np.float64), b.astype(np.float64)))
    rr = bb
    it = 0
    done = bb == 0.0
    while not done and it < max_iters:
        Ap = apply_A(D, p)
        pAp = T(np.vdot(p, Ap))
        if pAp == 0 or rz == 0:
            break
        alpha = T(rz / pAp)
        x = x + alpha * p
        r = r - alpha * Ap
        z = r / D
        rz_new = T(np.vdot(r, z))
        rr = float(np.vdot(r.astype(np.float64), r.astype(np.float64)))
        it += 1
        if rr <= tol * tol * bb:
            done = True
            break
        beta = T(rz_new / rz)
        p = z + beta * p
        rz = rz_new
    resid = float(np.sqrt(rr / bb)) if bb > 0 else 0.0
    return x, it, resid, bool(done)


# ------------------------------------------------------------------------------------------------- the device's own sums
# csrc/wgprims.h and csrc/poisson.hip write every fp64 sum's order down; these are those orders in numpy (the model is
# pointcloud_restatement._tree256).  Everything below is fp64 and vectorised over the leading axes.
CELLS_PER_BLOCK = 1024               # 256 lanes of 4 consecutive values
FINAL = 1024                         # threads of the one workgroup of the second level
S_RZ, S_PAP, S_RR, S_BB, S_ALPHA, S_BETA, S_DONE, S_ITERS = range(8)


def _wave_tree(w):
    """wave_sum: [..., 64] -> [...], the shuffle-down tree 32, 16, ... 1 as lane 0 sees it."""
    w = np.array(w, np.float64)
    for off in (32, 16, 8, 4, 2, 1):
        w[..., :off] = w[..., :off] + w[..., off:2 * off]
    return w[..., 0]


def _block_tree(v, waves):
    """block_sum<waves>: [..., 64 waves] -> [...], each wave's tree, then the waves in ascending order."""
    w = _wave_tree(np.asarray(v, np.float64).reshape(*np.shape(v)[:-1], waves, 64))
    s = w[..., 0]
    for k in range(1, waves):
        s = s + w[..., k]
    return s


def _lane4(a, from_zero=False):
    """[..., 4] -> [...]: ((a0 + a1) + a2) + a3, or (((0.0 + a0) + a1) + a2) + a3 for the mean's lanes."""
    s = (0.0 + a[..., 0]) if from_zero else a[..., 0]
    for k in range(1, 4):
        s = s + a[..., k]
    return s


def block_partials(values, from_zero=False):
    """The first level: [1024 nb] fp64 -> [nb], one partial per workgroup of 256 lanes with 4 consecutive values each."""
    v = np.asarray(values, np.float64).reshape(-1, CELLS_PER_BLOCK // 4, 4)
    return _block_tree(_lane4(v, from_zero), 4)


def second_level(partials):
    """final_sum: thread t adds partials t, t + 1024, ... in ascending order from 0.0, then block_sum over 16 waves.  (A thread's sum
    is never -0.0, so the zero padding of the last trip is no addition the device does not make in effect.)"""
    part = np.asarray(partials, np.float64).reshape(-1)
    trips = max((len(part) + FINAL - 1) // FINAL, 1)
    part = np.concatenate([part, np.zeros(trips * FINAL - len(part))]).reshape(trips, FINAL)
    s = np.zeros(FINAL)
    for k in range(trips):
        s = s + part[k]
    return float(_block_tree(s, FINAL // 64))


def dot_exact(a, b):
    """sum a b over a grid as the CG kernels form it: exact fp64 products of two floats, the lane's four cells, the workgroup's
    tree, the second level."""
    prod = np.asarray(a, np.float32).reshape(-1).astype(np.float64) * np.asarray(b, np.float32).reshape(-1).astype(np.float64)
    return second_level(block_partials(prod))


def mean_exact(values):
    """misplat_poisson_mean: the fp64 mean of n fp32 values; blocks of 1024 (the last one padded with 0.0, as the kernel adds 0.0
    past n), each lane 4 values in ascending order from 0.0, the second level, then the division by n."""
    v = np.asarray(values, np.float32).reshape(-1).astype(np.float64)
    n = len(v)
    nb = (n + CELLS_PER_BLOCK - 1) // CELLS_PER_BLOCK
    v = np.concatenate([v, np.zeros(nb * CELLS_PER_BLOCK - n)])
    return second_level(block_partials(v, from_zero=True)) / float(n)


def sum_path_length(n, lane_adds=3):
    """The largest number of fp64 additions any one of n summands passes through in the two-level sum: the lane's, 6 + 3 of the
    workgroup's tree, the thread's trips of the second level, 6 + 15 of its tree."""
    nb = (n + CELLS_PER_BLOCK - 1) // CELLS_PER_BLOCK
    return lane_adds + 6 + 3 + (nb + FINAL - 1) // FINAL + 6 + 15


def apply_A32(D, p):
    """cg_stencil_kernel's Ap in fp32: D p - (((((x- + x+) + y-) + y+) + z-) + z+), 0 outside the grid."""
    s = _shift(p, 0, -1) + _shift(p, 0, 1)
    for a in (1, 2):
        s = s + _shift(p, a, -1)
        s = s + _shift(p, a, 1)
    return D * p - s


def cg_exact(b, D, tol=1e-5, max_iters=None, n_steps=None, start=None):
    """The kernels' recurrence in their own order: (x, r, z, p, state [8] fp64, iterations, done) after n_steps iterations of
    misplat_poisson_cg_iterate (a no-op once done != 0), or at the stop when n_steps is None.  state is the workspace head (S_RZ,
    S_PAP, S_RR, S_BB, S_ALPHA, S_BETA, S_DONE, S_ITERS); done = 1 converged (rr <= tol^2 bb, or b = 0), 2 the cap, 3 p.Ap = 0 or
    r.z = 0.  alpha and beta are rounded through float as the kernels round them.  `start` = an earlier result, to go on from."""
    b, D = np.asarray(b, np.float32), np.asarray(D, np.float32)
    G = b.shape[0]
    max_iters = 8 * G if max_iters is None else int(max_iters)
    tol2 = float(tol) * float(tol)
    if start is None:
        x = np.zeros_like(b)
        r = b.copy()
        z = r / D
        p = z.copy()
        st = np.zeros(8)
        st[S_RZ] = dot_exact(r, z)
        st[S_RR] = st[S_BB] = dot_exact(b, b)
        st[S_DONE] = 1.0 if st[S_BB] == 0.0 else (2.0 if max_iters <= 0 else 0.0)
    else:
        x, r, z, p = (np.array(v, np.float32) for v in start[:4])
        st = np.array(start[4], np.float64)
    step = 0
    while st[S_DONE] == 0.0 and (n_steps is None or step < n_steps):
        step += 1
        Ap = apply_A32(D, p)
        pAp = dot_exact(p, Ap)
        st[S_PAP] = pAp
        if pAp == 0.0 or st[S_RZ] == 0.0:
            st[S_ALPHA] = 0.0
            st[S_DONE] = 3.0
            break
        alpha = F(st[S_RZ] / pAp)
        st[S_ALPHA] = float(alpha)
        x = x + alpha * p
        r = r - alpha * Ap
        z = r / D
        rz, rr = dot_exact(r, z), dot_exact(r, r)
        beta = F(rz / st[S_RZ])
        st[S_BETA] = float(beta)
        st[S_RZ], st[S_RR] = rz, rr
        st[S_ITERS] += 1.0
        if rr <= tol2 * st[S_BB]:
            st[S_DONE] = 1.0
        elif st[S_ITERS] >= float(max_iters):
            st[S_DONE] = 2.0
        else:
            p = z + beta * p
    return x, r, z, p, st, int(st[S_ITERS]), int(st[S_DONE])


def exact_info(st):
    """poisson._solve's info from a state."""
    return {"iterations": int(st[S_ITERS]), "residual": float(np.sqrt(st[S_RR] / st[S_BB])) if st[S_BB] > 0 else 0.0,
            "converged": bool(st[S_DONE] == 1.0)}


def true_residual(b, D, x):
    """|b - A x| / |b| in fp64."""
    b64, x64 = b.astype(np.float64), np.asarray(x).astype(np.float64)
    r = b64 - apply_A(D.astype(np.float64), x64)
    return float(np.sqrt(np.vdot(r, r) / np.vdot(b64, b64)))


# ---------------------------------------------------------------------------------------------------------------- sample
def sample(field, o, h, G, q):
    """Trilinear value of field [..., G, G, G] at q [n,3]: fp32, x then y then z; returns [n] or [n, C]."""
    f = np.asarray(field, np.float32)
    multi = f.ndim == 4
    f = f.reshape(-1, G ** 3)
    g = (np.asarray(q, np.float32) - o) / h - F(0.5)
    fl = np.clip(np.floor(g), F(0), F(G - 2)).astype(np.float32)
    t = np.clip(g - fl, F(0), F(1)).astype(np.float32)
    i0 = fl.astype(np.int64)
    base = i0[:, 0] + G * (i0[:, 1] + G * i0[:, 2])
    u = (F(1) - t).astype(np.float32)
    out = []
    for ch in range(f.shape[0]):
        v = lambda off: f[ch][base + off]
        x00 = v(0) * u[:, 0] + v(1) * t[:, 0]
        x10 = v(G) * u[:, 0] + v(G + 1) * t[:, 0]
        x01 = v(G * G) * u[:, 0] + v(G * G + 1) * t[:, 0]
        x11 = v(G * G + G) * u[:, 0] + v(G * G + G + 1) * t[:, 0]
        y0 = x00 * u[:, 1] + x10 * t[:, 1]
        y1 = x01 * u[:, 1] + x11 * t[:, 1]
        out.append((y0 * u[:, 2] + y1 * t[:, 2]).astype(np.float32))
    return np.stack(out, 1) if multi else out[0]


def iso_value(chi, o, h, G, points):
    """The fp64 mean over the points of the fp32 trilinear chi."""
    return float(sample(chi, o, h, G, points).astype(np.float64).sum() / len(points))


# --------------------------------------------------------------------------------------------------------------- extract
def extract(chi, iso, o, h, G, W=None, C=None):
    """(vertices [M,3], triangles [T,3] int32, colors [M,3], density [M]): marching cubes of chi - float32(iso) over the cell centres
    (the TSDF restatement's, on a fully allocated unit map with voxel_size 1), world = o + v h; density = trilinear W, colour =
    trilinear C / trilinear W (0 where that is 0)."""
    field = (np.asarray(chi, np.float32) - F(iso)).astype(np.float32)
    vol = RestatedTSDF(1.0, 1.0, 1.0)
    U = G // 16
    for uz in range(U):
        for uy in range(U):
            for ux in range(U):
                data = np.zeros((5, 4096), np.float32)
                gx, gy, gz = ux * 16 + LOCAL[:, 0], uy * 16 + LOCAL[:, 1], uz * 16 + LOCAL[:, 2]
                data[0] = field[gz, gy, gx]
                data[1] = F(1)
                vol.units[(ux, uy, uz)] = data
    v, t, _ = vol.extract_mesh()
    verts = (o[None, :] + v.astype(np.float32) * h).astype(np.float32)
    if W is None:
        return verts, t, None, None
    dens = sample(W, o, h, G, verts) if len(verts) else np.zeros(0, np.float32)
    cols = np.zeros((len(verts), 3), np.float32)
    if C is not None and len(verts):
        cs = sample(C, o, h, G, verts)
        with np.errstate(all="ignore"):
            cols = np.where(dens[:, None] > 0, cs / dens[:, None], F(0)).astype(np.float32)
    return verts, t, cols, dens


def reconstruct(points, normals, colors=None, depth=8, scale=1.1, point_weight=1.0, tol=1e-5, max_iters=None, dtype=np.float32):
    """The whole pipeline on the host; returns a dict of every intermediate."""
    o, h, G = grid(points, depth, scale)
    Wq, Vq, Cq = splat(points, normals, colors, o, h, G)
    W, b, D = system(Wq, Vq, point_weight)
    chi, it, resid, conv = cg(b, D, tol, max_iters, dtype)
    chi32 = chi.astype(np.float32)
    iso = iso_value(chi32, o, h, G, points)
    C = None if Cq is None else to_float(Cq)
    v, t, c, d = extract(chi32, iso, o, h, G, W, C)
    return dict(o=o, h=h, G=G, Wq=Wq, Vq=Vq, Cq=Cq, W=W, b=b, D=D, chi=chi, iterations=it, residual=resid, converged=conv, iso=iso,
                vertices=v, triangles=t, colors=c, density=d)


# ------------------------------------------------------------------------------------------------------------------ trim
def trim(vertices, triangles, density, quantile=0.01, min_density=None):
    """The reference's rule (mesh.py:817-818, np.quantile with linear interpolation) plus min_density: (vertices, triangles,
    density, vertex_index)."""
    d = np.asarray(density, np.float64)
    drop = d < np.quantile(d, quantile) if len(d) else np.zeros(0, bool)
    if min_density is not None:
        drop |= d < float(min_density)
    t = np.asarray(triangles, np.int64)
    keep_f = ~drop[t].any(1)
    kept = t[keep_f]
    used = np.zeros(len(d), bool)
    used[kept.reshape(-1)] = True
    index = np.nonzero(used)[0]
    remap = np.cumsum(used) - 1
    return np.asarray(vertices)[index], remap[kept].astype(np.int32), np.asarray(density)[index], index


# -------------------------------------------------------------------------------------------------------------- geometry
def signed_volume(v, t):
    a, b, c = (np.asarray(v, np.float64)[np.asarray(t)[:, k]] for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def euler(v, t):
    t = np.asarray(t, np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    return len(v) - len(np.unique(e, axis=0)) + len(t)
