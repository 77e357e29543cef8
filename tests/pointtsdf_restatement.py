"""fp32 numpy restatement of the point-cloud TSDF fusion with space carving: the oracle of
csrc/pointtsdf.hip.  The operation as the issue states it and nothing else: the plain voxel walk of every ray from its start (no
unit map, no re-entry, no lists), every expression in float32 in the kernels' order, integer sums.  vdbfusion is not pinned.
The extraction lays the finalised planes into ``tsdf_restatement.RestatedTSDF`` and uses its marching cubes (the shared one).
"""
from __future__ import annotations

import numpy as np

from tsdf_restatement import RestatedTSDF

F = np.float32
Q = F(16384.0)
MAX_COORD = F(4194304.0)                   # 2^22 voxels


def make_rays(points, origins, vs, trunc, carve):
    """The rays that take part: dict of fp32 arrays (o, p, ol, dl [n,3], s1 [n]), int64 (g0, step [n,3]) and ``index`` (the
    rays' positions in the input)."""
    vs, trunc = F(vs), F(trunc)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(origins, np.float32).reshape(-1, 3), p.shape)
    with np.errstate(all="ignore"):
        v = p - o
        L = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        ok = np.isfinite(p).all(1) & np.isfinite(o).all(1) & (L > 0) & np.isfinite(L)
        d = v / L[:, None]
        ol = o / vs
        dl = d / vs
        ok &= (np.abs(ol) < MAX_COORD).all(1) & (np.abs(p / vs) < MAX_COORD).all(1)
    idx = np.nonzero(ok)[0]
    p, o, L, ol, dl = p[idx], o[idx], L[idx], ol[idx], dl[idx]
    s0 = np.zeros_like(L) if carve else np.maximum(L - trunc, F(0))
    s1 = L + trunc
    g0 = np.floor(ol + s0[:, None] * dl).astype(np.int64)
    step = np.where(dl > 0, 1, np.where(dl < 0, -1, 0)).astype(np.int64)
    return dict(o=o, p=p, ol=ol, dl=dl, s1=s1, g0=g0, step=step, index=idx)


def walk(R):
    """(ray [n], voxel [n,3] int64): every voxel each ray visits, rays stepping side by side.  ``ray`` indexes R's rays."""
    n = len(R["s1"])
    act = np.arange(n)
    g = R["g0"].copy()
    rays, vox = [], []
    while len(act):
        rays.append(act)
        vox.append(g[act].copy())
        st, ol, dl = R["step"][act], R["ol"][act], R["dl"][act]
        k = np.where(st > 0, g[act] + 1, g[act]).astype(np.float32)
        with np.errstate(all="ignore"):
            t = np.where(st != 0, (k - ol) / dl, F(np.inf)).astype(np.float32)
        a = np.argmin(t, axis=1)                                                 # (the first minimum: ties to the lowest axis)
        tm = t[np.arange(len(act)), a]
        go = tm <= R["s1"][act]
        act, a = act[go], a[go]
        g[act, a] += R["step"][act, a]
    if not rays:
        return np.zeros(0, np.int64), np.zeros((0, 3), np.int64)
    return np.concatenate(rays), np.concatenate(vox)


def u8(rgb):
    with np.errstate(all="ignore"):
        c = np.asarray(rgb, np.float32) * F(255)
    c = np.where(c > 0, c, F(0))
    c = np.where(c < F(255), c, F(255))
    return c.astype(np.int64)


class RestatedPointTSDF:
    """``integrate`` any number of times, ``unit_arrays`` / ``extract_mesh`` at will.  ``bounds``: voxels of units that do not
    overlap the box are dropped (``floor(b / ulen)`` in float64 with the fp32 unit length, as the product clips its map)."""

    def __init__(self, voxel_size, sdf_trunc, space_carving=True, bounds=None):
        self.vs, self.trunc, self.carve = F(voxel_size), F(sdf_trunc), bool(space_carving)
        self.ulen = F(self.vs * F(16))
        self.clip = None
        if bounds is not None:
            b = np.asarray(bounds, np.float64).reshape(2, 3)
            ul = float(self.ulen)
            self.clip = (np.floor(b[0] / ul).astype(np.int64), np.floor(b[1] / ul).astype(np.int64))
        self.units = {}                    # (ux, uy, uz) -> dict(sum_q int64 [4096], count, rgb_sum [4096,3], rgb_count)

    def updates(self, points, origins, colors=None):
        """Per visited voxel (after the clip): (voxel [n,3], sdf [n] fp32, ray [n] indexing the input)."""
        R = make_rays(points, origins, self.vs, self.trunc, self.carve)
        ray, g = walk(R)
        if self.clip is not None:
            u = g >> 4
            keep = np.all((u >= self.clip[0]) & (u <= self.clip[1]), 1)
            ray, g = ray[keep], g[keep]
        c = (g.astype(np.float32) + F(0.5)) * self.vs
        p, o = R["p"][ray], R["o"][ray]
        pc, co = p - c, c - o
        dot = (co[:, 0] * pc[:, 0] + co[:, 1] * pc[:, 1]) + co[:, 2] * pc[:, 2]
        dist = np.sqrt((pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]) + pc[:, 2] * pc[:, 2])
        sdf = np.where(dot >= 0, dist, -dist).astype(np.float32)
        return g, sdf, R["index"][ray]

    def integrate(self, points, origins, colors=None):
        points = np.asarray(points, np.float32).reshape(-1, 3)
        g, sdf, ray = self.updates(points, origins)
        col = np.zeros((len(points), 3), np.int64) if colors is None else u8(np.asarray(colors).reshape(-1, 3))
        U = g >> 4
        i = (g[:, 0] & 15) | ((g[:, 1] & 15) << 4) | ((g[:, 2] & 15) << 8)
        key = (U[:, 0] + (1 << 20)) | ((U[:, 1] + (1 << 20)) << 21) | ((U[:, 2] + (1 << 20)) << 42)   # (|unit| < 2^19)
        key, first, inv = np.unique(key, return_index=True, return_inverse=True)
        uniq, inv = U[first], inv.reshape(-1)
        n = len(uniq)
        flat = inv * 4096 + i

        def total(sel, w=None):             # integer sums per voxel (bincount adds in float64: exact below 2^53)
            s = np.bincount(flat[sel], weights=None if w is None else w.astype(np.float64), minlength=n * 4096)
            return np.rint(s).astype(np.int64).reshape(n, 4096)

        upd = sdf > -self.trunc
        q = np.rint((np.minimum(self.trunc, sdf[upd]) / self.trunc) * Q).astype(np.int64)
        sum_q, count = total(upd, q), total(upd)
        band = upd & (np.abs(sdf) < self.trunc)
        rgb_sum = np.stack([total(band, col[ray[band], k]) for k in range(3)], -1)
        rgb_count = total(band)
        for k, u in enumerate(map(tuple, uniq)):                               # (a visited unit is allocated, updated or not)
            d = self.units.setdefault(u, dict(sum_q=np.zeros(4096, np.int64), count=np.zeros(4096, np.int64),
                                              rgb_sum=np.zeros((4096, 3), np.int64), rgb_count=np.zeros(4096, np.int64)))
            d["sum_q"] += sum_q[k]; d["count"] += count[k]; d["rgb_sum"] += rgb_sum[k]; d["rgb_count"] += rgb_count[k]

    def unit_arrays(self):
        """(coords [n,3] in map order, sum_q [n,4096], count, rgb_sum [n,4096,3], rgb_count): ``PointTSDFVolume.units()``."""
        if not self.units:
            z = np.zeros((0, 4096), np.int64)
            return np.zeros((0, 3), np.int64), z, z, np.zeros((0, 4096, 3), np.int64), z
        U = np.array(sorted(self.units, key=lambda c: (c[2], c[1], c[0])), np.int64)
        get = lambda k: np.stack([self.units[tuple(u)][k] for u in U])          # noqa: E731
        return U, get("sum_q"), get("count"), get("rgb_sum"), get("rgb_count")

    def finalised(self, min_weight=5):
        """(coords, tsdf, w, rgb 0..255) fp32: the pool's planes."""
        U, sq, cnt, rs, rc = self.unit_arrays()
        with np.errstate(all="ignore"):
            tsdf = np.where(cnt > 0, (sq.astype(np.float64) / cnt.astype(np.float64)).astype(np.float32) * (F(1) / Q), F(0))
            rgb = np.where(rc[..., None] > 0, (rs.astype(np.float64) / rc[..., None].astype(np.float64)).astype(np.float32), F(0))
        w = np.where(cnt >= min_weight, cnt.astype(np.float32), F(0))
        return U, tsdf.astype(np.float32), w.astype(np.float32), rgb.astype(np.float32)

    def extract_mesh(self, min_weight=5):
        U, tsdf, w, rgb = self.finalised(min_weight)
        r = RestatedTSDF(float(self.vs), float(self.trunc))
        for k, u in enumerate(map(tuple, U)):
            r.units[u] = np.concatenate([tsdf[k][None], w[k][None], rgb[k].T]).astype(np.float32)
        return r.extract_mesh()
