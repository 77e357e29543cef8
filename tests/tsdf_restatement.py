"""fp32 numpy restatement of the TSDF volume and its marching cubes: the oracle of csrc/tsdf.hip.

Every expression is evaluated in the kernels' order with float32 operands, so the voxel grids are bit-identical to the GPU's
and the meshes equal it exactly (triangles) and to rounding (vertices, colours).  Open3D itself is not pinned.
"""
from __future__ import annotations

import numpy as np

from collab_splats_amd.mc_tables import EDGES, tables

F = np.float32
UNIT = 16
LOCAL = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1)[..., ::-1].reshape(-1, 3)
# LOCAL[i] = (lx, ly, lz) with i = lx + 16 ly + 256 lz


def _valid_depth(d, mask, dtrunc):
    ok = (d > F(0)) & ~(d > dtrunc)
    if mask is not None:
        ok &= mask.astype(bool)
    return np.where(ok, d, F(0)).astype(np.float32)


def _u8(rgb):
    return np.clip(rgb.astype(np.float32) * F(255), F(0), F(255)).astype(np.int32).astype(np.float32)


class RestatedTSDF:
    def __init__(self, voxel_size, sdf_trunc, depth_trunc=3.0, bounds=None):
        self.vs, self.trunc, self.dtrunc = F(voxel_size), F(sdf_trunc), F(depth_trunc)
        self.ulen = F(self.vs * F(16))
        self.clip = None
        if bounds is not None:
            b = np.asarray(bounds, np.float64).reshape(2, 3)
            ul = float(self.ulen)
            self.clip = (np.floor(b[0] / ul).astype(np.int64), np.floor(b[1] / ul).astype(np.int64))
        self.units = {}                       # (ux, uy, uz) -> [5, 4096] float32 (tsdf, w, r, g, b)

    # --------------------------------------------------------------------------------------------------- allocation
    def sample_boxes(self, depth, viewmat, K, mask=None):
        """Per sample with data: the inclusive unit box [lo, hi] (int64 [n,2,3]) of p +- sdf_trunc."""
        H, W = depth.shape
        d = _valid_depth(depth, mask, self.dtrunc)[::4, ::4]
        vv, uu = np.meshgrid(np.arange(0, H, 4), np.arange(0, W, 4), indexing="ij")
        sel = d > 0
        d, u, v = d[sel], uu[sel].astype(np.float32), vv[sel].astype(np.float32)
        M, K = np.asarray(viewmat, np.float32), np.asarray(K, np.float32)
        fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
        xc, yc, zc = ((u - cx) * d) / fx, ((v - cy) * d) / fy, d
        dx, dy, dz = xc - M[0, 3], yc - M[1, 3], zc - M[2, 3]
        p = np.stack([(M[0, a] * dx + M[1, a] * dy) + M[2, a] * dz for a in range(3)], -1)
        lo = np.floor((p - self.trunc) / self.ulen).astype(np.int64)
        hi = np.floor((p + self.trunc) / self.ulen).astype(np.int64)
        if self.clip is not None:
            lo, hi = np.maximum(lo, self.clip[0]), np.minimum(hi, self.clip[1])
        return np.stack([lo, hi], 1)

    def touched_units(self, depth, viewmat, K, mask=None):
        """Sorted unique unit coordinates [n,3] the view touches."""
        boxes = self.sample_boxes(depth, viewmat, K, mask)
        if len(boxes) == 0:
            return np.zeros((0, 3), np.int64)
        ext = boxes[:, 1] - boxes[:, 0] + 1
        out = []
        if not np.any(np.all(ext > 0, 1)):                # the bounds leave no sample a unit
            return np.zeros((0, 3), np.int64)
        n = int(ext.max())
        for oz in range(n):
            for oy in range(n):
                for ox in range(n):
                    o = np.array([ox, oy, oz])
                    ok = np.all(o[None] < ext, 1)
                    out.append(boxes[ok, 0] + o[None])
        U = np.unique(np.concatenate(out), axis=0)
        return U[np.lexsort((U[:, 0], U[:, 1], U[:, 2]))]

    # --------------------------------------------------------------------------------------------------- integration
    def integrate(self, depths, viewmats, Ks, rgbs=None, masks=None):
        depths = np.asarray(depths, np.float32)
        if depths.ndim == 4:
            depths = depths[..., 0]
        for j in range(depths.shape[0]):
            m = None if masks is None else np.asarray(masks[j]).reshape(depths.shape[1:])
            c = None if rgbs is None else np.asarray(rgbs[j], np.float32)
            self.integrate_view(depths[j], np.asarray(viewmats[j], np.float32), np.asarray(Ks[j], np.float32), c, m)

    def integrate_view(self, depth, M, K, rgb=None, mask=None):
        H, W = depth.shape
        U = self.touched_units(depth, M, K, mask)
        if len(U) == 0:
            return
        for u in map(tuple, U):
            if u not in self.units:
                self.units[u] = np.zeros((5, 4096), np.float32)
        data = np.stack([self.units[u] for u in map(tuple, U)])                # [n,5,4096]
        g = (U[:, None, :] * 16 + LOCAL[None]).astype(np.float32)              # [n,4096,3]
        x, y, z = [((g[..., a] + F(0.5)) * self.vs) for a in range(3)]
        fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
        with np.errstate(all="ignore"):
            zc = ((M[2, 0] * x + M[2, 1] * y) + M[2, 2] * z) + M[2, 3]
            xc = ((M[0, 0] * x + M[0, 1] * y) + M[0, 2] * z) + M[0, 3]
            yc = ((M[1, 0] * x + M[1, 1] * y) + M[1, 2] * z) + M[1, 3]
            uf = ((xc * fx) / zc + cx) + F(0.5)
            vf = ((yc * fy) / zc + cy) + F(0.5)
            ok = (zc > 0) & (uf >= F(0.0001)) & (uf < F(W)) & (vf >= F(0.0001)) & (vf < F(H))
            ui = np.where(ok, uf, 0).astype(np.int64)
            vi = np.where(ok, vf, 0).astype(np.int64)
            dmap = _valid_depth(depth, mask, self.dtrunc)
            d = np.where(ok, dmap[vi, ui], F(0))
            ok &= d != 0
            a = (ui.astype(np.float32) - cx) / fx
            b = (vi.astype(np.float32) - cy) / fy
            sdf = (d - zc) * np.sqrt((F(1) + a * a) + b * b)
            ok &= sdf > -self.trunc
            tn = np.minimum(F(1), sdf / self.trunc)
        w = data[:, 1]
        w1 = w + F(1)
        data[:, 0] = np.where(ok, (data[:, 0] * w + tn) / w1, data[:, 0])
        col = _u8(rgb[vi, ui]) if rgb is not None else np.zeros(ui.shape + (3,), np.float32)
        for q in range(3):
            data[:, 2 + q] = np.where(ok, (data[:, 2 + q] * w + col[..., q]) / w1, data[:, 2 + q])
        data[:, 1] = np.where(ok, w1, w)
        for k, u in enumerate(map(tuple, U)):
            self.units[u] = data[k]

    def unit_arrays(self):
        """(coords [n,3] in map order, tsdf [n,4096], w, rgb [n,4096,3]) -- TSDFVolume.units()'s layout."""
        if not self.units:
            z = np.zeros((0, 4096), np.float32)
            return np.zeros((0, 3), np.int64), z, z, np.zeros((0, 4096, 3), np.float32)
        U = np.array(sorted(self.units, key=lambda c: (c[2], c[1], c[0])), np.int64)
        D = np.stack([self.units[tuple(u)] for u in U])
        return U, D[:, 0], D[:, 1], np.ascontiguousarray(D[:, 2:5].transpose(0, 2, 1))

    # --------------------------------------------------------------------------------------------------- extraction
    def extract_mesh(self):
        U, T, Wt, C = self.unit_arrays()
        if len(U) == 0:
            return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32)
        org = U.min(0) * 16 - 1
        shape = tuple(((U.max(0) - U.min(0) + 1) * 16 + 2)[::-1])               # [z, y, x]
        tsdf = np.zeros(shape, np.float32)
        w = np.zeros(shape, np.float32)
        alloc = np.zeros(shape, bool)
        rgb = np.zeros(shape + (3,), np.float32)
        G = (U[:, None, :] * 16 + LOCAL[None]).reshape(-1, 3)                    # ordered voxels, global coords
        Z, Y, X = (G - org)[:, 2], (G - org)[:, 1], (G - org)[:, 0]
        tsdf[Z, Y, X], w[Z, Y, X], alloc[Z, Y, X] = T.reshape(-1), Wt.reshape(-1), True
        rgb[Z, Y, X] = C.reshape(-1, 3)
        good = alloc & (w > 0)
        neg = tsdf < 0

        def at(arr, off, fill):
            """arr[p + off] for every voxel p of the padded array (fill outside)."""
            out = np.full_like(arr, fill)
            sz, sy, sx = [slice(max(0, -o), arr.shape[k] - max(0, o)) for k, o in zip(range(3), off[::-1])]
            dz, dy, dx = [slice(max(0, o), arr.shape[k] - max(0, -o)) for k, o in zip(range(3), off[::-1])]
            out[sz, sy, sx] = arr[dz, dy, dx]
            return out

        corners = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]
        valid = np.ones(shape, bool)
        cube = np.zeros(shape, np.int32)
        for c, o in enumerate(corners):
            valid &= at(good, o, False)
            cube |= at(neg, o, False).astype(np.int32) << c
        vmask = np.zeros(shape, np.int32)
        for a in range(3):
            b1, b2 = [x for x in range(3) if x != a]
            e = lambda *ax: tuple(-1 if k in ax else 0 for k in range(3))
            anyv = valid | at(valid, e(b1), False) | at(valid, e(b2), False) | at(valid, e(b1, b2), False)
            step = tuple(1 if k == a else 0 for k in range(3))
            vmask |= (anyv & (neg != at(neg, step, False))).astype(np.int32) << a
        ntri_t, tri_t, _ = tables()
        ntri = np.where(valid, ntri_t[cube].astype(np.int32), 0)

        vm = vmask[Z, Y, X]
        nv = (vm & 1) + ((vm >> 1) & 1) + ((vm >> 2) & 1)
        base = np.cumsum(nv) - nv
        vbase = np.zeros(shape, np.int64)
        vbase[Z, Y, X] = base
        # vertices: voxel-major, axis-minor
        pos, col = [], []
        p0 = (G.astype(np.float32) + F(0.5)) * self.vs
        f0 = np.abs(tsdf[Z, Y, X])
        for a in range(3):
            step = tuple(1 if k == a else 0 for k in range(3))
            f1 = np.abs(at(tsdf, step, F(0))[Z, Y, X])
            s = f0 + f1
            with np.errstate(all="ignore"):
                p = p0.copy()
                p[:, a] = p[:, a] + (f0 / s) * self.vs
                c1 = at(rgb, step, F(0))[Z, Y, X]
                c = ((f1[:, None] * rgb[Z, Y, X] + f0[:, None] * c1) / s[:, None]) / F(255)
            pos.append(p)
            col.append(c)
        sel = np.stack([(vm >> a) & 1 for a in range(3)], 1).astype(bool)
        verts = np.stack(pos, 1)[sel].astype(np.float32)
        cols = np.stack(col, 1)[sel].astype(np.float32)
        # triangles: voxel-major, table order
        nt = ntri[Z, Y, X]
        cb = cube[Z, Y, X]
        idx = np.full((len(G), tri_t.shape[1]), -1, np.int64)
        for q in range(tri_t.shape[1]):
            live = q < 3 * nt
            if not live.any():
                continue
            e = tri_t[cb[live], q].astype(np.int64)
            c0 = np.array([EDGES[k][0] for k in range(12)])[e]
            ax = e // 4
            o = np.stack([c0 & 1, (c0 >> 1) & 1, (c0 >> 2) & 1], 1)
            og = (G[live] - org) + o
            ob = vbase[og[:, 2], og[:, 1], og[:, 0]]
            om = vmask[og[:, 2], og[:, 1], og[:, 0]]
            below = om & ((1 << ax) - 1)
            idx[live, q] = ob + (below & 1) + ((below >> 1) & 1)
        tris = idx[idx >= 0].reshape(-1, 3).astype(np.int32)
        return verts, tris, cols
