"""The Gaussian density field of csrc/density.hip restated on the CPU: test infrastructure, never
imported by the package.

Two things:
  * the fp64 ORACLE: d, grad d, values and dominant straight from the definition over ALL Gaussians -- no units, no lists;
  * the fp32 RESTATEMENT: the Gaussians' frames, unit ranges, slab tests and per-unit lists in numpy fp32 in the kernels' operation
    order (every expression parenthesised as density.hip writes it: the integer structures are compared bit for bit), and the
    field summed in list order.

Definition: R = R(q / |q|) with columns e_a, A = diag(1 / s) R^T, m_g(x) = |A_g (x - mu_g)|^2,
    k_g(x) = o_g (exp(-m_g / 2) - exp(-r^2 / 2)) if m_g < r^2 else 0,   d = sum_g k_g,
    grad d = -sum_{m_g < r^2} o_g exp(-m_g / 2) A_g^T A_g (x - mu_g),
    dominant = the g of the largest k_g (the lowest at a tie, -1 where d = 0),  values = sum_g k_g v_g / d (0 where d = 0).
"""
import numpy as np

UNIT = 16
F = np.float32


def _rot(q):
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = q.dtype.type(1), q.dtype.type(2)
    R = np.empty((q.shape[0], 3, 3), q.dtype)
    R[:, 0, 0] = one - two * (y * y + z * z); R[:, 0, 1] = two * (x * y - r * z); R[:, 0, 2] = two * (x * z + r * y)
    R[:, 1, 0] = two * (x * y + r * z); R[:, 1, 1] = one - two * (x * x + z * z); R[:, 1, 2] = two * (y * z - r * x)
    R[:, 2, 0] = two * (x * z - r * y); R[:, 2, 1] = two * (y * z + r * x); R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def frames(means, quats, scales, opacities, cutoff, min_opacity, dtype):
    """(participates [N] bool, R [N,3,3], E [N,3]) in ``dtype`` in the kernels' operation order; the rule of participation is
    evaluated on the fp32 inputs against fp32(min_opacity) for either dtype."""
    mu32, q32, s32, o32 = (np.asarray(v, F) for v in (means, quats, scales, np.reshape(opacities, -1)))
    with np.errstate(all="ignore"):
        ok = np.isfinite(mu32).all(1) & np.isfinite(q32).all(1) & np.isfinite(s32).all(1) & (s32 > 0).all(1)
        ok &= np.isfinite(o32) & (o32 >= F(min_opacity))
        q, s = q32.astype(dtype), s32.astype(dtype)
        w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        n = np.sqrt(((w * w + x * x) + y * y) + z * z)
        ok &= np.isfinite(n) & (n > 0)
        R = _rot(q / n[:, None])
        a = R * s[:, None, :]
        E = dtype(cutoff) * np.sqrt((a[:, :, 0] * a[:, :, 0] + a[:, :, 1] * a[:, :, 1]) + a[:, :, 2] * a[:, :, 2])
        ok &= np.isfinite(E).all(1)
    return ok, R, E


# ------------------------------------------------------------------------------------------------------------------ oracle
class Oracle:
    """fp64, over all participating Gaussians."""

    def __init__(self, means, quats, scales, opacities, cutoff=3.0, min_opacity=1.0 / 255.0):
        ok, R, _ = frames(means, quats, scales, opacities, cutoff, min_opacity, np.float64)
        self.ids = np.nonzero(ok)[0]
        self.mu = np.asarray(means, F).astype(np.float64)[ok]
        s = np.asarray(scales, F).astype(np.float64)[ok]
        self.o = np.asarray(opacities, F).reshape(-1).astype(np.float64)[ok]
        self.A = np.transpose(R[ok], (0, 2, 1)) / s[:, :, None]            # A[g, a, i] = R[g, i, a] / s[g, a]
        self.r2 = float(cutoff) ** 2
        self.ecut = np.exp(-0.5 * self.r2)
        self.n_all = int(np.asarray(means).shape[0])

    def terms(self, points):
        """(k, t, inside, e) with k [P,G'] the terms, t [P,G',3] = A (x - mu), over the participating Gaussians (columns:
        self.ids).  t = A x - A mu through one matrix product: in fp64 the cancellation costs 1e-13 at most here."""
        p = np.asarray(points, np.float64)
        G = len(self.ids)
        Af = self.A.reshape(3 * G, 3)
        b = np.einsum("gai,gi->ga", self.A, self.mu).reshape(3 * G)
        t = (p @ Af.T - b[None, :]).reshape(-1, G, 3)
        m = (t * t).sum(-1)
        inside = m < self.r2
        e = np.exp(-0.5 * m)
        k = np.where(inside, self.o[None, :] * (e - self.ecut), 0.0)
        return k, t, inside, e

    def scale(self, points, chunk=8192):
        """S [P] = sum over g with m_g < r^2 (1 + 1e-3) of o_g (exp(-m_g / 2) (1 + m_g / 2) + exp(-r^2 / 2)): the size of the terms a
        point's density is made of, each with the factor 1 + m / 2 by which a relative error of the exponent's argument grows
        (d exp(-m / 2) = exp(-m / 2) (m / 2) dm / m).  The local scale an error at the point is measured against; 0 where no
        Gaussian comes within a thousandth of its cut-off."""
        p = np.asarray(points, np.float64).reshape(-1, 3)
        out = np.zeros(p.shape[0])
        if len(self.ids) == 0:
            return out
        for c0 in range(0, p.shape[0], chunk):
            sl = slice(c0, min(c0 + chunk, p.shape[0]))
            _, t, _, e = self.terms(p[sl])
            m = (t * t).sum(-1)
            out[sl] = np.where(m < self.r2 * (1.0 + 1e-3), self.o[None, :] * (e * (1.0 + 0.5 * m) + self.ecut), 0.0).sum(1)
        return out

    def evaluate(self, points, values=None, chunk=16384):
        """dict: density [P], grad [P,3], dominant [P] int32 (the lowest g among equal largest terms; -1 where d = 0), best and
        second [P] (the largest and second largest term), min_m [P] (the smallest m_g), values [P,D] or None."""
        p = np.asarray(points, np.float64).reshape(-1, 3)
        P, G = p.shape[0], len(self.ids)
        out = dict(density=np.zeros(P), grad=np.zeros((P, 3)), dominant=np.full(P, -1, np.int32), best=np.zeros(P),
                   second=np.zeros(P), min_m=np.full(P, np.inf), values=None)
        v = None
        if values is not None:
            v = np.asarray(values, np.float64)[self.ids]
            out["values"] = np.zeros((P, v.shape[1]))
        if G == 0:
            return out
        Af = self.A.reshape(3 * G, 3)
        for c0 in range(0, P, chunk):
            sl = slice(c0, min(c0 + chunk, P))
            k, t, inside, e = self.terms(p[sl])
            d = k.sum(1)
            out["density"][sl] = d
            out["min_m"][sl] = (t * t).sum(-1).min(1)
            w = np.where(inside, self.o[None, :] * e, 0.0)
            out["grad"][sl] = -((w[:, :, None] * t).reshape(-1, 3 * G) @ Af)
            best = np.argmax(k, axis=1)                                    # (the first, so the lowest g, among equals)
            rows = np.arange(k.shape[0])
            kb = k[rows, best]
            out["best"][sl] = kb
            if G > 1:
                k[rows, best] = -1.0
                out["second"][sl] = np.maximum(k.max(1), 0.0)
                k[rows, best] = kb
            out["dominant"][sl] = np.where(d > 0, self.ids[best], -1)
            if v is not None:
                out["values"][sl] = np.where(d[:, None] > 0, (k @ v) / np.where(d > 0, d, 1.0)[:, None], 0.0)
        return out


# ------------------------------------------------------------------------------------------------------------- restatement
class Restated:
    """fp32, in the kernels' operation order."""

    def __init__(self, means, quats, scales, opacities, voxel_size, cutoff=3.0, min_opacity=1.0 / 255.0, bounds=None):
        self.mu = np.ascontiguousarray(means, F)
        self.s = np.ascontiguousarray(scales, F)
        self.o = np.ascontiguousarray(opacities, F).reshape(-1)
        self.h64 = float(voxel_size)
        self.h = F(voxel_size)
        self.L = F(self.h * F(UNIT))
        self.r = F(cutoff)
        N = self.mu.shape[0]
        self.ok, self.R, self.E = frames(means, quats, scales, opacities, cutoff, min_opacity, F)
        with np.errstate(all="ignore"):
            self.A = np.transpose(self.R, (0, 2, 1)) / self.s[:, :, None]      # A[g, a, i] = R[g, i, a] / s[g, a]
        self.records = np.zeros((N, 16), F)
        self.records[:, 13:16] = -1
        k = self.ok
        self.records[k, 0:3] = self.mu[k]
        self.records[k, 3:12] = self.A[k].reshape(-1, 9)
        self.records[k, 12] = self.o[k]
        self.records[k, 13:16] = self.E[k]
        self.lo = np.zeros(3, np.int64)
        self.dims = np.zeros(3, np.int64)
        self.lists = {}                              # map index -> ascending list of g
        self.aabb_pairs = 0                          # pairs the range alone (no slab test) would give
        if bounds is None:
            if not k.any():
                return
            lo_w = (self.mu[k] - self.E[k]).min(0).astype(np.float64) - self.h64
            hi_w = (self.mu[k] + self.E[k]).max(0).astype(np.float64) + self.h64
        else:
            lo_w, hi_w = (np.asarray(b, np.float64) for b in bounds)
        ulen = float(self.L)
        self.lo = np.floor(lo_w / ulen).astype(np.int64)
        self.dims = np.floor(hi_w / ulen).astype(np.int64) - self.lo + 1
        self._build_lists()

    def _build_lists(self):
        h, L, r = self.h, self.L, self.r
        H = F(F(0.5) * L + h)
        for g in np.nonzero(self.ok)[0]:
            mu, E, R, s = self.mu[g], self.E[g], self.R[g], self.s[g]
            with np.errstate(all="ignore"):
                l = np.clip(np.floor(((mu - E) - h) / L), F(-1e6), F(1e6)).astype(np.int64)
                u = np.clip(np.floor(((mu + E) + h) / L), F(-1e6), F(1e6)).astype(np.int64)
            l = np.maximum(l, self.lo)
            u = np.minimum(u, self.lo + self.dims - 1)
            if np.any(l > u):
                continue
            self.aabb_pairs += int(np.prod(u - l + 1))
            bound = [F(r * s[a]) + F(H * F(F(abs(R[0, a]) + abs(R[1, a])) + abs(R[2, a]))) for a in range(3)]
            uz, uy, ux = np.meshgrid(np.arange(l[2], u[2] + 1), np.arange(l[1], u[1] + 1), np.arange(l[0], u[0] + 1), indexing="ij")
            ux, uy, uz = ux.ravel(), uy.ravel(), uz.ravel()                  # z, y, x order: ascending map index
            d0 = (ux.astype(F) + F(0.5)) * L - mu[0]
            d1 = (uy.astype(F) + F(0.5)) * L - mu[1]
            d2 = (uz.astype(F) + F(0.5)) * L - mu[2]
            keep = np.ones(ux.shape, bool)
            for a in range(3):
                p = (R[0, a] * d0 + R[1, a] * d1) + R[2, a] * d2
                keep &= np.abs(p) <= bound[a]
            m = (ux - self.lo[0]) + self.dims[0] * ((uy - self.lo[1]) + self.dims[1] * (uz - self.lo[2]))
            for mi in m[keep]:
                self.lists.setdefault(int(mi), []).append(int(g))

    # the structures the GPU is compared with, in map order
    def unit_coords(self):
        m = np.array(sorted(self.lists), np.int64)
        if len(m) == 0:
            return np.zeros((0, 3), np.int64)
        nx, ny = int(self.dims[0]), int(self.dims[1])
        return np.stack([m % nx, (m // nx) % ny, m // (nx * ny)], 1) + self.lo[None, :]

    def unit_lists(self):
        keys = sorted(self.lists)
        offsets = np.zeros(len(keys) + 1, np.int64)
        for i, m in enumerate(keys):
            offsets[i + 1] = offsets[i] + len(self.lists[m])
        ids = np.array([g for m in keys for g in self.lists[m]], np.int32)
        return offsets, ids

    @property
    def n_pairs(self):
        return sum(len(v) for v in self.lists.values())

    def _sum_list(self, lst, x, y, z, values=None):
        """fp32 sums over one list, in list order, at the fp32 positions x, y, z."""
        r2 = F(self.r * self.r)
        ecut = np.exp(F(F(-0.5) * r2))
        d = np.zeros(x.shape, F)
        grad = np.zeros(x.shape + (3,), F)
        vals = None if values is None else np.zeros(x.shape + (values.shape[1],), F)
        for g in lst:
            A, mu, o = self.A[g], self.mu[g], self.o[g]
            dx, dy, dz = x - mu[0], y - mu[1], z - mu[2]
            t = [(A[a, 0] * dx + A[a, 1] * dy) + A[a, 2] * dz for a in range(3)]
            mm = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
            inside = mm < r2
            e = np.exp(F(-0.5) * mm)
            k = np.where(inside, o * (e - ecut), F(0))
            d = d + k
            w = np.where(inside, o * e, F(0))
            for i in range(3):
                grad[..., i] = grad[..., i] - w * ((A[0, i] * t[0] + A[1, i] * t[1]) + A[2, i] * t[2])
            if vals is not None:
                vals = vals + k[..., None] * values[g][None, :]
        return d, grad, vals

    def unit_fields(self):
        """d [n,4096] fp32 at the voxel centres of the allocated units, in map order (voxel i = lx + 16 ly + 256 lz)."""
        coords = self.unit_coords()
        keys = sorted(self.lists)
        out = np.zeros((len(keys), UNIT ** 3), F)
        i = np.arange(UNIT ** 3)
        lx, ly, lz = i & 15, (i >> 4) & 15, i >> 8
        for n, m in enumerate(keys):
            c = coords[n]
            x = ((c[0] * 16 + lx).astype(F) + F(0.5)) * self.h
            y = ((c[1] * 16 + ly).astype(F) + F(0.5)) * self.h
            z = ((c[2] * 16 + lz).astype(F) + F(0.5)) * self.h
            out[n] = self._sum_list(self.lists[m], x, y, z)[0]
        return out

    def map_index(self, points):
        """[P] int64: the map index of the unit of each point's voxel floor(p / h) (the fp32 division the kernel makes), -1 for
        a non-finite point or one outside the map."""
        p = np.ascontiguousarray(points, F).reshape(-1, 3)
        with np.errstate(all="ignore"):
            fin = np.isfinite(p).all(1)
            vox = np.clip(np.floor(p / self.h), F(-3e7), F(3e7))
            vox = np.where(np.isfinite(vox), vox, 0).astype(np.int64)
        u = (vox >> 4) - self.lo[None, :]
        inside = fin & (u >= 0).all(1) & (u < self.dims[None, :]).all(1)
        return np.where(inside, u[:, 0] + self.dims[0] * (u[:, 1] + self.dims[1] * u[:, 2]), -1)

    def query(self, points, values=None):
        """fp32 (density, grad, values) at points, from the list of the unit of the point's voxel floor(p / h)."""
        p = np.ascontiguousarray(points, F).reshape(-1, 3)
        P = p.shape[0]
        v = None if values is None else np.ascontiguousarray(values, F)
        d = np.zeros(P, F)
        grad = np.zeros((P, 3), F)
        vals = None if v is None else np.zeros((P, v.shape[1]), F)
        if P == 0 or not self.lists:
            return d, grad, vals
        m = self.map_index(p)
        for mi in np.unique(m):
            if mi < 0 or int(mi) not in self.lists:
                continue
            sel = np.nonzero(m == mi)[0]
            dd, gg, vv = self._sum_list(self.lists[int(mi)], p[sel, 0], p[sel, 1], p[sel, 2], v)
            d[sel], grad[sel] = dd, gg
            if vals is not None:
                with np.errstate(all="ignore"):
                    vals[sel] = np.where(dd[:, None] > 0, vv / dd[:, None], F(0))
        return d, grad, vals

    def voxel_centres(self):
        """fp64 centres [n,4096,3] of the voxels of the allocated units, in map order: ((g + 0.5) h with the fp32 h the kernel
        holds, evaluated in fp32 as the kernel does, then widened -- the positions the GPU evaluates at)."""
        coords = self.unit_coords()
        i = np.arange(UNIT ** 3)
        l = np.stack([i & 15, (i >> 4) & 15, i >> 8], 1)
        g = coords[:, None, :] * 16 + l[None, :, :]
        return ((g.astype(F) + F(0.5)) * self.h).astype(np.float64)

    def map_voxel_centres(self):
        """The same for EVERY unit of the map, allocated or not: (centres [n_map,4096,3], allocated [n_map] bool)."""
        nx, ny, nz = (int(v) for v in self.dims)
        m = np.arange(nx * ny * nz)
        coords = np.stack([m % nx, (m // nx) % ny, m // (nx * ny)], 1) + self.lo[None, :]
        i = np.arange(UNIT ** 3)
        l = np.stack([i & 15, (i >> 4) & 15, i >> 8], 1)
        g = coords[:, None, :] * 16 + l[None, :, :]
        alloc = np.array([int(k) in self.lists for k in m], bool)
        return ((g.astype(F) + F(0.5)) * self.h).astype(np.float64), alloc
