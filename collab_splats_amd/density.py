"""The density of the Gaussian mixture itself on the MI355X, and marching-cubes meshes of its level sets (csrc/density.hip,
DESIGN.md section 25).

What the reference's ``MarchingCubesMesh`` and ``LevelSetExtractor`` reach through ``model.get_density`` /
``get_density_grad`` / ``get_closest_gaussians`` (collab_splats/utils/mesh.py:1234-1359, :1045-1230), restated from the
published definition (SuGaR's density): with ``A = diag(1 / s) R(q)^T`` and ``m_g(x) = |A_g (x - mu_g)|^2``,

    k_g(x) = o_g (exp(-m_g / 2) - exp(-r^2 / 2))  where m_g < r^2, else 0;      d(x) = sum_g k_g(x)

(continuous at the cut-off ``r``).  ``DensityField`` evaluates ``d`` on the TSDF volume's lattice (voxel ``g`` centred at
``(g + 0.5) voxel_size``, units of 16^3 voxels, only the units a Gaussian reaches allocated), answers point queries from the
same per-unit lists and extracts level sets through the TSDF volume's marching cubes.  ``DensityField.raycast`` and
``level_surface_points`` are the level-set search along rays that ``LevelSetExtractor`` asks of
``model.compute_level_surface_points`` (a dn-splatter / SuGaR method the reference's models lack).
Everything stays on the device; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from ._lib import MisplatError, load, ptr, require_gpu, run
from .meshmap import _prep
from .unitvolume import (MAX_UNITS, UNIT, UNIT_VOXELS, Grid, Stages, _unit_range, alloc_units, empty_mesh, make_grid, map_order,
                         map_span, marching_cubes, unit_coords, unit_lists)

REC = 16                             # floats per record (include/misplat.h MISPLAT_DENSITY_REC)
MAX_CHANNELS = 16                    # channels of query's values (MISPLAT_DENSITY_MAX_CHANNELS)
MAX_PAIRS = (1 << 31) - 4096
MAX_LEVELS = 4                       # levels of one raycast (passed to the kernel by value)


def _scalars(name: str, voxel_size, cutoff, min_opacity) -> Tuple[float, float, float]:
    try:
        h, r, mo = float(voxel_size), float(cutoff), float(min_opacity)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: voxel_size, cutoff and min_opacity must be numbers") from None
    if not (h > 0 and math.isfinite(h)):
        raise ValueError(f"{name}: voxel_size must be a finite number > 0, got {voxel_size!r}")
    if not 0 < r <= 6:
        raise ValueError(f"{name}: cutoff must be in (0, 6], got {cutoff!r}")
    if not 0 <= mo <= 1:
        raise ValueError(f"{name}: min_opacity must be in [0, 1], got {min_opacity!r}")
    return h, r, mo


def _gaussians(name: str, means, quats, scales, opacities) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    for label, t in (("means", means), ("quats", quats), ("scales", scales), ("opacities", opacities)):
        if not isinstance(t, Tensor) or not t.is_floating_point():
            raise ValueError(f"{name}: {label} must be a floating-point tensor")
    if means.dim() != 2 or means.shape[1] != 3:
        raise ValueError(f"{name}: means must be [N,3], got {tuple(means.shape)}")
    n = means.shape[0]
    if tuple(quats.shape) != (n, 4):
        raise ValueError(f"{name}: quats must be [{n},4], got {tuple(quats.shape)}")
    if tuple(scales.shape) != (n, 3):
        raise ValueError(f"{name}: scales must be [{n},3], got {tuple(scales.shape)}")
    if tuple(opacities.shape) not in ((n,), (n, 1)):
        raise ValueError(f"{name}: opacities must be [{n}] or [{n},1], got {tuple(opacities.shape)}")
    if n >= 1 << 31:
        raise ValueError(f"{name}: at most 2^31 - 1 Gaussians")
    return means, quats, scales, opacities.reshape(-1)


def _points(name: str, points) -> Tensor:
    if not isinstance(points, Tensor) or not points.is_floating_point() or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{name}: points must be a floating-point tensor [P,3], got "
                         f"{tuple(points.shape) if isinstance(points, Tensor) else type(points).__name__}")
    if points.shape[0] >= 1 << 31:
        raise ValueError(f"{name}: at most 2^31 - 1 points")
    return points


def _values(name: str, values, n: int) -> Optional[Tensor]:
    if values is None:
        return None
    if not isinstance(values, Tensor) or not values.is_floating_point() or values.dim() != 2 or values.shape[0] != n:
        raise ValueError(f"{name}: values must be a floating-point tensor [{n},D], got "
                         f"{tuple(values.shape) if isinstance(values, Tensor) else type(values).__name__}")
    if not 1 <= values.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"{name}: values must have 1..{MAX_CHANNELS} channels, got D = {values.shape[1]}")
    return values


def _rays(name: str, origins, dirs, t_near, t_far) -> int:
    for label, t in (("origins", origins), ("dirs", dirs)):
        if not isinstance(t, Tensor) or not t.is_floating_point() or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{name}: {label} must be a floating-point tensor [M,3], got "
                             f"{tuple(t.shape) if isinstance(t, Tensor) else type(t).__name__}")
    m = int(origins.shape[0])
    if dirs.shape[0] != m:
        raise ValueError(f"{name}: dirs must be [{m},3], got {tuple(dirs.shape)}")
    for label, t in (("t_near", t_near), ("t_far", t_far)):
        if not isinstance(t, Tensor) or not t.is_floating_point() or tuple(t.shape) != (m,):
            raise ValueError(f"{name}: {label} must be a floating-point tensor [{m}], got "
                             f"{tuple(t.shape) if isinstance(t, Tensor) else type(t).__name__}")
    if m >= 1 << 31:
        raise ValueError(f"{name}: at most 2^31 - 1 rays")
    return m


def _levels(name: str, levels) -> Tuple[float, ...]:
    try:
        lv = tuple(float(x) for x in levels)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: levels must be a sequence of numbers, got {levels!r}") from None
    if not 1 <= len(lv) <= MAX_LEVELS:
        raise ValueError(f"{name}: 1..{MAX_LEVELS} levels, got {len(lv)}")
    for x in lv:
        x32 = float(torch.tensor(x, dtype=torch.float32)) if math.isfinite(x) else x
        if not (x > 0 and math.isfinite(x) and x32 > 0 and math.isfinite(x32)):
            raise ValueError(f"{name}: every level must be a finite number > 0 (in fp32), got {x!r}")
    return lv


class DensityField:
    """The mixture's density on the lattice of voxel size ``voxel_size``.

    ``means [N,3]``, ``quats [N,4]`` (wxyz, normalised inside), ACTIVATED ``scales [N,3]`` > 0 and ``opacities [N]`` in [0,1]:
    the arguments of the ``rasterization()`` call.  A Gaussian with opacity below ``min_opacity`` or a non-finite parameter takes
    no part.  ``bounds`` (``[[min xyz], [max xyz]]``): the unit map covers the units overlapping the box and nothing outside is
    evaluated; without it the map covers the AABB of ``mu +- E`` over the participating Gaussians, padded by one voxel (``E``: the
    half sides of the support's box at the cut-off; one host read).  More than ``max_units`` map entries raise ``MisplatError``.
    Two more host reads give the number of (unit, Gaussian) pairs and of allocated units.  Two builds are bitwise equal."""

    def __init__(self, means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, voxel_size: float, cutoff: float = 3.0,
                 min_opacity: float = 1.0 / 255.0, bounds=None, max_units: int = MAX_UNITS, _flags: int = 0,
                 _timings: Optional[dict] = None):
        name = "DensityField"
        means, quats, scales, opacities = _gaussians(name, means, quats, scales, opacities)
        h, r, mo = _scalars(name, voxel_size, cutoff, min_opacity)
        clip = None
        if bounds is not None:
            b = np.asarray(bounds.detach().cpu() if isinstance(bounds, Tensor) else bounds, np.float64)
            if b.shape != (2, 3) or not np.all(np.isfinite(b)) or not np.all(b[1] >= b[0]):
                raise ValueError(f"{name}: bounds must be finite [[min xyz], [max xyz]] with max >= min")
            clip = b
        require_gpu(means, quats, scales, opacities)
        self.device = means.device
        self.voxel_size, self.cutoff, self.min_opacity = h, r, mo
        self.ulen = float(np.float32(h) * np.float32(UNIT))
        self.max_units = min(int(max_units), MAX_UNITS)
        self.n_gauss = int(means.shape[0])
        self.n_units = self.n_pairs = 0
        self.lo = np.zeros(3, np.int64)
        self.dims = np.zeros(3, np.int64)
        self._slot_map = self._pool = self._ids = self._ranges = self._touched = None
        self._records = torch.empty((self.n_gauss, REC), dtype=torch.float32, device=self.device)
        if self.n_gauss == 0:
            return
        lib = load()
        dev = self.device
        mark = Stages(_timings)                                # (scripts/density_bench.py: seconds per stage, synchronised)
        mu, q, s, o = _prep(means), _prep(quats), _prep(scales), _prep(opacities)
        run("misplat_density_records", ptr(mu), ptr(q), ptr(s), ptr(o), self.n_gauss, r, mo, ptr(self._records))
        mark("records")
        if clip is None:
            e = self._records[:, 13:16]
            part = e[:, 0] >= 0
            big = torch.full_like(e, float("inf"))
            lo_w = torch.where(part[:, None], self._records[:, 0:3] - e, big).amin(0)
            hi_w = torch.where(part[:, None], self._records[:, 0:3] + e, -big).amax(0)
            box = torch.stack([lo_w, hi_w]).double().cpu().numpy()                   # host read
            if not np.all(np.isfinite(box)):
                return                                                               # no Gaussian takes part
            clip = np.stack([box[0] - h, box[1] + h])               # (the one-voxel pad of the lists: every unit they reach)
        lo, hi = _unit_range(clip[0], clip[1], self.ulen)
        dims, n_map = map_span(name, "the bounds", lo, hi, self.max_units, "pass bounds= or a larger voxel_size")
        self.lo, self.dims = lo.astype(np.int64), dims
        mark("bounds")
        grid = self._grid()
        ws = torch.empty(int(lib.misplat_density_workspace(self.n_gauss, 0)), dtype=torch.uint8, device=dev)
        pair_off = torch.empty(self.n_gauss + 1, dtype=torch.int32, device=dev)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        run("misplat_density_count", C.byref(grid), ptr(mu), ptr(q), ptr(s), ptr(o), self.n_gauss, r, mo, ptr(ws), ws.numel(),
            ptr(pair_off), ptr(total))
        n_pairs = int(total.item())                                                  # host read
        self._slot_map = torch.full((n_map,), -1, dtype=torch.int32, device=dev)
        mark("count")
        if n_pairs == 0:
            return
        if n_pairs >= MAX_PAIRS:
            raise MisplatError(f"{name}: {n_pairs} (unit, Gaussian) pairs, above the cap of {MAX_PAIRS}: pass bounds= or a larger "
                               f"voxel_size")
        keys = torch.empty(n_pairs, dtype=torch.int32, device=dev)
        ids = torch.empty(n_pairs, dtype=torch.int32, device=dev)
        words = torch.zeros(n_map, dtype=torch.int64, device=dev)
        run("misplat_density_emit", C.byref(grid), ptr(mu), ptr(q), ptr(s), ptr(o), self.n_gauss, r, mo, ptr(pair_off), n_pairs,
            ptr(keys), ptr(ids), ptr(words))
        counters = torch.zeros(2, dtype=torch.int32, device=dev)
        touched = torch.empty(2 * min(n_map, n_pairs), dtype=torch.int32, device=dev)
        n_units, _ = alloc_units(grid, words, self._slot_map, counters, touched)    # host read: the pool's size
        del words
        mark("emit_alloc")
        self._ids, self._ranges = unit_lists(grid, self._slot_map, keys, ids, n_pairs, n_units)
        mark("lists")
        del keys, ids, ws
        self._touched = touched
        self._pool = torch.empty((n_units, 5, UNIT_VOXELS), dtype=torch.float32, device=dev)
        run("misplat_density_accumulate", C.byref(grid), ptr(touched), n_units, ptr(self._records), ptr(self._ids),
            ptr(self._ranges), r, int(_flags), ptr(self._pool))
        mark("accumulate")
        self.n_units, self.n_pairs = n_units, n_pairs

    # ------------------------------------------------------------------------------------------------------------ plumbing
    def _grid(self) -> Grid:
        # (sdf_trunc and depth_trunc: unused here, positive for tsdf.hip)
        return make_grid(self.voxel_size, self.voxel_size, 1.0, self.lo, self.dims)

    def _map_order(self) -> Tensor:
        return map_order(self._slot_map)

    # -------------------------------------------------------------------------------------------------------------- public
    def units(self):
        """The allocated units in map order, on the host (for tests and inspection): ``(coords [n,3] int64, d [n,4096],
        (offsets [n + 1] int64, ids int32))``; voxel i = lx + 16 ly + 256 lz; unit k's list is ``ids[offsets[k]:offsets[k + 1]]``,
        ascending."""
        if self.n_units == 0:
            return (np.zeros((0, 3), np.int64), np.zeros((0, UNIT_VOXELS), np.float32),
                    (np.zeros(1, np.int64), np.zeros(0, np.int32)))
        m = self._map_order()
        slots = self._slot_map[m].long()
        d = self._pool[slots, 0].cpu().numpy()
        rng = self._ranges[slots].cpu().numpy().astype(np.int64)
        ids = self._ids.cpu().numpy()
        coords = unit_coords(m.cpu().numpy(), self.lo, self.dims)
        # (the pairs are sorted by map index: the lists lie in map order, end to end)
        offsets = np.concatenate([rng[:, 0], rng[-1:, 1]])
        assert np.array_equal(rng[1:, 0], rng[:-1, 1]) and rng[0, 0] == 0 and rng[-1, 1] == len(ids)
        return coords, d, (offsets, ids)

    def dense(self) -> Tensor:
        """``[Dz 16, Dy 16, Dx 16]`` fp32 on the device, 0 in unallocated units: for inspection and small grids (torch ops)."""
        dx, dy, dz = (int(v) for v in self.dims)
        out = torch.zeros((dz, dy, dx, UNIT, UNIT, UNIT), dtype=torch.float32, device=self.device)
        if self.n_units:
            m = self._map_order()
            out.view(-1, UNIT, UNIT, UNIT)[m] = self._pool[self._slot_map[m].long(), 0].view(-1, UNIT, UNIT, UNIT)
        return out.permute(0, 3, 1, 4, 2, 5).reshape(dz * UNIT, dy * UNIT, dx * UNIT).contiguous()

    def query(self, points: Tensor, values: Optional[Tensor] = None) -> Dict[str, Optional[Tensor]]:
        """``{"density" [P], "grad" [P,3], "dominant" [P] int32, "values" [P,D] or None}`` at ``points [P,3]``, from the list of
        the unit that holds the point's voxel; ``values [N,D]`` (1 <= D <= 16): per-Gaussian attributes, blended by the terms.
        A point outside the map or in an unallocated unit gives 0 / 0 / -1 / 0.  One lane per point: points that arrive
        spatially ordered (marching-cubes vertices) read coherent lists; sorting arbitrary points by unit first is left for
        later."""
        name = "DensityField.query"
        points = _points(name, points)
        values = _values(name, values, self.n_gauss)
        require_gpu(points, values)
        P = int(points.shape[0])
        dev = self.device
        out = {"density": torch.zeros(P, dtype=torch.float32, device=dev),
               "grad": torch.zeros((P, 3), dtype=torch.float32, device=dev),
               "dominant": torch.full((P,), -1, dtype=torch.int32, device=dev),
               "values": None if values is None else torch.zeros((P, values.shape[1]), dtype=torch.float32, device=dev)}
        if P == 0 or self.n_units == 0:
            return out
        p32 = _prep(points)
        v32 = None if values is None else _prep(values)
        grid = self._grid()
        run("misplat_density_query", C.byref(grid), ptr(self._slot_map), ptr(self._records), ptr(self._ids), ptr(self._ranges),
            self.cutoff, ptr(p32), P, ptr(v32), 0 if v32 is None else int(v32.shape[1]), ptr(out["density"]), ptr(out["grad"]),
            ptr(out["dominant"]), ptr(out["values"]))
        return out

    def raycast(self, origins: Tensor, dirs: Tensor, t_near: Tensor, t_far: Tensor, levels) -> Dict[str, Tensor]:
        """The level-set search along rays: ``{"t": [L,M] fp32, "hit": [L,M] bool}`` for the rays
        ``origins + t dirs`` (``dirs`` used as given, not normalised) over ``t_near <= t <= t_far`` and 1..4 ``levels``, each
        finite and > 0.  Per ray: the density at 64 evenly spaced samples (each exactly what ``query`` gives there); per level the
        first pair of neighbours with ``d_k < level <= d_{k+1}``, 64 more samples inside it, and the linear interpolation in the
        first such pair of those.  A ray with no such pair, with a non-finite input or with ``t_far <= t_near`` misses (``hit``
        False, ``t`` 0); a ray that starts inside a level hits only after the density has dipped below it.  One wave per ray:
        a unit's list is read once for all the samples in it.  Two calls are bitwise equal."""
        name = "DensityField.raycast"
        M = _rays(name, origins, dirs, t_near, t_far)
        lv = _levels(name, levels)
        require_gpu(origins, dirs, t_near, t_far)
        dev = self.device
        t = torch.zeros((len(lv), M), dtype=torch.float32, device=dev)
        hit = torch.zeros((len(lv), M), dtype=torch.uint8, device=dev)
        if M == 0 or self.n_units == 0:
            return {"t": t, "hit": hit.view(torch.bool)}
        o32, v32, a32, b32 = _prep(origins), _prep(dirs), _prep(t_near), _prep(t_far)
        grid = self._grid()
        lv4 = lv + (lv[-1],) * (MAX_LEVELS - len(lv))
        run("misplat_density_raycast", C.byref(grid), ptr(self._slot_map), ptr(self._records), ptr(self._ids),
            ptr(self._ranges), self.cutoff, ptr(o32), ptr(v32), ptr(a32), ptr(b32), M, lv4[0], lv4[1], lv4[2], lv4[3], len(lv),
            ptr(t), ptr(hit))
        return {"t": t, "hit": hit.view(torch.bool)}

    def extract_mesh(self, iso: float = 0.5, values: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
        """Marching cubes of ``iso - d`` through the TSDF volume's extraction (csrc/tsdf.hip), in its deterministic order:
        ``(vertices [M,3] fp32, triangles [T,3] int32, values at the vertices [M,D] or None)``.  The field is negative inside, so
        triangles face decreasing density.  The vertex values are ``query(vertices, values)["values"]``.  The field's pool is
        not changed: any number of level sets may be extracted.  An empty field, or ``iso`` above the maximum, gives the empty
        triple."""
        name = "DensityField.extract_mesh"
        try:
            iso = float(iso)
        except (TypeError, ValueError):
            raise ValueError(f"{name}: iso must be a number") from None
        if not math.isfinite(iso):
            raise ValueError(f"{name}: iso must be finite, got {iso!r}")
        values = _values(name, values, self.n_gauss)
        require_gpu(values)
        dev = self.device
        D = None if values is None else int(values.shape[1])

        def empty():                                               # (the empty mesh, values in place of its colours)
            v, t, _ = empty_mesh(dev)
            return v, t, None if D is None else torch.zeros((0, D), dtype=torch.float32, device=dev)

        if self.n_units == 0:
            return empty()
        work = self._pool.clone()                                  # (the extraction takes 5 planes: DESIGN.md section 25)
        torch.sub(iso, self._pool[:, 0], out=work[:, 0])
        mesh = marching_cubes(self._grid(), self._slot_map, self.n_units, work)
        del work
        if mesh is None:
            return empty()
        vertices, triangles = mesh[:2]                             # (the pool carries no colour)
        del mesh
        return vertices, triangles, None if values is None else self.query(vertices, values)["values"]


def level_surface_points(field: DensityField, origins: Tensor, dirs: Tensor, t_near: Tensor, t_far: Tensor, levels,
                         values: Optional[Tensor] = None) -> Dict[float, Dict[str, Optional[Tensor]]]:
    """What the reference's ``LevelSetExtractor`` asks of ``model.compute_level_surface_points`` (mesh.py:1110), on the device:
    ``field.raycast``, the hit points ``origins + t dirs`` (a multiply, then an add, in fp32) and one ``field.query(points,
    values)`` per level.  ``{level: {"points" [P,3], "t" [P], "ray_ids" [P] int64, "density", "grad", "dominant", "values"}}``,
    the rays of a level in ascending order.  One host read per level (the number of hits)."""
    name = "level_surface_points"
    if not isinstance(field, DensityField):
        raise ValueError(f"{name}: field must be a DensityField, got {type(field).__name__}")
    _rays(name, origins, dirs, t_near, t_far)
    lv = _levels(name, levels)
    values = _values(name, values, field.n_gauss)
    cast = field.raycast(origins, dirs, t_near, t_far, lv)
    o32, v32 = _prep(origins), _prep(dirs)
    out: Dict[float, Dict[str, Optional[Tensor]]] = {}
    for i, level in enumerate(lv):
        ray_ids = torch.nonzero(cast["hit"][i])[:, 0]
        t = cast["t"][i][ray_ids]
        points = o32[ray_ids] + t[:, None] * v32[ray_ids]
        res = field.query(points, values)
        out[level] = {"points": points, "t": t, "ray_ids": ray_ids, **res}
    return out


def gaussian_density(points: Tensor, means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor,
                     voxel_size: Optional[float] = None, cutoff: float = 3.0, min_opacity: float = 1.0 / 255.0) -> Tensor:
    """``d`` [P] at ``points [P,3]``: a ``DensityField`` over the points' bounding box, queried once.  ``voxel_size`` only sizes the
    units the Gaussians are listed in (16 voxels a side): it changes the cost, not the value beyond the order of the sum's
    roundings.  None: 1/512 of the box's longest side (at most 33 units per axis)."""
    return _at_points("gaussian_density", points, means, quats, scales, opacities, voxel_size, cutoff, min_opacity)["density"]


def gaussian_density_grad(points: Tensor, means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor,
                          voxel_size: Optional[float] = None, cutoff: float = 3.0, min_opacity: float = 1.0 / 255.0) -> Tensor:
    """``grad d`` [P,3] at ``points [P,3]``; see ``gaussian_density``."""
    return _at_points("gaussian_density_grad", points, means, quats, scales, opacities, voxel_size, cutoff, min_opacity)["grad"]


def _at_points(name, points, means, quats, scales, opacities, voxel_size, cutoff, min_opacity) -> Dict[str, Optional[Tensor]]:
    points = _points(name, points)
    _gaussians(name, means, quats, scales, opacities)
    _scalars(name, 1.0 if voxel_size is None else voxel_size, cutoff, min_opacity)
    require_gpu(points, means, quats, scales, opacities)
    P = int(points.shape[0])
    if P == 0:
        return {"density": torch.zeros(0, dtype=torch.float32, device=points.device),
                "grad": torch.zeros((0, 3), dtype=torch.float32, device=points.device)}
    p = points.detach().double()
    fin = torch.isfinite(p).all(1)
    big = torch.full_like(p, float("inf"))
    box = torch.stack([torch.where(fin[:, None], p, big).amin(0), torch.where(fin[:, None], p, -big).amax(0)]).cpu().numpy()
    if not np.all(np.isfinite(box)):
        box = np.zeros((2, 3))                                       # no finite point: every answer is 0
    if voxel_size is None:
        side = float((box[1] - box[0]).max())
        voxel_size = side / 512.0 if side > 0 else 1.0
    field = DensityField(means, quats, scales, opacities, voxel_size, cutoff, min_opacity, bounds=box)
    return field.query(points)


__all__ = ["DensityField", "gaussian_density", "gaussian_density_grad", "level_surface_points", "MAX_CHANNELS", "MAX_LEVELS",
           "MisplatError"]
