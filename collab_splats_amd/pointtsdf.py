"""TSDF fusion of point clouds with origins, with space carving, on the MI355X (csrc/pointtsdf.hip).

``PointTSDFVolume`` restates what the reference's ``TSDFFusion`` (collab_splats/utils/mesh.py:1363-1469) asks of vdbfusion's
``VDBVolume(voxel_size, sdf_trunc, space_carving).integrate(points, origin)``: every point is integrated with the ray from its
origin through it, the ray's voxels take a truncated signed distance with weight 1, and with carving the free space between
origin and surface is integrated too, which is what removes floaters.  The sums are integers (``tsdf / sdf_trunc`` in fixed
point, 2^14), so the volume does not depend on the order of rays, on batching or on how calls are split.  The lattice is this
project's (voxel ``g`` centred at ``(g + 0.5) voxel_size``; vdbfusion centres voxels at ``g voxel_size``), extraction is the
TSDF volume's marching cubes.  Everything stays on the device; there is no CPU fallback.  vdbfusion itself is unpinned.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from ._lib import MisplatError, load, ptr, require_gpu, run
from .depthcloud import _backproject, _cameras, _depth, _flag, _map3
from .meshmap import _prep
from .unitvolume import (MAX_UNITS, UNIT_VOXELS, Grid, GrowingVolume, Stages, _unit_range, empty_mesh, make_grid, marching_cubes,
                         unit_coords, unit_lists)

CHUNK_RAYS = 1 << 20                 # rays per kernel chunk: their (unit, ray) pairs stay far below the sort's 2^31
MAX_PAIRS = (1 << 31) - 4096
MAX_COORD = float(1 << 22)           # voxels from the origin beyond which a ray is skipped (pointtsdf.hip kMaxCoord)
UNIT_BYTES = UNIT_VOXELS * (8 + 4 + 12 + 4)   # sum_q int64, count int32, rgb_sum 3 x int32, rgb_count int32


class PointTSDFVolume(GrowingVolume):
    """A TSDF volume fed with points and their origins.

    ``voxel_size`` / ``sdf_trunc`` / ``space_carving`` as vdbfusion's ``VDBVolume``.  ``bounds`` (optional, ``[[xmin, ymin,
    zmin], [xmax, ymax, zmax]]``): units that do not overlap the box are never allocated and a ray is walked only inside them.
    The dense unit map covers the points (padded by ``sdf_trunc`` and a voxel) and, with carving, the origins; it grows from
    call to call; more than ``max_units`` map entries raise ``MisplatError``.  A unit holds 112 KiB of integer planes."""

    _name, _what, _advice = "PointTSDFVolume", "the points and origins", "pass bounds= or a larger voxel_size"

    def __init__(self, voxel_size: float, sdf_trunc: float, space_carving: bool = True, bounds=None, device=None,
                 max_units: int = MAX_UNITS):
        if not (voxel_size > 0 and sdf_trunc > 0 and np.isfinite(voxel_size) and np.isfinite(sdf_trunc)):
            raise ValueError(f"PointTSDFVolume: voxel_size and sdf_trunc must be finite and positive, got {voxel_size!r} and "
                             f"{sdf_trunc!r}")
        super().__init__(voxel_size, device, max_units)
        self.sdf_trunc, self.space_carving = float(sdf_trunc), bool(space_carving)
        if bounds is not None:
            b = np.asarray(bounds.detach().cpu() if isinstance(bounds, Tensor) else bounds, np.float64)
            if b.shape != (2, 3) or not np.all(np.isfinite(b)) or not np.all(b[1] >= b[0]):
                raise ValueError("PointTSDFVolume: bounds must be finite [[min xyz], [max xyz]] with max >= min")
            self.clip = _unit_range(b[0], b[1], self.ulen)
        self.n_rays = 0                            # rays handed to integrate
        self.n_pairs = 0                           # (unit, ray) pairs so far
        self._sum_q = self._count = self._rgb_sum = self._rgb_count = None

    # ------------------------------------------------------------------------------------------------------------ plumbing
    def _grid(self) -> Grid:
        return make_grid(self.voxel_size, self.sdf_trunc, 1.0, self.lo, self.dims)      # (depth_trunc: unused, positive)

    def _box_units(self, points: Tensor, origins: Tensor) -> Optional[Tuple[np.ndarray, np.ndarray]]:
        """Units overlapping the box of the rays that can take part (one host read); None if there is none."""
        lim = MAX_COORD * self.voxel_size
        o = origins if origins.dim() == 2 else origins[None].expand_as(points)
        ok = (torch.isfinite(points).all(1) & torch.isfinite(o).all(1) & (points.abs() < lim).all(1) & (o.abs() < lim).all(1))
        big = torch.full_like(points, float("inf"))
        pad = self.sdf_trunc + self.voxel_size
        lo_w = torch.where(ok[:, None], points, big).amin(0) - pad
        hi_w = torch.where(ok[:, None], points, -big).amax(0) + pad
        if self.space_carving:
            lo_w = torch.minimum(lo_w, torch.where(ok[:, None], o, big).amin(0) - self.voxel_size)
            hi_w = torch.maximum(hi_w, torch.where(ok[:, None], o, -big).amax(0) + self.voxel_size)
        box = torch.stack([lo_w, hi_w]).double().cpu().numpy()                       # host read
        if not np.all(np.isfinite(box)):
            return None
        return _unit_range(box[0], box[1], self.ulen)

    def _grow_planes(self, n: int) -> None:
        cap = 0 if self._count is None else self._count.shape[0]
        if n <= cap:
            return
        cap = max(n, cap + cap // 2, 64)
        dev = self.device
        new = (torch.zeros((cap, UNIT_VOXELS), dtype=torch.int64, device=dev),
               torch.zeros((cap, UNIT_VOXELS), dtype=torch.int32, device=dev),
               torch.zeros((cap, 3, UNIT_VOXELS), dtype=torch.int32, device=dev),
               torch.zeros((cap, UNIT_VOXELS), dtype=torch.int32, device=dev))
        if self.n_units:
            for dst, src in zip(new, (self._sum_q, self._count, self._rgb_sum, self._rgb_count)):
                dst[:self.n_units] = src[:self.n_units]
        self._sum_q, self._count, self._rgb_sum, self._rgb_count = new

    # -------------------------------------------------------------------------------------------------------------- public
    def integrate(self, points: Tensor, origin: Tensor, colors: Optional[Tensor] = None, _timings: Optional[dict] = None) -> None:
        """Integrate the rays ``origin -> points``.  points [P,3]; origin [3] (one for all) or [P,3]; colors [P,3] in [0,1]
        (colour uint8(rgb * 255)) or None (black).  A point with a non-finite coordinate, at its origin, or beyond 2^22 voxels
        from the world origin is skipped.  Per chunk of 2^20 rays: one host read for the number of (unit, ray) pairs and one
        for the allocation.  Any number of calls; their order and the order of the points do not reach the result."""
        name = "PointTSDFVolume.integrate"
        if not isinstance(points, Tensor) or not points.is_floating_point() or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"{name}: points must be a floating-point tensor [P,3], got "
                             f"{tuple(points.shape) if isinstance(points, Tensor) else type(points).__name__}")
        P = int(points.shape[0])
        if not isinstance(origin, Tensor) or not origin.is_floating_point() or tuple(origin.shape) not in ((3,), (P, 3)):
            raise ValueError(f"{name}: origin must be a floating-point tensor [3] or [{P},3], got "
                             f"{tuple(origin.shape) if isinstance(origin, Tensor) else type(origin).__name__}")
        if colors is not None and (not isinstance(colors, Tensor) or not colors.is_floating_point() or tuple(colors.shape) != (P, 3)):
            raise ValueError(f"{name}: colors must be a floating-point tensor [{P},3] or None, got "
                             f"{tuple(colors.shape) if isinstance(colors, Tensor) else type(colors).__name__}")
        require_gpu(points, origin, colors)
        self._adopt_device(points)
        self.n_rays += P
        if P == 0:
            return
        p32, o32 = _prep(points), _prep(origin)
        c32 = None if colors is None else _prep(colors)
        per_point = o32.dim() == 2
        units = self._box_units(p32, o32)
        if units is None or not self._cover(*units):
            return                                 # no ray takes part, or every one lies outside the bounds
        lib, dev = load(), self.device
        grid = self._grid()
        g = C.byref(grid)
        carve = int(self.space_carving)
        mark = Stages(_timings)
        for c0 in range(0, P, CHUNK_RAYS):
            n = min(CHUNK_RAYS, P - c0)
            p, o = p32[c0:c0 + n], (o32[c0:c0 + n] if per_point else o32)
            col = None if c32 is None else c32[c0:c0 + n]
            stride = 3 if per_point else 0
            ws = torch.empty(int(lib.misplat_ptsdf_workspace(n, 0)), dtype=torch.uint8, device=dev)
            pair_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
            total = torch.empty(1, dtype=torch.int64, device=dev)
            run("misplat_ptsdf_count", g, ptr(p), ptr(o), stride, n, carve, ptr(ws), ws.numel(), ptr(pair_off), ptr(total))
            n_pairs = int(total.item())                                              # host read
            mark("count")
            if n_pairs == 0:
                continue
            if n_pairs >= MAX_PAIRS:
                raise MisplatError(f"{name}: {n_pairs} (unit, ray) pairs in one chunk, above the cap of {MAX_PAIRS}: pass bounds= "
                                   f"or a larger voxel_size")
            keys = torch.empty(n_pairs, dtype=torch.int32, device=dev)
            ids = torch.empty(n_pairs, dtype=torch.int32, device=dev)
            self._begin_batch()
            run("misplat_ptsdf_emit", g, ptr(p), ptr(o), stride, n, carve, ptr(pair_off), n_pairs, ptr(keys), ptr(ids),
                ptr(self._words))
            n_units, n_touched = self._alloc(grid)                                   # host read
            self._grow_planes(n_units)
            self.n_units = n_units
            mark("emit_alloc")
            ids_sorted, ranges = unit_lists(grid, self._slot_map, keys, ids, n_pairs, n_units)
            mark("lists")
            ws = torch.empty(int(lib.misplat_ptsdf_workspace(n_touched, 0)), dtype=torch.uint8, device=dev)
            run("misplat_ptsdf_accumulate", g, ptr(self._touched), n_touched, ptr(p), ptr(o), stride, ptr(col), carve,
                ptr(ids_sorted), ptr(ranges), n_pairs, ptr(ws), ws.numel(), ptr(self._sum_q), ptr(self._count), ptr(self._rgb_sum),
                ptr(self._rgb_count))
            mark("accumulate")
            self.n_pairs += n_pairs
            del keys, ids, ids_sorted, ws

    def integrate_depth(self, depths: Tensor, c2w: Tensor, intrinsics: Tensor, rgbs: Optional[Tensor] = None,
                        masks: Optional[Tensor] = None, _timings: Optional[dict] = None) -> None:
        """Integrate V depth maps as the reference's ``TSDFFusion`` does: EVERY pixel with a finite depth > 0 (and ``masks``
        true, when given) is lifted with ``depthcloud.backproject``'s arithmetic (``get_means3d_backproj``) and integrated
        from its camera's centre ``c2w[:, :, 3]``.  depths [V,H,W(,1)]; c2w [V,3,4] nerfstudio's OpenGL pose; intrinsics [V,4] =
        (fx, fy, cx, cy); rgbs [V,H,W,3] in [0,1] or None (black); masks [V,H,W(,1)] bool or None.  The reference sends a
        masked pixel to the camera centre; here it is no ray at all.  One more host read (the number of pixels)."""
        name = "PointTSDFVolume.integrate_depth"
        shape = _depth(name, depths)
        d = _prep(depths).reshape(shape)
        pose, intr = _cameras(name, c2w, intrinsics, shape[0])
        rgb = None if rgbs is None else _map3(name, "rgbs", rgbs, shape)
        m = _flag(name, "masks", masks, shape)
        require_gpu(depths, c2w, intrinsics, rgbs, masks)
        ok = (d > 0) & torch.isfinite(d)
        if m is not None:
            ok &= m != 0
        at = torch.nonzero(ok.reshape(shape[0], -1))                                 # host read; frame-major, then pixel
        if at.shape[0] == 0:
            return
        f, pix = at[:, 0].to(torch.int32).contiguous(), at[:, 1].to(torch.int32).contiguous()
        # (backproject gathers a colour per point: black stands in without rgbs)
        src = rgb if rgb is not None else torch.zeros(shape + (3,), dtype=torch.float32, device=d.device)
        points, _, colors = _backproject(d, src, None, pose, intr, shape, f, pix)
        self.integrate(points, pose[:, :, 3][f.long()].contiguous(), None if rgb is None else colors, _timings=_timings)

    def _pool(self, min_weight: int) -> Tensor:
        pool = torch.empty((self.n_units, 5, UNIT_VOXELS), dtype=torch.float32, device=self.device)
        run("misplat_ptsdf_finalize", self.n_units, ptr(self._sum_q), ptr(self._count), ptr(self._rgb_sum),
            ptr(self._rgb_count), int(min_weight), ptr(pool))
        return pool

    def extract_mesh(self, min_weight: int = 5) -> Tuple[Tensor, Tensor, Tensor]:
        """``TSDFVolume.extract_mesh``'s contract: (vertices [M,3] fp32, triangles [T,3] int32, colors [M,3] fp32 in [0,1]) on
        the device, in the deterministic order of DESIGN.md section 14.  A cell is extracted when all eight corners were
        updated at least ``min_weight`` times (vdbfusion's ``min_weight``); a vertex takes the mean colour of the rays that
        ended within ``sdf_trunc`` of its two voxels.  The integer planes are not changed: any ``min_weight`` may follow."""
        if not isinstance(min_weight, (int, np.integer)) or isinstance(min_weight, bool) or not 0 <= min_weight < 1 << 31:
            raise ValueError(f"PointTSDFVolume.extract_mesh: min_weight must be an integer in 0..2^31-1, got {min_weight!r}")
        mesh = marching_cubes(self._grid(), self._slot_map, self.n_units, self._pool(int(min_weight))) if self.n_units else None
        return mesh or empty_mesh(self.device)

    def units(self):
        """The allocated units in map order, on the host (for tests and inspection): (coords [n,3] int64, sum_q [n,4096] int64,
        count [n,4096] int64, rgb_sum [n,4096,3] int64, rgb_count [n,4096] int64); voxel i = lx + 16 ly + 256 lz."""
        if self.n_units == 0:
            z = np.zeros((0, UNIT_VOXELS), np.int64)
            return np.zeros((0, 3), np.int64), z, z, np.zeros((0, UNIT_VOXELS, 3), np.int64), z
        m = self._map_order()
        slots = self._slot_map[m].long()
        host = lambda t: t[slots].cpu().numpy().astype(np.int64)                     # noqa: E731
        coords = unit_coords(m.cpu().numpy(), self.lo, self.dims)
        return (coords, host(self._sum_q), host(self._count), np.ascontiguousarray(host(self._rgb_sum).transpose(0, 2, 1)),
                host(self._rgb_count))


__all__ = ["PointTSDFVolume", "CHUNK_RAYS", "MAX_UNITS", "UNIT_BYTES", "MisplatError"]
