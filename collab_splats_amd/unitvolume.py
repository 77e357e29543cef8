"""The sparse unit volume under TSDF fusion of depth maps and of point clouds, the density field and Poisson reconstruction
(csrc/unitgrid.h): units of 16^3 voxels, a dense unit map ``slot_map`` over ``lo .. lo + dims - 1`` (x
fastest, -1 = unallocated), a pool ``[slot, 5, 4096]`` fp32 (tsdf, weight, r, g, b; voxel i = lx + 16 ly + 256 lz), and the
marching cubes of csrc/tsdf.hip over it.  ``GrowingVolume``: the map that grows from call to call (``TSDFVolume``,
``PointTSDFVolume``).  ``alloc_units`` / ``unit_lists``: the host side of the list layer (csrc/unitlists.h).
"""
from __future__ import annotations

import ctypes as C
import time
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from ._lib import MisplatError, load, ptr, run

UNIT = 16
UNIT_VOXELS = UNIT ** 3
MAX_UNITS = 1 << 26                  # dense unit map cap (include/misplat.h MISPLAT_TSDF_MAX_UNITS)
MAX_COORD = 1 << 19                  # units per axis either side of the origin: voxel coordinates stay exact in fp32


class Grid(C.Structure):
    """Mirror of ``misplat_tsdf_grid`` (include/misplat.h)."""
    _fields_ = [("voxel_size", C.c_float), ("sdf_trunc", C.c_float), ("depth_trunc", C.c_float),
                ("lo", C.c_int32 * 3), ("dims", C.c_int32 * 3), ("reserved", C.c_int32)]


def make_grid(voxel_size: float, sdf_trunc: float, depth_trunc: float, lo, dims) -> Grid:
    int3 = C.c_int32 * 3
    return Grid(voxel_size, sdf_trunc, depth_trunc, int3(*(int(x) for x in lo)), int3(*(int(x) for x in dims)))


def _unit_range(lo_world, hi_world, ulen: float) -> Tuple[np.ndarray, np.ndarray]:
    """Inclusive unit-coordinate range of the units overlapping the world box [lo, hi]."""
    lo = np.floor(np.asarray(lo_world, np.float64) / ulen).astype(np.int64)
    hi = np.floor(np.asarray(hi_world, np.float64) / ulen).astype(np.int64)
    return lo, hi


def map_span(name: str, what: str, lo: np.ndarray, hi: np.ndarray, max_units: int, advice: str) -> Tuple[np.ndarray, int]:
    """(dims, entries) of the unit map over units lo..hi (inclusive); ``MisplatError`` (``name``: ``what`` ...: ``advice``) beyond
    the lattice's 2^19 units per axis or above ``max_units`` entries."""
    if np.any(np.abs(lo) >= MAX_COORD) or np.any(np.abs(hi) >= MAX_COORD - 1):
        raise MisplatError(f"{name}: {what} reach unit {max(np.abs(lo).max(), np.abs(hi).max())}, beyond the lattice's "
                           f"2^19 units per axis: {advice}")
    dims = hi - lo + 1
    n_map = int(np.prod(dims.astype(object)))
    if n_map > max_units:
        raise MisplatError(f"{name}: {what} span {n_map} units of {UNIT}^3 voxels, above the cap of {max_units}: {advice}")
    return dims.astype(np.int64), n_map


def unit_coords(m: np.ndarray, lo: np.ndarray, dims: np.ndarray) -> np.ndarray:
    """[n,3] int64 unit coordinates of the map indices ``m``."""
    nx, ny = int(dims[0]), int(dims[1])
    return np.stack([m % nx, (m // nx) % ny, m // (nx * ny)], 1) + lo[None, :]


def empty_mesh(device) -> Tuple[Tensor, Tensor, Tensor]:
    """(vertices [0,3] fp32, triangles [0,3] int32, colors [0,3] fp32): what an extraction without a crossed edge returns."""
    return (torch.zeros((0, 3), dtype=torch.float32, device=device), torch.zeros((0, 3), dtype=torch.int32, device=device),
            torch.zeros((0, 3), dtype=torch.float32, device=device))


def map_order(slot_map: Tensor) -> Tensor:
    """The map indices of the allocated units, ascending (int64, on the device)."""
    return torch.nonzero(slot_map >= 0).squeeze(1)


def alloc_units(grid: Grid, words: Tensor, slot_map: Tensor, counters: Tensor, touched: Tensor) -> Tuple[int, int]:
    """``misplat_tsdf_alloc`` over the marked ``words`` and its one host read: (allocated units so far, units touched now).
    ``counters`` {allocated slots, touched units}: the second zeroed by the caller."""
    run("misplat_tsdf_alloc", C.byref(grid), ptr(words), ptr(slot_map), ptr(counters), ptr(touched))
    n_units, n_touched = (int(x) for x in counters.tolist())                     # host read
    return n_units, n_touched


def unit_lists(grid: Grid, slot_map: Tensor, keys: Tensor, ids: Tensor, n_pairs: int, n_units: int) -> Tuple[Tensor, Tensor]:
    """The (unit map index, item) pairs sorted by unit, stable (``misplat_unit_lists``; ``keys`` and ``ids`` are used as
    scratch): (ids_sorted [n_pairs] int32, ranges [n_units, 2] int32), unit slot s owning ``ids_sorted[ranges[s, 0]:ranges[s,
    1]]``.  ``ranges`` starts as zeros: a unit allocated earlier and not listed now reads as the empty range."""
    dev = slot_map.device
    ws = torch.empty(int(load().misplat_density_workspace(0, n_pairs)), dtype=torch.uint8, device=dev)
    keys_sorted = torch.empty(n_pairs, dtype=torch.int32, device=dev)
    ids_sorted = torch.empty(n_pairs, dtype=torch.int32, device=dev)
    ranges = torch.zeros((n_units, 2), dtype=torch.int32, device=dev)
    run("misplat_unit_lists", C.byref(grid), ptr(slot_map), ptr(keys), ptr(ids), n_pairs, n_units, ptr(ws), ws.numel(),
        ptr(keys_sorted), ptr(ids_sorted), ptr(ranges))
    return ids_sorted, ranges


class Stages:
    """Seconds per stage added into a dict, each stage synchronised (scripts/density_bench.py, scripts/pointtsdf_bench.py);
    nothing at all without a dict."""

    def __init__(self, out: Optional[dict]):
        self.out = out
        if out is not None:
            torch.cuda.synchronize()
            self.t = time.perf_counter()

    def __call__(self, stage: str) -> None:
        if self.out is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            self.out[stage] = self.out.get(stage, 0.0) + (now - self.t)
            self.t = now


class GrowingVolume:
    """What ``TSDFVolume`` and ``PointTSDFVolume`` share: a unit map that grows to cover each call's units (clipped to the
    optional bounds ``clip``, a unit range), the batch's words and touched list, and the allocation counters.  A subclass
    sets ``_name``, ``_what`` and ``_advice`` (``map_span``'s error text), checks its own ``bounds`` and sets ``clip``."""

    _name = _what = _advice = ""

    def __init__(self, voxel_size: float, device, max_units: int):
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        if self.device.type != "cuda":
            raise MisplatError(f"{self._name} runs on the MI355X only: there is no CPU fallback")
        self.voxel_size = float(voxel_size)
        self.ulen = float(np.float32(self.voxel_size) * np.float32(UNIT))
        self.max_units = min(int(max_units), MAX_UNITS)
        self.clip = None                           # (lo, hi) unit range of the bounds
        self.lo = self.dims = None                 # unit map (none before the first integrate)
        self.n_units = 0                           # allocated units (= slots in use)
        self._slot_map = self._words = self._touched = None
        self._counters = None                      # device {allocated slots, touched units of the batch}

    def _cover(self, lo: np.ndarray, hi: np.ndarray) -> bool:
        """Make the unit map cover units lo..hi (inclusive, clipped to the bounds); False if there is no map."""
        if self.clip is not None:
            lo, hi = np.maximum(lo, self.clip[0]), np.minimum(hi, self.clip[1])
        if np.any(hi < lo):
            return self.lo is not None
        if self.lo is not None:
            old_hi = self.lo + self.dims - 1
            if np.all(lo >= self.lo) and np.all(hi <= old_hi):
                return True
            lo, hi = np.minimum(lo, self.lo), np.maximum(hi, old_hi)
        dims, n = map_span(self._name, self._what, lo, hi, self.max_units, self._advice)
        slot_map = torch.full((n,), -1, dtype=torch.int32, device=self.device)
        if self.n_units:                           # re-linearise the allocated units into the grown map
            m = self._map_order()
            nx, ny = int(self.dims[0]), int(self.dims[1])
            cx, cy, cz = m % nx, (m // nx) % ny, m // (nx * ny)
            o = self.lo - lo
            lin = (cx + int(o[0])) + int(dims[0]) * ((cy + int(o[1])) + int(dims[1]) * (cz + int(o[2])))
            slot_map[lin] = self._slot_map[m]
        self.lo, self.dims = lo.astype(np.int64), dims.astype(np.int64)
        self._slot_map = slot_map
        self._words = torch.zeros(n, dtype=torch.int64, device=self.device)
        self._touched = torch.empty(2 * n, dtype=torch.int32, device=self.device)
        return True

    def _begin_batch(self) -> None:
        """Zero the words and the touched count: the subclass's mark or emit launch sets the words next, then ``_alloc``."""
        if self._counters is None:
            self._counters = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._words.zero_()
        self._counters[1:].zero_()

    def _alloc(self, grid: Grid) -> Tuple[int, int]:
        """Slots for the batch's marked units: (allocated units so far, units touched by the batch); the batch's one host
        read."""
        return alloc_units(grid, self._words, self._slot_map, self._counters, self._touched)

    def _adopt_device(self, tensor: Tensor) -> None:
        """The first tensors name the device of a volume made without an index; later ones must lie on it."""
        if tensor.device != self.device and self.device.index is not None:
            raise MisplatError(f"{self._name} on {self.device} got tensors on {tensor.device}")
        if self.device.index is None:
            self.device = tensor.device

    def _map_order(self) -> Tensor:
        return map_order(self._slot_map)


def marching_cubes(grid: Grid, slot_map: Tensor, n_units: int, pool: Tensor, order: Optional[Tensor] = None
                   ) -> Optional[Tuple[Tensor, Tensor, Tensor]]:
    """(vertices [M,3] fp32 in lattice coordinates times ``grid.voxel_size``, triangles [T,3] int32, colors [M,3] fp32 in [0,1])
    of the ``n_units`` allocated units, in the deterministic order of DESIGN.md section 14.1, or None when no edge is crossed.
    ``order``: the allocated units' map indices, ascending (``misplat_tsdf_order`` finds them when None).  One host read."""
    dev, n, g = pool.device, n_units, C.byref(grid)
    if order is None:
        nb = (grid.dims[0] * grid.dims[1] * grid.dims[2] + 4095) // 4096
        scratch = torch.empty(2 * nb + 1, dtype=torch.int32, device=dev)
        order = torch.empty(n, dtype=torch.int32, device=dev)
        run("misplat_tsdf_order", g, ptr(slot_map), ptr(scratch), ptr(order))
    code = torch.empty(n * UNIT_VOXELS, dtype=torch.int16, device=dev)
    cnt = torch.empty(n * UNIT_VOXELS, dtype=torch.uint8, device=dev)
    unit_counts = torch.empty(2 * n, dtype=torch.int32, device=dev)
    unit_offs = torch.empty(2 * n, dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    run("misplat_tsdf_mc_count", g, ptr(slot_map), ptr(order), n, ptr(pool), ptr(code), ptr(cnt), ptr(unit_counts),
        ptr(unit_offs), ptr(totals))
    M, T = (int(x) for x in totals.tolist())                        # host read
    if M == 0:
        return None
    vert_base = torch.empty(n * UNIT_VOXELS, dtype=torch.int32, device=dev)
    vertices = torch.empty((M, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((M, 3), dtype=torch.float32, device=dev)
    triangles = torch.empty((T, 3), dtype=torch.int32, device=dev)
    run("misplat_tsdf_mc_emit", g, ptr(slot_map), ptr(order), n, ptr(pool), ptr(code), ptr(cnt), ptr(unit_offs), ptr(vert_base),
        ptr(vertices), ptr(colors), ptr(triangles))
    return vertices, triangles, colors
