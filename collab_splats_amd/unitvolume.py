"""The sparse unit volume under TSDF fusion, the density field and Poisson reconstruction (csrc/unitgrid.h, DESIGN.md section
14.5): units of 16^3 voxels, a dense unit map ``slot_map`` over ``lo .. lo + dims - 1`` (x fastest, -1 = unallocated), a pool
``[slot, 5, 4096]`` fp32 (tsdf, weight, r, g, b; voxel i = lx + 16 ly + 256 lz), and the marching cubes of csrc/tsdf.hip over it.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from ._lib import MisplatError, check, load, ptr, stream_ptr

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


def marching_cubes(grid: Grid, slot_map: Tensor, n_units: int, pool: Tensor, order: Optional[Tensor] = None
                   ) -> Optional[Tuple[Tensor, Tensor, Tensor]]:
    """(vertices [M,3] fp32 in lattice coordinates times ``grid.voxel_size``, triangles [T,3] int32, colors [M,3] fp32 in [0,1])
    of the ``n_units`` allocated units, in the deterministic order of DESIGN.md section 14.1, or None when no edge is crossed.
    ``order``: the allocated units' map indices, ascending (``misplat_tsdf_order`` finds them when None).  One host read."""
    lib, dev, n, g = load(), pool.device, n_units, C.byref(grid)
    if order is None:
        nb = (grid.dims[0] * grid.dims[1] * grid.dims[2] + 4095) // 4096
        scratch = torch.empty(2 * nb + 1, dtype=torch.int32, device=dev)
        order = torch.empty(n, dtype=torch.int32, device=dev)
        check(lib.misplat_tsdf_order(g, ptr(slot_map), ptr(scratch), ptr(order), stream_ptr()), "misplat_tsdf_order")
    code = torch.empty(n * UNIT_VOXELS, dtype=torch.int16, device=dev)
    cnt = torch.empty(n * UNIT_VOXELS, dtype=torch.uint8, device=dev)
    unit_counts = torch.empty(2 * n, dtype=torch.int32, device=dev)
    unit_offs = torch.empty(2 * n, dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    check(lib.misplat_tsdf_mc_count(g, ptr(slot_map), ptr(order), n, ptr(pool), ptr(code), ptr(cnt), ptr(unit_counts),
                                    ptr(unit_offs), ptr(totals), stream_ptr()), "misplat_tsdf_mc_count")
    M, T = (int(x) for x in totals.tolist())                        # host read
    if M == 0:
        return None
    vert_base = torch.empty(n * UNIT_VOXELS, dtype=torch.int32, device=dev)
    vertices = torch.empty((M, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((M, 3), dtype=torch.float32, device=dev)
    triangles = torch.empty((T, 3), dtype=torch.int32, device=dev)
    check(lib.misplat_tsdf_mc_emit(g, ptr(slot_map), ptr(order), n, ptr(pool), ptr(code), ptr(cnt), ptr(unit_offs),
                                   ptr(vert_base), ptr(vertices), ptr(colors), ptr(triangles), stream_ptr()),
          "misplat_tsdf_mc_emit")
    return vertices, triangles, colors
