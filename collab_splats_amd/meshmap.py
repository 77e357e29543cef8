"""kNN mapping of per-Gaussian values onto mesh vertices on the MI355X (csrc/meshmap.hip).

``features2vertex`` / ``normals2vertex`` restate the reference's maps of the same names (what ``Open3DTSDFFusion.main`` runs
after the mesh is extracted, collab_splats/utils/mesh.py:1661-1702) in fp32: every point takes its k nearest vertices;
a point whose nearest vertex is further than ``sdf_trunc`` contributes nothing; the others spread their value over their k
vertices with Gaussian weights of the distance (sigma = the mean distance of the valid rows), normalised per row; a vertex
holds the weighted mean of what it received (0 if nothing).  Everything stays on the device; there is no CPU fallback.
"""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor

from ._lib import MisplatError, load, ptr, require_gpu, run

MAX_K = 16
COORD_CELLS = 2.0 ** 18              # every vertex: |x| / sdf_trunc < 2^18 per axis (csrc/meshmap.hip kCoordCells)


def _check(name: str, mesh_vertices: Tensor, points: Tensor, values, k: int, sdf_trunc: float):
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise ValueError(f"{name}: k must be an integer in 1..{MAX_K}, got {k!r}")
    if not sdf_trunc > 0:
        raise ValueError(f"{name}: sdf_trunc must be positive, got {sdf_trunc!r}")
    if mesh_vertices.dim() != 2 or mesh_vertices.shape[1] != 3:
        raise ValueError(f"{name}: mesh_vertices must be [M,3], got {tuple(mesh_vertices.shape)}")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{name}: points must be [N,3], got {tuple(points.shape)}")
    if values is not None and (values.dim() != 2 or values.shape[0] != points.shape[0] or values.shape[1] < 1):
        raise ValueError(f"{name}: values must be [N,D] with N = {points.shape[0]} and D >= 1, got {tuple(values.shape)}")
    M = mesh_vertices.shape[0]
    if M < k:
        raise ValueError(f"{name}: {M} mesh vertices, fewer than k = {k}")
    require_gpu(mesh_vertices, points, values)


def _workspace(M: int, N: int, k: int, D: int, device) -> Tensor:
    n = int(load().misplat_meshmap_workspace(M, N, k, D))
    if n < 0:
        raise ValueError(f"meshmap: sizes M={M}, N={N}, k={k}, D={D} are beyond the library's limits")
    return torch.empty(n, dtype=torch.uint8, device=device)


def _knn_ws(vertices: Tensor, points: Tensor, k: int, sdf_trunc: float, ws: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    M, N = vertices.shape[0], points.shape[0]
    dev = vertices.device
    bad = (~torch.isfinite(vertices)).any() | ((vertices.abs() * (1.0 / float(sdf_trunc))) >= COORD_CELLS).any()
    if bool(bad):                                               # the call's one host read
        raise ValueError("meshmap: mesh vertices must be finite and within 2^18 sdf_trunc of the origin on every axis")
    idx = torch.empty((N, k), dtype=torch.int32, device=dev)
    dist = torch.empty((N, k), dtype=torch.float32, device=dev)
    valid = torch.empty(N, dtype=torch.uint8, device=dev)
    run("misplat_meshmap_knn", ptr(vertices), M, ptr(points), N, k, sdf_trunc, ptr(ws), ws.numel(), ptr(idx), ptr(dist),
        ptr(valid))
    return idx, dist, valid


def _prep(x: Tensor) -> Tensor:
    return x.detach().to(torch.float32).contiguous()


def _knn(mesh_vertices: Tensor, points: Tensor, k: int = 5, sdf_trunc: float = 0.03) -> Tuple[Tensor, Tensor, Tensor]:
    """k nearest vertices of every point: (idx [N,k] int32, d [N,k] fp32 ascending by (d, index), valid [N] bool).  An
    invalid row (nearest vertex further than sdf_trunc) holds idx -1 and d +inf."""
    _check("meshmap._knn", mesh_vertices, points, None, k, sdf_trunc)
    v, p = _prep(mesh_vertices), _prep(points)
    ws = _workspace(v.shape[0], p.shape[0], k, 1, v.device)
    idx, dist, valid = _knn_ws(v, p, k, sdf_trunc, ws)
    return idx, dist, valid.bool()


def _aggregate(M: int, idx: Tensor, dist: Tensor, valid: Tensor, values: Tensor, n_unit: int, ws: Tensor) -> Tensor:
    N, k = idx.shape
    D = values.shape[1]
    out = torch.empty((M, D), dtype=torch.float32, device=values.device)
    run("misplat_meshmap_aggregate", M, N, k, ptr(idx), ptr(dist), ptr(valid), ptr(values), D, n_unit, ptr(ws), ws.numel(),
        ptr(out))
    return out


def map_to_vertices(mesh_vertices: Tensor, points: Tensor, values: Tensor, k: int = 5, sdf_trunc: float = 0.03,
                    n_unit: int = 0) -> Tensor:
    """The map of ``values`` [N,D] onto the vertices, [M,D] fp32 on the device; with ``n_unit`` = 3 the first three channels
    are then divided by (their norm + 1e-8).  One kNN for all D channels: each channel equals a call with it alone."""
    _check("map_to_vertices", mesh_vertices, points, values, k, sdf_trunc)
    if n_unit not in (0, 3) or values.shape[1] < n_unit:
        raise ValueError("map_to_vertices: n_unit must be 0 or 3 (with at least 3 channels)")
    v, p, f = _prep(mesh_vertices), _prep(points), _prep(values)
    M, N, D = v.shape[0], p.shape[0], f.shape[1]
    ws = _workspace(M, N, k, D, v.device)
    if N == 0:
        idx = torch.empty((0, k), dtype=torch.int32, device=v.device)
        return _aggregate(M, idx, idx.float(), idx[:, 0].to(torch.uint8), f, n_unit, ws)
    idx, dist, valid = _knn_ws(v, p, k, sdf_trunc, ws)
    return _aggregate(M, idx, dist, valid, f, n_unit, ws)


def features2vertex(mesh_vertices: Tensor, points: Tensor, features: Tensor, k: int = 5, sdf_trunc: float = 0.03) -> Tensor:
    """Weighted mean of the per-point ``features`` [N,D] over the points that take each vertex among their k nearest:
    [M,D] fp32 on the device (``x.double().cpu()`` is the reference's float64 CPU result)."""
    return map_to_vertices(mesh_vertices, points, features, k, sdf_trunc)


def normals2vertex(mesh_vertices: Tensor, points: Tensor, normals: Tensor, k: int = 5, sdf_trunc: float = 0.03) -> Tensor:
    """``features2vertex`` of the per-point ``normals`` [N,3], divided by (norm + 1e-8): [M,3] fp32 on the device."""
    if normals.dim() != 2 or normals.shape[1] != 3:
        raise ValueError(f"normals2vertex: normals must be [N,3], got {tuple(normals.shape)}")
    return map_to_vertices(mesh_vertices, points, normals, k, sdf_trunc, n_unit=3)


__all__ = ["features2vertex", "normals2vertex", "map_to_vertices", "MisplatError"]
