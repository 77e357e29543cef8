"""Point-cloud cleaning on the MI355X (csrc/pointcloud.hip).

The reference cleans point clouds through Open3D and scipy (collab_splats/utils/pointcloud.py ``clean_pcd``,
``remove_far_points``, ``density_filter``; the Poisson exporters' ``voxel_down_sample`` + ``remove_statistical_outlier``,
collab_splats/utils/mesh.py:798-805, 1014, 1171; ``calculate_accuracy`` / ``calculate_completeness``,
collab_splats/utils/utils.py:43-60).  Here the same stages run on [N,3] device tensors: an exact k-nearest mean distance with
no distance cut-off, the statistical-outlier rule, radius counts and the voxel reduction are HIP kernels; the rest is thin
torch on the device.  There is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from ._lib import MisplatError, load, ptr, require_gpu, run
from .meshmap import COORD_CELLS, _prep

MAX_K = 32
VOXEL_CELLS = 2.0 ** 20              # |cell| < 2^20 per axis (csrc/pointcloud.hip voxel_cell)

# Tuning values of the kNN; neither changes a result (tests/test_pointcloud_gpu.py forces others).
CELL_EDGE: Optional[float] = None    # edge of the finest hash level; None: from the occupancy measure (_auto_edge)
LANES_PER_QUERY = 8                  # 1 or 8 lanes per query (DESIGN.md section 17.3 holds the measurement)
OCCUPANCY_PER_K = 1.0                # _auto_edge aims at this many points per occupied cell, times k

_CELLS, _KNN, _RADIUS, _OUTLIER, _VOXEL = range(5)


# ---------------------------------------------------------------------------------------------------------- helpers
def _cloud(name: str, what: str, x: Tensor) -> None:
    if not isinstance(x, Tensor) or x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{name}: {what} must be [N,3], got {tuple(x.shape) if isinstance(x, Tensor) else type(x).__name__}")


def _positive(name: str, what: str, v) -> float:
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: {what} must be a positive finite number, got {v!r}") from None
    if not (f > 0 and math.isfinite(f)):
        raise ValueError(f"{name}: {what} must be positive and finite, got {v!r}")
    return f


def _positive32(name: str, what: str, v) -> float:
    f = _positive(name, what, v)
    f32 = torch.tensor(f, dtype=torch.float32)
    if not (bool(torch.isfinite(f32)) and bool(torch.isfinite(1.0 / f32)) and float(f32) > 0):
        raise ValueError(f"{name}: {what} must be positive and finite in fp32 (and so must its inverse), got {v!r}")
    return float(f32)


def _finite(name: str, *clouds: Tensor) -> None:
    bad = None
    for x in clouds:
        if x is not None and x.numel():
            b = (~torch.isfinite(x)).any()
            bad = b if bad is None else bad | b
    if bad is not None and bool(bad):
        raise ValueError(f"{name}: points must be finite")


def _workspace(n: int, kind: int, device) -> Tensor:
    b = int(load().misplat_pointcloud_workspace(n, kind))
    if b < 0:
        raise ValueError(f"pointcloud: {n} points are beyond the library's limits")
    return torch.empty(b, dtype=torch.uint8, device=device)


def _occupied_cells(p: Tensor, edge: float, ws: Tensor) -> int:
    out = torch.empty(1, dtype=torch.int32, device=p.device)
    run("misplat_pointcloud_cells", ptr(p), p.shape[0], edge, ptr(ws), ws.numel(), ptr(out))
    return int(out.item())


def _auto_edge(p: Tensor, k: int, floor: float, extent: Sequence[float], ws: Tensor) -> float:
    """The edge at which an occupied cell holds about OCCUPANCY_PER_K k points: start from the bounding box as if it were
    filled, measure the occupied cells on the device, rescale as for a surface (occupancy ~ edge^2), at most four times."""
    n = p.shape[0]
    want = max(1.0, OCCUPANCY_PER_K * k)
    dims = [e for e in extent if e > 0]
    h = (math.prod(dims) * want / n) ** (1.0 / len(dims)) if dims else 1.0
    h = min(max(h, floor, 1e-30), 1e30)
    for _ in range(4):
        occ = n / max(1, _occupied_cells(p, h, ws))                # one host read
        if 0.5 * want <= occ <= 2.0 * want or (occ < want and n <= want):
            break
        nxt = min(max(h * min(max(math.sqrt(want / occ), 0.25), 4.0), floor, 1e-30), 1e30)
        if nxt == h:
            break
        h = nxt
    return h


# -------------------------------------------------------------------------------------------------------------- kNN
def knn_mean_distance(points: Tensor, k: int, queries: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(mean [Nq] fp32, nearest [Nq] fp32): per query the k_eff = min(k, N) smallest d2 = ((dx dx + dy dy) + dz dz) (fp32)
    among ALL points, no distance cut-off; mean = the fp32 sum of sqrtf(d2) in ascending order / float(k_eff), nearest = sqrtf
    of the smallest.  ``queries`` None: the points query themselves and each counts among its own neighbours, at distance 0
    (Open3D's SearchKNN).  Exact; two runs are bitwise equal; the tuning values of this module change no result."""
    name = "knn_mean_distance"
    _cloud(name, "points", points)
    if queries is not None:
        _cloud(name, "queries", queries)
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise ValueError(f"{name}: k must be an integer in 1..{MAX_K}, got {k!r}")
    if LANES_PER_QUERY not in (1, 8):
        raise ValueError(f"{name}: pointcloud.LANES_PER_QUERY must be 1 or 8, got {LANES_PER_QUERY!r}")
    forced = None if CELL_EDGE is None else _positive32(name, "pointcloud.CELL_EDGE", CELL_EDGE)
    p = _prep(points)
    q = None if queries is None else _prep(queries)
    n, nq = p.shape[0], (p.shape[0] if q is None else q.shape[0])
    if n == 0 and nq > 0:
        raise ValueError(f"{name}: {nq} queries against an empty cloud")
    if nq == 0:
        _finite(name, p)
        require_gpu(points, queries)
        return torch.empty(0, dtype=torch.float32, device=p.device), torch.empty(0, dtype=torch.float32, device=p.device)
    if q is not None and q.device != p.device:
        require_gpu(points, queries)
    both = p if q is None else torch.cat([p, q])
    lo, hi = p.amin(0), p.amax(0)
    head = torch.cat([(~torch.isfinite(both)).any().to(torch.float32)[None], both.abs().amax()[None], hi - lo]).tolist()   # host read
    if head[0] != 0 or not all(math.isfinite(v) for v in head[1:]):
        raise ValueError(f"{name}: points must be finite (and their extent must be finite in fp32)")
    if head[1] >= 1e30:
        raise ValueError(f"{name}: coordinates of magnitude {head[1]:.3g} are beyond the index's range (|x| < 1e30)")
    require_gpu(points, queries)
    mean = torch.empty(nq, dtype=torch.float32, device=p.device)
    nearest = torch.empty(nq, dtype=torch.float32, device=p.device)
    floor = head[1] / 2.0 ** 17                                     # every |x| / edge stays below 2^18 (cellhash.h)
    ws = _workspace(n, _KNN, p.device)
    if forced is not None:
        edge = max(forced, floor)
    else:
        edge = _auto_edge(p, min(k, n), floor, head[2:], ws)
    run("misplat_pointcloud_knn", ptr(p), n, ptr(q), nq, min(k, n), edge, LANES_PER_QUERY, ptr(ws), ws.numel(), ptr(mean),
        ptr(nearest))
    return mean, nearest


# ---------------------------------------------------------------------------------------------- statistical outliers
def statistical_outlier_mask(points: Tensor, nb_neighbors: int = 20, std_ratio: float = 2.0) -> Tuple[Tensor, Tensor]:
    """(keep [N] bool, mean [N] fp32): Open3D's remove_statistical_outlier.  avg_i = the mean distance to the nb_neighbors
    nearest points, the point itself included; a point is valid iff avg_i > 0; mu and sigma (n_valid - 1 in the denominator)
    over the valid avg in fp64; keep iff avg_i > 0 and double(avg_i) < mu + std_ratio sigma.  With fewer than two valid points
    there is no threshold: keep = avg > 0 (Open3D's threshold is NaN there)."""
    name = "statistical_outlier_mask"
    _cloud(name, "points", points)
    if not isinstance(nb_neighbors, int) or isinstance(nb_neighbors, bool) or not 1 <= nb_neighbors <= MAX_K:
        raise ValueError(f"{name}: nb_neighbors must be an integer in 1..{MAX_K}, got {nb_neighbors!r}")
    try:
        ratio = float(std_ratio)
    except (TypeError, ValueError):
        ratio = math.nan
    if not math.isfinite(ratio):
        raise ValueError(f"{name}: std_ratio must be a finite number, got {std_ratio!r}")
    _finite(name, points)
    require_gpu(points)
    n = points.shape[0]
    if n == 0:
        return (torch.zeros(0, dtype=torch.bool, device=points.device), torch.zeros(0, dtype=torch.float32, device=points.device))
    mean, _ = knn_mean_distance(points, nb_neighbors)
    keep = torch.empty(n, dtype=torch.uint8, device=mean.device)
    ws = _workspace(n, _OUTLIER, mean.device)
    run("misplat_pointcloud_outlier_mask", ptr(mean), n, ratio, ptr(ws), ws.numel(), ptr(keep))
    return keep.bool(), mean


def remove_statistical_outlier(points: Tensor, nb_neighbors: int = 20, std_ratio: float = 2.0) -> Tuple[Tensor, Tensor]:
    """Open3D's shape of ``statistical_outlier_mask``: (points[ind], ind int64 ascending)."""
    keep, _ = statistical_outlier_mask(points, nb_neighbors, std_ratio)
    ind = torch.nonzero(keep)[:, 0]
    return points[ind], ind


# ----------------------------------------------------------------------------------------------------- radius count
def radius_count(points: Tensor, radius: float, queries: Optional[Tensor] = None) -> Tensor:
    """[Nq] int32: the number of points with d2 < r2, d2 = ((dx dx + dy dy) + dz dz) and r2 = r r in fp32, r =
    float32(radius): strict, as ``cluster_labels``.  ``queries`` None: the points themselves, each counting itself."""
    name = "radius_count"
    _cloud(name, "points", points)
    if queries is not None:
        _cloud(name, "queries", queries)
    r = _positive32(name, "radius", radius)
    p = _prep(points)
    q = None if queries is None else _prep(queries)
    n, nq = p.shape[0], (p.shape[0] if q is None else q.shape[0])
    if n:
        bad = (~torch.isfinite(p)).any() | ((p.abs() * (1.0 / r)) >= COORD_CELLS).any()
        if q is not None and nq:
            bad = bad | (~torch.isfinite(q)).any()
        if bool(bad):                                               # the call's host read
            raise ValueError(f"{name}: points must be finite and within 2^18 radius of the origin on every axis")
    else:
        _finite(name, q)
    require_gpu(points, queries)
    counts = torch.zeros(nq, dtype=torch.int32, device=p.device)
    if n == 0 or nq == 0:
        return counts
    ws = _workspace(n, _RADIUS, p.device)
    run("misplat_pointcloud_radius_count", ptr(p), n, ptr(q), nq, r, ptr(ws), ws.numel(), ptr(counts))
    return counts


def _percentile(sorted_values: Tensor, percentile: float) -> float:
    """numpy.percentile's default (linear) rule in fp64 on an ascending device tensor: two elements are read."""
    n = sorted_values.shape[0]
    pos = (n - 1) * (percentile / 100.0)
    lo = min(max(int(math.floor(pos)), 0), n - 1)
    hi = min(lo + 1, n - 1)
    a, b = (float(v) for v in sorted_values[[lo, hi]].to(torch.float64).tolist())
    t = pos - lo
    return b - (b - a) * (1.0 - t) if t >= 0.5 else a + (b - a) * t


def _check_percentile(name: str, percentile) -> float:
    try:
        f = float(percentile)
    except (TypeError, ValueError):
        f = math.nan
    if not 0.0 <= f <= 100.0:
        raise ValueError(f"{name}: percentile must be in 0..100, got {percentile!r}")
    return f


def density_filter(points: Tensor, radius: float = 0.03, percentile: float = 10) -> Tuple[Tensor, Tensor]:
    """The reference's ``density_filter``: keep the points whose ``radius_count`` is >= numpy.percentile(counts, percentile)
    (linear interpolation, fp64).  Returns (points[ind], ind int64 ascending)."""
    pct = _check_percentile("density_filter", percentile)
    counts = radius_count(points, radius)
    if counts.shape[0] == 0:
        ind = torch.zeros(0, dtype=torch.int64, device=points.device)
        return points[ind], ind
    thr = _percentile(torch.sort(counts).values, pct)
    ind = torch.nonzero(counts.to(torch.float64) >= thr)[:, 0]
    return points[ind], ind


# ------------------------------------------------------------------------------------------------------------ voxel
def voxel_down_sample(points: Tensor, voxel_size: float, attributes: Sequence[Tensor] = (),
                      min_bound: Optional[Sequence[float]] = None) -> Tuple[Tensor, Tuple[Tensor, ...], Tensor, Tensor]:
    """Open3D's voxel_down_sample: origin = min_bound - voxel_size / 2 (``min_bound`` defaults to the per-axis minimum), cell
    = floor((p - origin) / voxel_size), all in fp64; an output point, and a row of each of ``attributes`` ([N,D] fp32), is
    the mean over the cell's members: summed in fp64 in ascending point index, the quotient rounded to fp32.  Voxels are
    numbered in ascending order of their smallest member.  Returns (points [V,3], attributes (a tuple of [V,D]), first_index
    [V] int64: that smallest member, counts [V] int32)."""
    name = "voxel_down_sample"
    _cloud(name, "points", points)
    vs = _positive(name, "voxel_size", voxel_size)
    attributes = tuple(attributes)
    n = points.shape[0]
    for a in attributes:
        if not isinstance(a, Tensor) or a.dim() != 2 or a.shape[0] != n or a.shape[1] < 1:
            raise ValueError(f"{name}: every attribute must be [N,D] with N = {n} and D >= 1, got "
                             f"{tuple(a.shape) if isinstance(a, Tensor) else type(a).__name__}")
    if min_bound is not None:
        mb = [float(v) for v in (min_bound.tolist() if isinstance(min_bound, Tensor) else min_bound)]
        if len(mb) != 3 or not all(math.isfinite(v) for v in mb):
            raise ValueError(f"{name}: min_bound must be three finite numbers, got {min_bound!r}")
    p = _prep(points)
    vals = [_prep(a) for a in attributes]
    dev = p.device
    if n == 0:
        require_gpu(points, *attributes)
        return (p, tuple(torch.zeros((0, a.shape[1]), dtype=torch.float32, device=dev) for a in vals),
                torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev))
    head = torch.cat([(~torch.isfinite(p)).any().to(torch.float64)[None], p.amin(0).double(), p.amax(0).double()]).tolist()   # host read 1 of 2
    if head[0] != 0:
        raise ValueError(f"{name}: points must be finite")
    lo, hi = head[1:4], head[4:7]
    origin = [(lo[a] if min_bound is None else mb[a]) - vs / 2 for a in range(3)]
    for a in range(3):
        if not (math.floor((lo[a] - origin[a]) / vs) > -VOXEL_CELLS and math.floor((hi[a] - origin[a]) / vs) < VOXEL_CELLS):
            raise ValueError(f"{name}: the points span more than 2^20 voxels of size {voxel_size!r} from the origin of the grid")
    require_gpu(points, *attributes)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws = _workspace(n, _VOXEL, dev)
    run("misplat_pointcloud_voxel_group", ptr(p), n, origin[0], origin[1], origin[2], vs, ptr(ws), ws.numel(), ptr(order),
        ptr(offsets), ptr(count))
    v = int(count.item())                                           # host read 2 of 2
    outs = []
    for x in [p] + vals:
        out = torch.empty((v, x.shape[1]), dtype=torch.float32, device=dev)
        run("misplat_pointcloud_voxel_mean", ptr(x), n, x.shape[1], ptr(order), ptr(offsets), v, ptr(out))
        outs.append(out)
    first = order[offsets[:v].long()].long()
    return outs[0], tuple(outs[1:]), first, offsets[1:v + 1] - offsets[:v]


# ----------------------------------------------------------------------------------------------------- compositions
def remove_far_points(points: Tensor, max_distance: Optional[float] = None, n_points: Optional[int] = None,
                      reference: str = "centroid") -> Tuple[Tensor, Tensor]:
    """The reference's ``remove_far_points``: (points[mask], mask [N] bool).  The points within ``max_distance`` (<=) of the
    centroid or of the origin, or else the ``n_points`` nearest to it (ties by index).  torch only, in the points' precision."""
    name = "remove_far_points"
    _cloud(name, "points", points)
    if max_distance is None and n_points is None:
        raise ValueError(f"{name}: specify either max_distance or n_points")
    if reference not in ("centroid", "origin"):
        raise ValueError(f"{name}: reference must be 'origin' or 'centroid', got {reference!r}")
    if max_distance is not None and not float(max_distance) >= 0:
        raise ValueError(f"{name}: max_distance must be >= 0, got {max_distance!r}")
    n = points.shape[0]
    if max_distance is None and (not isinstance(n_points, int) or isinstance(n_points, bool) or not 0 <= n_points <= n):
        raise ValueError(f"{name}: n_points must be an integer in 0..N = {n}, got {n_points!r}")
    require_gpu(points)
    x = points.detach()
    x = x if x.dtype in (torch.float32, torch.float64) else x.to(torch.float32)
    ref = x.mean(0) if (reference == "centroid" and n > 0) else torch.zeros(3, dtype=x.dtype, device=x.device)
    dist = (x - ref).norm(dim=1)
    if max_distance is not None:
        mask = dist <= float(max_distance)
    else:
        mask = torch.zeros(n, dtype=torch.bool, device=x.device)
        mask[torch.sort(dist, stable=True).indices[:n_points]] = True
    return points[mask], mask


def clean_pcd(points: Tensor, voxel_size: float = 0.015, radius: float = 0.05, max_distance: float = 1.0,
              downsample: bool = True, outlier_removal: bool = True, distance_removal: bool = True,
              reference: str = "centroid") -> Tuple[Tensor, Tensor]:
    """The reference's ``clean_pcd`` on a device tensor, its stages in its order: the voxel reduction (for N > 10 000 at the
    adaptive size voxel_size clamp(50 / avg, 0.5, 2.0), avg the mean ``radius_count`` at 2 radius of the first min(1000, N)
    points), ``remove_statistical_outlier(20, 2.0)``, ``remove_far_points(max_distance, reference)``.  Returns (points [M,3]
    fp32, indices [M] int64): the row of the input each survivor stands for (after the voxel reduction a survivor is a voxel's
    mean and its index the voxel's smallest member; without it points == input[indices])."""
    name = "clean_pcd"
    _cloud(name, "points", points)
    vs = _positive(name, "voxel_size", voxel_size)
    r = _positive32(name, "radius", radius)
    if reference not in ("centroid", "origin"):
        raise ValueError(f"{name}: reference must be 'origin' or 'centroid', got {reference!r}")
    if distance_removal and not float(max_distance) >= 0:
        raise ValueError(f"{name}: max_distance must be >= 0, got {max_distance!r}")
    _finite(name, points)
    require_gpu(points)
    pts = _prep(points)
    indices = torch.arange(pts.shape[0], dtype=torch.int64, device=pts.device)
    if downsample and pts.shape[0] > 0:
        if pts.shape[0] > 10000:
            avg = float(radius_count(pts, 2.0 * r, queries=pts[:1000]).double().mean())
            vs = vs * max(0.5, min(2.0, 50.0 / max(1e-6, avg)))
        pts, _, first, _ = voxel_down_sample(pts, vs)
        indices = indices[first]
    if outlier_removal and pts.shape[0] > 0:
        pts, ind = remove_statistical_outlier(pts, 20, 2.0)
        indices = indices[ind]
    if distance_removal:
        pts, mask = remove_far_points(pts, max_distance=max_distance, reference=reference)
        indices = indices[mask]
    return pts, indices


def calculate_accuracy(reconstructed: Tensor, reference: Tensor, percentile: float = 90) -> float:
    """The reference's ``calculate_accuracy``: numpy.percentile (linear) of the distance from every reconstructed point to
    its nearest reference point."""
    pct = _check_percentile("calculate_accuracy", percentile)
    _, nearest = knn_mean_distance(reference, 1, queries=reconstructed)
    if nearest.shape[0] == 0:
        raise ValueError("calculate_accuracy: no reconstructed points")
    return _percentile(torch.sort(nearest).values, pct)


def calculate_completeness(reconstructed: Tensor, reference: Tensor, threshold: float = 0.05) -> float:
    """The reference's ``calculate_completeness``: the percentage of reference points whose nearest reconstructed point is
    closer than ``threshold``."""
    _, nearest = knn_mean_distance(reconstructed, 1, queries=reference)
    if nearest.shape[0] == 0:
        raise ValueError("calculate_completeness: no reference points")
    return float((nearest.double() < float(threshold)).sum()) / nearest.shape[0] * 100


__all__ = ["knn_mean_distance", "statistical_outlier_mask", "remove_statistical_outlier", "radius_count", "density_filter",
           "voxel_down_sample", "remove_far_points", "clean_pcd", "calculate_accuracy", "calculate_completeness", "MisplatError"]
