"""Mesh finishing on the MI355X (csrc/meshclean.hip).

The reference's production mesher (collab_splats/utils/mesh.py ``Open3DTSDFFusion.main``) cleans the extracted mesh with
MeshLib (``clean_repair_mesh``, mesh.py:227-407: drop floating components, measure edges, fill holes) and aligns it to its
floor with Open3D (``align_geometry_floor``, mesh.py:410-515: sample the surface, RANSAC plane, rotate, translate).  Here the
same steps run on device tensors: the edge table of the welded mesh, the edge-connected components, the boundary loops, the
RANSAC hypotheses, their inlier counts and the refit's moments are HIP kernels; the rest is thin torch on the device and a
3x3 eigenproblem on the host.  ``smooth_laplacian`` is the Laplacian smoothing that ends the reference's ``LevelSetExtractor``
(mesh.py:1217-1223, Open3D's ``filter_smooth_laplacian``).  There is no CPU fallback.

``fill_holes`` is the reference's *fallback*, MeshLib's ``fillHoleTrivially``: one new vertex per hole and a fan of triangles to
it.  What stands where the reference's default, ``fillHoleNicely``, stands (the fan subdivided to the mesh's edge length, its
new vertices positioned smoothly) is ``meshfill.fill_holes_nicely``, which shares the fans built here;
``meshfill.triangulate_holes`` (section 30) closes the same loops without a centre vertex and keeps the fan for the loops it
cannot triangulate.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from ._lib import MisplatError, load, ptr, require_gpu, run
from .meshmap import _prep
from .pointcloud import _cloud, _positive32

# Hypotheses per workgroup of the inlier count: 8, 16 or 32.  It changes no result (DESIGN.md section 18.3 holds the measurement).
PLANE_TILE = 16

_STATS, _COMPONENTS, _HOLES, _MOMENTS, _SMOOTH = range(5)
MAX_PLANES = 1 << 24


# ---------------------------------------------------------------------------------------------------------- helpers
def _mesh(name: str, vertices: Tensor, triangles: Tensor) -> Tuple[Tensor, Tensor]:
    """(vertices fp32 [M,3], triangles int32 [T,3]), both contiguous, after the host check of every index (one host read)."""
    _cloud(name, "vertices", vertices)
    if not isinstance(triangles, Tensor) or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError(f"{name}: triangles must be [T,3], got {tuple(triangles.shape) if isinstance(triangles, Tensor) else type(triangles).__name__}")
    if triangles.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name}: triangles must be int32 or int64, got {triangles.dtype}")
    m, t = vertices.shape[0], triangles.shape[0]
    if t >= 1 << 30 or m >= 1 << 31:
        raise ValueError(f"{name}: {t} triangles over {m} vertices are beyond the library's limits (T < 2^30, M < 2^31)")
    if t > 0:
        lo, hi = (int(x) for x in torch.aminmax(triangles))         # the call's host read
        if lo < 0 or hi >= m:
            raise ValueError(f"{name}: triangle indices must lie in 0..{m - 1}, found {lo if lo < 0 else hi}")
    return _prep(vertices), triangles.detach().to(torch.int32).contiguous()


def _attributes(name: str, attributes: Sequence[Tensor], m: int, floating: bool) -> Tuple[Tensor, ...]:
    attributes = tuple(attributes)
    for a in attributes:
        if not isinstance(a, Tensor) or a.dim() < 1 or a.shape[0] != m:
            raise ValueError(f"{name}: every attribute must have one row per vertex ({m}), got "
                             f"{tuple(a.shape) if isinstance(a, Tensor) else type(a).__name__}")
        if floating and (a.dim() != 2 or a.shape[1] < 1 or a.dtype != torch.float32):
            raise ValueError(f"{name}: every attribute must be [M,D] float32 (it is averaged), got {tuple(a.shape)} {a.dtype}")
    return attributes


def _workspace(n_vertices: int, n_triangles: int, kind: int, device) -> Tensor:
    b = int(load().misplat_meshclean_workspace(n_vertices, n_triangles, kind))
    if b < 0:
        raise ValueError(f"meshclean: {n_triangles} triangles / {n_vertices} vertices or points are beyond the library's limits")
    return torch.empty(b, dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------------------------- edge table
def mesh_edge_stats(vertices: Tensor, triangles: Tensor) -> dict:
    """``{"n_edges", "n_boundary", "n_nonmanifold", "mean_edge_length"}`` of the mesh's undirected edges: an edge is a
    boundary edge with exactly one incident face and non-manifold with more than two; the mean (the reference's
    ``_compute_avg_edge_length``) is the fp64 mean of the fp32 lengths sqrt((dx dx + dy dy) + dz dz), summed in a fixed order.
    A corner repeated inside a triangle is allowed: its edge (a, a) is ignored."""
    v, t = _mesh("mesh_edge_stats", vertices, triangles)
    require_gpu(vertices, triangles)
    counts = torch.empty(3, dtype=torch.int32, device=v.device)
    mean = torch.empty(1, dtype=torch.float64, device=v.device)
    ws = _workspace(v.shape[0], t.shape[0], _STATS, v.device)
    run("misplat_meshclean_edge_stats", ptr(v), v.shape[0], ptr(t), t.shape[0], ptr(ws), ws.numel(), ptr(counts), ptr(mean))
    e, b, nm = counts.tolist()
    return {"n_edges": e, "n_boundary": b, "n_nonmanifold": nm, "mean_edge_length": float(mean.item())}


# ------------------------------------------------------------------------------------------------------- components
def mesh_components(vertices: Tensor, triangles: Tensor) -> Tuple[Tensor, Tensor]:
    """(face_labels [T] int32, sizes [C] int32).  Two faces are in one component iff a chain of shared undirected edges links
    them (MeshLib's default, per-edge incidence): faces that touch only at a vertex are separate, all faces around a
    non-manifold edge are joined.  Components are numbered in ascending order of their smallest face index."""
    v, t = _mesh("mesh_components", vertices, triangles)
    require_gpu(vertices, triangles)
    return _components(v, t)


def _components(v: Tensor, t: Tensor) -> Tuple[Tensor, Tensor]:
    n = t.shape[0]
    labels = torch.empty(n, dtype=torch.int32, device=v.device)
    sizes = torch.empty(n, dtype=torch.int32, device=v.device)
    count = torch.empty(1, dtype=torch.int32, device=v.device)
    ws = _workspace(v.shape[0], n, _COMPONENTS, v.device)
    run("misplat_meshclean_components", ptr(t), v.shape[0], n, ptr(ws), ws.numel(), ptr(labels), ptr(sizes), ptr(count))
    return labels, sizes[:int(count.item())].clone()


def filter_mesh_components(vertices: Tensor, triangles: Tensor, use_largest: bool = False, attributes: Sequence[Tensor] = ()
                           ) -> Tuple[Tensor, Tensor, Tensor, Tuple[Tensor, ...], int]:
    """The reference's ``_filter_mesh_components``: keep the component with the most faces (a tie goes to the smaller
    number) and, unless ``use_largest``, every component whose axis-aligned bounding box (over the vertices of its faces) lies
    inside the largest one's, closed on all six sides, in fp32.  Returns (vertices [M',3], triangles [T',3], vertex_index [M']
    int64, attributes, n_removed): the kept faces in their original order, the vertices they reference in their original order
    and re-indexed, the old index of each kept vertex, each of ``attributes`` (one row per vertex) gathered by that index, and
    the number of components dropped.  Unreferenced vertices are dropped.  Attributes are carried exactly: the reference
    recolours by kNN (mesh.py:1655) only because MeshLib drops them."""
    name = "filter_mesh_components"
    v, t = _mesh(name, vertices, triangles)
    attributes = _attributes(name, attributes, v.shape[0], False)
    require_gpu(vertices, triangles, *attributes)
    dev = v.device
    if t.shape[0] == 0:
        idx = torch.zeros(0, dtype=torch.int64, device=dev)
        return v[idx], t.to(triangles.dtype), idx, tuple(a[idx] for a in attributes), 0
    labels, sizes = _components(v, t)
    n_comp = sizes.shape[0]
    lab = labels.long()
    largest = torch.nonzero(sizes == sizes.max())[0, 0]             # ties: the smaller number
    keep_comp = torch.zeros(n_comp, dtype=torch.bool, device=dev)
    keep_comp[largest] = True
    if not use_largest and n_comp > 1:
        # the largest component's box by a plain reduction (scattering its faces would queue them all on six addresses), the
        # other components' by a scatter of minima and maxima: exact in any order
        corners = v[t.long()]                                       # [T,3,3]
        fmin, fmax = corners.amin(1), corners.amax(1)
        big = lab == largest
        lo_big, hi_big = fmin[big].amin(0), fmax[big].amax(0)
        ix = lab[~big][:, None].expand(-1, 3)
        lo = torch.full((n_comp, 3), math.inf, device=dev).scatter_reduce(0, ix, fmin[~big], "amin")
        hi = torch.full((n_comp, 3), -math.inf, device=dev).scatter_reduce(0, ix, fmax[~big], "amax")
        keep_comp |= ((lo >= lo_big) & (hi <= hi_big)).all(1)
    keep_face = keep_comp[lab]
    kept = t[keep_face].long()
    used = torch.zeros(v.shape[0], dtype=torch.bool, device=dev)
    used[kept.reshape(-1)] = True
    index = torch.nonzero(used)[:, 0]
    remap = torch.cumsum(used, 0) - 1
    new_t = remap[kept].to(triangles.dtype)
    n_removed = n_comp - int(keep_comp.sum())
    return v[index], new_t, index, tuple(a[index] for a in attributes), n_removed


# ------------------------------------------------------------------------------------------------------------ holes
def mesh_holes(vertices: Tensor, triangles: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(loop_of_edge [B] int32, edges [B,2] int32, n_edges [L] int32, perimeter [L] fp64).  The boundary edges (exactly one
    incident face) in ascending (face, corner) order, each directed as its face traverses it.  A loop is a set of boundary
    edges connected through shared vertices: two holes pinched at one vertex count as ONE loop (MeshLib, which walks half
    edges, would count two).  Loops are numbered in ascending order of their smallest vertex index; a perimeter is the fp64 sum
    of the loop's fp32 edge lengths in list order."""
    v, t = _mesh("mesh_holes", vertices, triangles)
    require_gpu(vertices, triangles)
    return _holes(v, t)[:4]


def _segment_sum(values: Tensor, order: Tensor, offsets: Tensor, n: int) -> Tensor:
    out = torch.empty(n, dtype=torch.float64, device=values.device)
    run("misplat_meshclean_segment_sum", ptr(values), ptr(order), ptr(offsets), n, ptr(out))
    return out


def _holes(v: Tensor, t: Tensor):
    dev = v.device
    n = t.shape[0]
    edges = torch.empty((3 * n, 2), dtype=torch.int32, device=dev)
    loop = torch.empty(3 * n, dtype=torch.int32, device=dev)
    length = torch.empty(3 * n, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    ws = _workspace(v.shape[0], n, _HOLES, dev)
    run("misplat_meshclean_holes", ptr(v), v.shape[0], ptr(t), n, ptr(ws), ws.numel(), ptr(edges), ptr(loop), ptr(length),
        ptr(counts))
    b, n_loops = counts.tolist()                                    # the call's host read
    edges, loop, length = edges[:b].clone(), loop[:b].clone(), length[:b].clone()
    order = torch.sort(loop, stable=True).indices.to(torch.int32)   # edges by loop, in list order inside a loop
    n_edges = torch.bincount(loop, minlength=n_loops).to(torch.int32)
    offsets = torch.zeros(n_loops + 1, dtype=torch.int32, device=dev)
    offsets[1:] = torch.cumsum(n_edges, 0)
    perimeter = _segment_sum(length, order, offsets, n_loops)
    return loop, edges, n_edges, perimeter, order


def fill_holes(vertices: Tensor, triangles: Tensor, max_hole_size: float = 3.0, attributes: Sequence[Tensor] = ()
               ) -> Tuple[Tensor, Tensor, Tuple[Tensor, ...], int]:
    """Close every loop of ``mesh_holes`` whose perimeter is below ``max_hole_size`` (the reference's default 3.0 is what keeps
    the outer rim of an open scene unfilled) with a fan: one appended vertex, the fp64 mean of the loop's distinct vertices
    rounded to fp32 (``attributes``, [M,D] float32, are averaged the same way), and for each boundary edge a -> b of the loop
    the triangle (b, a, c).  Loops go in rank order, their edges in list order.  Returns (vertices, triangles, attributes,
    n_filled).

    This is MeshLib's ``fillHoleTrivially``, the reference's *fallback* (mesh.py:312): no triangulation metric, no subdivision,
    no smoothing.  ``meshfill.fill_holes_nicely`` subdivides and fairs these same fans, as the reference's default
    ``fillHoleNicely`` does its patches."""
    name = "fill_holes"
    v, t = _mesh(name, vertices, triangles)
    attributes = _attributes(name, attributes, v.shape[0], True)
    limit = _limit(name, max_hole_size)
    require_gpu(vertices, triangles, *attributes)
    attributes = tuple(_prep(a) for a in attributes)
    filled = _fans(v, t, attributes, limit) if t.shape[0] else None
    if filled is None:
        return v, t.to(triangles.dtype), attributes, 0
    return filled[0], filled[1].to(triangles.dtype), filled[2], filled[3]


def _limit(name: str, max_hole_size) -> float:
    try:
        limit = float(max_hole_size)
    except (TypeError, ValueError):
        limit = math.nan
    if math.isnan(limit):
        raise ValueError(f"{name}: max_hole_size must be a number, got {max_hole_size!r}")
    return limit


def _fans(v: Tensor, t: Tensor, attributes: Tuple[Tensor, ...], limit: float):
    """The fans of ``fill_holes`` over a prepared mesh with at least one face: (vertices, triangles int64, attributes,
    n_filled), or None where no loop is below the limit.  Shared with ``meshfill.fill_holes_nicely``."""
    loop, edges, _, perimeter, order = _holes(v, t)
    fill = perimeter < limit
    n_fill = int(fill.sum())
    if n_fill == 0:
        return None
    fans, _, outs = _fan_patches(v, attributes, loop, edges, order, fill, n_fill)
    return outs[0], torch.cat([t.long(), fans]), tuple(outs[1:]), n_fill


def _fan_patches(v: Tensor, attributes: Tuple[Tensor, ...], loop: Tensor, edges: Tensor, order: Tensor, fill: Tensor, n_fill: int):
    """The fans of the ``n_fill`` loops of the mask ``fill`` ([L] bool): (faces [F,3] int64, the fan each face belongs to [F]
    int64, (vertices, *attributes) with the fans' centres appended).  Fans go in loop rank order, their edges in list order;
    fan r's centre is vertex M + r.  Shared with ``meshfill.triangulate_holes`` (the loops it does not triangulate)."""
    m = v.shape[0]
    new_id = torch.cumsum(fill, 0) - 1                              # rank of a filled loop among the filled ones
    order = order.long()
    chosen = order[fill[loop.long()[order]]]                        # the fans' edges: loops in rank order, edges in list order
    a, b, l = edges[chosen, 0].long(), edges[chosen, 1].long(), loop.long()[chosen]
    fans = torch.stack([b, a, m + new_id[l]], 1)
    keys = torch.unique(torch.cat([new_id[l] * m + a, new_id[l] * m + b]))      # the distinct (loop, vertex) pairs, sorted
    members = (keys % m).to(torch.int32)
    offsets = torch.zeros(n_fill + 1, dtype=torch.int32, device=v.device)
    offsets[1:] = torch.cumsum(torch.bincount(keys // m, minlength=n_fill), 0)
    outs = []
    for x in (v,) + attributes:
        mean = torch.empty((n_fill, x.shape[1]), dtype=torch.float32, device=v.device)
        run("misplat_pointcloud_voxel_mean", ptr(x), m, x.shape[1], ptr(members), ptr(offsets), n_fill, ptr(mean))
        outs.append(torch.cat([x, mean]))
    return fans, new_id[l], outs


# -------------------------------------------------------------------------------------------------------- smoothing
def smooth_laplacian(vertices: Tensor, triangles: Tensor, iterations: int = 1, lam: float = 0.5, attributes: Sequence[Tensor] = ()
                     ) -> Tuple[Tensor, Tuple[Tensor, ...]]:
    """Open3D's ``filter_smooth_laplacian`` restated [UNVERIFIED-UPSTREAM], what the reference's ``LevelSetExtractor`` ends
    with (mesh.py:1217-1223): ``(vertices', attributes')``.  Per iteration, from the previous iteration's positions: with
    ``N(i)`` the distinct vertices that share a triangle edge with ``i`` and ``w_ij = 1 / (|x_i - x_j| + 1e-12)``,
    ``x_i' = x_i + lam (sum_j w_ij x_j / sum_j w_ij - x_i)``; every row of ``attributes`` ([M,D] float32) is smoothed with the
    same weights; a vertex without a neighbour is unchanged.  The neighbours are gathered in ascending order from a CSR built
    once per call (the directed edges sorted by source, then target); sums in fp64 in that order, stores in fp32: two runs are
    bitwise equal."""
    name = "smooth_laplacian"
    v, t = _mesh(name, vertices, triangles)
    attributes = _attributes(name, attributes, v.shape[0], True)
    if not isinstance(iterations, int) or isinstance(iterations, bool) or iterations < 0:
        raise ValueError(f"{name}: iterations must be a non-negative integer, got {iterations!r}")
    try:
        lam = float(lam)
    except (TypeError, ValueError):
        lam = math.nan
    if not math.isfinite(lam):
        raise ValueError(f"{name}: lam must be a finite number")
    if 6 * t.shape[0] >= (1 << 31) - 4096:
        raise ValueError(f"{name}: {t.shape[0]} triangles are beyond the library's limits (6 T < 2^31 - 4096)")
    require_gpu(vertices, triangles, *attributes)
    attributes = tuple(_prep(a) for a in attributes)
    m, n = v.shape[0], t.shape[0]
    if iterations == 0 or m == 0 or n == 0:
        return v.clone(), tuple(a.clone() for a in attributes)
    dev = v.device
    widths = [a.shape[1] for a in attributes]
    d = sum(widths)
    att = torch.cat(attributes, 1).contiguous() if d else None
    v_out, a_out = torch.empty_like(v), None if att is None else torch.empty_like(att)
    v_tmp = torch.empty_like(v) if iterations > 1 else None
    a_tmp = torch.empty_like(att) if iterations > 1 and att is not None else None
    ws = _workspace(m, n, _SMOOTH, dev)
    run("misplat_meshclean_smooth", ptr(v), m, ptr(t), n, ptr(att), d, iterations, lam, ptr(ws), ws.numel(), ptr(v_out),
        ptr(a_out), ptr(v_tmp), ptr(a_tmp))
    return v_out, (tuple(x.contiguous() for x in torch.split(a_out, widths, 1)) if d else ())


# ------------------------------------------------------------------------------------------------------------ plane
def _threshold(name: str, v) -> float:
    return _positive32(name, "distance_threshold", v)


def _planes_arg(name: str, planes: Tensor) -> None:
    if not isinstance(planes, Tensor) or planes.dim() != 2 or planes.shape[1] != 4:
        raise ValueError(f"{name}: planes must be [H,4], got {tuple(planes.shape) if isinstance(planes, Tensor) else type(planes).__name__}")
    if planes.shape[0] > MAX_PLANES:
        raise ValueError(f"{name}: at most {MAX_PLANES} planes, got {planes.shape[0]}")


def plane_inlier_counts(points: Tensor, planes: Tensor, distance_threshold: float) -> Tensor:
    """[H] int32: per plane (a, b, c, d) the number of points with |((a x + b y) + c z) + d| < t in fp32, t =
    float32(distance_threshold); the comparison is strict.  A plane with a NaN counts 0."""
    name = "plane_inlier_counts"
    _cloud(name, "points", points)
    _planes_arg(name, planes)
    t = _threshold(name, distance_threshold)
    if PLANE_TILE not in (8, 16, 32):
        raise ValueError(f"{name}: meshclean.PLANE_TILE must be 8, 16 or 32, got {PLANE_TILE!r}")
    require_gpu(points, planes)
    p, pl = _prep(points), _prep(planes)
    return _plane_counts(p, pl, t)


def _plane_counts(p: Tensor, pl: Tensor, t: float) -> Tensor:
    counts = torch.empty(pl.shape[0], dtype=torch.int32, device=p.device)
    run("misplat_meshclean_plane_count", ptr(p), p.shape[0], ptr(pl), pl.shape[0], t, PLANE_TILE, ptr(counts))
    return counts


def ransac_planes(points: Tensor, num_iterations: int = 1000, seed: int = 0, triples: Optional[Tensor] = None
                  ) -> Tuple[Tensor, Tensor]:
    """(triples [H,3] int32, planes [H,4] fp32): hypothesis i takes three distinct point indices from a counter-based
    integer hash of (seed, i, draw), redrawing on a repeat (or takes row i of ``triples``), and the plane through the three
    points, built in fp32 in a fixed operation order: unit normal (p1 - p0) x (p2 - p0) / |.| and d = -n . p0.  A triple
    that spans no plane (collinear or repeated points) gives four NaN: it scores 0."""
    name = "ransac_planes"
    _cloud(name, "points", points)
    n = points.shape[0]
    if n < 3:
        raise ValueError(f"{name}: a plane needs at least 3 points, got {n}")
    if n >= 1 << 30:
        raise ValueError(f"{name}: {n} points are beyond the library's limits")
    if triples is not None:
        if not isinstance(triples, Tensor) or triples.dim() != 2 or triples.shape[1] != 3 or triples.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{name}: triples must be an integer [H,3] tensor")
        h = triples.shape[0]
        if h and (int(triples.min()) < 0 or int(triples.max()) >= n):
            raise ValueError(f"{name}: triples must index the points (0..{n - 1})")
    else:
        if not isinstance(num_iterations, int) or isinstance(num_iterations, bool):
            raise ValueError(f"{name}: num_iterations must be an integer, got {num_iterations!r}")
        h = num_iterations
    if not 1 <= h <= MAX_PLANES:
        raise ValueError(f"{name}: the number of hypotheses must be in 1..{MAX_PLANES}, got {h}")
    if not isinstance(seed, int) or isinstance(seed, bool) or not 0 <= seed < 1 << 32:
        raise ValueError(f"{name}: seed must be an integer in 0..2^32-1, got {seed!r}")
    require_gpu(points, triples)
    p = _prep(points)
    given = None if triples is None else triples.detach().to(torch.int32).contiguous()
    out = given if given is not None else torch.empty((h, 3), dtype=torch.int32, device=p.device)
    planes = torch.empty((h, 4), dtype=torch.float32, device=p.device)
    run("misplat_meshclean_plane_build", ptr(p), n, ptr(given), seed, h, ptr(None if given is not None else out), ptr(planes))
    return out, planes


def segment_plane(points: Tensor, distance_threshold: float = 0.02, ransac_n: int = 3, num_iterations: int = 1000, seed: int = 0,
                  triples: Optional[Tensor] = None, return_index: bool = False):
    """Open3D's ``segment_plane``: (plane [4] fp64 on the host, inliers int64 on the device).  ``num_iterations`` hypotheses
    (``ransac_planes``), each scored by ``plane_inlier_counts``; the winner has the most inliers, a tie goes to the lowest
    hypothesis index (a deviation: Open3D breaks ties by rmse and stops early by a probability estimate; every hypothesis is
    scored here).  The refit is Open3D's: the fp64 mean and covariance of the winner's inliers (fixed-order sums on the
    device), the 3x3 eigenproblem on the host; the normal is the eigenvector of the smallest eigenvalue, signed to agree with
    the hypothesis, d = -n . mean.  The inliers are the winner's (before the refit), ascending.  Only ``ransac_n == 3`` is
    supported.  ``triples`` replaces the drawn hypotheses; ``return_index`` appends the winner's index."""
    name = "segment_plane"
    _cloud(name, "points", points)
    if ransac_n != 3:
        raise ValueError(f"{name}: only ransac_n == 3 is supported, got {ransac_n!r}")
    t = _threshold(name, distance_threshold)
    if PLANE_TILE not in (8, 16, 32):
        raise ValueError(f"{name}: meshclean.PLANE_TILE must be 8, 16 or 32, got {PLANE_TILE!r}")
    _, planes = ransac_planes(points, num_iterations, seed, triples)
    p = _prep(points)
    n = p.shape[0]
    counts = _plane_counts(p, planes, t)
    best = torch.nonzero(counts == counts.max())[0, 0]              # ties: the lowest index
    mask = torch.empty(n, dtype=torch.uint8, device=p.device)
    moments = torch.empty(10, dtype=torch.float64, device=p.device)
    ws = _workspace(n, 0, _MOMENTS, p.device)
    run("misplat_meshclean_plane_moments", ptr(p), n, ptr(planes[best]), t, ptr(ws), ws.numel(), ptr(mask), ptr(moments))
    host = torch.cat([moments, planes[best].double(), best[None].double()]).tolist()       # the call's host read
    mom, hyp, index = host[:10], host[10:14], int(host[14])
    if mom[0] < 3 or any(math.isnan(x) for x in hyp):
        raise ValueError(f"{name}: no hypothesis has three inliers (are the points collinear?)")
    mean = torch.tensor(mom[1:4], dtype=torch.float64) / mom[0]
    xx, xy, xz, yy, yz, zz = (x / mom[0] for x in mom[4:])
    cov = torch.tensor([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], dtype=torch.float64)
    normal = torch.linalg.eigh(cov).eigenvectors[:, 0]
    if float(normal @ torch.tensor(hyp[:3], dtype=torch.float64)) < 0:
        normal = -normal
    plane = torch.cat([normal, -(normal @ mean)[None]])
    inliers = torch.nonzero(mask)[:, 0]
    return (plane, inliers, index) if return_index else (plane, inliers)


def sample_surface(vertices: Tensor, triangles: Tensor, n: int, seed: int = 0) -> Tuple[Tensor, Tensor]:
    """(points [n,3] fp32, triangle [n] int64): Open3D's ``sample_points_uniformly``: a triangle chosen with probability
    proportional to its area, a point in it by square-root barycentrics (1 - sqrt(u), sqrt(u) (1 - w), sqrt(u) w).  Plain
    torch on the device, fp64, from a generator seeded with ``seed``; not a hot path."""
    name = "sample_surface"
    v, t = _mesh(name, vertices, triangles)
    if not isinstance(n, int) or isinstance(n, bool) or n < 0:
        raise ValueError(f"{name}: n must be a non-negative integer, got {n!r}")
    if t.shape[0] == 0:
        raise ValueError(f"{name}: the mesh has no triangle")
    require_gpu(vertices, triangles)
    c = v.double()[t.long()]
    area = 0.5 * torch.linalg.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]).norm(dim=1)
    cdf = torch.cumsum(area, 0)
    total = cdf[-1]
    if not float(total) > 0:
        raise ValueError(f"{name}: the mesh has no area")
    gen = torch.Generator(device=v.device)
    gen.manual_seed(int(seed))
    u = torch.rand((n, 3), dtype=torch.float64, device=v.device, generator=gen)
    tri = torch.searchsorted(cdf, u[:, 0] * total, right=True).clamp_(max=t.shape[0] - 1)
    r = torch.sqrt(u[:, 1])
    w = torch.stack([1 - r, r * (1 - u[:, 2]), r * u[:, 2]], 1)
    pts = (w[:, :, None] * c[tri]).sum(1)
    return pts.float(), tri


# -------------------------------------------------------------------------------------------------------- alignment
def floor_rotation(plane) -> Tuple[Tensor, float]:
    """mesh.py:448-473 on the host in fp64: normalise the normal, flip it (and d) to n_z >= 0, the axis-angle rotation that
    takes it onto +z (Rodrigues), the identity when |n x z| < 1e-6.  Returns (R [3,3], d)."""
    a, b, c, d = (float(x) for x in plane)
    norm = math.sqrt(a * a + b * b + c * c)
    n = [a / norm, b / norm, c / norm]
    if n[2] < 0:
        n = [-x for x in n]
        d = -d
    axis = [n[1], -n[0], 0.0]                                       # n x z
    s = math.sqrt(axis[0] * axis[0] + axis[1] * axis[1])
    R = torch.eye(3, dtype=torch.float64)
    if s < 1e-6:
        return R, d
    angle = math.acos(min(1.0, max(-1.0, n[2])))
    kx, ky = axis[0] / s, axis[1] / s
    K = torch.tensor([[0.0, 0.0, ky], [0.0, 0.0, -kx], [-ky, kx, 0.0]], dtype=torch.float64)
    return R + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K), d


def apply_rigid(points: Tensor, R: Tensor, translation: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(rotated, moved): rotated = fp32 of ((R0 x + R1 y) + R2 z) per row of R in fp64 (about the origin); moved = fp32 of
    rotated + translation in fp64 (rotated itself without one).  Elementwise, so it equals the same expression anywhere."""
    x, y, z = (points[:, i].double() for i in range(3))
    Rl = R.tolist()
    rot = torch.stack([(Rl[i][0] * x + Rl[i][1] * y) + Rl[i][2] * z for i in range(3)], 1).float()
    if translation is None:
        return rot, rot
    tl = translation.tolist()
    return rot, torch.stack([rot[:, i].double() + tl[i] for i in range(3)], 1).float()


def align_floor(points_or_mesh: Union[Tensor, Tuple[Tensor, Tensor]], dist_threshold: float = 0.02, ransac_n: int = 3,
                num_iterations: int = 1000, num_sample_points: int = 10000, seed: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
    """The reference's ``align_geometry_floor`` (mesh.py:410-498): (aligned vertices or points [M,3] fp32 on the device, R
    [3,3] and translation [3], fp64 on the host).  Fit the floor (``segment_plane``), rotate its upward normal onto +z about
    the origin (``floor_rotation``), fit again and translate by (0, 0, -d_new).  A cloud ([N,3]) is fitted to its own points; a
    mesh ((vertices, triangles)) to ``num_sample_points`` samples of its surface (``sample_surface``, seeds ``seed`` and
    ``seed + 1``); the hypotheses of both fits use ``seed``.

    One deviation: the reference takes d_new with whatever sign Open3D gave the refitted normal, and (0, 0, -d_new) puts the
    floor at z = 0 only when that normal points down (with it pointing up the floor lands at twice its height).  Here d_new
    is always taken for the downward normal, so the floor ends at z = 0."""
    name = "align_floor"
    if isinstance(points_or_mesh, Tensor):
        _cloud(name, "points", points_or_mesh)
        require_gpu(points_or_mesh)
        pts, tris = _prep(points_or_mesh), None
    else:
        try:
            vertices, triangles = points_or_mesh
        except (TypeError, ValueError):
            raise ValueError(f"{name}: pass a point cloud [N,3] or a (vertices, triangles) pair") from None
        pts, tris = _mesh(name, vertices, triangles)
        require_gpu(vertices, triangles)
    fit = (lambda x, sd: x) if tris is None else (lambda x, sd: sample_surface(x, tris, num_sample_points, sd)[0])
    plane, _ = segment_plane(fit(pts, seed), dist_threshold, ransac_n, num_iterations, seed)
    R, _ = floor_rotation(plane)
    rotated, _ = apply_rigid(pts, R)
    plane2, _ = segment_plane(fit(rotated, seed + 1), dist_threshold, ransac_n, num_iterations, seed)
    d_new = float(plane2[3]) if float(plane2[2]) < 0 else -float(plane2[3])     # d of the refitted plane with its normal pointing down
    translation = torch.tensor([0.0, 0.0, -d_new], dtype=torch.float64)
    return apply_rigid(pts, R, translation)[1], R, translation


__all__ = ["mesh_edge_stats", "mesh_components", "filter_mesh_components", "mesh_holes", "fill_holes", "plane_inlier_counts",
           "ransac_planes", "segment_plane", "sample_surface", "floor_rotation", "apply_rigid", "align_floor", "smooth_laplacian",
           "MisplatError"]
