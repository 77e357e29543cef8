"""Screened Poisson surface reconstruction of an oriented point cloud on the MI355X (csrc/poisson.hip).

Three of the reference's mesh exporters (``GaussiansToPoisson``, ``DepthAndNormalMapsPoisson``, ``LevelSetExtractor``,
collab_splats/utils/mesh.py:809-818, 1023-1032, 1191-1201) end in Open3D's ``create_from_point_cloud_poisson(pcd, depth=9)`` and
``remove_vertices_by_mask(densities < np.quantile(densities, 0.01))``.  Here the same step runs on device tensors as a RESTATED
dense-grid solve: the points' normals are splatted onto a uniform grid of 2^depth cells per axis, a 7-point screened Poisson system
is solved with Jacobi-preconditioned conjugate gradients, and the level set through the samples is extracted with the project's
marching cubes.  It is neither Kazhdan's adaptive octree nor Open3D's code, and parity with Open3D is not pinned: the oracle is
tests/poisson_restatement.py.  There is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from ._lib import MisplatError, load, ptr, require_gpu, run
from .meshclean import _attributes, _mesh
from .meshmap import _prep
from .pointcloud import _cloud, _finite, _positive32
from .unitvolume import UNIT, UNIT_VOXELS, make_grid, marching_cubes

MIN_DEPTH, MAX_DEPTH = 4, 9          # include/misplat.h MISPLAT_POISSON_MIN_DEPTH / MAX_DEPTH: 2^27 cells, 7 int64 grids of them
FIX = 2.0 ** 30                      # the fixed point of the splat (csrc/poisson.hip kFix)
CHECK_EVERY = 16                     # iterations between two host reads of the solver's state; it changes no result

_F = np.float32


# ---------------------------------------------------------------------------------------------------------- helpers
def _depth(name: str, depth) -> int:
    if not isinstance(depth, int) or isinstance(depth, bool) or not MIN_DEPTH <= depth <= MAX_DEPTH:
        raise ValueError(f"{name}: depth must be an integer in {MIN_DEPTH}..{MAX_DEPTH} (2^depth cells per axis, dense), got {depth!r}")
    return depth


def _workspace(depth: int, n_points: int, device) -> Tensor:
    b = int(load().misplat_poisson_workspace(depth, n_points))
    if b < 0:
        raise ValueError(f"poisson: depth {depth} with {n_points} points is beyond the library's limits")
    return torch.empty(b, dtype=torch.uint8, device=device)


def _grid(name: str, p: Tensor, depth: int, scale) -> Tuple[np.ndarray, np.float32]:
    """(origin [3] fp32, h fp32) after the call's host read: c = (lo + hi) / 2, s = scale max(hi - lo), h = s / G, o = c - s / 2."""
    sc = _positive32(name, "scale", scale)
    if p.shape[0] == 0:
        raise ValueError(f"{name}: no points")
    head = torch.cat([(~torch.isfinite(p)).any().to(torch.float32)[None], p.amin(0), p.amax(0)]).tolist()      # host read
    if head[0] != 0:
        raise ValueError(f"{name}: points must be finite")
    lo, hi = np.asarray(head[1:4], _F), np.asarray(head[4:7], _F)
    with np.errstate(all="ignore"):
        c = (lo + hi) / _F(2)
        s = _F(sc) * (hi - lo).max()
        h = _F(s / _F(1 << depth))
        o = (c - s / _F(2)).astype(_F)
    if not (s > 0 and np.isfinite(s) and h > 0 and np.isfinite(_F(1) / h) and np.isfinite(o).all()):
        raise ValueError(f"{name}: the points' extent must be positive and finite in fp32 (a single point, or coincident points, "
                         f"span no grid), got {float(s)!r}")
    return o, h


def _oriented(name: str, points, normals, colors) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    _cloud(name, "points", points)
    _cloud(name, "normals", normals)
    if colors is not None:
        _cloud(name, "colors", colors)
    for what, x in (("normals", normals), ("colors", colors)):
        if x is not None and x.shape[0] != points.shape[0]:
            raise ValueError(f"{name}: {what} must have one row per point ({points.shape[0]}), got {tuple(x.shape)}")
    require_gpu(points, normals, colors)
    _finite(name, normals, colors)
    return _prep(points), _prep(normals), None if colors is None else _prep(colors)


def _sample(field: Tensor, depth: int, o: np.ndarray, h, queries: Tensor) -> Tensor:
    """[Nq, C] fp32: the trilinear value of field [C,G,G,G] at the queries."""
    nch = field.shape[0]
    out = torch.empty((queries.shape[0], nch), dtype=torch.float32, device=field.device)
    run("misplat_poisson_sample", ptr(field), nch, depth, o[0], o[1], o[2], h, ptr(queries), queries.shape[0], ptr(out))
    return out


def _grids(name: str, W: Tensor, V: Tensor) -> int:
    if not isinstance(W, Tensor) or not isinstance(V, Tensor):
        raise TypeError(f"{name}: W and V must be tensors (poisson_splat's)")
    if W.dtype != torch.int64 or V.dtype != torch.int64:
        raise TypeError(f"{name}: W and V must be int64 fixed-point grids (poisson_splat's), got {W.dtype} and {V.dtype}")
    G = W.shape[0] if W.dim() == 3 else 0
    depth = G.bit_length() - 1
    if W.dim() != 3 or tuple(W.shape) != (G, G, G) or G != 1 << depth or not MIN_DEPTH <= depth <= MAX_DEPTH or \
            tuple(V.shape) != (3, G, G, G):
        raise ValueError(f"{name}: W must be [G,G,G] and V [3,G,G,G] with G = 2^depth, depth in {MIN_DEPTH}..{MAX_DEPTH}, got "
                         f"{tuple(W.shape)} and {tuple(V.shape)}")
    return depth


# ------------------------------------------------------------------------------------------------------------- grid
def poisson_grid(points: Tensor, depth: int = 8, scale: float = 1.1) -> dict:
    """``{"origin": [3] fp32 (numpy), "h": fp32, "G": 2^depth, "depth"}``: the cube the solve runs in.  lo, hi = the per-axis
    extremes of the points; c = (lo + hi) / 2, s = scale max(hi - lo) (Open3D's default scale 1.1), h = s / G, origin = c - s / 2,
    all in fp32; cell (i, j, k) has its centre at origin + (idx + 0.5) h.  A zero or non-finite extent is a ValueError."""
    name = "poisson_grid"
    _cloud(name, "points", points)
    d = _depth(name, depth)
    require_gpu(points)
    o, h = _grid(name, _prep(points), d, scale)
    return {"origin": o, "h": h, "G": 1 << d, "depth": d}


# ------------------------------------------------------------------------------------------------------------ splat
def _splat(p: Tensor, n: Tensor, c: Optional[Tensor], depth: int, o: np.ndarray, h) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    G = 1 << depth
    dev = p.device
    W = torch.empty((G, G, G), dtype=torch.int64, device=dev)
    V = torch.empty((3, G, G, G), dtype=torch.int64, device=dev)
    Cq = None if c is None else torch.empty((3, G, G, G), dtype=torch.int64, device=dev)
    run("misplat_poisson_splat", ptr(p), ptr(n), ptr(c), p.shape[0], depth, o[0], o[1], o[2], h, ptr(W), ptr(V), ptr(Cq))
    return W, V, Cq


def poisson_splat(points: Tensor, normals: Tensor, colors: Optional[Tensor] = None, depth: int = 8, scale: float = 1.1
                  ) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """(W [G,G,G], V [3,G,G,G], C [3,G,G,G] or None), int64 fixed point (x 2^30), indexed [z, y, x] on ``poisson_grid``'s grid.
    Per point g = (p - origin) / h - 0.5, i0 = floor(g), f = g - i0; each of the eight surrounding cells (clamped to the grid) takes
    w = (wx wy) wz: W += w, V_a += w n_a, C_c += w c_c, each as llrint(x 2^30) added with 64-bit integer atomics.  The sums are
    exact and independent of order: the grids equal the restatement's.  |w n| and |w c| must stay below 2^33."""
    name = "poisson_splat"
    p, n, c = _oriented(name, points, normals, colors)
    d = _depth(name, depth)
    o, h = _grid(name, p, d, scale)
    return _splat(p, n, c, d, o, h)


# ----------------------------------------------------------------------------------------------------------- system
def _system(W: Tensor, V: Tensor, depth: int, point_weight: float, ws: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    G = 1 << depth
    Wf, b, D = (torch.empty((G, G, G), dtype=torch.float32, device=W.device) for _ in range(3))
    run("misplat_poisson_system", ptr(W), ptr(V), depth, point_weight, ptr(ws), ws.numel(), ptr(Wf), ptr(b), ptr(D))
    return Wf, b, D


def _point_weight(name: str, v) -> float:
    try:
        f = float(v)
    except (TypeError, ValueError):
        f = math.nan
    if not (f >= 0 and math.isfinite(float(_F(f)))):
        raise ValueError(f"{name}: point_weight must be a finite number >= 0, got {v!r}")
    return float(_F(f))


def poisson_system(W: Tensor, V: Tensor, point_weight: float = 1.0) -> Tuple[Tensor, Tensor, Tensor]:
    """(W fp32, b, D), each [G,G,G]: the sampling density W = float(W) 2^-30, the right-hand side b(i) = -0.5 ((dVx + dVy) + dVz)
    with dV_a = V_a(i + e_a) - V_a(i - e_a) (V = 0 outside the grid), and the diagonal D(i) = #in-grid neighbours + point_weight
    W(i) / Wbar, Wbar = sum W / #{W > 0} from the integer sums, of the operator (A chi)(i) = D(i) chi(i) - sum of the in-grid
    neighbours of chi: the 7-point Laplacian with Neumann borders plus a mass-lumped screening term that pulls chi to 0 at the
    samples.  fp32 in one written order: b and D equal the restatement's bit for bit."""
    name = "poisson_system"
    depth = _grids(name, W, V)
    pw = _point_weight(name, point_weight)
    require_gpu(W, V)
    return _system(W.contiguous(), V.contiguous(), depth, pw, _workspace(depth, 0, W.device))


# ------------------------------------------------------------------------------------------------------------ solve
def _solve(b: Tensor, D: Tensor, depth: int, tol: float, max_iters: int, ws: Tensor) -> Tuple[Tensor, dict]:
    x, r, z, p, ap = (torch.empty_like(b) for _ in range(5))
    run("misplat_poisson_cg_init", ptr(b), ptr(D), depth, max_iters, ptr(ws), ws.numel(), ptr(x), ptr(r), ptr(z), ptr(p))
    state = ws[:64].view(torch.float64)
    while True:
        st = state.tolist()                                         # the host read, every CHECK_EVERY iterations
        if st[6] != 0:
            break
        run("misplat_poisson_cg_iterate", ptr(D), depth, CHECK_EVERY, tol, max_iters, ptr(ws), ws.numel(), ptr(x), ptr(r), ptr(z),
            ptr(p), ptr(ap))
    info = {"iterations": int(st[7]), "residual": math.sqrt(st[2] / st[3]) if st[3] > 0 else 0.0, "converged": st[6] == 1.0}
    return x, info


def _solve_args(name: str, depth: int, tol, max_iters) -> Tuple[float, int]:
    try:
        t = float(tol)
    except (TypeError, ValueError):
        t = math.nan
    if not (t >= 0 and math.isfinite(t)):
        raise ValueError(f"{name}: tol must be a finite number >= 0, got {tol!r}")
    if max_iters is None:
        max_iters = 8 << depth
    if not isinstance(max_iters, int) or isinstance(max_iters, bool) or not 0 <= max_iters < 1 << 30:
        raise ValueError(f"{name}: max_iters must be a non-negative integer, got {max_iters!r}")
    return t, max_iters


def poisson_solve(W: Tensor, V: Tensor, point_weight: float = 1.0, tol: float = 1e-5, max_iters: Optional[int] = None
                  ) -> Tuple[Tensor, dict]:
    """(chi [G,G,G] fp32, info): Jacobi-preconditioned conjugate gradients on ``poisson_system``'s A chi = b from chi = 0, until the
    recurrence residual satisfies |r| <= tol |b| or ``max_iters`` (default 8 G) iterations have run.  info = {"iterations",
    "residual": |r| / |b|, "converged"}; non-convergence does not raise.  1e-5 is about the floor fp32 reaches.  The dot products
    are fixed two-level reductions in fp64, alpha, beta and the stop flag stay on the device and the host looks every CHECK_EVERY
    iterations (the kernels are no-ops once the flag is set): two runs are bitwise equal."""
    name = "poisson_solve"
    depth = _grids(name, W, V)
    pw = _point_weight(name, point_weight)
    t, cap = _solve_args(name, depth, tol, max_iters)
    require_gpu(W, V)
    ws = _workspace(depth, 0, W.device)
    _, b, D = _system(W.contiguous(), V.contiguous(), depth, pw, ws)
    return _solve(b, D, depth, t, cap, ws)


# ---------------------------------------------------------------------------------------------------------- extract
def _iso(chi: Tensor, depth: int, o: np.ndarray, h, p: Tensor, ws: Tensor) -> float:
    vals = _sample(chi[None], depth, o, h, p).reshape(-1)
    mean = torch.empty(1, dtype=torch.float64, device=chi.device)
    run("misplat_poisson_mean", ptr(vals), vals.shape[0], ptr(ws), ws.numel(), ptr(mean))
    return float(mean.item())                                       # host read


def _extract(chi: Tensor, iso: float, depth: int, o: np.ndarray, h, Wf: Tensor, Cq: Optional[Tensor]
             ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Marching cubes of chi - float32(iso) over the cell centres, through the TSDF volume's extraction (csrc/tsdf.hip) on a fully
    allocated unit map with voxel_size 1; then world = origin + v h and the trilinear density and colour."""
    dev = chi.device
    U = (1 << depth) // UNIT
    n = U ** 3
    pool = torch.empty((n, 5, UNIT_VOXELS), dtype=torch.float32, device=dev)
    run("misplat_poisson_mc_pool", ptr(chi), depth, iso, ptr(pool))
    slot_map = torch.arange(n, dtype=torch.int32, device=dev)       # every unit allocated, in map order: the order too
    mesh = marching_cubes(make_grid(1.0, 1.0, 1.0, (0, 0, 0), (U, U, U)), slot_map, n, pool, order=slot_map)
    del pool
    if mesh is None:
        z3 = torch.zeros((0, 3), dtype=torch.float32, device=dev)
        return z3, torch.zeros((0, 3), dtype=torch.int32, device=dev), z3.clone(), torch.zeros(0, dtype=torch.float32, device=dev)
    v, triangles = mesh[:2]                                         # (the pool carries no colour)
    del mesh
    vertices = torch.as_tensor(o, device=dev)[None, :] + v * float(h)
    density = _sample(Wf[None], depth, o, h, vertices).reshape(-1)
    if Cq is None:
        colors = torch.zeros_like(vertices)
    else:
        cs = _sample(Cq.to(torch.float32) * (1.0 / FIX), depth, o, h, vertices)
        colors = torch.where(density[:, None] > 0, cs / density[:, None], torch.zeros_like(cs))
    return vertices, triangles, colors, density


def poisson_reconstruct(points: Tensor, normals: Tensor, colors: Optional[Tensor] = None, depth: int = 8, scale: float = 1.1,
                        point_weight: float = 1.0, tol: float = 1e-5, max_iters: Optional[int] = None
                        ) -> Tuple[Tensor, Tensor, Tensor, Tensor, dict]:
    """(vertices [M,3] fp32, triangles [T,3] int32, colors [M,3] fp32, density [M] fp32, info): ``poisson_splat``,
    ``poisson_solve``, then the level set chi = iso, iso the fp64 fixed-order mean over the points of the trilinear chi(p),
    extracted by marching cubes over the cell centres in the TSDF volume's deterministic order (units of 16^3 cells in map order, a
    unit's cells x-fastest, a cell's vertices +x, +y, +z, triangles in table order).  The field is negative inside: triangles face
    increasing chi, the side the normals point to.  ``density`` is the trilinear W at the vertex (what ``poisson_trim`` cuts by),
    ``colors`` the trilinear C over the trilinear W (0 where that is 0, or without ``colors``).  info = ``poisson_solve``'s plus
    "iso", "origin", "h", "G" and "chi" (the [G,G,G] solution on the device).  Two runs are bitwise equal."""
    name = "poisson_reconstruct"
    p, n, c = _oriented(name, points, normals, colors)
    d = _depth(name, depth)
    pw = _point_weight(name, point_weight)
    t, cap = _solve_args(name, d, tol, max_iters)
    o, h = _grid(name, p, d, scale)
    ws = _workspace(d, p.shape[0], p.device)
    W, V, Cq = _splat(p, n, c, d, o, h)
    Wf, b, D = _system(W, V, d, pw, ws)
    del W, V
    chi, info = _solve(b, D, d, t, cap, ws)
    del b, D
    iso = _iso(chi, d, o, h, p, ws)
    vertices, triangles, cols, density = _extract(chi, iso, d, o, h, Wf, Cq)
    info.update(iso=iso, origin=o, h=h, G=1 << d, chi=chi)
    return vertices, triangles, cols, density, info


# ------------------------------------------------------------------------------------------------------------- trim
def _quantile(sorted_values: Tensor, q: float) -> float:
    """numpy.quantile's default (linear) rule in fp64 on an ascending device tensor: ``pointcloud._percentile`` with the position
    (n - 1) q taken from q itself (100 q / 100 is not always q); two elements are read."""
    n = sorted_values.shape[0]
    pos = (n - 1) * q
    lo = min(max(int(math.floor(pos)), 0), n - 1)
    hi = min(lo + 1, n - 1)
    a, b = (float(v) for v in sorted_values[[lo, hi]].to(torch.float64).tolist())
    t = pos - lo
    return b - (b - a) * (1.0 - t) if t >= 0.5 else a + (b - a) * t


def poisson_trim(vertices: Tensor, triangles: Tensor, density: Tensor, quantile: float = 0.01, min_density: Optional[float] = None,
                 attributes: Sequence[Tensor] = ()) -> Tuple[Tensor, Tensor, Tensor, Tuple[Tensor, ...], Tensor]:
    """The reference's density trim, ``remove_vertices_by_mask(densities < np.quantile(densities, quantile))`` (mesh.py:817-818;
    numpy's linear-interpolation quantile in fp64), and, with ``min_density``, also the vertices with density < min_density: what
    closes an open surface lies where no sample is.  Every triangle that touches a dropped vertex goes, and so does a vertex left
    without a triangle (Open3D would keep it); the rest keeps its order and is re-indexed.  Returns (vertices, triangles, density,
    attributes, vertex_index [M'] int64: the row of the input each vertex was); each of ``attributes`` has one row per vertex."""
    name = "poisson_trim"
    v, t = _mesh(name, vertices, triangles)
    if not isinstance(density, Tensor) or density.dim() != 1 or density.shape[0] != v.shape[0]:
        raise ValueError(f"{name}: density must be [M] with M = {v.shape[0]}, got "
                         f"{tuple(density.shape) if isinstance(density, Tensor) else type(density).__name__}")
    attributes = _attributes(name, attributes, v.shape[0], False)
    try:
        q = float(quantile)
    except (TypeError, ValueError):
        q = math.nan
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"{name}: quantile must be in 0..1, got {quantile!r}")
    if min_density is not None and not math.isfinite(float(min_density)):
        raise ValueError(f"{name}: min_density must be a finite number or None, got {min_density!r}")
    require_gpu(vertices, triangles, density, *attributes)
    d64 = density.detach().to(torch.float64)
    if v.shape[0] == 0:
        idx = torch.zeros(0, dtype=torch.int64, device=v.device)
        return v, t.to(triangles.dtype), density[idx], tuple(a[idx] for a in attributes), idx
    drop = d64 < _quantile(torch.sort(d64).values, q)
    if min_density is not None:
        drop |= d64 < float(min_density)
    tl = t.long()
    kept = tl[~drop[tl].any(1)]
    used = torch.zeros(v.shape[0], dtype=torch.bool, device=v.device)
    used[kept.reshape(-1)] = True
    index = torch.nonzero(used)[:, 0]
    remap = torch.cumsum(used, 0) - 1
    return v[index], remap[kept].to(triangles.dtype), density[index], tuple(a[index] for a in attributes), index


__all__ = ["poisson_grid", "poisson_splat", "poisson_system", "poisson_solve", "poisson_reconstruct", "poisson_trim", "MIN_DEPTH",
           "MAX_DEPTH", "MisplatError"]
