"""Hole filling at the mesh's own resolution on the MI355X (csrc/meshfill.hip).

The reference's ``clean_repair_mesh`` (collab_splats/utils/mesh.py:359-407) closes every hole below ``max_hole_size`` with
MeshLib's ``fillHoleNicely`` (``maxEdgeLen`` = the mesh's average edge length, ``maxEdgeSplits`` = 10000; the fallback is
``fillHole`` + ``subdivideMesh`` + ``positionVertsSmoothly``, :317-356): the hole is triangulated by a metric, the patch is
subdivided to the mesh's edge length while its edges are flipped, and its new vertices are positioned smoothly.  Here the same
steps run on device tensors: the fan of ``fill_holes`` or the minimum-area triangulation of the loop (``triangulate_holes``,
csrc/meshtri.hip), longest-edge bisection of the patch's faces in rounds (``subdivide_mesh``), Delaunay-like
flips of its edges (``flip_edges``, section 30), membrane fairing of the created vertices with the rim held fixed
(``fair_vertices``).  Behind options: Liepa's angle-and-area weight for the triangulation
(``metric="angle_area"``) and a thin-plate solve after the membrane (``fair_vertices_curvature``, ``fairing="curvature"``).
Restated from the published methods [UNVERIFIED-UPSTREAM]: MeshLib is not available to compare with and its output cannot be
pinned; its own universal-metric formula is NOT built.  The oracles are tests/meshfill_restatement.py,
tests/meshtri_restatement.py and tests/meshsmooth_restatement.py, bit for bit.  There is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from ._lib import load, ptr, require_gpu, run
from .meshclean import _attributes, _fan_patches, _fans, _holes, _limit, _mesh, mesh_edge_stats
from .meshmap import _prep
from .pointcloud import _positive32

# A patch of at most LDS_MAX_VERTICES free vertices runs all its iterations in one workgroup, both iterates in LDS (the mirror
# of MISPLAT_MESHFILL_LDS_VERTICES in include/misplat.h; DESIGN.md section 29.4 holds the arithmetic and the measurement).
# ENABLE_LDS_FAIR = False sends every patch through one launch per iteration: the default, because that path measured no
# slower on the timed meshes (section 29.5), whose large patches are above the cut-off.  Neither changes a result.
ENABLE_LDS_FAIR = False
LDS_MAX_VERTICES = 4096

# A hole loop of at most LDS_LOOP edges keeps the table of its minimum-area triangulation in a workgroup's LDS, a longer one, up to
# MAX_LOOP, in a workspace; beyond MAX_LOOP a loop gets the fan (the mirrors of MISPLAT_MESHTRI_LDS_LOOP and
# MISPLAT_MESHTRI_MAX_LOOP in include/misplat.h; DESIGN.md section 30.4 holds the arithmetic).  Loops of at most SMALL_LOOP edges
# (MISPLAT_MESHTRI_SMALL_LOOP) run in a smaller workgroup; none of the three changes a result.
LDS_LOOP = 176
MAX_LOOP = 1024
SMALL_LOOP = 64
# The angle-and-area weight of ``triangulate_holes(metric="angle_area")`` keeps 12 bytes an entry and 28 a polygon vertex: its
# table fits a workgroup's LDS up to ANGLE_LDS_LOOP edges (MISPLAT_MESHTRI_ANGLE_LDS_LOOP; DESIGN.md section 31.2 holds the
# arithmetic).  ANGLE_STEPS (MISPLAT_MESHTRI_ANGLE_STEPS) is the number of buckets a crease's badness is quantised to.
ANGLE_LDS_LOOP = 163
ANGLE_STEPS = 1024
METRICS = ("area", "angle_area")
# fair_vertices_curvature leaves a patch of more free vertices unchanged (MISPLAT_MESHFILL_CG_VERTICES: a stated limit of the
# one-workgroup-per-patch solve, not a measurement).
CG_VERTICES = 65536
FAIRINGS = ("membrane", "curvature")


def _count(name: str, what: str, x) -> int:
    if not isinstance(x, int) or isinstance(x, bool) or x < 0:
        raise ValueError(f"{name}: {what} must be a non-negative integer, got {x!r}")
    return x


def _grown(x: Tensor, rows: int) -> Tensor:
    """x with room for at least `rows` rows (at least doubled: a round adds to four arrays, rarely to their storage)."""
    if x.shape[0] >= rows:
        return x
    out = torch.empty((max(rows, 2 * x.shape[0]),) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    out[:x.shape[0]] = x
    return out


# ------------------------------------------------------------------------------------------------------ subdivision
def subdivide_mesh(vertices: Tensor, triangles: Tensor, max_edge_len: float, max_edge_splits: int = 10000,
                   region: Optional[Tensor] = None, attributes: Sequence[Tensor] = (), max_rounds: int = 256
                   ) -> Tuple[Tensor, Tensor, Tuple[Tensor, ...], Tensor, int, int]:
    """Longest-edge bisection of the faces of ``region`` (bool [T]; None: all) until no splittable edge is longer than
    ``max_edge_len``: ``(vertices', triangles', attributes', origin [T'] int64, n_splits, rounds)``.

    An undirected edge is splittable iff it has one incident face or two distinct ones, every incident face is in the region
    and has three distinct corners, and its fp32 length sqrt((dx dx + dy dy) + dz dz) is > float32(max_edge_len): an edge
    between a region face and another face is never split, nor is a non-manifold edge.  Priority: the larger length bits,
    then the smaller ``mix32(lo, hi, 0)`` (a fixed mixing of the edge's ends: the spokes of a regular fan are equal to the
    bit), then the smaller key.  Each round splits every splittable edge that is first in priority among the splittable edges
    of each of its faces (such edges share no face); the round that would exceed ``max_edge_splits`` splits only the first in
    priority that still fit, and is the last.  Selected edge number s (numbered over the (face, corner) slots, each edge at
    the lowest corner of its smallest face) creates vertex M + s at ``0.5 (x_lo + x_hi)``, every attribute ([M,D] float32)
    the same; face f = (a, b, c), rotated so that a -> b is the edge, becomes (a, m, c) in its slot and (m, b, c) in slot T +
    rank(f): orientation is kept, faces that are not split keep their slot and their bits.  ``origin[f']`` is the input face
    an output face descends from; the triangles come back in the dtype they came in.  One host read per round (the numbers of
    selected edges and split faces), one more in a round cut by the budget.  Two runs are bitwise equal.

    MeshLib's ``subdivideMesh`` also flips edges while it splits; here the flips are ``flip_edges``, which ``fill_holes_nicely``
    runs between subdivisions."""
    name = "subdivide_mesh"
    v, t = _mesh(name, vertices, triangles)
    attributes = _attributes(name, attributes, v.shape[0], True)
    max_len = _positive32(name, "max_edge_len", max_edge_len)
    budget = _count(name, "max_edge_splits", max_edge_splits)
    max_rounds = _count(name, "max_rounds", max_rounds)
    m, n = v.shape[0], t.shape[0]
    if region is not None and (not isinstance(region, Tensor) or region.dtype != torch.bool or tuple(region.shape) != (n,)):
        raise ValueError(f"{name}: region must be a bool tensor [{n}]")
    if sum(a.shape[1] for a in attributes) > 4096:
        raise ValueError(f"{name}: {sum(a.shape[1] for a in attributes)} attribute channels in all, the limit is 4096")
    if 6 * (n + 2 * budget) >= (1 << 31) - 4096 or m + budget >= 1 << 31:
        raise ValueError(f"{name}: {n} triangles and {budget} splits are beyond the library's limits "
                         f"(6 (T + 2 max_edge_splits) < 2^31 - 4096)")
    require_gpu(vertices, triangles, region, *attributes)
    dev = v.device
    widths = [a.shape[1] for a in attributes]
    d = sum(widths)
    pos, tri = v.clone(), t.clone()
    att = torch.cat([_prep(a) for a in attributes], 1).contiguous() if d else None
    reg = (torch.ones(n, dtype=torch.uint8, device=dev) if region is None else region.detach().to(torch.uint8)).contiguous()
    origin = torch.arange(n, dtype=torch.int32, device=dev)
    n_splits = rounds = 0
    if n > 0 and budget > 0:
        lib = load()
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        ws, ws_faces = None, 0
        while rounds < max_rounds and n_splits < budget:
            if ws is None or n > ws_faces:
                ws_faces = 2 * n
                ws = torch.empty(int(lib.misplat_meshfill_workspace(m, ws_faces)), dtype=torch.uint8, device=dev)
            # (the workspace is carved for the current n: both calls of a round see the same layout)
            b = int(lib.misplat_meshfill_workspace(m, n))
            run("misplat_meshfill_round", ptr(pos), m, ptr(tri), n, ptr(reg), max_len, ptr(ws), b, ptr(counts))
            n_sel, n_faces = counts.tolist()                        # the round's host read
            if n_sel == 0:
                break
            rounds += 1
            left = budget - n_splits
            cut = n_sel > left
            take = left if cut else n_sel
            pos, tri = _grown(pos, m + take), _grown(tri, n + min(n_faces, 2 * take))
            reg, origin = _grown(reg, tri.shape[0]), _grown(origin, tri.shape[0])
            if d:
                att = _grown(att, pos.shape[0])
            run("misplat_meshfill_apply", ptr(pos), m, ptr(tri), n, ptr(reg), ptr(origin), ptr(att), d, n_sel,
                take if cut else -1, ptr(ws), b, ptr(counts))
            if cut:
                n_faces = counts.tolist()[1]                        # the faces the edges that fitted split
            m, n, n_splits = m + take, n + n_faces, n_splits + take
            if cut:
                break
    out_att = tuple(x.contiguous() for x in torch.split(att[:m], widths, 1)) if d else ()
    return pos[:m].clone(), tri[:n].to(triangles.dtype), out_att, origin[:n].long(), n_splits, rounds


# ---------------------------------------------------------------------------------------------------------- fairing
def fair_vertices(vertices: Tensor, triangles: Tensor, free: Tensor, tolerance: float, max_iterations: int = 10000,
                  attributes: Sequence[Tensor] = ()) -> Tuple[Tensor, Tuple[Tensor, ...], Tensor]:
    """Membrane fairing of the ``free`` vertices (bool [M]; every other vertex is fixed): ``(vertices', attributes',
    iterations [P] int32)``.

    A patch is a connected set of free vertices, joined by mesh edges whose ends are both free; patches are numbered by their
    smallest vertex.  Per patch, Jacobi iteration from the previous iterate: a free vertex i with distinct edge-neighbours
    N(i), free or fixed, in ascending index moves to ``fp32(sum_j (double) x_j / |N(i)|)``, the sum in fp64 in that order; a free
    vertex with no neighbour is unchanged.  The patch stops after the first iteration whose displacement, the maximum over
    its vertices and coordinates of ``|x_i' - x_i|`` in fp32, is < float32(tolerance), or after ``max_iterations``;
    ``iterations[p]`` is the count.  Every attribute ([M,D] float32) takes exactly ``iterations[p]`` iterations of the same
    operator and has no part in the test.  The host reads the patches' state every 32 iterations.  Two runs are bitwise
    equal."""
    name = "fair_vertices"
    v, t = _mesh(name, vertices, triangles)
    attributes = _attributes(name, attributes, v.shape[0], True)
    m, n = v.shape[0], t.shape[0]
    if not isinstance(free, Tensor) or free.dtype != torch.bool or tuple(free.shape) != (m,):
        raise ValueError(f"{name}: free must be a bool tensor [{m}]")
    tol = _positive32(name, "tolerance", tolerance)
    max_iterations = _count(name, "max_iterations", max_iterations)
    if max_iterations >= (1 << 31) - 64:
        raise ValueError(f"{name}: max_iterations must be below 2^31 - 64, got {max_iterations}")
    if sum(a.shape[1] for a in attributes) > 4096:
        raise ValueError(f"{name}: {sum(a.shape[1] for a in attributes)} attribute channels in all, the limit is 4096")
    if 6 * n >= (1 << 31) - 4096:
        raise ValueError(f"{name}: {n} triangles are beyond the library's limits (6 T < 2^31 - 4096)")
    require_gpu(vertices, triangles, free, *attributes)
    dev = v.device
    attributes = tuple(_prep(a) for a in attributes)
    none = torch.zeros(0, dtype=torch.int32, device=dev)
    if m == 0:
        return v.clone(), tuple(a.clone() for a in attributes), none
    lib = load()
    fr = free.detach().contiguous().view(torch.uint8)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)

    def workspace(n_free, n_edges):
        return torch.empty(int(lib.misplat_meshfill_fair_workspace(m, n, n_free, n_edges)), dtype=torch.uint8, device=dev)

    ws = workspace(0, 0)
    run("misplat_meshfill_fair_count", ptr(t), n, ptr(fr), m, ptr(ws), ws.numel(), ptr(counts))
    n_free, n_edges = counts.tolist()[:2]                           # the free vertices and the directed edges that leave them
    if n_free == 0:
        return v.clone(), tuple(a.clone() for a in attributes), none
    ws = workspace(n_free, n_edges)
    iters = torch.empty(n_free, dtype=torch.int32, device=dev)
    run("misplat_meshfill_fair_build", ptr(t), n, ptr(fr), m, n_free, n_edges, ptr(ws), ws.numel(), ptr(iters), ptr(counts))

    def step(a, b, first, count, fixed):
        """Iterations first .. first + count - 1: an odd one reads a and writes b, an even one the other way."""
        run("misplat_meshfill_fair_step", ptr(a), ptr(b), m, n, a.shape[1], n_free, n_edges, first, count, tol,
            int(fixed), ptr(ws), ws.numel(), ptr(iters), ptr(counts))

    pos = v.clone()
    n_patches = counts.tolist()[2]
    left = n_patches                                                # the patches that still have to run
    if ENABLE_LDS_FAIR and max_iterations > 0:
        run("misplat_meshfill_fair_lds", ptr(pos), m, n, n_free, n_edges, n_patches, tol, max_iterations, ptr(ws),
            ws.numel(), ptr(iters), ptr(counts))
        left = counts.tolist()[3]                                   # the patches too large for a workgroup's LDS
    done = 0
    other = pos.clone() if left and max_iterations > 0 else None    # (after the LDS path: what it has finished is in both)
    while left and done < max_iterations:
        batch = min(32, max_iterations - done)
        step(pos, other, done + 1, batch, False)
        done += batch
        left = counts.tolist()[3]                                   # the patches that are still running
    run("misplat_meshfill_fair_finish", n_free, done, ptr(iters), ptr(counts))
    if done & 1:
        pos = other
    iterations = iters[:n_patches].clone()
    out = []
    most = int(iterations.max()) if attributes else 0               # attributes: the same operator, iterations[p] times per patch
    for a in attributes:
        a = a.clone()
        b = a.clone() if most else None
        for first in range(1, most + 1, 1024):
            step(a, b, first, min(1024, most - first + 1), True)
        out.append(b if most & 1 else a)
    return pos, tuple(out), iterations


# ------------------------------------------------------------------------------------------------ curvature fairing
def fair_vertices_curvature(vertices: Tensor, triangles: Tensor, free: Tensor, rtol: float = 1e-6,
                            max_iterations: Optional[int] = None) -> Tuple[Tensor, dict]:
    """Thin-plate fairing of the ``free`` vertices (bool [M]; every other vertex is fixed): ``(vertices', info)``.  Positions
    only.

    N(i) is ``fair_vertices``'s distinct edge-neighbours of vertex i in ascending order, n_i their number; F the free set, R the
    fixed vertices with a free neighbour, S their union.  The umbrella ``U_i(x) = (sum_{j in N(i)} x_j) / (double) n_i - x_i`` is
    taken in fp64 (fixed coordinates are the doubles of their fp32), and the energy ``sum_{i in S} |U_i|^2`` is minimised over
    the free coordinates: ``A x_F = b`` with ``A = L^T L``, L the rows of S and the columns of F of the umbrella operator,
    symmetric positive definite whenever the patch has a fixed neighbour.  A patch is a connected set of free vertices, two
    being connected when they are adjacent or share a neighbour in R (two holes that share a rim vertex are one patch: every
    row of R belongs to exactly one); patches are numbered by their smallest free vertex.

    Per patch, plain conjugate gradients without a preconditioner, all state fp64, from the input positions; the result is
    rounded to fp32 once.  The three coordinates are three independent CGs (a column whose ``p.q`` is 0 takes alpha = beta = 0)
    with one stop: after iteration k, iff ``sum_c r_c.r_c <= rtol^2 sum_c r0_c.r0_c`` (0 iterations if the right-hand side is 0),
    or at ``max_iterations`` (None: the patch's free count, CG's own bound in exact arithmetic).  Applying A to p is two gathers
    over the same rows, ``t_i = (sum_{j in N(i) and F} p_j) / n_i - [i in F] p_i`` over S and ``q_i = (sum_{j in N(i)} t_j / n_j) -
    t_i`` over F; dot products are summed in a fixed order.  One workgroup runs a patch's whole solve: no host read and no launch
    inside the iteration.  ``info``: ``iterations`` [P] int32, ``converged`` [P] bool, ``residual`` [P] fp64 (the square root of
    the final ratio) and ``code`` [P] int32: 0 solved; 1 no neighbour at all, 2 no fixed neighbour (a closed free component), 3
    more than ``CG_VERTICES`` free vertices (a stated limit) -- all three unchanged.  The CSR of the rows of S and the lists by
    patch are index plumbing on the device (sorts, scans); the components and the solve are csrc/meshfill.hip's.  Two runs are
    bitwise equal."""
    name = "fair_vertices_curvature"
    v, t = _mesh(name, vertices, triangles)
    m = v.shape[0]
    if not isinstance(free, Tensor) or free.dtype != torch.bool or tuple(free.shape) != (m,):
        raise ValueError(f"{name}: free must be a bool tensor [{m}]")
    try:
        rtol = float(rtol)
    except (TypeError, ValueError):
        rtol = math.nan
    if not (0.0 <= rtol < math.inf):
        raise ValueError(f"{name}: rtol must be a finite number >= 0")
    if max_iterations is not None:
        max_iterations = _count(name, "max_iterations", max_iterations)
        if max_iterations >= 1 << 31:
            raise ValueError(f"{name}: max_iterations must be below 2^31, got {max_iterations}")
    if 6 * t.shape[0] >= (1 << 31) - 4096:
        raise ValueError(f"{name}: {t.shape[0]} triangles are beyond the library's limits (6 T < 2^31 - 4096)")
    require_gpu(vertices, triangles, free)
    dev = v.device
    i32 = dict(dtype=torch.int32, device=dev)
    fr = free.detach().contiguous()
    flist = torch.nonzero(fr).view(-1)                              # ascending
    n_free = flist.shape[0]
    if n_free == 0:
        return v.clone(), {"iterations": torch.zeros(0, **i32), "converged": torch.zeros(0, dtype=torch.bool, device=dev),
                           "residual": torch.zeros(0, dtype=torch.float64, device=dev), "code": torch.zeros(0, **i32)}
    lib = load()
    # the directed edges that leave a row of S, distinct, by source and then by target
    tl = t.long()
    src, tgt = tl[:, [0, 1, 2, 1, 2, 0]].reshape(-1), tl[:, [1, 2, 0, 0, 1, 2]].reshape(-1)
    keep = src != tgt
    src, tgt = src[keep], tgt[keep]
    in_r = torch.zeros(m, dtype=torch.bool, device=dev)
    in_r[src[fr[tgt]]] = True
    in_r &= ~fr
    keep = (fr | in_r)[src]
    key = torch.unique(src[keep] * m + tgt[keep])                   # sorted
    es, et = (key // m).to(torch.int32), (key % m).to(torch.int32)
    n_entries = es.shape[0]
    parent = torch.arange(m, **i32)
    root = torch.empty(m, **i32)
    run("misplat_meshfill_curv_patches", ptr(es), ptr(et), n_entries, ptr(fr.view(torch.uint8)), m, ptr(parent), ptr(root))
    # patches by their smallest free vertex; the free vertices and the rows of R by patch and then by vertex
    roots, of_free = torch.unique(root[flist].long(), return_inverse=True)
    n_patches = roots.shape[0]
    first = torch.full((n_patches,), m, dtype=torch.int64, device=dev).scatter_reduce(0, of_free, flist, "amin")
    rank = torch.empty(n_patches, dtype=torch.int64, device=dev)
    rank[torch.argsort(first)] = torch.arange(n_patches, device=dev)
    patch_of_root = torch.full((m,), -1, dtype=torch.int64, device=dev)
    patch_of_root[roots] = rank
    rlist = torch.nonzero(in_r).view(-1)
    pf, pr = rank[of_free], patch_of_root[root[rlist].long()]
    flist, rlist = flist[torch.sort(pf, stable=True).indices], rlist[torch.sort(pr, stable=True).indices]
    n_f, n_r = torch.bincount(pf, minlength=n_patches), torch.bincount(pr, minlength=n_patches)
    foff, roff = torch.zeros(n_patches + 1, **i32), torch.zeros(n_patches + 1, **i32)
    foff[1:], roff[1:] = torch.cumsum(n_f, 0), torch.cumsum(n_r, 0)
    slist = torch.cat([flist, rlist])
    n_rows = slist.shape[0]
    place_of = torch.full((m,), -1, **i32)
    place_of[slist] = torch.arange(n_rows, **i32)
    degree_of = torch.bincount(es.long(), minlength=m)
    start_of = torch.cumsum(degree_of, 0) - degree_of
    has_degree = torch.zeros(n_patches, dtype=torch.bool, device=dev)
    has_degree[pf[degree_of[torch.nonzero(fr).view(-1)] > 0]] = True
    code = torch.where(~has_degree, 1, torch.where(n_r == 0, 2, torch.where(n_f > CG_VERTICES, 3, 0))).to(torch.int32)
    ws = torch.empty(int(lib.misplat_meshfill_curv_workspace(n_free, n_rows)), dtype=torch.uint8, device=dev)
    out = v.clone()
    iterations = torch.empty(n_patches, **i32)
    converged = torch.empty(n_patches, dtype=torch.uint8, device=dev)
    residual = torch.empty(n_patches, dtype=torch.float64, device=dev)
    vertex, row, degree = slist.to(torch.int32), start_of[slist].to(torch.int32), degree_of[slist].to(torch.int32)
    place = place_of[et.long()].contiguous()
    run("misplat_meshfill_curv_solve", ptr(v), ptr(out), m, ptr(foff), ptr(roff), ptr(vertex), ptr(row), ptr(degree), ptr(et),
        ptr(place), n_free, n_rows, n_entries, ptr(code), n_patches, rtol, -1 if max_iterations is None else max_iterations,
        ptr(ws), ws.numel(), ptr(iterations), ptr(converged), ptr(residual))
    return out, {"iterations": iterations, "converged": converged.bool(), "residual": residual, "code": code}


# --------------------------------------------------------------------------------------------------------- the fill
def fill_holes_nicely(vertices: Tensor, triangles: Tensor, max_hole_size: float = 3.0, max_edge_len: Optional[float] = None,
                      max_edge_splits: int = 10000, tolerance: Optional[float] = None, max_iterations: int = 10000,
                      attributes: Sequence[Tensor] = (), triangulation: str = "fan", flip: bool = False, max_passes: int = 4,
                      metric: str = "area", fairing: str = "membrane") -> Tuple[Tensor, Tensor, Tuple[Tensor, ...], int, dict]:
    """``fill_holes`` whose patches are subdivided to the mesh's edge length and faired: ``(vertices', triangles', attributes',
    n_filled, info)``; ``info`` holds ``n_splits``, ``rounds``, ``iterations`` ([P] int32, one entry per patch of created
    vertices), ``n_new_vertices``, ``n_flips``, ``flip_rounds``, ``passes``, ``n_triangulated`` and ``n_fans``.

    The same loops as ``fill_holes``, closed by its fans (``triangulation="fan"``) or by ``triangulate_holes``
    (``"min_area"``: a fan only where a loop cannot be triangulated); then ``subdivide_mesh`` with ``region`` = the faces the call
    created (a rim edge has a face outside the region: no input face changes) and ``fair_vertices`` with ``free`` = every vertex
    the call created, the fans' centres and the split midpoints.  ``flip=True`` runs up to ``max_passes`` passes of
    ``subdivide_mesh`` followed by ``flip_edges`` over the region (which follows ``origin`` through the subdivision), and stops
    after the pass whose ``flip_edges`` made no flip or when the split budget is spent; the fairing runs once, at the end.
    ``max_edge_len=None`` is the input mesh's ``mean_edge_length``, measured before the fill (the reference's order,
    mesh.py:386-390); ``tolerance=None`` is ``1e-3 max_edge_len`` (a chosen default).  The reference's ``maxEdgeSplits`` is per
    hole; here the call's total is ``max_edge_splits * n_filled``, the same worst case: a single hole may take more than its
    share.  The input's vertices and faces are a bit-identical prefix of the output; loops at or above ``max_hole_size`` are
    untouched.  The defaults (``"fan"``, no flips, ``"area"``, ``"membrane"``) give what they always gave, bit for bit.

    ``metric="angle_area"`` is passed to ``triangulate_holes`` (it needs ``triangulation="min_area"``).  ``fairing="curvature"``
    runs ``fair_vertices`` as above, which yields the attributes and the start of the solve, and then
    ``fair_vertices_curvature`` on the same free set: the patch continues the rim's tangent planes instead
    of spanning it like a membrane; a patch whose ``curvature_code`` is not 0 keeps the membrane's result.  ``info`` then gains
    ``curvature_iterations``, ``curvature_converged`` and ``curvature_code``.

    This stands where MeshLib's ``fillHoleNicely`` stands in the reference, restated from the published methods (minimum-area
    triangulation and Liepa's angle-and-area weight, longest-edge bisection, Delaunay flips, membrane and thin-plate fairing
    with the rim fixed): MeshLib's own universal-metric formula is not built, and nothing here can be compared with MeshLib's
    output."""
    name = "fill_holes_nicely"
    v, t = _mesh(name, vertices, triangles)
    attributes = _attributes(name, attributes, v.shape[0], True)
    limit = _limit(name, max_hole_size)
    if max_edge_len is not None:
        max_edge_len = _positive32(name, "max_edge_len", max_edge_len)
    if tolerance is not None:
        tolerance = _positive32(name, "tolerance", tolerance)
    per_hole = _count(name, "max_edge_splits", max_edge_splits)
    max_iterations = _count(name, "max_iterations", max_iterations)
    if triangulation not in ("fan", "min_area"):
        raise ValueError(f"{name}: triangulation must be 'fan' or 'min_area', got {triangulation!r}")
    if metric not in METRICS:
        raise ValueError(f"{name}: metric must be 'area' or 'angle_area', got {metric!r}")
    if metric != "area" and triangulation != "min_area":
        raise ValueError(f"{name}: metric={metric!r} needs triangulation='min_area'")
    if fairing not in FAIRINGS:
        raise ValueError(f"{name}: fairing must be 'membrane' or 'curvature', got {fairing!r}")
    max_passes = _count(name, "max_passes", max_passes)
    if flip and max_passes < 1:
        raise ValueError(f"{name}: max_passes must be at least 1 with flip=True, got {max_passes}")
    require_gpu(vertices, triangles, *attributes)
    attributes = tuple(_prep(a) for a in attributes)
    m, n = v.shape[0], t.shape[0]
    info = {"n_splits": 0, "rounds": 0, "iterations": torch.zeros(0, dtype=torch.int32, device=v.device), "n_new_vertices": 0,
            "n_flips": 0, "flip_rounds": 0, "passes": 0, "n_triangulated": 0, "n_fans": 0}
    if fairing == "curvature":
        info.update(curvature_iterations=torch.zeros(0, dtype=torch.int32, device=v.device),
                    curvature_converged=torch.zeros(0, dtype=torch.bool, device=v.device),
                    curvature_code=torch.zeros(0, dtype=torch.int32, device=v.device))
    if triangulation == "min_area":
        filled = _triangulated(v, t, attributes, limit, metric) if n else None
    else:
        filled = _fans(v, t, attributes, limit) if n else None
    if filled is None:
        return v, t.to(triangles.dtype), attributes, 0, info
    if max_edge_len is None:
        max_edge_len = _positive32(name, "the mesh's mean edge length", mesh_edge_stats(v, t)["mean_edge_length"])
    if tolerance is None:
        tolerance = _positive32(name, "tolerance", 1e-3 * max_edge_len)
    v3, t3, a3, n_filled = filled[:4]
    n_triangulated = filled[4]["n_triangulated"] if triangulation == "min_area" else 0
    region = torch.arange(t3.shape[0], device=v.device) >= n
    budget = per_hole * n_filled
    n_splits = rounds = n_flips = flip_rounds = passes = 0
    while True:
        passes += 1
        v3, t3, a3, origin, k, r = subdivide_mesh(v3, t3, max_edge_len, budget - n_splits, region, a3)
        n_splits, rounds = n_splits + k, rounds + r
        if not flip:
            break
        region = region[origin]
        t3, k, r = flip_edges(v3, t3, region)
        n_flips, flip_rounds = n_flips + k, flip_rounds + r
        if k == 0 or n_splits >= budget or passes >= max_passes:
            break
    free = torch.arange(v3.shape[0], device=v.device) >= m
    v4, a4, iterations = fair_vertices(v3, t3, free, tolerance, max_iterations, a3)
    info.update(n_splits=n_splits, rounds=rounds, iterations=iterations, n_new_vertices=v4.shape[0] - m, n_flips=n_flips,
                flip_rounds=flip_rounds, passes=passes, n_triangulated=n_triangulated, n_fans=n_filled - n_triangulated)
    if fairing == "curvature":
        v4, cinfo = fair_vertices_curvature(v4, t3, free)
        info.update(curvature_iterations=cinfo["iterations"], curvature_converged=cinfo["converged"], curvature_code=cinfo["code"])
    return v4, t3.to(triangles.dtype), a4, n_filled, info


# ---------------------------------------------------------------------------------------------------- triangulation
def triangulate_holes(vertices: Tensor, triangles: Tensor, max_hole_size: float = 3.0, attributes: Sequence[Tensor] = (),
                      metric: str = "area") -> Tuple[Tensor, Tensor, Tuple[Tensor, ...], int, dict]:
    """Close every loop of ``mesh_holes`` whose perimeter is below ``max_hole_size`` with the triangulation of its polygon of
    least total area: ``(vertices', triangles', attributes', n_filled, info)``.

    A loop of n boundary edges is triangulated iff it is a simple cycle (its n tails are distinct, its n heads are distinct
    and they are the same vertices: every vertex has one outgoing and one incoming edge of the loop) and ``3 <= n <=
    MAX_LOOP``; every other loop -- pinched, two edges, too long -- gets ``fill_holes``'s fan, the same appended vertex and the
    same faces.  The polygon: p_0 the loop's smallest vertex, p_{i+1} the head of the edge whose tail is p_i (edges run as
    their face does), q_0 = p_0, q_i = p_{n-i}; a face (q_i, q_k, q_j), i < k < j, is then oriented like the faces around it.
    ``W[i][i+1] = 0``, ``W[i][j] = min over i < k < j of ((W[i][k] + W[k][j]) + (double) A(i,k,j))`` in fp64, the first minimum
    in ascending k, A the fp32 area ``0.5f sqrtf((cx cx + cy cy) + cz cz)`` of the cross product of ``q_k - q_i`` and ``q_j -
    q_i``.  Loops go in rank order; a triangulated loop contributes its n - 2 faces by ascending apex k = 1 .. n - 2 (every k
    is the apex of exactly one face of the optimal tree) and creates no vertex; the input is a bit-identical prefix of the
    output, and where every loop falls back the result is ``fill_holes``'s.  ``info``: ``n_triangulated``, ``n_fans``, ``area``
    ([n_triangulated] fp64, the minima W[0][n-1]) and ``fallback`` (int32 per filled loop: 0 triangulated, 1 not simple, 2 too
    short, 3 too long).  Two host reads: the counts of ``mesh_holes`` and the counts of the classification.  Two runs are
    bitwise equal.

    ``metric="angle_area"`` (Liepa's angle-and-area weight restated) keeps the loops, the polygon, the
    fallback codes and the face order and weighs a table entry by the pair (b, a): a the area sum above, b the integer badness
    of the sharpest crease among the entry's faces and against the rim.  The badness of two oriented faces with fp64 cross
    products n1, n2 (edge vectors in fp64 from the fp32 coordinates, dots as ``(x x' + y y') + z z'``) is ``clamp((int)
    floor((1 - c) * 0.5 * ANGLE_STEPS), 0, ANGLE_STEPS)``, ``c = dot(n1, n2) / sqrt(dot(n1, n1) dot(n2, n2))``, and 0 where
    either squared length is 0.  Candidate k of entry (i, j), face T = (q_i, q_k, q_j): its neighbour across (i, k) is the rim
    face ``(q_{i+1}, q_i, o_i)`` if k - i = 1 (o_i the third corner of the mesh face that holds that boundary edge), else ``(q_i,
    q_{S[i][k]}, q_k)`` with S the stored split, and likewise across (k, j); ``b = max(W[i][k].b, W[k][j].b, bad(T, left),
    bad(T, right))``, for the top entry (0, n - 1) also ``bad(T, (q_0, q_{n-1}, o_{n-1}))``.  Entries compare lexicographically
    on (b, a) with a strict < in ascending k: on a nearly flat hole every crease falls into bucket 0 (bucket 1 starts at about
    3.6 degrees) and the area decides.  An entry's neighbour is what its sub-problem chose: the recurrence, not a global optimum.
    ``info`` gains ``badness`` (int32 per triangulated loop, the top entry's b)."""
    name = "triangulate_holes"
    v, t = _mesh(name, vertices, triangles)
    attributes = _attributes(name, attributes, v.shape[0], True)
    limit = _limit(name, max_hole_size)
    if metric not in METRICS:
        raise ValueError(f"{name}: metric must be 'area' or 'angle_area', got {metric!r}")
    require_gpu(vertices, triangles, *attributes)
    attributes = tuple(_prep(a) for a in attributes)
    filled = _triangulated(v, t, attributes, limit, metric) if t.shape[0] else None
    if filled is None:
        none = {"n_triangulated": 0, "n_fans": 0, "area": torch.zeros(0, dtype=torch.float64, device=v.device),
                "fallback": torch.zeros(0, dtype=torch.int32, device=v.device)}
        if metric == "angle_area":
            none["badness"] = torch.zeros(0, dtype=torch.int32, device=v.device)
        return v, t.to(triangles.dtype), attributes, 0, none
    return filled[0], filled[1].to(triangles.dtype), filled[2], filled[3], filled[4]


def _triangulated(v: Tensor, t: Tensor, attributes: Tuple[Tensor, ...], limit: float, metric: str = "area"):
    """``triangulate_holes`` over a prepared mesh with at least one face: (vertices, triangles int64, attributes, n_filled,
    info), or None where no loop is below the limit."""
    dev = v.device
    loop, edges, n_edges, perimeter, order = _holes(v, t)
    n_loops, n_boundary = n_edges.shape[0], edges.shape[0]
    if n_loops == 0:
        return None
    lib = load()
    fill = perimeter < limit
    offsets = torch.zeros(n_loops + 1, dtype=torch.int32, device=dev)
    offsets[1:] = torch.cumsum(n_edges, 0)
    code = torch.empty(n_loops, dtype=torch.int32, device=dev)
    polygon = torch.empty(n_boundary, dtype=torch.int32, device=dev)
    angle = metric == "angle_area"
    if angle:
        if 6 * t.shape[0] >= (1 << 31) - 4096:
            raise ValueError(f"triangulate_holes: {t.shape[0]} triangles are beyond the library's limits (6 T < 2^31 - 4096)")
        rim = torch.empty(n_boundary, dtype=torch.int32, device=dev)
        ws = torch.empty(int(lib.misplat_meshtri_rim_workspace(t.shape[0])), dtype=torch.uint8, device=dev)
        run("misplat_meshtri_order_rim", ptr(edges), ptr(order), ptr(offsets), ptr(fill.view(torch.uint8)), n_boundary, n_loops,
            ptr(t), t.shape[0], ptr(ws), ws.numel(), ptr(code), ptr(polygon), ptr(rim))
    else:
        run("misplat_meshtri_order", ptr(edges), ptr(order), ptr(offsets), ptr(fill.view(torch.uint8)), n_boundary, n_loops,
            ptr(code), ptr(polygon))
    lds_loop = ANGLE_LDS_LOOP if angle else LDS_LOOP
    n = n_edges.long()
    tri, fan = code == 0, code > 0
    faces_of = torch.where(tri, n - 2, torch.where(fan, n, torch.zeros_like(n)))
    face_base = (torch.cumsum(faces_of, 0) - faces_of).to(torch.int32)
    area_slot = (torch.cumsum(tri, 0) - 1).to(torch.int32)
    entries = torch.where(tri & (n > lds_loop), n * (n - 1) // 2, torch.zeros_like(n))
    slab_offset = torch.cumsum(entries, 0) - entries
    small, medium = tri & (n <= SMALL_LOOP), tri & (n > SMALL_LOOP) & (n <= lds_loop)
    n_tri, n_fans, n_faces, n_entries, n_small, n_medium = torch.stack(
        [tri.sum(), fan.sum(), faces_of.sum(), entries.sum(), small.sum(), medium.sum()]).tolist()    # the call's second host read
    if n_tri + n_fans == 0:
        return None
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    area = torch.empty(n_tri, dtype=torch.float64, device=dev)
    badness = torch.empty(n_tri, dtype=torch.int32, device=dev) if angle else None
    if n_tri:
        paths = (1 if n_small else 0) | (2 if n_medium else 0) | (4 if n_entries else 0)
        ws = None
        if n_entries:
            size = lib.misplat_meshtri_angle_workspace if angle else lib.misplat_meshtri_workspace
            ws = torch.empty(int(size(n_entries)), dtype=torch.uint8, device=dev)
    if n_tri and angle:
        run("misplat_meshtri_angle_dp", ptr(v), v.shape[0], ptr(polygon), ptr(rim), ptr(offsets), ptr(code), n_loops, paths,
            ptr(slab_offset), n_entries, ptr(ws), ws.numel() if n_entries else 0, ptr(face_base), n_faces, ptr(area_slot),
            n_tri, ptr(faces), ptr(area), ptr(badness))
    elif n_tri:
        run("misplat_meshtri_dp", ptr(v), v.shape[0], ptr(polygon), ptr(offsets), ptr(code), n_loops, paths, ptr(slab_offset),
            n_entries, ptr(ws), ws.numel() if n_entries else 0, ptr(face_base), n_faces, ptr(area_slot), n_tri, ptr(faces),
            ptr(area))
    outs = [v, *attributes]
    if n_fans:
        fans, fan_of, outs = _fan_patches(v, attributes, loop, edges, order, fan, n_fans)
        first = torch.cumsum(n[fan], 0) - n[fan]                    # where a fan's faces start among the fans' faces
        at = face_base[fan].long()[fan_of] + (torch.arange(fans.shape[0], device=dev) - first[fan_of])
        faces[at] = fans.to(torch.int32)
    info = {"n_triangulated": n_tri, "n_fans": n_fans, "area": area, "fallback": code[code >= 0].clone()}
    if angle:
        info["badness"] = badness
    return outs[0], torch.cat([t.long(), faces.long()]), tuple(outs[1:]), n_tri + n_fans, info


# ------------------------------------------------------------------------------------------------------------ flips
def flip_edges(vertices: Tensor, triangles: Tensor, region: Optional[Tensor] = None, max_rounds: int = 256,
               min_violation: float = 1e-9) -> Tuple[Tensor, int, int]:
    """Delaunay-like flips of the edges inside ``region`` (bool [T]; None: all faces) in rounds, until no edge is flippable:
    ``(triangles', n_flips, rounds)``.  Vertices are untouched, faces keep their slots.

    An undirected edge (lo, hi) is flippable iff it has exactly two distinct incident faces, both in the region and with three
    distinct corners; with f_min the smaller face index rotated to (a, b, c), a -> b the edge, f_max holds b -> a and the
    opposite corner d; c != d; the edge (c, d) is not in the round's mesh; the fp64 sum ``cot(c) + cot(d)`` is ``<
    -min_violation`` (each cotangent ``dot / |cross|`` of the two edge vectors at that corner, from the fp32 coordinates); and
    each new face's normal has a positive dot product with the sum of the two old faces' unnormalised normals (no fold is
    created).  ``min_violation`` is a chosen default: it keeps a co-circular pair, whose sum is 0 up to rounding, from flipping
    back and forth.  Priority: the larger fp64 bits of ``-(cot c + cot d)``, then the smaller ``mix32(lo, hi, 0)``, then the
    smaller key.  A round selects every flippable edge that is first in priority among the flippable edges of each of its two
    faces (selected edges share no face); of the selected edges that want to create the same new edge the smallest key flips,
    the others wait; a flip sets f_min <- (a, d, c) and f_max <- (d, b, c).  One host read per round, the flips applied; the
    call stops at 0 or after ``max_rounds`` (flips of a non-planar region are not proven to terminate).  Two runs are bitwise
    equal."""
    name = "flip_edges"
    v, t = _mesh(name, vertices, triangles)
    m, n = v.shape[0], t.shape[0]
    if region is not None and (not isinstance(region, Tensor) or region.dtype != torch.bool or tuple(region.shape) != (n,)):
        raise ValueError(f"{name}: region must be a bool tensor [{n}]")
    max_rounds = _count(name, "max_rounds", max_rounds)
    try:
        min_violation = float(min_violation)
    except (TypeError, ValueError):
        min_violation = math.nan
    if not (0.0 <= min_violation < math.inf):
        raise ValueError(f"{name}: min_violation must be a finite number >= 0")
    if 6 * n >= (1 << 31) - 4096:
        raise ValueError(f"{name}: {n} triangles are beyond the library's limits (6 T < 2^31 - 4096)")
    require_gpu(vertices, triangles, region)
    tri = t.clone()
    n_flips = rounds = 0
    if n > 0 and max_rounds > 0:
        lib = load()
        dev = v.device
        reg = (torch.ones(n, dtype=torch.uint8, device=dev) if region is None else region.detach().to(torch.uint8)).contiguous()
        counts = torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.empty(int(lib.misplat_meshtri_flip_workspace(m, n)), dtype=torch.uint8, device=dev)
        while rounds < max_rounds:
            run("misplat_meshtri_flip_round", ptr(v), m, ptr(tri), n, ptr(reg), min_violation, ptr(ws), ws.numel(), ptr(counts))
            k = int(counts.item())                                  # the round's host read
            if k == 0:
                break
            rounds += 1
            n_flips += k
    return tri.to(triangles.dtype), n_flips, rounds


__all__ = ["subdivide_mesh", "fair_vertices", "fair_vertices_curvature", "fill_holes_nicely", "triangulate_holes", "flip_edges"]
