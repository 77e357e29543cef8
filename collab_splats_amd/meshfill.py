"""Hole filling at the mesh's own resolution on the MI355X (csrc/meshfill.hip).

The reference's ``clean_repair_mesh`` (collab_splats/utils/mesh.py:359-407) closes every hole below ``max_hole_size`` with
MeshLib's ``fillHoleNicely`` (``maxEdgeLen`` = the mesh's average edge length, ``maxEdgeSplits`` = 10000; the fallback is
``fillHole`` + ``subdivideMesh`` + ``positionVertsSmoothly``, :317-356): the hole is triangulated by a metric, the patch is
subdivided to the mesh's edge length while its edges are flipped, and its new vertices are positioned smoothly.  Here the same
steps run on device tensors: the fan of ``fill_holes`` or the minimum-area triangulation of the loop (``triangulate_holes``,
csrc/meshtri.hip), longest-edge bisection of the patch's faces in rounds (``subdivide_mesh``), Delaunay-like
flips of its edges (``flip_edges``, section 30), membrane fairing of the created vertices with the rim held fixed
(``fair_vertices``).  Restated from the published methods [UNVERIFIED-UPSTREAM]: MeshLib is not available to compare with and
its output cannot be pinned; its universal metric (with a dihedral term) and its curvature fairing are NOT built.  The oracles
are tests/meshfill_restatement.py and tests/meshtri_restatement.py, bit for bit.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from ._lib import check, load, ptr, require_gpu, stream_ptr
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
                ws = torch.empty(int(lib.misplat_meshfill_workspace(C.c_int64(m), C.c_int64(ws_faces))), dtype=torch.uint8, device=dev)
            # (the workspace is carved for the current n: both calls of a round see the same layout)
            b = int(lib.misplat_meshfill_workspace(C.c_int64(m), C.c_int64(n)))
            check(lib.misplat_meshfill_round(ptr(pos), C.c_int64(m), ptr(tri), C.c_int64(n), ptr(reg), C.c_float(max_len), ptr(ws),
                                             C.c_int64(b), ptr(counts), stream_ptr()), "misplat_meshfill_round")
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
            check(lib.misplat_meshfill_apply(ptr(pos), C.c_int64(m), ptr(tri), C.c_int64(n), ptr(reg), ptr(origin), ptr(att), d,
                                             C.c_int64(n_sel), C.c_int64(take if cut else -1), ptr(ws), C.c_int64(b), ptr(counts),
                                             stream_ptr()), "misplat_meshfill_apply")
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
        return torch.empty(int(lib.misplat_meshfill_fair_workspace(C.c_int64(m), C.c_int64(n), C.c_int64(n_free), C.c_int64(n_edges))),
                           dtype=torch.uint8, device=dev)

    ws = workspace(0, 0)
    check(lib.misplat_meshfill_fair_count(ptr(t), C.c_int64(n), ptr(fr), C.c_int64(m), ptr(ws), C.c_int64(ws.numel()), ptr(counts),
                                          stream_ptr()), "misplat_meshfill_fair_count")
    n_free, n_edges = counts.tolist()[:2]                           # the free vertices and the directed edges that leave them
    if n_free == 0:
        return v.clone(), tuple(a.clone() for a in attributes), none
    ws = workspace(n_free, n_edges)
    iters = torch.empty(n_free, dtype=torch.int32, device=dev)
    sizes = (C.c_int64(m), C.c_int64(n))
    check(lib.misplat_meshfill_fair_build(ptr(t), sizes[1], ptr(fr), sizes[0], C.c_int64(n_free), C.c_int64(n_edges), ptr(ws),
                                          C.c_int64(ws.numel()), ptr(iters), ptr(counts), stream_ptr()), "misplat_meshfill_fair_build")

    def run(a, b, first, count, fixed):
        """Iterations first .. first + count - 1: an odd one reads a and writes b, an even one the other way."""
        check(lib.misplat_meshfill_fair_step(ptr(a), ptr(b), sizes[0], sizes[1], a.shape[1], C.c_int64(n_free), C.c_int64(n_edges),
                                             first, count, C.c_float(tol), int(fixed), ptr(ws), C.c_int64(ws.numel()), ptr(iters),
                                             ptr(counts), stream_ptr()), "misplat_meshfill_fair_step")

    pos = v.clone()
    n_patches = counts.tolist()[2]
    left = n_patches                                                # the patches that still have to run
    if ENABLE_LDS_FAIR and max_iterations > 0:
        check(lib.misplat_meshfill_fair_lds(ptr(pos), sizes[0], sizes[1], C.c_int64(n_free), C.c_int64(n_edges), n_patches,
                                            C.c_float(tol), max_iterations, ptr(ws), C.c_int64(ws.numel()), ptr(iters), ptr(counts),
                                            stream_ptr()), "misplat_meshfill_fair_lds")
        left = counts.tolist()[3]                                   # the patches too large for a workgroup's LDS
    done = 0
    other = pos.clone() if left and max_iterations > 0 else None    # (after the LDS path: what it has finished is in both)
    while left and done < max_iterations:
        batch = min(32, max_iterations - done)
        run(pos, other, done + 1, batch, False)
        done += batch
        left = counts.tolist()[3]                                   # the patches that are still running
    check(lib.misplat_meshfill_fair_finish(C.c_int64(n_free), done, ptr(iters), ptr(counts), stream_ptr()),
          "misplat_meshfill_fair_finish")
    if done & 1:
        pos = other
    iterations = iters[:n_patches].clone()
    out = []
    most = int(iterations.max()) if attributes else 0               # attributes: the same operator, iterations[p] times per patch
    for a in attributes:
        a = a.clone()
        b = a.clone() if most else None
        for first in range(1, most + 1, 1024):
            run(a, b, first, min(1024, most - first + 1), True)
        out.append(b if most & 1 else a)
    return pos, tuple(out), iterations


# --------------------------------------------------------------------------------------------------------- the fill
def fill_holes_nicely(vertices: Tensor, triangles: Tensor, max_hole_size: float = 3.0, max_edge_len: Optional[float] = None,
                      max_edge_splits: int = 10000, tolerance: Optional[float] = None, max_iterations: int = 10000,
                      attributes: Sequence[Tensor] = (), triangulation: str = "fan", flip: bool = False, max_passes: int = 4
                      ) -> Tuple[Tensor, Tensor, Tuple[Tensor, ...], int, dict]:
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
    untouched.  The defaults (``"fan"``, no flips) give what they always gave, bit for bit.

    This stands where MeshLib's ``fillHoleNicely`` stands in the reference, restated from the published methods (minimum-area
    triangulation, longest-edge bisection, Delaunay flips, membrane fairing with the rim fixed): MeshLib's universal metric and
    its curvature fairing are not built, and nothing here can be compared with MeshLib's output."""
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
    max_passes = _count(name, "max_passes", max_passes)
    if flip and max_passes < 1:
        raise ValueError(f"{name}: max_passes must be at least 1 with flip=True, got {max_passes}")
    require_gpu(vertices, triangles, *attributes)
    attributes = tuple(_prep(a) for a in attributes)
    m, n = v.shape[0], t.shape[0]
    info = {"n_splits": 0, "rounds": 0, "iterations": torch.zeros(0, dtype=torch.int32, device=v.device), "n_new_vertices": 0,
            "n_flips": 0, "flip_rounds": 0, "passes": 0, "n_triangulated": 0, "n_fans": 0}
    if triangulation == "min_area":
        filled = _triangulated(v, t, attributes, limit) if n else None
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
    return v4, t3.to(triangles.dtype), a4, n_filled, info


# ---------------------------------------------------------------------------------------------------- triangulation
def triangulate_holes(vertices: Tensor, triangles: Tensor, max_hole_size: float = 3.0, attributes: Sequence[Tensor] = ()
                      ) -> Tuple[Tensor, Tensor, Tuple[Tensor, ...], int, dict]:
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
    bitwise equal."""
    name = "triangulate_holes"
    v, t = _mesh(name, vertices, triangles)
    attributes = _attributes(name, attributes, v.shape[0], True)
    limit = _limit(name, max_hole_size)
    require_gpu(vertices, triangles, *attributes)
    attributes = tuple(_prep(a) for a in attributes)
    filled = _triangulated(v, t, attributes, limit) if t.shape[0] else None
    if filled is None:
        none = {"n_triangulated": 0, "n_fans": 0, "area": torch.zeros(0, dtype=torch.float64, device=v.device),
                "fallback": torch.zeros(0, dtype=torch.int32, device=v.device)}
        return v, t.to(triangles.dtype), attributes, 0, none
    return filled[0], filled[1].to(triangles.dtype), filled[2], filled[3], filled[4]


def _triangulated(v: Tensor, t: Tensor, attributes: Tuple[Tensor, ...], limit: float):
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
    check(lib.misplat_meshtri_order(ptr(edges), ptr(order), ptr(offsets), ptr(fill.view(torch.uint8)), C.c_int64(n_boundary),
                                    C.c_int64(n_loops), ptr(code), ptr(polygon), stream_ptr()), "misplat_meshtri_order")
    n = n_edges.long()
    tri, fan = code == 0, code > 0
    faces_of = torch.where(tri, n - 2, torch.where(fan, n, torch.zeros_like(n)))
    face_base = (torch.cumsum(faces_of, 0) - faces_of).to(torch.int32)
    area_slot = (torch.cumsum(tri, 0) - 1).to(torch.int32)
    entries = torch.where(tri & (n > LDS_LOOP), n * (n - 1) // 2, torch.zeros_like(n))
    slab_offset = torch.cumsum(entries, 0) - entries
    small, medium = tri & (n <= SMALL_LOOP), tri & (n > SMALL_LOOP) & (n <= LDS_LOOP)
    n_tri, n_fans, n_faces, n_entries, n_small, n_medium = torch.stack(
        [tri.sum(), fan.sum(), faces_of.sum(), entries.sum(), small.sum(), medium.sum()]).tolist()    # the call's second host read
    if n_tri + n_fans == 0:
        return None
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    area = torch.empty(n_tri, dtype=torch.float64, device=dev)
    if n_tri:
        paths = (1 if n_small else 0) | (2 if n_medium else 0) | (4 if n_entries else 0)
        ws = None
        if n_entries:
            ws = torch.empty(int(lib.misplat_meshtri_workspace(C.c_int64(n_entries))), dtype=torch.uint8, device=dev)
        check(lib.misplat_meshtri_dp(ptr(v), C.c_int64(v.shape[0]), ptr(polygon), ptr(offsets), ptr(code), C.c_int64(n_loops), paths,
                                     ptr(slab_offset), C.c_int64(n_entries), ptr(ws), C.c_int64(ws.numel() if n_entries else 0),
                                     ptr(face_base), C.c_int64(n_faces), ptr(area_slot), C.c_int64(n_tri), ptr(faces), ptr(area),
                                     stream_ptr()), "misplat_meshtri_dp")
    outs = [v, *attributes]
    if n_fans:
        fans, fan_of, outs = _fan_patches(v, attributes, loop, edges, order, fan, n_fans)
        first = torch.cumsum(n[fan], 0) - n[fan]                    # where a fan's faces start among the fans' faces
        at = face_base[fan].long()[fan_of] + (torch.arange(fans.shape[0], device=dev) - first[fan_of])
        faces[at] = fans.to(torch.int32)
    info = {"n_triangulated": n_tri, "n_fans": n_fans, "area": area, "fallback": code[code >= 0].clone()}
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
        ws = torch.empty(int(lib.misplat_meshtri_flip_workspace(C.c_int64(m), C.c_int64(n))), dtype=torch.uint8, device=dev)
        while rounds < max_rounds:
            check(lib.misplat_meshtri_flip_round(ptr(v), C.c_int64(m), ptr(tri), C.c_int64(n), ptr(reg), C.c_double(min_violation),
                                                 ptr(ws), C.c_int64(ws.numel()), ptr(counts), stream_ptr()), "misplat_meshtri_flip_round")
            k = int(counts.item())                                  # the round's host read
            if k == 0:
                break
            rounds += 1
            n_flips += k
    return tri.to(triangles.dtype), n_flips, rounds


__all__ = ["subdivide_mesh", "fair_vertices", "fill_holes_nicely", "triangulate_holes", "flip_edges"]
