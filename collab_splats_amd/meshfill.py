"""Hole filling at the mesh's own resolution on the MI355X (csrc/meshfill.hip).

The reference's ``clean_repair_mesh`` (collab_splats/utils/mesh.py:359-407) closes every hole below ``max_hole_size`` with
MeshLib's ``fillHoleNicely`` (``maxEdgeLen`` = the mesh's average edge length, ``maxEdgeSplits`` = 10000; the fallback is
``fillHole`` + ``subdivideMesh`` + ``positionVertsSmoothly``, :317-356): the patch is subdivided to the mesh's edge length and its
new vertices are positioned smoothly.  Here the same steps run on device tensors: the fan of ``fill_holes``, longest-edge
bisection of the fan's faces in rounds (``subdivide_mesh``), membrane fairing of the created vertices with the rim held fixed
(``fair_vertices``).  Restated from the published methods [UNVERIFIED-UPSTREAM]: MeshLib is not available to compare with and
its output cannot be pinned; its edge flips during subdivision and its minimum-area triangulation in place of the fan are NOT
built.  The oracle is tests/meshfill_restatement.py, bit for bit.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from ._lib import check, load, ptr, require_gpu, stream_ptr
from .meshclean import _attributes, _fans, _limit, _mesh, mesh_edge_stats
from .meshmap import _prep
from .pointcloud import _positive32

# A patch of at most LDS_MAX_VERTICES free vertices runs all its iterations in one workgroup, both iterates in LDS (the mirror
# of MISPLAT_MESHFILL_LDS_VERTICES in include/misplat.h; DESIGN.md section 29.4 holds the arithmetic and the measurement).
# ENABLE_LDS_FAIR = False sends every patch through one launch per iteration: the default, because that path measured no
# slower on the timed meshes (section 29.5), whose large patches are above the cut-off.  Neither changes a result.
ENABLE_LDS_FAIR = False
LDS_MAX_VERTICES = 4096


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

    MeshLib's ``subdivideMesh`` also flips edges while it splits; that is not built."""
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
                      attributes: Sequence[Tensor] = ()) -> Tuple[Tensor, Tensor, Tuple[Tensor, ...], int, dict]:
    """``fill_holes`` whose patches are subdivided to the mesh's edge length and faired: ``(vertices', triangles', attributes',
    n_filled, info)``; ``info`` holds ``n_splits``, ``rounds``, ``iterations`` ([P] int32, one entry per patch of created
    vertices) and ``n_new_vertices``.

    The same loops and the same fans as ``fill_holes``; then ``subdivide_mesh`` with ``region`` = the fans' faces (a rim edge has a
    face outside the region: no input face changes) and ``fair_vertices`` with ``free`` = every vertex the call created, the
    fans' centres and the split midpoints.  ``max_edge_len=None`` is the input mesh's ``mean_edge_length``, measured before the
    fill (the reference's order, mesh.py:386-390); ``tolerance=None`` is ``1e-3 max_edge_len`` (a chosen default).  The
    reference's ``maxEdgeSplits`` is per hole; here the call's total is ``max_edge_splits * n_filled``, the same worst case: a
    single hole may take more than its share.  The input's vertices and faces are a bit-identical prefix of the output; loops
    at or above ``max_hole_size`` are untouched.

    This stands where MeshLib's ``fillHoleNicely`` stands in the reference, restated from the published methods (longest-edge
    bisection, membrane fairing with the rim fixed): MeshLib's minimum-area triangulation in place of the fan and its edge flips
    during subdivision are not built, and nothing here can be compared with MeshLib's output."""
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
    require_gpu(vertices, triangles, *attributes)
    attributes = tuple(_prep(a) for a in attributes)
    m, n = v.shape[0], t.shape[0]
    info = {"n_splits": 0, "rounds": 0, "iterations": torch.zeros(0, dtype=torch.int32, device=v.device), "n_new_vertices": 0}
    filled = _fans(v, t, attributes, limit) if n else None
    if filled is None:
        return v, t.to(triangles.dtype), attributes, 0, info
    if max_edge_len is None:
        max_edge_len = _positive32(name, "the mesh's mean edge length", mesh_edge_stats(v, t)["mean_edge_length"])
    if tolerance is None:
        tolerance = _positive32(name, "tolerance", 1e-3 * max_edge_len)
    v2, t2, a2, n_filled = filled
    region = torch.arange(t2.shape[0], device=v.device) >= n
    v3, t3, a3, _, n_splits, rounds = subdivide_mesh(v2, t2, max_edge_len, per_hole * n_filled, region, a2)
    free = torch.arange(v3.shape[0], device=v.device) >= m
    v4, a4, iterations = fair_vertices(v3, t3, free, tolerance, max_iterations, a3)
    info.update(n_splits=n_splits, rounds=rounds, iterations=iterations, n_new_vertices=v4.shape[0] - m)
    return v4, t3.to(triangles.dtype), a4, n_filled, info


__all__ = ["subdivide_mesh", "fair_vertices", "fill_holes_nicely"]
