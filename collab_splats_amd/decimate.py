"""Quadric-error mesh simplification on the MI355X (csrc/decimate.hip).

The reference's mesh exporters end in Open3D's ``simplify_quadric_decimation(target_triangles)`` (collab_splats/utils/mesh.py
:1350-1352 for ``MarchingCubesMesh``, default 1 000 000; :1460-1461 for ``TSDFFusion``).  Here the step runs on device tensors:
Garland-Heckbert quadrics and edge collapses, applied in rounds of mutually independent edges instead of one at a time from a
heap.  Restated from the published method [UNVERIFIED-UPSTREAM]: Open3D is not available to compare with, and the output is
not expected to equal Open3D's triangle for triangle (another collapse order, the link condition added).  The oracle is
tests/decimate_restatement.py, bit for bit.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch
from torch import Tensor

from ._lib import MisplatError, load, ptr, require_gpu, run
from .meshclean import _attributes, _mesh
from .meshmap import _prep


def simplify_quadric_decimation(vertices: Tensor, triangles: Tensor, target_triangles: int, attributes: Sequence[Tensor] = (),
                                max_rounds: int = 256) -> Tuple[Tensor, Tensor, Tuple[Tensor, ...], Tensor, int]:
    """Collapse edges until at most ``target_triangles`` triangles are left: ``(vertices [M',3], triangles [T',3], attributes,
    vertex_map [M] int64, rounds)``.

    Triangles with a repeated corner are dropped first.  Every vertex gets the fp64 quadric of its faces' planes (weighted by
    area) and of the planes through its boundary edges perpendicular to their face.  An edge collapses to the minimiser of the
    summed quadric (or, where the 3x3 system is singular, to the cheapest of its ends and their midpoint), rounded to fp32; its
    cost there is its priority, ties broken by a fixed mixing of the edge key.  It may collapse only if it has at most two
    faces, its ends' common neighbours are exactly those faces' third corners, it is not an interior edge between two boundary
    vertices, no surviving face around it turns over and no two surviving faces become equal.  Each round collapses every valid
    edge that has the smallest priority among all edges within one ring of both its ends; the last round takes only as many, in
    ascending (cost, edge key), as reach the target: ``T' <= target_triangles`` and ``T' > target_triangles - 2``, unless no valid
    collapse is left (or ``max_rounds`` is reached) first.  The surviving end takes the target position and ``0.5 (x_lo + x_hi)``
    of every attribute ([M,D] float32).

    The output keeps the surviving vertices and faces in their original order; unreferenced vertices are dropped; the triangles
    come back in the dtype they came in; ``vertex_map[i]`` is the output vertex input vertex ``i`` ended in, -1 if it was
    dropped.  ``target_triangles >= T`` returns the mesh compacted and otherwise unchanged.  One host read per round (the
    number of selected edges and of the faces they remove), one before the first (the degenerate faces) and one at the end (the
    output's sizes).  Two runs are bitwise equal."""
    name = "simplify_quadric_decimation"
    v, t = _mesh(name, vertices, triangles)
    attributes = _attributes(name, attributes, v.shape[0], True)
    for what, x in (("target_triangles", target_triangles), ("max_rounds", max_rounds)):
        if not isinstance(x, int) or isinstance(x, bool) or x < 0:
            raise ValueError(f"{name}: {what} must be a non-negative integer, got {x!r}")
    if sum(a.shape[1] for a in attributes) > 4096:
        raise ValueError(f"{name}: {sum(a.shape[1] for a in attributes)} attribute channels in all, the limit is 4096")
    m, n_slots = v.shape[0], t.shape[0]
    if 6 * n_slots >= (1 << 31) - 4096:
        raise ValueError(f"{name}: {n_slots} triangles are beyond the library's limits (6 T < 2^31 - 4096)")
    require_gpu(vertices, triangles, *attributes)
    dev = v.device
    lib = load()
    pos, tri = v.clone(), t.clone()
    widths = [a.shape[1] for a in attributes]
    d = sum(widths)
    att = torch.cat([_prep(a) for a in attributes], 1).contiguous() if d else None
    alive = ((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])).to(torch.int32)
    into = torch.full((m,), -1, dtype=torch.int32, device=dev)
    n_alive = int(alive.sum()) if n_slots else 0                    # the host read before the first round
    rounds = 0
    if n_alive > target_triangles and max_rounds > 0:
        b = int(lib.misplat_decimate_workspace(m, n_slots))
        if b < 0:
            raise ValueError(f"{name}: {n_slots} triangles over {m} vertices are beyond the library's limits")
        ws = torch.empty(b, dtype=torch.uint8, device=dev)
        quadrics = torch.empty((m, 10), dtype=torch.float64, device=dev)
        counts = torch.empty(3, dtype=torch.int32, device=dev)
        while rounds < max_rounds and n_alive > target_triangles:
            run("misplat_decimate_round", ptr(pos), m, ptr(tri), n_slots, ptr(alive), n_alive, ptr(quadrics), int(rounds == 0),
                ptr(ws), b, ptr(counts))
            found, n_selected, n_removed = counts.tolist()          # the round's host read
            if found != n_alive:
                raise MisplatError(f"{name}: {found} live faces found where {n_alive} were expected")
            if n_selected == 0:
                break
            rounds += 1
            need = n_alive - target_triangles
            last = n_removed > need
            run("misplat_decimate_apply", ptr(pos), m, ptr(tri), n_slots, ptr(alive), n_alive, ptr(att), d, ptr(quadrics),
                ptr(into), n_selected, need if last else -1, ptr(ws), b)
            if last:
                break
            n_alive -= n_removed
    # the output: the live faces and the vertices they reference, both in their original order
    root = torch.empty(m, dtype=torch.int32, device=dev)
    run("misplat_decimate_resolve", ptr(into), m, ptr(root))
    kept = tri[alive.bool()].long()
    used = torch.zeros(m, dtype=torch.bool, device=dev)
    used[kept.reshape(-1)] = True
    new = torch.cumsum(used, 0) - 1
    root = root.long()
    vertex_map = torch.where(used[root], new[root], torch.full_like(new, -1))
    out_att = tuple(x[used].contiguous() for x in torch.split(att, widths, 1)) if d else ()
    return pos[used], new[kept].to(triangles.dtype), out_att, vertex_map, rounds


__all__ = ["simplify_quadric_decimation"]
