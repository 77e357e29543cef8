"""Marching-cubes tables, derived from first principles (no table is typed in).

Cube conventions (shared with csrc/tsdf.hip and the fp32 restatement under tests/):
  corner c = dx + 2 dy + 4 dz, (dx, dy, dz) in {0, 1}^3 -- the cell's origin voxel and its +x/+y/+z neighbours;
  edge e = 4 a + (b1 + 2 b2): axis a (0 x, 1 y, 2 z) and the offsets b1, b2 on the other two axes in increasing order;
  its first corner has coordinate 0 on axis a, and that corner's voxel OWNS the edge (edges 0, 4, 8 are the cell's own);
  bit c of the cube index is set iff corner c is negative (tsdf < 0).

Construction of one case:
  1. on each of the 6 faces connect the crossed edges into segments; a face with 4 crossed edges (ambiguous) is resolved by
     ONE rule: the negative corners are separated (each is cut off by its own segment).  A face's segments therefore depend
     on its 4 corner signs only, and neighbouring cells agree on the face they share: the surface is watertight;
  2. orient every segment so that the surface it bounds faces the positive side; every crossed edge then has one segment
     leaving it and one entering it, and the segments chain into closed loops;
  3. fan-triangulate each loop (from the first root whose fan keeps every triangle facing the positive corners).

``python -m collab_splats_amd.mc_tables`` writes csrc/mc_tables.h; tests check the committed file equals ``header_text()``.
"""
from __future__ import annotations

import os
from functools import lru_cache

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mc_tables.h")


def corner_pos(c: int) -> np.ndarray:
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def edge_corners(e: int):
    a, o = divmod(e, 4)
    others = [x for x in range(3) if x != a]
    c0 = ((o & 1) << others[0]) | (((o >> 1) & 1) << others[1])
    return c0, c0 | (1 << a)


EDGES = [edge_corners(e) for e in range(12)]


def edge_axis(e: int) -> int:
    return e // 4


def edge_mid(e: int) -> np.ndarray:
    c0, c1 = EDGES[e]
    return 0.5 * (corner_pos(c0) + corner_pos(c1))


def faces():
    """(axis, side, corners in cyclic order, edges of the face)."""
    out = []
    for a in range(3):
        o1, o2 = [x for x in range(3) if x != a]
        for s in (0, 1):
            base = s << a
            cyc = [base, base | (1 << o1), base | (1 << o1) | (1 << o2), base | (1 << o2)]
            fe = [e for e in range(12) if edge_axis(e) != a and (EDGES[e][0] >> a) & 1 == s]
            out.append((a, s, cyc, fe))
    return out


FACES = faces()


def face_segments(case: int, face) -> list:
    """Unoriented segments (pairs of crossed edges) on one face; depends on the face's 4 corner signs only."""
    a, s, cyc, fe = face
    neg = lambda c: (case >> c) & 1
    crossed = [e for e in fe if neg(EDGES[e][0]) != neg(EDGES[e][1])]
    if not crossed:
        return []
    if len(crossed) == 2:
        return [tuple(crossed)]
    segs = []                                         # 4 crossed: cut off every negative corner of the face
    for c in cyc:
        if neg(c):
            segs.append(tuple(e for e in fe if c in EDGES[e]))
    return segs


def _oriented(case: int, face, seg):
    a, s, cyc, fe = face
    n_out = np.zeros(3)
    n_out[a] = 1.0 if s else -1.0
    negs = [c for c in cyc if (case >> c) & 1]
    # the negative corner on the negative side of this segment: the corner it cuts off (ambiguous face) or any negative one
    cut = [c for c in negs if all(c in EDGES[e] for e in seg)]
    N = corner_pos(cut[0] if cut else negs[0])
    A, B = edge_mid(seg[0]), edge_mid(seg[1])
    d = np.dot(np.cross(B - A, -n_out), N - 0.5 * (A + B))
    return seg if d < 0 else (seg[1], seg[0])


def _tri_ok(case: int, tri) -> bool:
    P = [edge_mid(e) for e in tri]
    n = np.cross(P[1] - P[0], P[2] - P[0])
    dots = []
    for e in tri:                                     # the normal against each crossed edge, negative -> positive end
        c0, c1 = EDGES[e]
        pos, neg = (c0, c1) if not (case >> c0) & 1 else (c1, c0)
        dots.append(float(np.dot(n, corner_pos(pos) - corner_pos(neg))))
    return min(dots) >= 0.0 and sum(dots) > 1e-9


def case_triangles(case: int) -> list:
    nxt = {}
    for f in FACES:
        for seg in face_segments(case, f):
            a, b = _oriented(case, f, seg)
            assert a not in nxt, (case, a)
            nxt[a] = b
    tris, seen = [], set()
    for start in range(12):
        if start not in nxt or start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, (case, loop)
        n = len(loop)
        for r in range(n):
            L = loop[r:] + loop[:r]
            fan = [(L[0], L[i], L[i + 1]) for i in range(1, n - 1)]
            if all(_tri_ok(case, t) for t in fan):
                tris += fan
                break
        else:
            raise AssertionError(f"case {case}: no fan root keeps the triangles facing the positive corners")
    return tris


@lru_cache(maxsize=1)
def tables():
    """(ntri[256], tri[256][3 * max_tri] padded with -1, max_tri)."""
    per = [case_triangles(c) for c in range(256)]
    max_tri = max(len(t) for t in per)
    tri = np.full((256, 3 * max_tri), -1, dtype=np.int8)
    for c, ts in enumerate(per):
        for k, t in enumerate(ts):
            tri[c, 3 * k:3 * k + 3] = t
    return np.array([len(t) for t in per], dtype=np.int8), tri, max_tri


def header_text() -> str:
    ntri, tri, max_tri = tables()
    lines = ["// mc_tables.h -- GENERATED by `python -m collab_splats_amd.mc_tables` (collab_splats_amd/mc_tables.py); do not edit.",
             "// Marching-cubes triangulations derived from first principles: ambiguous faces separate their negative corners.",
             "// corner c = dx + 2 dy + 4 dz; edge e = 4 axis + (b1 + 2 b2); bit c of the case is set iff corner c has tsdf < 0;",
             "// triangles face the positive corners (right-hand rule).",
             "#pragma once",
             "#ifndef MC_QUAL",
             "#define MC_QUAL static const",
             "#endif",
             f"#define MC_MAX_TRI {max_tri}",
             "",
             "// first and second corner of every edge",
             "MC_QUAL signed char MC_EDGE_CORNERS[12][2] = {" + ", ".join("{%d, %d}" % EDGES[e] for e in range(12)) + "};",
             "",
             "MC_QUAL signed char MC_NTRI[256] = {"]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(int(x)) for x in ntri[r:r + 32]) + ",")
    lines.append("};")
    lines.append("")
    lines.append(f"MC_QUAL signed char MC_TRI[256][{3 * max_tri}] = {{")
    for c in range(256):
        lines.append("    {" + ", ".join(str(int(x)) for x in tri[c]) + "},")
    lines.append("};")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    with open(HEADER, "w") as f:
        f.write(header_text())
    print(HEADER, "max triangles per cell", tables()[2])
