"""Meshes for the regimes of the hole fill that a real TSDF mesh reaches and the scenes of tests/mesh{fill,tri,smooth}_scenes.py do
not (DESIGN.md sections 29.6, 30.6, 31.6): several holes in a call, fans beside triangulations, two slab loops, vertex indices
past 65 536, a budget cut of more than a sort tile, rows longer than a chunk, iteration counts at the host's batch edges.  FAIR,
SUBDIVIDE, TRIANGULATE, FLIP and FILL name the cases; tests/test_meshfill_regimes_host.py asserts on the restatement that each
case reaches its regime, tests/test_meshfill_regimes_gpu.py compares the device with it (reference: computed once per process)."""
from __future__ import annotations

import numpy as np

import meshsmooth_scenes as SS
import meshtri_scenes as TS
from meshclean_scenes import BOW_TIE, THREE_HOLES, F, icosphere, merge, sheet  # noqa: F401
from meshfill_scenes import _block, boundary_edges, colour_ramp, edge_counts, grid  # noqa: F401

PAD = 70001                             # unreferenced vertices in front of a mesh: every index is then past 65 536 (three digits)
KTILE = 4096                            # radixsort.h's kTile, the items of one sort block
_MESHES, _REFERENCES = {}, {}


def padded(V, T, k, *per_vertex):
    """(V, T) behind k unreferenced vertices: every referenced index is >= k and M = k + len(V); arrays with a row per vertex
    (a free mask, attributes) get k rows of zeros in front.  The tie-break hashes the indices: the result of a call on the
    padded mesh is not a shifted copy, and is compared with the restatement run on the padded mesh itself."""
    V2 = np.concatenate([np.full((k, 3), 0.5, F), np.asarray(V, F)])
    rows = [np.concatenate([np.zeros((k,) + x.shape[1:], x.dtype), x]) for x in per_vertex]
    return (V2, np.asarray(T, np.int64) + k, *rows)


def radix_passes(max_key):
    """radixsort.h's: the 8-bit digits of max_key, at least one and at most four."""
    passes = 1
    while passes < 4 and (max_key >> (8 * passes)) > 0:
        passes += 1
    return passes


def channels(V, width):
    """An attribute of `width` channels that differ, none of them linear in the position (the membrane leaves a linear function
    on a regular grid where it is: such an attribute would show no iteration at all)."""
    ramp = colour_ramp(V).astype(np.float64)
    c = np.arange(width)
    return np.sin((1.0 + c) * (1.7 * ramp[:, :1] + 2.3 * ramp[:, 1:2] + 3.1 * ramp[:, 2:]) + c).astype(F)


# ---------------------------------------------------------------------------------------------------------- fairing
def noisy_blocks(n, blocks, pad=0, seed=3, noise=0.05):
    """sheet(n) with the vertices i0 <= i < i1, j0 <= j < j1 of every block (i0, i1, j0, j1) free and lifted off the plane by
    noise, behind `pad` unreferenced vertices.  On a dyadic sheet a free vertex keeps its x and y to the bit (the mean of its six
    neighbours' is exact): only z moves, towards the fixed z = 0, so the displacement falls for thousands of iterations."""
    V, T = sheet(n)
    free = np.zeros(len(V), bool)
    for i0, i1, j0, j1 in blocks:
        free[_block(n, i0, i1, j0, j1)] = True
    V = V.copy()
    V[free, 2] += (noise * np.random.default_rng(seed).standard_normal(int(free.sum()))).astype(F)
    return padded(V, T, pad, free)


def spoke_fan(n, opened=(), free_rim=(), seed=5):
    """A fan of n spokes about vertex 0 (rim vertex 1 + i on the unit circle, lifted by noise; face i = (0, 1 + i, 1 + (i + 1) %
    n)) without the faces `opened`; the centre and the rim vertices `free_rim` are free.  A spoke with both its faces has two
    entries in the centre's row, twins side by side; a spoke beside an opened face has one, which shifts every later pair by an
    entry."""
    a = 2 * np.pi * np.arange(n) / n
    z = 0.1 * np.random.default_rng(seed).standard_normal(n)
    V = np.concatenate([[[0.1, -0.05, 0.5]], np.stack([np.cos(a), np.sin(a), z], 1)]).astype(F)
    i = np.arange(n)
    T = np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], 1)
    T = T[~np.isin(i, list(opened))]
    free = np.zeros(n + 1, bool)
    free[[0, *free_rim]] = True
    return V, T, free


def sorted_row(T, v):
    """The targets of the directed edges that leave vertex v, every face's three edges both ways, ascending: the row that
    fair_build's two sorts leave for a free vertex, twins included."""
    T = np.asarray(T, np.int64).reshape(-1, 3)
    src = np.concatenate([T.reshape(-1), T[:, [1, 2, 0]].reshape(-1)])
    tgt = np.concatenate([T[:, [1, 2, 0]].reshape(-1), T.reshape(-1)])
    return np.sort(tgt[(src == v) & (tgt != v)])


def twins_across(row, chunk):
    """The twin pairs of a sorted row whose second entry opens a chunk of `chunk` entries."""
    at = np.arange(chunk, len(row), chunk)
    return int((row[at] == row[at - 1]).sum())


BATCH = [(3, 8, 3, 8), (12, 25, 14, 27)]                             # a 5 x 5 and a 13 x 13 block of sheet(32)
STRIPS = [(4, 5, 4, 25), (6, 9, 4, 25), (10, 15, 4, 25)]            # columns 4, 6 - 8 and 10 - 14 of sheet(32), rows 4 - 24


def _stop_at(make, patch, count):
    """The tolerance whose bits are patch `patch`'s displacement in iteration count - 1: with a falling sequence the patch stops
    at exactly `count` (the host test asserts that it does)."""
    def tolerance():
        import meshfill_restatement as R
        V, T, free = make()
        return float(R.fair_displacements(V, T, free, count - 1)[count - 2, patch:patch + 1].view(F)[0])
    return tolerance


def _batch():
    return noisy_blocks(32, BATCH)


def _block21():
    return noisy_blocks(32, [(6, 27, 6, 27)], PAD, seed=8)


# name -> (mesh and free, tolerance or a function that gives it, max_iterations, attribute widths)
FAIR = {
    # (radix_passes(M - 1), radix_passes(n - 1)): where fair_step and fair_lds look for the sorted rows
    "passes_1_1": (lambda: noisy_blocks(8, [(1, 3, 1, 3), (4, 7, 4, 7)], 256 - 81), 1e-4, 10000, (3,)),
    "passes_2_1": (lambda: noisy_blocks(8, [(1, 3, 1, 3), (4, 7, 4, 7)], 257 - 81), 1e-4, 10000, (3,)),
    "passes_3_1": (lambda: noisy_blocks(32, [(3, 6, 3, 6), (12, 21, 14, 23)], PAD), 1e-4, 10000, (3,)),
    "passes_3_2": (_block21, 1e-4, 10000, (3,)),
    # rows of 34 and 66 entries, closed and opened
    "fan17": (lambda: spoke_fan(17), 1e-4, 10000, (3,)),
    "fan33": (lambda: spoke_fan(33), 1e-4, 10000, (3,)),
    "fan17_open": (lambda: spoke_fan(17, (16,)), 1e-4, 10000, (3,)),
    "fan33_open": (lambda: spoke_fan(33, (32,)), 1e-4, 10000, (3,)),
    "fan33_open2": (lambda: spoke_fan(33, (32, 20)), 1e-4, 10000, (3,)),
    "fan33_open_rim": (lambda: spoke_fan(33, (32,), (9,)), 1e-4, 10000, (3,)),
    # the small patch stops at the host's batch edge, the large one runs on; then the cap at and about the edge
    "stop_32": (_batch, _stop_at(_batch, 0, 32), 10000, (3,)),
    "stop_33": (_batch, _stop_at(_batch, 0, 33), 10000, (3,)),
    "cap_31": (_batch, _stop_at(_batch, 0, 32), 31, (3,)),
    "cap_32": (_batch, _stop_at(_batch, 0, 32), 32, (3,)),
    "cap_33": (_batch, _stop_at(_batch, 0, 32), 33, (3,)),
    "cap_64": (_batch, _stop_at(_batch, 0, 32), 64, (3,)),
    # more than 1024 iterations: the attributes re-run in two chunks
    # (attributes that are 0 on the fixed vertices: like z they decay for good and never reach a fixed point of the rounding)
    "counted": (_block21, _stop_at(_block21, 0, 1101), 10000, (1, 7)),
    # three patches alternate in the free list
    "interleaved": (lambda: noisy_blocks(32, STRIPS, seed=9), 1e-5, 10000, (3,)),
}


DECAYING = {"counted"}


def fair_case(name):
    """(V, T, free, attributes, tolerance, max_iterations); the arrays are shared: do not write to them."""
    make, tol, max_it, widths = FAIR[name]
    key = ("fair", name)
    if key not in _MESHES:
        V, T, free = make()
        att = tuple(channels(V, w) * (free[:, None] if name in DECAYING else 1) for w in widths)
        _MESHES[key] = (V, T, free, tuple(a.astype(F) for a in att), tol() if callable(tol) else tol)
    return _MESHES[key] + (max_it,)


def fair_reference(name):
    key = ("fair", name)
    if key not in _REFERENCES:
        import meshfill_restatement as R
        V, T, free, att, tol, max_it = fair_case(name)
        _REFERENCES[key] = R.fair(V, T, free, tol, max_it, att)
    return _REFERENCES[key]


def patches_per_wave(T, free, channels_per_vertex=3, wave=64):
    """The number of distinct patches among the lanes of every wave of fair_step's launch: lane k D + c is channel c of the
    k-th free vertex."""
    import meshfill_restatement as R
    _, _, _, patch = R.free_rows(T, free)
    lane_patch = np.repeat(patch, channels_per_vertex)
    return [len(np.unique(lane_patch[at:at + wave])) for at in range(0, len(lane_patch), wave)]


# ------------------------------------------------------------------------------------------------------ subdivision
def _grid80():
    return grid(80, 80)


def _half_region():
    V, T = grid(12, 12)
    return V, T, np.arange(len(T)) < len(T) // 2


def _late_cut_budget():
    """All of the first two rounds and half of the third."""
    import meshfill_restatement as R
    V, T = grid(20, 20)
    rounds = []
    R.subdivide(V, T, 0.4, 1 << 20, on_round=lambda rd, sel: rounds.append(len(sel)))
    return rounds[0] + rounds[1] + rounds[2] // 2


# name -> (mesh and optional region, pad, max_edge_len, max_edge_splits or a function that gives it, attribute widths)
SUBDIVIDE = {
    "cut_5000": (_grid80, 0, 1.2, 5000, (3,)),
    "cut_4096": (_grid80, 0, 1.2, KTILE, (3,)),
    "cut_4097": (_grid80, 0, 1.2, KTILE + 1, (3,)),
    "cut_5000_padded": (_grid80, PAD, 1.2, 5000, (3,)),
    "cut_m255": (lambda: grid(15, 15), 0, 1.2, 100, (3,)),
    "cut_m256": (lambda: grid(15, 15), 1, 1.2, 100, (3,)),
    "late_cut": (lambda: grid(20, 20), 0, 0.4, _late_cut_budget, (3,)),
    "region_widths": (_half_region, 0, 0.7, 10000, (1, 5)),
}


def subdivide_case(name):
    """(V, T, region or None, attributes, max_edge_len, max_edge_splits)."""
    make, pad, max_len, budget, widths = SUBDIVIDE[name]
    key = ("subdivide", name)
    if key not in _MESHES:
        got = make()
        V, T = padded(got[0], got[1], pad)
        _MESHES[key] = (V, T, got[2] if len(got) > 2 else None, tuple(channels(V, w) for w in widths),
                        budget() if callable(budget) else budget)
    V, T, region, att, budget = _MESHES[key]
    return V, T, region, att, max_len, budget


def subdivide_reference(name):
    """(the restatement's result, per round (selected in all, applied, the round itself and the edges it took))."""
    key = ("subdivide", name)
    if key not in _REFERENCES:
        import meshfill_restatement as R
        V, T, region, att, max_len, budget = subdivide_case(name)
        rounds = []
        res = R.subdivide(V, T, max_len, budget, region, att, on_round=lambda rd, sel: rounds.append((int(rd.selected.sum()), len(sel), rd, sel)))
        _REFERENCES[key] = (res, rounds)
    return _REFERENCES[key]


# ------------------------------------------------------------------------------------- triangulation and flips
def _shift(mesh, x):
    return mesh[0] + F([x, 0, 0]), mesh[1]


def _mixed():
    """In loop rank: sheet(64)'s outline (above the limit) and its pinched loop (a fan), a dome of 9 (triangulated, as every
    dome's outer loop is), a loop of two edges (a fan), a dome of 14, a rim of MAX_LOOP + 1 edges (a fan, as is its outer
    loop), a dome of 5."""
    return merge(sheet(64, BOW_TIE), _shift(SS.dome(9, 0.1, 0.05, 2), 2), _shift(TS.two_edge_loop(), 3), _shift(SS.dome(14, 0.1, 0.05, 3), 5),
                 _shift(TS.annulus(TS.circle(TS.MAX_LOOP + 1, 0.1, 0.0005, 6)), 6), _shift(SS.dome(5, 0.1, 0.05, 1), 7))


def _slabs():
    """Domes of 40, 100, 190 and 200 rim edges: under either metric the first is a small instance, the second keeps its table in
    LDS and the last two in the workspace, the second of them behind the first; the four outer loops are below the limit too."""
    return merge(SS.dome(40, 0.1, 0.05, 11), _shift(SS.dome(100, 0.1, 0.05, 12), 1), _shift(SS.dome(190, 0.1, 0.05, 13), 2),
                 _shift(SS.dome(200, 0.1, 0.05, 14), 3))


# name -> (mesh, pad, max_hole_size); every case runs under both metrics
TRIANGULATE = {
    "mixed": (_mixed, 0, 3.0),
    "slabs": (_slabs, 0, 3.0),
    "three_loops_padded": (SS._three_loops, PAD, 1.0),
}


def triangulate_case(name):
    """(V, T, attributes, max_hole_size)."""
    make, pad, size = TRIANGULATE[name]
    key = ("triangulate", name)
    if key not in _MESHES:
        V, T = padded(*make(), pad)
        _MESHES[key] = (np.ascontiguousarray(V, F), np.ascontiguousarray(T, np.int64), (colour_ramp(V),))
    return _MESHES[key] + (size,)


def triangulate_reference(name, metric):
    key = ("triangulate", name, metric)
    if key not in _REFERENCES:
        import meshsmooth_restatement as R
        V, T, att, size = triangulate_case(name)
        _REFERENCES[key] = R.triangulate_holes(V, T, size, att, metric)
    return _REFERENCES[key]


def loop_sizes(name):
    """(edges, filled) of every loop of a triangulation case, in loop rank."""
    import meshclean_restatement as MC
    V, T, _, size = triangulate_case(name)
    _, _, n_edges, perimeter = MC.mesh_holes(V, T)
    return n_edges.astype(np.int64), perimeter < size


# name -> (a case of tests/meshtri_scenes.py's FLIP, pad)
FLIP = {
    "grid37x41_padded": ("grid37x41", PAD),
    "octahedron_padded": ("octahedron", PAD),
}


def flip_case(name):
    """(V, T)."""
    key = ("flip", name)
    if key not in _MESHES:
        V, T, _ = TS.flip_case(FLIP[name][0])
        _MESHES[key] = padded(V, T, FLIP[name][1])
    return _MESHES[key]


def flip_reference(name):
    """(the restatement's result, per round (selected, flipped))."""
    key = ("flip", name)
    if key not in _REFERENCES:
        import meshtri_restatement as R
        V, T = flip_case(name)
        rounds = []
        res = R.flip_edges(V, T, on_round=lambda rd: rounds.append((int(rd.selected.sum()), len(rd.flips))))
        _REFERENCES[key] = (res, rounds)
    return _REFERENCES[key]


# --------------------------------------------------------------------------------------------------------- the fill
TIE = [(36, 40, 10, 14), (40, 44, 14, 18)]                          # BOW_TIE moved clear of THREE_HOLES
HOLE_BOXES = [(i0 / 64, i1 / 64, j0 / 64, j1 / 64) for i0, i1, j0, j1 in THREE_HOLES]


def three_holes():
    """sheet(64) without an 8 x 12, a 4 x 10 and a 10 x 4 block of quads (perimeters 0.625, 0.4375, 0.4375; the outline's is 4)."""
    return sheet(64, THREE_HOLES)


def bumpy_holes(seed=21):
    """three_holes with smooth bumps in z and every vertex jittered by up to a fifth of a quad: no two edges of equal length, no
    four points on a circle, rims that are not planar."""
    V, T = three_holes()
    V = V.astype(np.float64)
    rng = np.random.default_rng(seed)
    V[:, 2] = 0.05 * np.sin(9.0 * V[:, 0]) * np.cos(7.0 * V[:, 1])
    V += rng.uniform(-0.2 / 64, 0.2 / 64, V.shape)
    return V.astype(F), T


CAPS = [((-1, (1 + 5 ** 0.5) / 2, 0), 0.965), ((1, -0.3, 0.2), 0.95), ((-0.2, -1, 0.5), 0.93), ((0.1, 0.2, -1), 0.91)]


def capped_sphere(level=4, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """icosphere(level) without the faces that touch a vertex of four caps of different size: the first about a vertex of the
    icosahedron (valence 5), the others in general position."""
    V, T = icosphere(level)
    for d, cut in CAPS:
        d = np.asarray(d, np.float64) / np.linalg.norm(d)
        T = T[~np.isin(T, np.flatnonzero(V.astype(np.float64) @ d > cut)).any(1)]
    return (V.astype(np.float64) * radius + np.asarray(centre, np.float64)).astype(F), T


def holes_and_tie():
    """three_holes and a pinched loop clear of them: under ``min_area`` that loop gets the fan, the others the triangulation."""
    return sheet(64, THREE_HOLES + TIE)


DEFAULT = {}
MIN_AREA = dict(triangulation="min_area", flip=True)
SMOOTH = SS.SMOOTH
HOW = {"default": DEFAULT, "min_area": MIN_AREA, "smooth": SMOOTH}

# name -> (mesh, pad, max_hole_size, max_edge_len or None for the mesh's mean edge length, further keywords)
FILL = {
    "three_holes": (three_holes, 0, 1.0, 1.0 / 64, {}),
    "bumpy_holes": (bumpy_holes, 0, 1.0, None, {}),
    "capped_sphere": (capped_sphere, 0, 6.0, None, {}),
    "holes_and_tie": (holes_and_tie, 0, 1.0, 1.0 / 64, {}),
    "shared_budget": (three_holes, 0, 1.0, 1.0 / 64, dict(max_edge_splits=30)),
    "three_holes_padded": (three_holes, PAD, 1.0, 1.0 / 64, {}),
}


def fill_case(name):
    """(V, T, attributes, max_hole_size, max_edge_len, keywords)."""
    make, pad, size, max_len, kw = FILL[name]
    key = ("fill", name)
    if key not in _MESHES:
        V, T = padded(*make(), pad)
        _MESHES[key] = (np.ascontiguousarray(V, F), np.ascontiguousarray(T, np.int64), (colour_ramp(V),))
    return _MESHES[key] + (size, max_len, kw)


def fill_reference(name, how):
    """(the restatement's result, per pass (splits, flips)) of FILL[name] under HOW[how]."""
    key = ("fill", name, how)
    if key not in _REFERENCES:
        import meshfill_restatement as MF
        import meshsmooth_restatement as R
        import meshtri_restatement as MT
        V, T, att, size, max_len, kw = fill_case(name)
        passes = []
        subdivide, flip_edges = MF.subdivide, MT.flip_edges

        def logged_subdivide(*a, **k):
            out = subdivide(*a, **k)
            passes.append([out[4], 0])
            return out

        def logged_flips(*a, **k):
            out = flip_edges(*a, **k)
            passes[-1][1] = out[1]
            return out

        MF.subdivide, MT.flip_edges = logged_subdivide, logged_flips
        try:
            res = R.fill_holes_nicely(V, T, size, max_len, attributes=att, **kw, **HOW[how])
        finally:
            MF.subdivide, MT.flip_edges = subdivide, flip_edges
        _REFERENCES[key] = (res, [tuple(p) for p in passes])
    return _REFERENCES[key]

