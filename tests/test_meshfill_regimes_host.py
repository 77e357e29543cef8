"""CPU: every scene of tests/meshfill_regimes_scenes.py reaches the regime it was built for, asserted on the restatements
(tests/mesh{fill,tri,smooth}_restatement.py): a scene that drifts out of its regime fails here instead of passing vacuously in
tests/test_meshfill_regimes_gpu.py, which compares the device with the same references."""
import numpy as np
import pytest

import meshclean_restatement as MC
import meshfill_regimes_scenes as S
import meshfill_restatement as R
import meshsmooth_scenes as SS
import meshtri_restatement as MT
import meshtri_scenes as TS


def test_padded_moves_every_index_and_nothing_else():
    V, T = S.grid(3, 2)
    free = np.arange(len(V)) % 2 == 0
    V2, T2, free2 = S.padded(V, T, 7, free)
    assert len(V2) == len(V) + 7 and T2.min() == 7 and np.array_equal(T2 - 7, T) and np.array_equal(V2[7:], V)
    assert not free2[:7].any() and np.array_equal(free2[7:], free)
    assert [S.radix_passes(x) for x in (0, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, 1 << 40)] == [1, 1, 2, 2, 3, 3, 4, 4]


# ---------------------------------------------------------------------------------------------------------- fairing
@pytest.mark.parametrize("name", list(S.FAIR))
def test_fair_invariants(name):
    V0, T, free, att, tol, max_it = S.fair_case(name)
    V, A, it = S.fair_reference(name)
    assert len(free) == len(V0) and T.max() < len(V0) and len(A) == len(att) == len(S.FAIR[name][3])
    assert np.array_equal(V[~free], V0[~free]) and (it >= 1).all() and (it <= max_it).all()
    for x, x0, width in zip(A, att, S.FAIR[name][3]):
        assert x.shape == (len(V0), width) and np.array_equal(x[~free], x0[~free]) and not np.array_equal(x[free], x0[free])


def test_fair_reaches_four_pairs_of_pass_counts():
    """fair_build sorts by target with radix_passes(M - 1) passes and by source with radix_passes(n - 1); fair_step and fair_lds
    find the sorted arrays from the parity of the two."""
    pairs = {}
    for name in ("passes_1_1", "passes_2_1", "passes_3_1", "passes_3_2"):
        V, _, free, _, _, _ = S.fair_case(name)
        pairs[name] = (S.radix_passes(len(V) - 1), S.radix_passes(int(free.sum()) - 1))
        assert len(np.unique(S.fair_reference(name)[2])) == len(S.fair_reference(name)[2])       # patches that stop on their own
    assert pairs == {"passes_1_1": (1, 1), "passes_2_1": (2, 1), "passes_3_1": (3, 1), "passes_3_2": (3, 2)}
    assert len(S.fair_case("passes_1_1")[0]) - 1 == 255 and len(S.fair_case("passes_2_1")[0]) - 1 == 256
    for name in ("passes_3_1", "passes_3_2"):
        V, T, free, _, _, _ = S.fair_case(name)
        assert len(V) > 65536 and T.min() >= 65536
    assert int(S.fair_case("passes_3_1")[2].sum()) <= 256 < int(S.fair_case("passes_3_2")[2].sum()) <= 65536
    assert len(S.fair_reference("passes_3_1")[2]) == 2


def test_fan_rows_cross_the_chunks_of_both_kernels():
    """membrane() reads a row 32 entries at a time and the LDS kernel 16, both carry `prev` across to skip a twin."""
    rows = {name: S.sorted_row(S.fair_case(name)[1], 0) for name in S.FAIR if name.startswith("fan")}
    assert [len(rows[k]) for k in ("fan17", "fan33", "fan17_open", "fan33_open", "fan33_open2", "fan33_open_rim")] == [34, 66, 32, 64, 62, 64]
    for name in ("fan17", "fan33"):                                 # closed: every spoke twice, the pairs aligned
        assert np.array_equal(rows[name][0::2], rows[name][1::2]) and S.twins_across(rows[name], 16) == 0
    assert S.twins_across(rows["fan17_open"], 16) >= 1
    for name in ("fan33_open", "fan33_open2", "fan33_open_rim"):    # the centre lies on the boundary: an end spoke comes once
        assert S.twins_across(rows[name], 16) >= 1 and S.twins_across(rows[name], 32) >= 1
        free = S.fair_case(name)[2]
        assert free[0] and (S.boundary_edges(S.fair_case(name)[1]) >> 32 == 0).sum() == 2 + 2 * (name == "fan33_open2")
    row, free = rows["fan33_open_rim"], S.fair_case("fan33_open_rim")[2]
    assert row[15] == row[16] == 9 and free[9] and int(free[row].sum()) == 2 and int(free.sum()) == 2     # the free twin straddles
    assert len(S.fair_reference("fan33_open_rim")[2]) == 1          # one patch: the centre's row holds free and fixed entries


def test_patches_stop_and_are_capped_at_the_batch_edges():
    """The driver reads the patches' state every 32 iterations; finish_kernel fills in what was never seen stopped."""
    counts = {name: S.fair_reference(name)[2].tolist() for name in S.FAIR if name.startswith(("stop_", "cap_"))}
    assert counts["stop_32"][0] == 32 and counts["stop_32"][1] > 64
    assert counts["stop_33"][0] == 33 and counts["stop_33"][1] > 64
    assert (counts["cap_31"], counts["cap_32"], counts["cap_33"], counts["cap_64"]) == ([31, 31], [32, 32], [32, 33], [32, 64])
    V, T, free, _, tol, _ = S.fair_case("stop_32")
    d = R.fair_displacements(V, T, free, 40)
    bits = np.array([tol], np.float32).view(np.uint32)[0]
    assert (d[:31, 0] >= bits).all() and d[31, 0] < bits            # the restated sequence: not below before iteration 32


def test_counted_mode_runs_past_a_chunk():
    """The attributes re-run in chunks of 1024 iterations."""
    V, T, free, att, _, _ = S.fair_case("counted")
    it = S.fair_reference("counted")[2]
    assert it.max() > 1024 and [a.shape[1] for a in att] == [1, 7] and int(free.sum()) == 21 * 21
    _, A, _ = S.fair_reference("counted")
    _, short, _ = R.fair(V, T, free, S.fair_case("counted")[4], 1024, att)
    for x, y in zip(A, short):                                      # the iterations of the second chunk still change bits
        assert (x[free].view(np.uint32) != y[free].view(np.uint32)).mean() > 0.9


def test_a_wave_holds_three_patches():
    V, T, free, _, _, _ = S.fair_case("interleaved")
    it = S.fair_reference("interleaved")[2]
    assert max(S.patches_per_wave(T, free, 3)) >= 3 and len(it) == 3 and 3 * it.min() < it.max()


# ------------------------------------------------------------------------------------------------------ subdivision
@pytest.mark.parametrize("name", list(S.SUBDIVIDE))
def test_subdivide_invariants(name):
    V0, T0, region, att, max_len, budget = S.subdivide_case(name)
    (V, T, A, origin, n_splits, rounds), per_round = S.subdivide_reference(name)
    assert rounds == len(per_round) < 256 and n_splits == sum(x[1] for x in per_round) == len(V) - len(V0) <= budget
    reg = np.ones(len(T0), bool) if region is None else region
    if n_splits < budget:
        assert len(R.splittable_lengths(V, T, max_len, reg[origin])) == 0
    assert np.array_equal(origin[:len(T0)], np.arange(len(T0))) and np.array_equal(V[:len(V0)], V0)
    assert np.array_equal(T[:len(T0)][~reg], T0[~reg]) and reg[origin[len(T0):]].all()
    assert len(A) == len(att)
    for x, x0 in zip(A, att):
        assert x.shape == (len(V), x0.shape[1]) and np.array_equal(x[:len(V0)], x0)


@pytest.mark.parametrize("name,budget", [("cut_5000", 5000), ("cut_4096", 4096), ("cut_4097", 4097), ("cut_5000_padded", 5000)])
def test_the_cut_spans_two_sort_tiles(name, budget):
    """6400 diagonals of bit-equal length: the mixed key and the edge key decide which `budget` of them are split, and the
    landing sort runs over more than one tile."""
    _, per_round = S.subdivide_reference(name)
    assert [(x[0], x[1]) for x in per_round] == [(6400, budget)] and 6400 > S.KTILE
    _, _, rd, sel = per_round[0]
    everyone = np.flatnonzero(rd.selected)
    assert len(np.unique(rd.length[everyone].view(np.uint32))) == 1
    assert rd.rank[sel].max() < np.sort(rd.rank[everyone])[budget]  # the first in priority
    slots = everyone[np.argsort(rd.owner_slot(everyone))]
    assert not np.array_equal(np.sort(slots[:budget]), np.sort(sel))        # and not the first in slot order


def test_the_cut_at_the_index_digits_edges():
    for name, top, passes in (("cut_m255", 255, 1), ("cut_m256", 256, 2), ("cut_5000_padded", None, 3)):
        V, T, _, _, _, _ = S.subdivide_case(name)
        _, per_round = S.subdivide_reference(name)
        assert S.radix_passes(len(V) - 1) == passes and (top is None or len(V) - 1 == top) and per_round[0][1] < per_round[0][0]
    V, T, _, _, _, _ = S.subdivide_case("cut_5000_padded")
    assert T.min() >= 65536


def test_the_cut_falls_in_the_third_round():
    _, _, _, _, _, budget = S.subdivide_case("late_cut")
    (_, _, _, _, n_splits, rounds), per_round = S.subdivide_reference("late_cut")
    assert rounds == 3 and n_splits == budget
    assert all(x[0] == x[1] for x in per_round[:2]) and 0 < per_round[2][1] < per_round[2][0]


def test_region_with_two_attributes():
    V0, T0, region, att, _, _ = S.subdivide_case("region_widths")
    (V, T, A, origin, n_splits, rounds), _ = S.subdivide_reference("region_widths")
    assert [a.shape[1] for a in A] == [1, 5] and 0 < region.sum() < len(region) and n_splits > 0 and rounds >= 2


# ------------------------------------------------------------------------------------- triangulation and flips
@pytest.mark.parametrize("metric", ["area", "angle_area"])
def test_fans_and_triangulations_interleave(metric):
    """face_base, area_slot and the fans' places `at` with both kinds of loop in one call."""
    n_edges, filled = S.loop_sizes("mixed")
    _, _, _, n_filled, info = S.triangulate_reference("mixed", metric)
    code = info["fallback"].tolist()
    assert code == [MT.NOT_SIMPLE, 0, 0, MT.TOO_SHORT, 0, 0, MT.TOO_LONG, MT.TOO_LONG, 0, 0]
    assert info["n_fans"] >= 2 and info["n_triangulated"] >= 2 and n_filled == 10 and not filled.all()
    assert n_edges[filled].tolist() == [32, 9, 9, 2, 14, 14, TS.MAX_LOOP + 1, TS.MAX_LOOP + 1, 5, 5]
    assert len(info["area"]) == info["n_triangulated"] == 6


@pytest.mark.parametrize("metric,cutoff", [("area", TS.LDS_LOOP), ("angle_area", SS.ANGLE_LDS_LOOP)])
def test_several_slab_loops_beside_the_other_instances(metric, cutoff):
    """slab_offset[l] > 0 for every slab loop but the first, and small, LDS and slab instances in one launch (paths == 7)."""
    n_edges, filled = S.loop_sizes("slabs")
    _, _, _, n_filled, info = S.triangulate_reference("slabs", metric)
    assert filled.all() and n_filled == 8 and info["n_fans"] == 0
    n = n_edges
    assert int((n > cutoff).sum()) == 4 and int((n <= SS.SMALL_LOOP).sum()) >= 1 and int(((n > SS.SMALL_LOOP) & (n <= cutoff)).sum()) >= 1
    entries = np.where(n > cutoff, n * (n - 1) // 2, 0)
    assert (np.cumsum(entries) - entries)[n > cutoff].tolist() == [0, 17955, 35910, 55810]
    assert n.max() <= TS.MAX_LOOP


def test_high_indices_in_triangulation_and_flips():
    V, T, _, _ = S.triangulate_case("three_loops_padded")
    assert T.min() >= 65536
    for metric in ("area", "angle_area"):
        info = S.triangulate_reference("three_loops_padded", metric)[4]
        assert info["fallback"].tolist() == [0, 0]
    for name in S.FLIP:
        assert S.flip_case(name)[1].min() >= 65536
    (_, n_flips, rounds), per_round = S.flip_reference("grid37x41_padded")
    assert rounds == len(per_round) >= 3 and n_flips > 1000
    assert S.flip_reference("octahedron_padded")[1] == [(2, 1)]     # two flips want one edge: one waits


# --------------------------------------------------------------------------------------------------------- the fill
N_FILLED = {"three_holes": 3, "bumpy_holes": 3, "capped_sphere": 4, "holes_and_tie": 4, "shared_budget": 3, "three_holes_padded": 3}


@pytest.mark.parametrize("how", list(S.HOW))
@pytest.mark.parametrize("name", list(S.FILL))
def test_fill_invariants(name, how):
    V0, T0, att, size, max_len, kw = S.fill_case(name)
    (V, T, A, n_filled, info), passes = S.fill_reference(name, how)
    assert n_filled == N_FILLED[name] == len(info["iterations"]) and info["passes"] == len(passes)
    if how == "smooth":
        assert len(info["curvature_iterations"]) == len(info["curvature_converged"]) == len(info["curvature_code"]) == n_filled
        assert info["curvature_converged"].all() and (info["curvature_code"] == 0).all()
    assert np.array_equal(V[:len(V0)], V0) and np.array_equal(T[:len(T0)], T0) and np.array_equal(A[0][:len(V0)], att[0])     # the prefix
    assert info["n_new_vertices"] == len(V) - len(V0) == info["n_splits"] + info["n_fans"]
    assert S.edge_counts(T)[2] == (name == "holes_and_tie")         # (the fan's spoke to the pinched vertex has four faces)
    assert (info["n_flips"] > 0) == (how != "default") and info["n_triangulated"] + info["n_fans"] == n_filled
    loop, edges, _, perimeter = MC.mesh_holes(V0, T0)
    keys = (edges.min(1).astype(np.int64) << 32) | edges.max(1).astype(np.int64)
    after = S.boundary_edges(T)
    gone = (perimeter < size)[loop]
    assert int((perimeter < size).sum()) == n_filled
    assert not np.isin(keys[gone], after).any() and np.array_equal(np.sort(keys[~gone]), after)      # filled: none; unfilled: all


def test_fill_cases_are_what_they_are_for():
    _, _, n_edges, _ = MC.mesh_holes(*S.fill_case("capped_sphere")[:2])
    assert sorted(n_edges.tolist()) == [25, 33, 36, 40]            # four caps of different size, 24 - 42 rim edges
    V0, T0 = S.fill_case("capped_sphere")[:2]
    valence = np.bincount(np.unique(np.sort(np.concatenate([T0[:, [0, 1]], T0[:, [1, 2]], T0[:, [2, 0]]]), 1), axis=0).reshape(-1))
    assert len(S.boundary_edges(S.fill_reference("capped_sphere", "smooth")[0][1])) == 0 and valence.max() == 6
    V, _ = S.fill_case("bumpy_holes")[:2]
    assert len(np.unique(V[:, 2])) > 4000                           # nothing planar, nothing regular
    for how in ("min_area", "smooth"):                              # the pinched loop gets the fan, the others the triangulation
        info = S.fill_reference("holes_and_tie", how)[0][4]
        assert (info["n_fans"], info["n_triangulated"]) == (1, 3)
    assert S.fill_case("three_holes_padded")[1].min() >= 65536
    V, T = S.capped_sphere(3, 0.3, (0.1, -0.05, 0.2))               # (what finish_mesh is given: four holes, all below its limit)
    _, _, n_edges, perimeter = MC.mesh_holes(V, T)
    assert len(n_edges) == 4 and len(set(n_edges.tolist())) >= 3 and perimeter.max() < 3.0


@pytest.mark.parametrize("how", list(S.HOW))
def test_the_budget_is_shared_and_spent(how):
    V0, T0, _, _, _, kw = S.fill_case("shared_budget")
    (V, _, _, n_filled, info), passes = S.fill_reference("shared_budget", how)
    budget = kw["max_edge_splits"] * n_filled
    assert info["n_splits"] == budget < S.fill_reference("three_holes", how)[0][4]["n_splits"]       # the budget ended the splits
    new = V[len(V0):]
    per_hole = [int(((new[:, 0] > x0) & (new[:, 0] < x1) & (new[:, 1] > y0) & (new[:, 1] < y1)).sum()) for x0, x1, y0, y1 in S.HOLE_BOXES]
    assert sum(per_hole) == len(new) and max(per_hole) > kw["max_edge_splits"] + 1     # one hole takes more than its share
    if how != "default":                                            # the pass loop ends on n_splits >= budget: flips were made,
        assert passes[-1][1] > 0 and info["passes"] < 4             # and max_passes was not reached
