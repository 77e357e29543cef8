"""CPU: the public surface of the hole triangulation and the edge flips (exports, entry points, constants, argument checks before
any GPU use) and the invariants of tests/meshtri_restatement.py on every scene of tests/meshtri_scenes.py: what the GPU tests
assert about a result beyond its equality with the restatement is established here, on the restatement."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import meshclean_restatement as MC
import meshtri_restatement as R
import meshtri_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------- surface
def test_exports_and_entry_points():
    import collab_splats_amd as m
    from collab_splats_amd import _lib, meshfill
    for name in ("triangulate_holes", "flip_edges"):
        assert callable(getattr(m, name)) and name in meshfill.__all__
    for name in ("order", "workspace", "dp", "flip_workspace", "flip_round"):
        assert "misplat_meshtri_" + name in _lib.SYMBOLS


def test_the_cutoffs_are_one_number_each():
    from collab_splats_amd import meshfill
    header = open(os.path.join(ROOT, "include", "misplat.h")).read()
    lds = int(re.search(r"#define MISPLAT_MESHTRI_LDS_LOOP (\d+)", header).group(1))
    most = int(re.search(r"#define MISPLAT_MESHTRI_MAX_LOOP (\d+)", header).group(1))
    assert lds == meshfill.LDS_LOOP == S.LDS_LOOP == R.LDS_LOOP and most == meshfill.MAX_LOOP == S.MAX_LOOP == R.MAX_LOOP
    entries = lds * (lds - 1) // 2
    assert 10 * entries + 16 * lds <= 160 * 1024                    # weights, splits, the polygon's points and indices
    assert 10 * ((lds + 1) * lds // 2) + 16 * (lds + 1) > 154 * 1024   # the next length is over the 154 KB the table is given
    assert most < 1 << 16                                           # a split is kept in 16 bits
    small = int(re.search(r"#define MISPLAT_MESHTRI_SMALL_LOOP (\d+)", header).group(1))
    assert 3 <= small == meshfill.SMALL_LOOP <= lds                 # the host chooses the launches by it, the kernels the loops


def _mesh():
    V, T = S.kite(0.5)
    return torch.from_numpy(V), torch.from_numpy(T)


@pytest.mark.parametrize("kw", [dict(max_hole_size=float("nan")), dict(max_hole_size="wide"), dict(attributes=(torch.zeros(3, 2),)),
                                dict(attributes=(torch.zeros(4, 2, dtype=torch.float64),))])
def test_triangulate_arguments(kw):
    from collab_splats_amd import triangulate_holes
    with pytest.raises(ValueError, match="triangulate_holes"):
        triangulate_holes(*_mesh(), **kw)


@pytest.mark.parametrize("kw", [dict(region=torch.ones(3, dtype=torch.bool)), dict(region=torch.ones(2, dtype=torch.uint8)),
                                dict(max_rounds=-1), dict(max_rounds=1.5), dict(max_rounds=True), dict(min_violation=-1e-9),
                                dict(min_violation=float("nan")), dict(min_violation=float("inf")), dict(min_violation="small")])
def test_flip_arguments(kw):
    from collab_splats_amd import flip_edges
    with pytest.raises(ValueError, match="flip_edges"):
        flip_edges(*_mesh(), **kw)


@pytest.mark.parametrize("kw", [dict(triangulation="delaunay"), dict(max_passes=-1), dict(max_passes=1.5), dict(flip=True, max_passes=0)])
def test_fill_arguments(kw):
    from collab_splats_amd import fill_holes_nicely
    with pytest.raises(ValueError, match="fill_holes_nicely"):
        fill_holes_nicely(*_mesh(), **kw)


def test_no_cpu_fallback():
    from collab_splats_amd import MisplatError, flip_edges, triangulate_holes
    with pytest.raises(MisplatError):
        triangulate_holes(*_mesh())
    with pytest.raises(MisplatError):
        flip_edges(*_mesh())


def test_finish_mesh_names_its_fills():
    import tsdf_scenes
    model = tsdf_scenes.sphere_gaussians(10)
    v, t = _mesh()
    with pytest.raises(ValueError, match="min_area"):
        model.finish_mesh(v, t, torch.zeros(4, 3), fill="nice")


# ---------------------------------------------------------------------------------------------------- triangulation
def _patch(name):
    V, T, att, size = S.triangulate_case(name)
    v, t, a, n_filled, info = S.triangulate_reference(name)
    assert np.array_equal(v[:len(V)].view(np.int32), V.view(np.int32)) and np.array_equal(t[:len(T)], T)     # the prefix
    return V, T, v, t, n_filled, info


@pytest.mark.parametrize("name,polygon", [("convex", S.convex_polygon), ("c_shape", S.c_polygon)])
def test_planar_dyadic_polygons_get_their_area_exactly(name, polygon):
    P = polygon()
    for trio in itertools.combinations(range(len(P)), 3):           # no three on a line: no triangle of the table is degenerate
        assert abs(S.polygon_area(P[list(trio)])) > 0
    V, T, v, t, n_filled, info = _patch(name)
    assert n_filled == 1 and info["n_triangulated"] == 1 and len(v) == len(V) and len(t) == len(T) + len(P) - 2
    assert info["area"][0] == S.polygon_area(P)                     # exactly: every area and every sum is dyadic
    assert (S.face_normals(v, t[len(T):])[:, 2] > 0).all() and (S.face_normals(v, t[len(T):])[:, :2] == 0).all()
    assert S.total_area(v, t[len(T):]) == S.polygon_area(P)


def test_the_fan_of_the_c_shape_is_folded():
    """The defect the minimum-area triangulation removes: the mean of the C's vertices lies outside it."""
    V, T, _, size = S.triangulate_case("c_shape")
    fv, ft, n_filled = MC.fill_holes(V, T, size)
    assert n_filled == 1 and (S.face_normals(fv, ft[len(T):])[:, 2] < 0).any()


@pytest.mark.parametrize("name", ["triangle", "bent_quad", "pentagon", "square_tie", "convex", "c_shape", "three_loops", "cutoff"])
def test_every_apex_once_and_closure(name):
    V, T, v, t, n_filled, info = _patch(name)
    assert info["n_fans"] == 0 and n_filled == info["n_triangulated"] > 0 and len(v) == len(V)
    loop, edges, n_edges, perimeter = MC.mesh_holes(V, T)
    size = S.triangulate_case(name)[3]
    at = len(T)
    for l in np.flatnonzero(perimeter < size):
        code, q = R.loop_polygon(edges[loop == l])
        n = len(q)
        faces = t[at:at + n - 2]
        at += n - 2
        place = {int(x): i for i, x in enumerate(q)}
        ikj = np.array([[place[int(x)] for x in f] for f in faces])
        assert np.array_equal(ikj[:, 1], np.arange(1, n - 1)) and (ikj[:, 0] < ikj[:, 1]).all() and (ikj[:, 1] < ikj[:, 2]).all()
    assert at == len(t)
    e0, b0, _ = S.edge_counts(T)
    e1, b1, nm = S.edge_counts(t)
    chi = lambda n_e, n_t: len(V) - n_e + n_t                       # noqa: E731  (no vertex is created)
    assert nm == 0 and chi(e1, len(t)) == chi(e0, len(T)) + n_filled    # each disc closes one loop: the count of boundary loops falls
    assert b1 == b0 - int(n_edges[perimeter < size].sum())          # the filled rims are closed, no other boundary edge appears


def test_euler_characteristic_rises_by_one_per_closed_loop_and_fans_add_a_vertex():
    V, T, v, t, n_filled, info = _patch("fallbacks")
    assert info["fallback"].tolist() == [R.NOT_SIMPLE, R.TOO_SHORT, R.TOO_LONG, R.TOO_LONG] and info["n_triangulated"] == 0
    assert len(v) == len(V) + info["n_fans"]
    # a fan adds a vertex, a spoke per distinct rim vertex and a face per rim edge: the Euler characteristic rises by 1 for a
    # simple cycle (as many vertices as edges), by 2 for the pinched loop (a vertex fewer), by 0 for the open chain of two edges
    loop, edges, n_edges, perimeter = MC.mesh_holes(V, T)
    rise = sum(1 - len(np.unique(edges[loop == l])) + int(n_edges[l]) for l in np.flatnonzero(perimeter < S.triangulate_case("fallbacks")[3]))
    assert rise == 2 + 0 + 1 + 1 and (len(v) - S.edge_counts(t)[0] + len(t)) - (len(V) - S.edge_counts(T)[0] + len(T)) == rise
    fv, ft, n = MC.fill_holes(V, T, S.triangulate_case("fallbacks")[3])
    assert n == n_filled and np.array_equal(ft, t) and np.array_equal(fv.view(np.int32), v.view(np.int32))   # fill_holes's fans


def test_ties_go_to_the_smallest_k_and_the_smaller_area_wins():
    _, T, _, t, _, info = _patch("square_tie")
    assert t[len(T):].tolist() == [[0, 1, 3], [1, 2, 3]] and info["area"][0] == 1.0
    V, T, _, t, _, info = _patch("bent_quad")
    Q = V[:4]
    other = float(R.area(Q, 0, 1, 2)) + float(R.area(Q, 0, 2, 3))
    assert t[len(T):].tolist() == [[0, 1, 3], [1, 2, 3]] and info["area"][0] < other


def test_three_loops_leave_the_large_one():
    V, T, v, t, n_filled, info = _patch("three_loops")
    assert n_filled == 2 and len(t) == len(T) + 3 + 7
    rim = S.boundary_edges(t)
    on = np.unique(np.concatenate([rim >> 32, rim & 0xFFFFFFFF]))
    assert np.array_equal(on, np.concatenate([np.arange(5, 10), np.arange(19, 56)]))     # the rims 0 .. 4 and 10 .. 18 are closed, 28 .. 41 is not


def test_a_closed_mesh_has_nothing_to_fill():
    V, T, v, t, n_filled, info = _patch("closed")
    assert n_filled == 0 and len(t) == len(T) and info["area"].shape == (0,)


# ------------------------------------------------------------------------------------------------------------ flips
@pytest.mark.parametrize("name", sorted(S.FLIP))
def test_flips_keep_the_mesh_and_end(name):
    V, T, region = S.flip_case(name)
    (t, n_flips, rounds), per_round = S.flip_reference(name)
    assert rounds < 256 and len(per_round) == rounds and n_flips == sum(f for _, f in per_round)
    assert t.shape == T.shape and len(R.flippable_edges(V, t, region)) == 0
    assert np.array_equal(np.sort(np.bincount(t.reshape(-1), minlength=len(V))) > 0, np.sort(np.bincount(T.reshape(-1), minlength=len(V))) > 0)
    assert S.edge_counts(t)[0] == S.edge_counts(T)[0] and S.edge_counts(t)[2] == S.edge_counts(T)[2]
    if np.all(V[:, 2] == 0) and name != "valence_three":            # planar, embedded, dyadic: orientation and area are kept exactly
        assert (S.face_normals(V, t)[:, 2] > 0).all() and S.total_area(V, t) == S.total_area(V, T)
    if region is not None:
        assert np.array_equal(t[~region], T[~region])


def test_flip_scenes_do_what_they_were_chosen_for():
    ref = {name: S.flip_reference(name) for name in S.FLIP}
    assert ref["bad_diagonal"][0][0].tolist() == [[2, 3, 1], [3, 0, 1]] and ref["bad_diagonal"][1] == [(1, 1)]
    for name in ("delaunay_pair", "cocircular", "valence_three", "defective"):
        assert ref[name][0][1:] == (0, 0) and np.array_equal(ref[name][0][0], S.flip_case(name)[1])
    assert ref["octahedron"][1] == [(2, 1)]                         # two selected, both want 4 - 5, one flips; the other is then blocked
    assert S.edge_counts(ref["octahedron"][0][0])[2] == 0
    V, T, region = S.flip_case("region_border")
    border = np.intersect1d(S.boundary_edges(T[region]), S.boundary_edges(T[~region]))
    t = ref["region_border"][0][0]
    assert len(border) > 0 and np.isin(border, S.boundary_edges(t[region])).all() and ref["region_border"][0][1] > 0
    (t, n_flips, rounds), per_round = ref["grid37x41"]
    assert rounds >= 3 and (3 * len(t)) % 256 != 0 and 3 * len(t) > 4 * 256


def test_valence_three_is_blocked_by_the_existing_edge_alone():
    """The edge 0 - 3 violates and would not fold: only the existing edge 1 - 2 keeps it."""
    V, T, _ = S.flip_case("valence_three")
    t, n_flips, _ = R.flip_edges(V, T[:2])                          # without the face that holds 1 - 2
    assert n_flips == 1 and np.array_equal(np.sort(t, 1), [[1, 2, 3], [0, 1, 2]])


# --------------------------------------------------------------------------------------------------------- the fill
@pytest.mark.parametrize("name", sorted(S.FILL))
def test_fill_with_min_area_and_flips(name):
    V, T, att, size, max_len = S.fill_case(name)
    v, t, a, n_filled, info = S.fill_reference(name)
    assert n_filled == 1 and info["n_fans"] == 0 and info["n_triangulated"] == 1 and 1 <= info["passes"] <= 4
    assert info["flip_rounds"] < 256 * info["passes"] and info["n_flips"] > 0 and info["n_new_vertices"] == info["n_splits"] > 0
    assert np.array_equal(v[:len(V)].view(np.int32), V.view(np.int32)) and np.array_equal(t[:len(T)], T)
    before, after = S.boundary_edges(T), S.boundary_edges(t)
    assert S.edge_counts(t)[2] == 0 and np.isin(after, before).all() and len(after) < len(before)
    if name == "open_cube":
        assert len(after) == 0 and len(v) - S.edge_counts(t)[0] + len(t) == 2
    # against the fan pipeline on the same scene: the direction is asserted where the restatement shows it
    fv, ft, _, _, finfo = S.fill_reference(name, "fan", False)
    valence, angle = R.patch_quality(v, t, len(T))
    fan_valence, fan_angle = R.patch_quality(fv, ft, len(T))
    assert valence <= fan_valence
    if name == "c_sheet":
        assert angle >= fan_angle
        assert (S.face_normals(fv, ft[len(T):])[:, 2] < 0).any() and (S.face_normals(v, t[len(T):])[:, 2] > 0).all()


def test_defaults_are_the_fan_pipeline():
    import meshfill_restatement as MF
    V, T, att, size, max_len = S.fill_case("open_cube")
    a = MF.fill_holes_nicely(V, T, size, max_len, attributes=att)
    b = R.fill_holes_nicely(V, T, size, max_len, attributes=att)
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])
    assert {k: b[4][k] for k in ("n_flips", "flip_rounds", "passes", "n_triangulated", "n_fans")} == \
        {"n_flips": 0, "flip_rounds": 0, "passes": 1, "n_triangulated": 0, "n_fans": 1}
