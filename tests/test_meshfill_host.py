"""CPU: the public surface of the hole fill (exports, entry points, argument checks before any GPU use) and the invariants of
tests/meshfill_restatement.py on every scene of tests/meshfill_scenes.py: what the GPU tests assert about a result beyond its
equality with the restatement is established here, on the restatement."""
import os
import re

import numpy as np
import pytest
import torch

import meshfill_restatement as R
import meshfill_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------- surface
def test_exports_and_entry_points():
    import collab_splats_amd as m
    from collab_splats_amd import _lib, meshfill
    for name in ("subdivide_mesh", "fair_vertices", "fill_holes_nicely"):
        assert callable(getattr(m, name)) and name in meshfill.__all__
    for name in ("workspace", "round", "apply", "fair_workspace", "fair_count", "fair_build", "fair_step", "fair_lds", "fair_finish"):
        assert "misplat_meshfill_" + name in _lib.SYMBOLS


def test_the_cutoff_is_one_number():
    from collab_splats_amd import meshfill
    header = open(os.path.join(ROOT, "include", "misplat.h")).read()
    assert int(re.search(r"#define MISPLAT_MESHFILL_LDS_VERTICES (\d+)", header).group(1)) == meshfill.LDS_MAX_VERTICES == S.LDS_MAX_VERTICES
    assert 24 * meshfill.LDS_MAX_VERTICES + 1024 <= 160 * 1024       # both iterates and the waves' maxima fit a workgroup's LDS


def _mesh():
    V, T = S.two_triangles()
    return torch.from_numpy(V), torch.from_numpy(T)


@pytest.mark.parametrize("kw", [dict(max_edge_len=0.0), dict(max_edge_len=float("nan")), dict(max_edge_len=-1.0),
                                dict(max_edge_splits=-1), dict(max_edge_splits=1.5), dict(max_rounds=True),
                                dict(region=torch.ones(3, dtype=torch.bool)), dict(region=torch.ones(2, dtype=torch.uint8)),
                                dict(attributes=(torch.zeros(3, 2),)), dict(attributes=(torch.zeros(4, 2, dtype=torch.float64),)),
                                dict(max_edge_splits=1 << 28)])
def test_subdivide_arguments(kw):
    from collab_splats_amd import subdivide_mesh
    v, t = _mesh()
    args = dict(max_edge_len=0.5)
    args.update(kw)
    with pytest.raises(ValueError, match="subdivide_mesh"):
        subdivide_mesh(v, t, **args)


@pytest.mark.parametrize("kw", [dict(free=torch.ones(3, dtype=torch.bool)), dict(free=torch.ones(4)), dict(tolerance=0.0),
                                dict(tolerance=float("inf")), dict(max_iterations=-1), dict(max_iterations=2.0),
                                dict(attributes=(torch.zeros(4),))])
def test_fair_arguments(kw):
    from collab_splats_amd import fair_vertices
    v, t = _mesh()
    args = dict(free=torch.ones(4, dtype=torch.bool), tolerance=1e-3)
    args.update(kw)
    with pytest.raises(ValueError, match="fair_vertices"):
        fair_vertices(v, t, **args)


@pytest.mark.parametrize("kw", [dict(max_hole_size="wide"), dict(max_edge_len=0.0), dict(tolerance=-1.0), dict(max_edge_splits=-3),
                                dict(max_iterations=None), dict(attributes=(torch.zeros(4, 3, dtype=torch.int32),))])
def test_fill_arguments(kw):
    from collab_splats_amd import fill_holes_nicely
    v, t = _mesh()
    with pytest.raises(ValueError, match="fill_holes_nicely"):
        fill_holes_nicely(v, t, **kw)


def test_bad_triangles_and_cpu_tensors():
    from collab_splats_amd import MisplatError, fair_vertices, fill_holes_nicely, subdivide_mesh
    v, t = _mesh()
    with pytest.raises(ValueError, match="triangle indices"):
        subdivide_mesh(v, t + 2, 0.5)
    with pytest.raises(MisplatError, match="no CPU fallback"):
        subdivide_mesh(v, t, 0.5)
    with pytest.raises(MisplatError, match="no CPU fallback"):
        fair_vertices(v, t, torch.ones(4, dtype=torch.bool), 1e-3)
    with pytest.raises(MisplatError, match="no CPU fallback"):
        fill_holes_nicely(v, t)


def test_finish_mesh_refuses_an_unknown_fill():
    import tsdf_scenes
    v, t = _mesh()
    model = tsdf_scenes.sphere_gaussians(16)
    with pytest.raises(ValueError, match="fill must be 'fan' or 'nicely'"):
        model.finish_mesh(v, t, torch.zeros(4, 3), fill="bogus")


# ------------------------------------------------------------------------------------------------------ restatement
def test_mix32_is_the_shared_hash():
    import meshclean_restatement as MC
    for seed, i, draw in ((0, 0, 0), (7, 12345, 3), (0xFFFFFFFF, 0xFFFFFFFE, 0), (3, 9, 0)):
        assert (int(R.mix32(seed, i, draw)) * 1000) >> 32 == MC.draw_index(seed, i, draw, 1000)


def _euler(V, T):
    used = len(np.unique(T))
    return used - S.edge_counts(T)[0] + len(T)


@pytest.mark.parametrize("name", list(S.SUBDIVIDE))
def test_subdivide_invariants(name):
    V0, T0, region, att, max_len, budget = S.subdivide_case(name)
    (V, T, A, origin, n_splits, rounds), per_round = S.subdivide_reference(name)
    assert rounds < 256 and rounds == len(per_round) and n_splits == sum(x[1] for x in per_round) == len(V) - len(V0)
    assert _euler(V, T) == _euler(V0, T0)
    e0, b0, n0 = S.edge_counts(T0)
    e1, b1, n1 = S.edge_counts(T)
    assert n1 == n0 and (b1 == 0) == (b0 == 0)                      # watertight stays watertight, no edge becomes non-manifold
    reg = np.ones(len(T0), bool) if region is None else region
    if n_splits < budget:
        assert len(R.splittable_lengths(V, T, max_len, reg[origin])) == 0
    assert np.array_equal(origin[:len(T0)], np.arange(len(T0))) and np.array_equal(V[:len(V0)], V0)
    assert np.array_equal(T[:len(T0)][~reg], T0[~reg]) and reg[origin[len(T0):]].all()
    n0, n1 = S.face_normals(V0, T0), S.face_normals(V, T)
    assert ((n0[origin] * n1).sum(1) >= 0).all()                    # orientation is kept
    assert abs(S.total_area(V, T) - S.total_area(V0, T0)) <= 1e-6 * max(1.0, S.total_area(V0, T0))
    for x, x0 in zip(A, att):
        assert x.shape == (len(V), x0.shape[1]) and x.min() >= x0.min() and x.max() <= x0.max()


def test_subdivide_cases_are_what_they_are_for():
    per_round = {name: S.subdivide_reference(name)[1] for name in S.SUBDIVIDE}
    assert per_round["one_triangle"] == [(1, 1)] and per_round["two_triangles"] == [(1, 1)]
    assert per_round["equal_spokes"][0][0] > 1                      # equal lengths: the mixed key selects several spokes at once
    V, T = S.equal_spoke_fan()
    assert len(np.unique(R.edge_length(V, np.zeros(12, np.int64), np.arange(1, 13)).view(np.uint32))) == 1
    assert per_round["budget"] == [(64, 10)]                        # more selected than the budget leaves
    V, T, _, _, _, _ = S.subdivide_case("grid37x41")
    assert (3 * len(T)) % 256 != 0 and 3 * len(T) > 4 * 256


def test_budget_keeps_the_first_in_priority():
    V0, T0, _, att, max_len, budget = S.subdivide_case("budget")
    taken = []
    R.subdivide(V0, T0, max_len, budget, on_round=lambda rd, sel: taken.append((rd, sel)))
    rd, sel = taken[0]
    everyone = np.flatnonzero(rd.selected)
    assert len(sel) == budget and rd.rank[sel].max() < np.sort(rd.rank[everyone])[budget]


def test_dyadic_grid_keeps_its_area_exactly():
    V0, T0 = S.sheet(8)                                             # coordinates k / 8: every midpoint down to 2^-10 is exact
    V, T, _, _, n_splits, rounds = R.subdivide(V0, T0, 1.0 / 32)
    assert n_splits > 1000 and rounds < 256 and len(R.splittable_lengths(V, T, 1.0 / 32)) == 0
    assert np.array_equal(V * 1024, np.round(V * 1024)) and S.total_area(V, T) == 1.0


@pytest.mark.parametrize("name", list(S.FAIR))
def test_fair_invariants(name):
    V0, T, free, att, tol, max_it = S.fair_case(name)
    V, A, it = S.fair_reference(name)
    assert np.array_equal(V[~free], V0[~free]) and np.array_equal(A[0][~free], att[0][~free])
    if name == "single_fan_once":
        assert it.tolist() == [1]
        return
    assert (it >= 1).all() and (it < max_it).all()
    again, _, more = R.fair(V, T, free, tol, max_it)                # a faired patch stops at once
    assert (more == 1).all() and np.abs(again - V).max() < tol
    assert A[0][free].min() >= att[0].min() and A[0][free].max() <= att[0].max()


def test_fair_cases_are_what_they_are_for():
    assert S.fair_reference("single_fan")[2].tolist() == [2]
    it = S.fair_reference("two_patches")[2].tolist()
    assert len(it) == 3 and it[0] != it[1] and it[2] == 1
    V, T, free, _, _, _ = S.fair_case("cutoff")
    _, _, _, patch = R.free_rows(T, free)
    assert sorted(np.bincount(patch).tolist()) == [S.LDS_MAX_VERTICES, S.LDS_MAX_VERTICES + 1]


@pytest.mark.parametrize("name", list(S.FILL))
def test_fill_invariants(name):
    import meshclean_restatement as MC
    V0, T0, att, size, max_len = S.fill_case(name)
    V, T, A, n_filled, info = S.fill_reference(name)
    assert n_filled == MC.fill_holes(V0, T0, size)[2] == 1 and info["n_new_vertices"] == info["n_splits"] + n_filled
    assert info["rounds"] < 256 and (info["iterations"] < 10000).all() and info["n_splits"] > 0
    assert np.array_equal(V[:len(V0)], V0) and np.array_equal(T[:len(T0)], T0) and np.array_equal(A[0][:len(V0)], att[0])
    assert S.edge_counts(T)[2] == 0
    fan = MC.fill_holes(V0, T0, size)[1]
    assert np.array_equal(S.boundary_edges(T), S.boundary_edges(fan))
    if name == "holed_sheet":
        assert (V[len(V0):, 2] == 0).all() and len(S.boundary_edges(T)) == 64 + 128
    else:
        assert len(S.boundary_edges(T)) == 0 and _euler(V, T) == 2
