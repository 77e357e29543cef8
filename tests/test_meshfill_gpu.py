"""GPU: subdivision, fairing and the nice hole fill (csrc/meshfill.hip) against tests/meshfill_restatement.py.  Every case
compares with the restatement for equality (position and attribute bits, triangles, origin, counts) and a second run with the
first.  What is asserted about a result beyond that was first checked on the restatement's output, on the CPU
(tests/test_meshfill_host.py)."""
import numpy as np
import pytest
import torch

import meshfill_restatement as R
import meshfill_scenes as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(x):
    return x.detach().cpu().numpy().view(np.int32)


def _same_bits(got, ref):
    assert tuple(got.shape) == ref.shape and np.array_equal(_bits(got), np.ascontiguousarray(ref).view(np.int32))


def _same_all(a, b):
    """Two results of one call: tensors by their bits, tuples and dicts entry by entry, the rest by value."""
    assert type(a) is type(b)
    if isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same_all(x, y)
    elif isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            _same_all(a[k], b[k])
    else:
        assert a == b


# ------------------------------------------------------------------------------------------------------ subdivision
def _subdivide(name, dtype=torch.int64):
    from collab_splats_amd import subdivide_mesh
    V, T, region, att, max_len, budget = S.subdivide_case(name)
    args = (_t(V), _t(T, dtype), max_len, budget, None if region is None else _t(region), tuple(_t(a) for a in att))
    got = subdivide_mesh(*args)
    _same_all(got, subdivide_mesh(*args))
    v, t, a, origin, n_splits, rounds = got
    (rv, rt, ra, ro, rn, rr), _ = S.subdivide_reference(name)
    assert t.dtype == dtype and origin.dtype == torch.int64 and (n_splits, rounds) == (rn, rr)
    assert tuple(t.shape) == rt.shape and np.array_equal(t.cpu().numpy().astype(np.int64), rt)
    assert np.array_equal(origin.cpu().numpy(), ro)
    _same_bits(v, rv)
    assert len(a) == len(ra)
    for x, rx in zip(a, ra):
        _same_bits(x, rx)
    return (V, T, region, att, max_len, budget), got


def test_one_triangle_one_split():
    (V, _, _, _, _, _), (v, t, _, origin, n_splits, rounds) = _subdivide("one_triangle")
    assert (n_splits, rounds) == (1, 1) and t.shape[0] == 2 and origin.tolist() == [0, 0]
    assert v[3].tolist() == [2.0, 0.5, 0.0]                         # the midpoint of the hypotenuse, exact
    assert t.tolist() == [[1, 3, 0], [3, 2, 0]]


def test_two_triangles_split_their_diagonal():
    (V, T, _, _, _, _), (v, t, _, origin, n_splits, _) = _subdivide("two_triangles")
    assert n_splits == 1 and t.shape[0] == 4 and v[4].tolist() == [0.5, 0.5, 0.0]
    n = S.face_normals(v.cpu().numpy(), t.cpu().numpy())
    assert (n[:, 2] > 0).all() and sorted(origin.tolist()) == [0, 0, 1, 1]


def test_equal_spokes_are_decided_by_the_mixed_key():
    _, (v, t, _, _, n_splits, rounds) = _subdivide("equal_spokes")
    _, per_round = S.subdivide_reference("equal_spokes")
    assert per_round[0][0] > 1 and n_splits == 12 and rounds == len(per_round)


def test_region_border_is_never_split():
    (V, T, region, _, _, _), (v, t, _, origin, _, _) = _subdivide("strip_half")
    out = ~region
    assert np.array_equal(t.cpu().numpy()[:len(T)][out], T[out])    # faces outside the region: their slot, their bits
    inside = region[origin.cpu().numpy()]
    assert np.array_equal(np.flatnonzero(~inside), np.flatnonzero(out))
    border = np.intersect1d(S.boundary_edges(T[region]), S.boundary_edges(T[out]))
    assert len(border) == 1 and np.isin(border, S.boundary_edges(t.cpu().numpy()[inside])).all()


def test_budget_takes_the_first_in_priority():
    (V, T, _, _, _, budget), (v, t, _, _, n_splits, rounds) = _subdivide("budget")
    _, per_round = S.subdivide_reference("budget")
    assert per_round == [(64, 10)] and n_splits == budget and rounds == 1 and v.shape[0] == len(V) + budget


def test_icosahedron_stays_closed():
    from collab_splats_amd import mesh_edge_stats
    (_, _, _, _, max_len, _), (v, t, _, _, _, _) = _subdivide("icosahedron")
    st = mesh_edge_stats(v, t)
    assert st["n_boundary"] == 0 and st["n_nonmanifold"] == 0 and v.shape[0] - st["n_edges"] + t.shape[0] == 2
    assert len(R.splittable_lengths(v.cpu().numpy(), t.cpu().numpy(), max_len)) == 0


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_grid_of_several_workgroups(dtype):
    (V, T, _, _, _, _), (v, t, _, _, _, rounds) = _subdivide("grid37x41", dtype)
    assert (3 * len(T)) % 256 != 0 and 3 * len(T) > 4 * 256 and rounds >= 2
    assert abs(S.total_area(v.cpu().numpy(), t.cpu().numpy()) - 37 * 41) == 0


def test_defects_are_carried_not_split():
    (V, T, _, _, _, _), (v, t, _, origin, _, _) = _subdivide("defective")
    tt = t.cpu().numpy()
    assert np.array_equal(tt[8], T[8]) and (origin == 8).sum() == 1  # the face with the repeated corner
    keys = (np.sort(tt[:, [0, 1]], 1), np.sort(tt[:, [1, 2]], 1), np.sort(tt[:, [2, 0]], 1))
    shared = sum(int(((k[:, 0] == 0) & (k[:, 1] == 1)).sum()) for k in keys)
    assert shared == 4                                              # the non-manifold edge 0 - 1 still has its four faces


# ---------------------------------------------------------------------------------------------------------- fairing
def _fair(name, lds=True):
    from collab_splats_amd import fair_vertices, meshfill
    V, T, free, att, tol, max_it = S.fair_case(name)
    args = (_t(V), _t(T), _t(free), tol, max_it, tuple(_t(a) for a in att))
    saved = meshfill.ENABLE_LDS_FAIR
    meshfill.ENABLE_LDS_FAIR = lds
    try:
        got = fair_vertices(*args)
        _same_all(got, fair_vertices(*args))
    finally:
        meshfill.ENABLE_LDS_FAIR = saved
    v, a, it = got
    rv, ra, rit = S.fair_reference(name)
    assert it.dtype == torch.int32 and np.array_equal(it.cpu().numpy(), rit)
    _same_bits(v, rv)
    for x, rx in zip(a, ra):
        _same_bits(x, rx)
    return (V, T, free, att), got


@pytest.mark.parametrize("lds", [True, False])
def test_single_fan_moves_to_the_mean_of_its_rim(lds):
    (V, _, _, _), (v, _, it) = _fair("single_fan_once", lds)
    mean = (V[1:].astype(np.float64).sum(0) / 12.0).astype(np.float32)          # (numpy adds the twelve rows in order)
    assert it.tolist() == [1] and np.array_equal(_bits(v[0]), mean.view(np.int32))
    assert torch.equal(v[1:].cpu(), torch.from_numpy(V[1:]))
    _, (_, _, it) = _fair("single_fan", lds)
    assert it.tolist() == [2]                                       # the second iteration does not move it: it stops there


@pytest.mark.parametrize("lds", [True, False])
def test_patches_stop_on_their_own(lds):
    (V, _, free, _), (v, a, it) = _fair("two_patches", lds)
    counts = it.tolist()
    assert len(counts) == 3 and counts[0] != counts[1] and counts[2] == 1 and max(counts) < 10000
    lone = len(V) - 3
    assert torch.equal(v[lone].cpu(), torch.from_numpy(V[lone]))    # no neighbour: unchanged
    fixed = torch.from_numpy(~free)
    assert torch.equal(v.cpu()[fixed], torch.from_numpy(V)[fixed])


def test_lds_path_equals_the_launch_per_iteration():
    """A patch of exactly LDS_MAX_VERTICES free vertices (one workgroup takes it) and one of a vertex more (it does not), on
    both paths: the same bits and the same counts as the restatement, hence as each other."""
    from collab_splats_amd import meshfill
    assert meshfill.LDS_MAX_VERTICES == S.LDS_MAX_VERTICES
    (_, _, free, _), (v1, a1, it1) = _fair("cutoff", True)
    _, (v0, a0, it0) = _fair("cutoff", False)
    _same_all((v1, a1, it1), (v0, a0, it0))
    assert it1.shape[0] == 2 and int(free.sum()) == 2 * S.LDS_MAX_VERTICES + 1


# --------------------------------------------------------------------------------------------------------- the fill
def _fill(name):
    from collab_splats_amd import fill_holes, fill_holes_nicely
    V, T, att, size, max_len = S.fill_case(name)
    args = (_t(V), _t(T), size, max_len)
    kw = dict(attributes=tuple(_t(a) for a in att))
    got = fill_holes_nicely(*args, **kw)
    _same_all(got, fill_holes_nicely(*args, **kw))
    v, t, a, n_filled, info = got
    rv, rt, ra, rn, rinfo = S.fill_reference(name)
    assert n_filled == rn == fill_holes(_t(V), _t(T), size)[3]
    assert (info["n_splits"], info["rounds"], info["n_new_vertices"]) == (rinfo["n_splits"], rinfo["rounds"], rinfo["n_new_vertices"])
    assert np.array_equal(info["iterations"].cpu().numpy(), rinfo["iterations"])
    assert np.array_equal(t.cpu().numpy(), rt)
    _same_bits(v, rv)
    _same_bits(a[0], ra[0])
    assert np.array_equal(_bits(v[:len(V)]), V.view(np.int32)) and np.array_equal(t.cpu().numpy()[:len(T)], T)      # the prefix
    assert np.array_equal(_bits(a[0][:len(V)]), att[0].view(np.int32))
    return (V, T, att), got


def test_fill_open_cube():
    from collab_splats_amd import mesh_edge_stats
    (V, T, att), (v, t, a, n_filled, info) = _fill("open_cube")
    st = mesh_edge_stats(v, t)
    assert n_filled == 1 and st["n_boundary"] == 0 and st["n_nonmanifold"] == 0 and v.shape[0] - st["n_edges"] + t.shape[0] == 2
    assert info["n_splits"] > 0 and info["n_new_vertices"] == info["n_splits"] + 1 and 0 < int(info["iterations"].max()) < 10000
    b = S.boundary_edges(T)
    rim = np.unique(np.concatenate([b >> 32, b & 0xFFFFFFFF]))
    lo, hi = att[0][rim].min(0), att[0][rim].max(0)
    new = a[0][len(V):].cpu().numpy()
    assert (new >= lo).all() and (new <= hi).all()                  # a mean of means of the rim's colours


def test_fill_sheet_leaves_the_large_hole():
    from collab_splats_amd import mesh_edge_stats
    (V, T, _), (v, t, _, n_filled, info) = _fill("holed_sheet")
    before, after = S.boundary_edges(T), S.boundary_edges(t.cpu().numpy())
    small = before[np.isin(before >> 32, S._block(32, 4, 9, 4, 9)) & np.isin(before & 0xFFFFFFFF, S._block(32, 4, 9, 4, 9))]
    assert n_filled == 1 and len(small) == 16 and not np.isin(small, after).any()
    assert np.array_equal(np.setdiff1d(before, small), after)       # the large hole's and the outline's edges are all still there
    assert mesh_edge_stats(v, t)["n_nonmanifold"] == 0
    assert bool((v[len(V):, 2] == 0).all()) and v.shape[0] > len(V) + 1         # a planar rim: every created vertex at z = 0 exactly


def test_fill_default_edge_length_is_the_mean_before_the_fill():
    from collab_splats_amd import fill_holes_nicely, mesh_edge_stats
    V, T, _, size, _ = S.fill_case("holed_sheet")
    mean = mesh_edge_stats(_t(V), _t(T))["mean_edge_length"]
    _same_all(fill_holes_nicely(_t(V), _t(T), size), fill_holes_nicely(_t(V), _t(T), size, mean, tolerance=float(R.default_tolerance(mean))))


def test_finish_mesh_fill_keyword():
    import tsdf_scenes
    V, T = S.icosphere(3, 0.3, (0.1, -0.05, 0.2))
    T = T[~np.isin(T, np.flatnonzero(V[:, 1] > 0.2)).any(1)]        # a cap cut off: one hole
    v, t, c = _t(V), _t(T), _t(S.colour_ramp(V))
    model = tsdf_scenes.sphere_gaussians(2000).to(DEV)
    model.eval()
    fan = model.finish_mesh(v, t, c, align=False)
    _same_all(fan, model.finish_mesh(v, t, c, align=False))
    nice = model.finish_mesh(v, t, c, align=False, fill="nicely")
    _same_all(fan, model.finish_mesh(v, t, c, align=False, fill="fan"))
    assert set(nice) == set(fan) | {"fill_info"} and nice["n_filled"] == fan["n_filled"] == 1
    m = nice["vertices"].shape[0]
    created = nice["fill_info"]["n_new_vertices"]
    assert created > 1 and m == fan["vertices"].shape[0] - 1 + created
    for k in ("colors", "normals"):
        assert nice[k].shape == (m, 3)
    index = nice["vertex_index"]
    assert index.shape == (m,) and bool((index[m - created:] == -1).all()) and bool((index[:m - created] >= 0).all())
    assert int(nice["triangles"].max()) == m - 1
