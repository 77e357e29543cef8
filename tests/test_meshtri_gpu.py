"""GPU: the minimum-area hole triangulation and the edge flips (csrc/meshtri.hip) and the fill that uses them against
tests/meshtri_restatement.py.  Every case compares with the restatement for equality (position and attribute bits, triangles,
counts, the fp64 bits of the minima) and a second run with the first.  What is asserted about a result beyond that was first
checked on the restatement's output, on the CPU (tests/test_meshtri_host.py)."""
import numpy as np
import pytest
import torch

import meshtri_restatement as R
import meshtri_scenes as S

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
        floating = {torch.float32: torch.int32, torch.float64: torch.int64}
        assert torch.equal(a.view(floating[a.dtype]) if a.dtype in floating else a, b.view(floating[b.dtype]) if b.dtype in floating else b)
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


# ---------------------------------------------------------------------------------------------------- triangulation
def _triangulate(name, dtype=torch.int64):
    from collab_splats_amd import triangulate_holes
    V, T, att, size = S.triangulate_case(name)
    args = (_t(V), _t(T, dtype), size, tuple(_t(a) for a in att))
    got = triangulate_holes(*args)
    _same_all(got, triangulate_holes(*args))
    v, t, a, n_filled, info = got
    rv, rt, ra, rn, rinfo = S.triangulate_reference(name)
    assert t.dtype == dtype and n_filled == rn and (info["n_triangulated"], info["n_fans"]) == (rinfo["n_triangulated"], rinfo["n_fans"])
    assert tuple(t.shape) == rt.shape and np.array_equal(t.cpu().numpy().astype(np.int64), rt)
    assert info["fallback"].dtype == torch.int32 and np.array_equal(info["fallback"].cpu().numpy(), rinfo["fallback"])
    assert info["area"].dtype == torch.float64
    assert np.array_equal(info["area"].cpu().numpy().view(np.int64), rinfo["area"].view(np.int64))
    _same_bits(v, rv)
    _same_bits(a[0], ra[0])
    assert np.array_equal(_bits(v[:len(V)]), V.view(np.int32)) and np.array_equal(t.cpu().numpy()[:len(T)], T)      # the prefix
    return (V, T, att, size), got


@pytest.mark.parametrize("name,n", [("triangle", 3), ("bent_quad", 4), ("pentagon", 5)])
def test_small_loops(name, n):
    (V, T, _, _), (v, t, _, n_filled, info) = _triangulate(name)
    assert n_filled == 1 and info["fallback"].tolist() == [0] and v.shape[0] == len(V) and t.shape[0] == len(T) + n - 2
    if name == "bent_quad":
        assert t[len(T):].tolist() == [[0, 1, 3], [1, 2, 3]]        # the diagonal of the smaller area


def test_a_tie_goes_to_the_smallest_k():
    (_, T, _, _), (_, t, _, _, info) = _triangulate("square_tie")
    assert t[len(T):].tolist() == [[0, 1, 3], [1, 2, 3]] and info["area"].tolist() == [1.0]


@pytest.mark.parametrize("name", ["convex", "c_shape"])
def test_planar_polygons_face_up(name):
    (_, T, _, _), (v, t, _, _, info) = _triangulate(name)
    P = S.convex_polygon() if name == "convex" else S.c_polygon()
    assert info["area"].tolist() == [S.polygon_area(P)]
    assert (S.face_normals(v.cpu().numpy(), t.cpu().numpy()[len(T):])[:, 2] > 0).all()


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_three_loops_in_one_call(dtype):
    (V, T, _, _), (v, t, _, n_filled, info) = _triangulate("three_loops", dtype)
    assert n_filled == 2 and t.shape[0] == len(T) + 3 + 7 and info["fallback"].tolist() == [0, 0]
    rim = S.boundary_edges(t.cpu().numpy())
    on = np.unique(np.concatenate([rim >> 32, rim & 0xFFFFFFFF]))
    assert np.array_equal(on, np.concatenate([np.arange(5, 10), np.arange(19, 56)]))     # the loop above the limit is left alone


def test_lds_and_workspace_paths_at_the_cutoff():
    """A loop of LDS_LOOP edges (its table in LDS) and one of an edge more (in the workspace): both equal the restatement."""
    from collab_splats_amd import meshfill
    assert meshfill.LDS_LOOP == S.LDS_LOOP
    (_, T, _, _), (_, t, _, n_filled, info) = _triangulate("cutoff")
    assert n_filled == 2 and t.shape[0] == len(T) + (S.LDS_LOOP - 2) + (S.LDS_LOOP - 1)


def test_fallbacks_get_the_fan_of_fill_holes():
    from collab_splats_amd import fill_holes
    (V, T, att, size), (v, t, a, n_filled, info) = _triangulate("fallbacks")
    assert info["fallback"].tolist() == [R.NOT_SIMPLE, R.TOO_SHORT, R.TOO_LONG, R.TOO_LONG] and info["n_triangulated"] == 0
    _same_all((v, t, a, n_filled), fill_holes(_t(V), _t(T), size, tuple(_t(x) for x in att)))


def test_no_hole():
    (V, T, _, _), (v, t, _, n_filled, info) = _triangulate("closed")
    assert n_filled == 0 and t.shape[0] == len(T) and info["area"].shape == (0,)


# ------------------------------------------------------------------------------------------------------------ flips
def _flip(name, dtype=torch.int64):
    from collab_splats_amd import flip_edges
    V, T, region = S.flip_case(name)
    args = (_t(V), _t(T, dtype), None if region is None else _t(region))
    got = flip_edges(*args)
    _same_all(got, flip_edges(*args))
    t, n_flips, rounds = got
    (rt, rn, rr), per_round = S.flip_reference(name)
    assert t.dtype == dtype and (n_flips, rounds) == (rn, rr)
    assert tuple(t.shape) == rt.shape and np.array_equal(t.cpu().numpy().astype(np.int64), rt)
    return (V, T, region), got, per_round


def test_a_bad_diagonal_is_flipped():
    _, (t, n_flips, rounds), _ = _flip("bad_diagonal")
    assert (n_flips, rounds) == (1, 1) and t.tolist() == [[2, 3, 1], [3, 0, 1]]


@pytest.mark.parametrize("name", ["delaunay_pair", "cocircular", "valence_three", "defective"])
def test_nothing_to_flip(name):
    """A Delaunay pair; four points on a circle; an edge whose flip would create an edge that exists; a non-manifold edge and a
    face with a repeated corner, carried through untouched."""
    (_, T, _), (t, n_flips, rounds), _ = _flip(name)
    assert (n_flips, rounds) == (0, 0) and np.array_equal(t.cpu().numpy(), T)


def test_two_flips_that_want_one_edge():
    _, (t, n_flips, rounds), per_round = _flip("octahedron")
    assert per_round == [(2, 1)] and (n_flips, rounds) == (1, 1)
    assert S.edge_counts(t.cpu().numpy()) == (12, 0, 0)             # no duplicate edge


def test_region_border_is_never_flipped():
    (V, T, region), (t, n_flips, _), _ = _flip("region_border")
    tt = t.cpu().numpy()
    assert n_flips > 0 and np.array_equal(tt[~region], T[~region])  # faces outside the region: their slot, their bits
    border = np.intersect1d(S.boundary_edges(T[region]), S.boundary_edges(T[~region]))
    assert len(border) > 0 and np.isin(border, S.boundary_edges(tt[region])).all()


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_grid_of_several_workgroups(dtype):
    (V, T, _), (t, n_flips, rounds), per_round = _flip("grid37x41", dtype)
    assert (3 * len(T)) % 256 != 0 and 3 * len(T) > 4 * 256 and rounds == len(per_round) >= 3
    tt = t.cpu().numpy()
    assert S.total_area(V, tt) == 37 * 41 and (S.face_normals(V, tt)[:, 2] > 0).all()
    assert len(R.flippable_edges(V, tt)) == 0


# --------------------------------------------------------------------------------------------------------- the fill
@pytest.mark.parametrize("name", sorted(S.FILL))
def test_fill_min_area_with_flips(name):
    from collab_splats_amd import fill_holes_nicely, mesh_edge_stats
    V, T, att, size, max_len = S.fill_case(name)
    args = (_t(V), _t(T), size, max_len)
    kw = dict(attributes=tuple(_t(a) for a in att), triangulation="min_area", flip=True)
    got = fill_holes_nicely(*args, **kw)
    _same_all(got, fill_holes_nicely(*args, **kw))
    v, t, a, n_filled, info = got
    rv, rt, ra, rn, rinfo = S.fill_reference(name)
    assert n_filled == rn
    for k in ("n_splits", "rounds", "n_new_vertices", "n_flips", "flip_rounds", "passes", "n_triangulated", "n_fans"):
        assert info[k] == rinfo[k], k
    assert np.array_equal(info["iterations"].cpu().numpy(), rinfo["iterations"])
    assert np.array_equal(t.cpu().numpy(), rt)
    _same_bits(v, rv)
    _same_bits(a[0], ra[0])
    assert info["n_fans"] == 0 and info["passes"] <= 4 and info["n_flips"] > 0
    assert np.array_equal(_bits(v[:len(V)]), V.view(np.int32)) and np.array_equal(t.cpu().numpy()[:len(T)], T)      # the prefix
    assert np.array_equal(_bits(a[0][:len(V)]), att[0].view(np.int32))
    st = mesh_edge_stats(v, t)
    before, after = S.boundary_edges(T), S.boundary_edges(t.cpu().numpy())
    assert st["n_nonmanifold"] == 0 and np.isin(after, before).all() and len(after) < len(before)     # the hole is closed
    if name == "open_cube":
        assert st["n_boundary"] == 0 and v.shape[0] - st["n_edges"] + t.shape[0] == 2
    if name == "c_sheet":
        assert (S.face_normals(v.cpu().numpy(), t.cpu().numpy()[len(T):])[:, 2] > 0).all()           # no face of the patch is folded


def test_fill_min_area_without_flips():
    from collab_splats_amd import fill_holes_nicely
    V, T, att, size, max_len = S.fill_case("c_sheet")
    args, kw = (_t(V), _t(T), size, max_len), dict(attributes=(_t(att[0]),), triangulation="min_area")
    got = fill_holes_nicely(*args, **kw)
    _same_all(got, fill_holes_nicely(*args, **kw))
    v, t, a, n_filled, info = got
    rv, rt, ra, rn, rinfo = S.fill_reference("c_sheet", "min_area", False)
    assert (n_filled, info["passes"], info["n_flips"], info["n_splits"]) == (rn, 1, 0, rinfo["n_splits"])
    assert np.array_equal(t.cpu().numpy(), rt)
    _same_bits(v, rv)
    _same_bits(a[0], ra[0])


def test_finish_mesh_min_area():
    import tsdf_scenes
    V, T = S.icosphere(3, 0.3, (0.1, -0.05, 0.2))
    T = T[~np.isin(T, np.flatnonzero(V[:, 1] > 0.2)).any(1)]        # a cap cut off: one hole
    v, t, c = _t(V), _t(T), _t(S.colour_ramp(V))
    model = tsdf_scenes.sphere_gaussians(2000).to(DEV)
    model.eval()
    out = model.finish_mesh(v, t, c, align=False, fill="min_area")
    _same_all(out, model.finish_mesh(v, t, c, align=False, fill="min_area"))
    info = out["fill_info"]
    assert out["n_filled"] == 1 and info["n_triangulated"] == 1 and info["n_fans"] == 0 and info["passes"] <= 4
    m, created = out["vertices"].shape[0], info["n_new_vertices"]
    assert created == info["n_splits"] > 0 and m == len(np.unique(T)) + created     # the triangulation itself creates no vertex
    for k in ("colors", "normals"):
        assert out[k].shape == (m, 3)
    index = out["vertex_index"]
    assert index.shape == (m,) and bool((index[m - created:] == -1).all()) and bool((index[:m - created] >= 0).all())
    assert len(S.boundary_edges(out["triangles"].cpu().numpy())) == 0
