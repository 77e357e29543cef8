"""GPU: the angle-and-area hole triangulation (csrc/meshtri.hip), the curvature fairing (csrc/meshfill.hip) and the fill that
uses them against tests/meshsmooth_restatement.py.  Every case compares with the restatement for equality
(faces, codes, the fp64 bits of the areas and residuals, the badness, position and attribute bits, counts) and a second run
with the first.  What is asserted about a result
beyond that was first checked on the restatement's output, on the CPU (tests/test_meshsmooth_host.py)."""
import numpy as np
import pytest
import torch

import meshsmooth_restatement as R
import meshsmooth_scenes as S
import meshtri_restatement as MT

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
def _triangulate(name, dtype=torch.int64, metric="angle_area"):
    from collab_splats_amd import triangulate_holes
    V, T, att, size = S.triangulate_case(name)
    args = (_t(V), _t(T, dtype), size, tuple(_t(a) for a in att))
    got = triangulate_holes(*args, metric=metric)
    _same_all(got, triangulate_holes(*args, metric=metric))
    v, t, a, n_filled, info = got
    rv, rt, ra, rn, rinfo = S.triangulate_reference(name, metric)
    assert t.dtype == dtype and n_filled == rn and (info["n_triangulated"], info["n_fans"]) == (rinfo["n_triangulated"], rinfo["n_fans"])
    assert tuple(t.shape) == rt.shape and np.array_equal(t.cpu().numpy().astype(np.int64), rt)
    assert info["fallback"].dtype == torch.int32 and np.array_equal(info["fallback"].cpu().numpy(), rinfo["fallback"])
    assert info["area"].dtype == torch.float64
    assert np.array_equal(info["area"].cpu().numpy().view(np.int64), rinfo["area"].view(np.int64))
    assert sorted(info) == sorted(rinfo)
    if metric == "angle_area":
        assert info["badness"].dtype == torch.int32 and np.array_equal(info["badness"].cpu().numpy(), rinfo["badness"])
    _same_bits(v, rv)
    _same_bits(a[0], ra[0])
    assert np.array_equal(_bits(v[:len(V)]), V.view(np.int32)) and np.array_equal(t.cpu().numpy()[:len(T)], T)      # the prefix
    return (V, T, att, size), got


@pytest.mark.parametrize("name,n", [("triangle", 3), ("ridge_quad", 4), ("pentagon", 5)])
def test_small_loops(name, n):
    (V, T, _, _), (v, t, _, n_filled, info) = _triangulate(name)
    assert n_filled == 1 and info["fallback"].tolist() == [0] and v.shape[0] == len(V) and t.shape[0] == len(T) + n - 2


def test_the_ridge_quad_takes_the_other_diagonal():
    (V, T, _, _), (_, t, _, _, info) = _triangulate("ridge_quad")
    _, (_, ta, _, _, _) = _triangulate("ridge_quad", metric="area")
    assert ta[len(T):].tolist() == [[0, 1, 3], [1, 2, 3]] and t[len(T):].tolist() == [[0, 1, 2], [0, 2, 3]]
    assert info["badness"].tolist() == [72] and R.triangulation_badness(V, T, ta.cpu().numpy()[len(T):]) == 149


@pytest.mark.parametrize("name", ["square_tie", "convex", "c_shape", "collinear"])
def test_planar_holes_are_decided_by_the_area(name):
    """Every crease of a planar hole falls into bucket 0: the faces and the area bits of ``metric="area"``, the smallest k on a
    tie; a candidate of area 0 is not preferred for having no normal."""
    (_, T, _, _), (_, t, _, _, info) = _triangulate(name)
    _, (_, ta, _, _, infoa) = _triangulate(name, metric="area")
    assert torch.equal(t, ta) and torch.equal(info["area"].view(torch.int64), infoa["area"].view(torch.int64))
    assert info["badness"].tolist() == [0]
    if name == "square_tie":
        assert t[len(T):].tolist() == [[0, 1, 3], [1, 2, 3]] and info["area"].tolist() == [1.0]


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_three_loops_in_one_call(dtype):
    (V, T, _, _), (v, t, _, n_filled, info) = _triangulate("three_loops", dtype)
    assert n_filled == 2 and t.shape[0] == len(T) + 3 + 7 and info["fallback"].tolist() == [0, 0]
    rim = S.boundary_edges(t.cpu().numpy())
    on = np.unique(np.concatenate([rim >> 32, rim & 0xFFFFFFFF]))
    assert np.array_equal(on, np.concatenate([np.arange(5, 10), np.arange(19, 56)]))     # the loop above the limit is left alone


@pytest.mark.parametrize("name,n", [("small_cutoff", S.SMALL_LOOP), ("lds_cutoff", S.ANGLE_LDS_LOOP)])
def test_instances_at_their_cutoffs(name, n):
    """A loop of n edges and one of an edge more run in different instances (the small workgroup and the LDS table; the LDS
    table and the workspace): both equal the restatement."""
    from collab_splats_amd import meshfill
    assert (meshfill.SMALL_LOOP, meshfill.ANGLE_LDS_LOOP) == (S.SMALL_LOOP, S.ANGLE_LDS_LOOP)
    (_, T, _, _), (_, t, _, n_filled, info) = _triangulate(name)
    assert n_filled == 2 and t.shape[0] == len(T) + (n - 2) + (n - 1) and int(info["badness"].min()) > 0


def test_fallbacks_get_the_fan_of_fill_holes():
    from collab_splats_amd import fill_holes
    (V, T, att, size), (v, t, a, n_filled, info) = _triangulate("fallbacks")
    assert info["fallback"].tolist() == [MT.NOT_SIMPLE, MT.TOO_SHORT, MT.TOO_LONG, MT.TOO_LONG] and info["n_triangulated"] == 0
    assert info["badness"].shape == (0,)
    _same_all((v, t, a, n_filled), fill_holes(_t(V), _t(T), size, tuple(_t(x) for x in att)))


def test_no_hole():
    (V, T, _, _), (v, t, _, n_filled, info) = _triangulate("closed")
    assert n_filled == 0 and t.shape[0] == len(T) and info["area"].shape == (0,) and info["badness"].shape == (0,)


def test_an_unknown_metric_is_refused():
    from collab_splats_amd import triangulate_holes
    V, T, _, size = S.triangulate_case("triangle")
    with pytest.raises(ValueError, match="metric"):
        triangulate_holes(_t(V), _t(T), size, metric="dihedral")


# ---------------------------------------------------------------------------------------------------------- fairing
def _fair(name, dtype=torch.int64):
    from collab_splats_amd import fair_vertices_curvature
    V, T, free, kw = S.fair_case(name)
    args = (_t(V), _t(T, dtype), _t(free))
    got = fair_vertices_curvature(*args, **kw)
    _same_all(got, fair_vertices_curvature(*args, **kw))
    v, info = got
    rv, rinfo = S.fair_reference(name)
    assert sorted(info) == sorted(rinfo)
    assert info["iterations"].dtype == torch.int32 and np.array_equal(info["iterations"].cpu().numpy(), rinfo["iterations"])
    assert info["code"].dtype == torch.int32 and np.array_equal(info["code"].cpu().numpy(), rinfo["code"])
    assert info["converged"].dtype == torch.bool and np.array_equal(info["converged"].cpu().numpy(), rinfo["converged"])
    assert info["residual"].dtype == torch.float64
    assert np.array_equal(info["residual"].cpu().numpy().view(np.int64), rinfo["residual"].view(np.int64))
    _same_bits(v, rv)
    assert np.array_equal(_bits(v)[~free], V.view(np.int32)[~free])             # a fixed vertex keeps its bits
    return (V, T, free), got


def test_one_free_vertex():
    _, (_, info) = _fair("one_vertex")
    assert info["iterations"].tolist() == [1] and info["converged"].tolist() == [True] and info["code"].tolist() == [0]


def test_a_planar_fan_keeps_the_bits_of_its_z():
    (V, _, free), (v, info) = _fair("planar_fan")
    assert np.array_equal(_bits(v)[:, 2], V.view(np.int32)[:, 2]) and not np.array_equal(_bits(v)[free, :2], V.view(np.int32)[free, :2])


def test_a_sphere_cap_comes_back_to_the_sphere():
    (V, T, free), (v, info) = _fair("sphere_cap")
    assert info["converged"].tolist() == [True] and int(info["iterations"][0]) < int(free.sum())
    from collab_splats_amd import fair_vertices
    membrane = fair_vertices(_t(V), _t(T), _t(free), 1e-3 * S.mean_edge_length(V, T))[0]
    assert S.radial_error(v.cpu().numpy(), free) < 0.25 * S.radial_error(membrane.cpu().numpy(), free)


@pytest.mark.parametrize("n,dtype", [(1023, torch.int64), (1024, torch.int32), (1025, torch.int64)])
def test_the_ragged_last_trip_of_the_strided_sums(n, dtype):
    (_, _, free), (_, info) = _fair(f"block_{n}", dtype)
    assert int(free.sum()) == n and info["converged"].tolist() == [True] and 3 < int(info["iterations"][0]) < n


def test_patches_of_different_size_and_a_lone_vertex():
    (V, _, free), (v, info) = _fair("two_patches")
    assert info["code"].tolist() == [0, 0, 0, 1] and info["iterations"][2:].tolist() == [1, 0]
    assert info["converged"].tolist() == [True, True, True, False]
    assert np.array_equal(_bits(v)[-1], V.view(np.int32)[-1])                   # no neighbour at all: unchanged


def test_two_fans_that_share_a_rim_vertex_are_one_patch():
    (_, _, free), (_, info) = _fair("shared_rim")
    assert int(free.sum()) == 2 and info["code"].tolist() == [0] and info["converged"].tolist() == [True]


@pytest.mark.parametrize("name,code", [("closed", 2), ("too_large", 3)])
def test_patches_that_are_left_unchanged(name, code):
    (V, _, _), (v, info) = _fair(name)
    assert info["code"].tolist() == [code] and info["iterations"].tolist() == [0] and info["converged"].tolist() == [False]
    assert np.array_equal(_bits(v), V.view(np.int32))


def test_max_iterations_ends_a_patch():
    _, (_, info) = _fair("capped")
    assert info["iterations"].tolist() == [3] and info["converged"].tolist() == [False] and float(info["residual"][0]) > 1e-6


# --------------------------------------------------------------------------------------------------------- the fill
@pytest.mark.parametrize("name", sorted(S.FILL))
def test_fill_smooth(name):
    from collab_splats_amd import fill_holes_nicely, mesh_edge_stats
    V, T, att, size, max_len = S.fill_case(name)
    args, kw = (_t(V), _t(T), size, max_len), dict(attributes=tuple(_t(a) for a in att), **S.SMOOTH)
    got = fill_holes_nicely(*args, **kw)
    _same_all(got, fill_holes_nicely(*args, **kw))
    v, t, a, n_filled, info = got
    rv, rt, ra, rn, rinfo = S.fill_reference(name, **S.SMOOTH)
    assert n_filled == rn and sorted(info) == sorted(rinfo)
    for k in ("n_splits", "rounds", "n_new_vertices", "n_flips", "flip_rounds", "passes", "n_triangulated", "n_fans"):
        assert info[k] == rinfo[k], k
    for k in ("iterations", "curvature_iterations", "curvature_converged", "curvature_code"):
        assert np.array_equal(info[k].cpu().numpy(), rinfo[k]), k
    assert np.array_equal(t.cpu().numpy(), rt)
    _same_bits(v, rv)
    _same_bits(a[0], ra[0])
    assert info["n_fans"] == 0 and info["curvature_code"].tolist() == [0] and info["curvature_converged"].tolist() == [True]
    assert np.array_equal(_bits(v[:len(V)]), V.view(np.int32)) and np.array_equal(t.cpu().numpy()[:len(T)], T)      # the prefix
    st = mesh_edge_stats(v, t)
    before, after = S.boundary_edges(T), S.boundary_edges(t.cpu().numpy())
    assert st["n_nonmanifold"] == 0 and np.isin(after, before).all() and len(after) < len(before)     # the hole is closed
    if name == "cut_sphere":
        used = len(np.unique(t.cpu().numpy()))                      # (the cap's own vertices stay in the list, unreferenced)
        assert st["n_boundary"] == 0 and used - st["n_edges"] + t.shape[0] == 2
        membrane = fill_holes_nicely(*args, attributes=kw["attributes"], triangulation="min_area", metric="angle_area", flip=True)
        new = np.arange(v.shape[0]) >= len(V)
        assert torch.equal(membrane[1], t) and torch.equal(membrane[2][0], a[0])          # the attributes stay with the membrane
        assert S.radial_error(v.cpu().numpy(), new) < S.radial_error(membrane[0].cpu().numpy(), new)


def test_fill_defaults_are_unchanged():
    """The new keywords at their defaults, and ``metric="area"`` spelled out, give section 29's and section 30's bits."""
    import meshtri_scenes as TS
    from collab_splats_amd import fill_holes_nicely
    V, T, att, size, max_len = TS.fill_case("holed_sheet")
    args, at = (_t(V), _t(T), size, max_len), (_t(att[0]),)
    for how in (dict(triangulation="fan", flip=False), dict(triangulation="min_area", flip=True)):
        v, t, a, n_filled, info = fill_holes_nicely(*args, attributes=at, metric="area", fairing="membrane", **how)
        _same_all((v, t, a, n_filled, info), fill_holes_nicely(*args, attributes=at, **how))
        rv, rt, ra, rn, rinfo = TS.fill_reference("holed_sheet", how["triangulation"], how["flip"])
        assert n_filled == rn and np.array_equal(t.cpu().numpy(), rt) and sorted(info) == sorted(rinfo)
        _same_bits(v, rv)
        _same_bits(a[0], ra[0])


def test_fill_refuses_the_angle_metric_on_a_fan():
    from collab_splats_amd import fill_holes_nicely
    V, T, _, size, max_len = S.fill_case("holed_sheet")
    with pytest.raises(ValueError, match="needs triangulation='min_area'"):
        fill_holes_nicely(_t(V), _t(T), size, max_len, metric="angle_area")
    with pytest.raises(ValueError, match="fairing"):
        fill_holes_nicely(_t(V), _t(T), size, max_len, fairing="willmore")


def test_finish_mesh_smooth():
    import tsdf_scenes
    V, T = S.icosphere(3, 0.3, (0.1, -0.05, 0.2))
    T = T[~np.isin(T, np.flatnonzero(V[:, 1] > 0.2)).any(1)]        # a cap cut off: one hole
    v, t, c = _t(V), _t(T), _t(S.colour_ramp(V))
    model = tsdf_scenes.sphere_gaussians(2000).to(DEV)
    model.eval()
    out = model.finish_mesh(v, t, c, align=False, fill="smooth")
    _same_all(out, model.finish_mesh(v, t, c, align=False, fill="smooth"))
    info = out["fill_info"]
    assert out["n_filled"] == 1 and info["n_triangulated"] == 1 and info["n_fans"] == 0 and info["passes"] <= 4
    assert info["curvature_code"].tolist() == [0] and info["curvature_converged"].tolist() == [True]
    m, created = out["vertices"].shape[0], info["n_new_vertices"]
    assert created == info["n_splits"] > 0 and m == len(np.unique(T)) + created
    centre = np.array([0.1, -0.05, 0.2])
    radial = np.abs(np.linalg.norm(out["vertices"].cpu().numpy()[m - created:].astype(np.float64) - centre, axis=1) - 0.3).max()
    plain = model.finish_mesh(v, t, c, align=False, fill="min_area")
    radial_plain = np.abs(np.linalg.norm(plain["vertices"].cpu().numpy()[m - created:].astype(np.float64) - centre, axis=1) - 0.3).max()
    assert plain["vertices"].shape[0] == m and radial < radial_plain
    assert len(S.boundary_edges(out["triangles"].cpu().numpy())) == 0
