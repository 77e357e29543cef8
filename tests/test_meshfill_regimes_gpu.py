"""GPU: the hole fill (csrc/meshfill.hip, csrc/meshtri.hip, collab_splats_amd/meshfill.py) in the regimes of
tests/meshfill_regimes_scenes.py against the restatements.  Every case compares with the restatement for equality (position and
attribute bits, triangles, origin, codes, the fp64 bits of areas, counts) and a second run with the first; no tolerance
anywhere.  That each scene reaches its regime is asserted on the restatement, on the CPU
(tests/test_meshfill_regimes_host.py)."""
import numpy as np
import pytest
import torch

import meshfill_regimes_scenes as S

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


# ---------------------------------------------------------------------------------------------------------- fairing
def _fair(name, lds):
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
    print(name, "lds" if lds else "launches", "iterations", it.tolist(), "restated", rit.tolist())
    assert it.dtype == torch.int32 and np.array_equal(it.cpu().numpy(), rit)
    _same_bits(v, rv)
    assert len(a) == len(ra)
    for x, rx in zip(a, ra):
        _same_bits(x, rx)
    return got


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", ["passes_1_1", "passes_2_1", "passes_3_1", "passes_3_2"])
def test_sorted_rows_are_found_after_every_pass_count(name, lds):
    _fair(name, lds)


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", ["fan17", "fan33", "fan17_open", "fan33_open", "fan33_open2", "fan33_open_rim"])
def test_rows_longer_than_a_chunk(name, lds):
    _fair(name, lds)


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name,counts", [("stop_32", None), ("stop_33", None), ("cap_31", [31, 31]), ("cap_32", [32, 32]),
                                         ("cap_33", [32, 33]), ("cap_64", [32, 64])])
def test_counts_at_the_batch_edges(name, counts, lds):
    _, _, it = _fair(name, lds)
    if counts is None:
        assert int(it[0]) == int(name[-2:]) and int(it[1]) > 64
    else:
        assert it.tolist() == counts


@pytest.mark.parametrize("lds", [True, False])
def test_attributes_of_two_widths_past_a_chunk_of_iterations(lds):
    _, a, it = _fair("counted", lds)
    assert int(it.max()) > 1024 and [x.shape[1] for x in a] == [1, 7]


@pytest.mark.parametrize("lds", [True, False])
def test_three_patches_in_a_wave(lds):
    _, _, it = _fair("interleaved", lds)
    assert it.shape[0] == 3 and 3 * int(it.min()) < int(it.max())


# ------------------------------------------------------------------------------------------------------ subdivision
@pytest.mark.parametrize("name", list(S.SUBDIVIDE))
def test_subdivide(name):
    from collab_splats_amd import subdivide_mesh
    V, T, region, att, max_len, budget = S.subdivide_case(name)
    args = (_t(V), _t(T), max_len, budget, None if region is None else _t(region), tuple(_t(a) for a in att))
    got = subdivide_mesh(*args)
    _same_all(got, subdivide_mesh(*args))
    v, t, a, origin, n_splits, rounds = got
    (rv, rt, ra, ro, rn, rr), per_round = S.subdivide_reference(name)
    print(name, "splits", n_splits, "rounds", rounds, "restated", rn, rr)
    assert (n_splits, rounds) == (rn, rr) and n_splits <= budget
    assert tuple(t.shape) == rt.shape and np.array_equal(t.cpu().numpy(), rt)
    assert np.array_equal(origin.cpu().numpy(), ro)
    _same_bits(v, rv)
    assert len(a) == len(ra)
    for x, rx in zip(a, ra):
        _same_bits(x, rx)


# ------------------------------------------------------------------------------------- triangulation and flips
@pytest.mark.parametrize("metric", ["area", "angle_area"])
@pytest.mark.parametrize("name", list(S.TRIANGULATE))
def test_triangulate(name, metric):
    from collab_splats_amd import triangulate_holes
    V, T, att, size = S.triangulate_case(name)
    args = (_t(V), _t(T), size, tuple(_t(a) for a in att))
    got = triangulate_holes(*args, metric=metric)
    _same_all(got, triangulate_holes(*args, metric=metric))
    v, t, a, n_filled, info = got
    rv, rt, ra, rn, rinfo = S.triangulate_reference(name, metric)
    print(name, metric, "fallback", info["fallback"].tolist(), "restated", rinfo["fallback"].tolist())
    assert n_filled == rn and (info["n_triangulated"], info["n_fans"]) == (rinfo["n_triangulated"], rinfo["n_fans"])
    assert sorted(info) == sorted(rinfo) and np.array_equal(info["fallback"].cpu().numpy(), rinfo["fallback"])
    assert tuple(t.shape) == rt.shape and np.array_equal(t.cpu().numpy(), rt)
    assert np.array_equal(info["area"].cpu().numpy().view(np.int64), rinfo["area"].view(np.int64))
    if metric == "angle_area":
        assert np.array_equal(info["badness"].cpu().numpy(), rinfo["badness"])
    _same_bits(v, rv)
    _same_bits(a[0], ra[0])
    assert np.array_equal(_bits(v[:len(V)]), V.view(np.int32)) and np.array_equal(t.cpu().numpy()[:len(T)], T)      # the prefix


@pytest.mark.parametrize("name", list(S.FLIP))
def test_flips_at_high_indices(name):
    from collab_splats_amd import flip_edges
    V, T = S.flip_case(name)
    got = flip_edges(_t(V), _t(T))
    _same_all(got, flip_edges(_t(V), _t(T)))
    t, n_flips, rounds = got
    (rt, rn, rr), _ = S.flip_reference(name)
    assert (n_flips, rounds) == (rn, rr) and np.array_equal(t.cpu().numpy(), rt)


# --------------------------------------------------------------------------------------------------------- the fill
COUNTS = ("n_splits", "rounds", "n_new_vertices", "n_flips", "flip_rounds", "passes", "n_triangulated", "n_fans")
ARRAYS = ("iterations", "curvature_iterations", "curvature_converged", "curvature_code")


@pytest.mark.parametrize("how", list(S.HOW))
@pytest.mark.parametrize("name", list(S.FILL))
def test_fill(name, how):
    from collab_splats_amd import fill_holes_nicely
    V, T, att, size, max_len, kw = S.fill_case(name)
    args, kw = (_t(V), _t(T), size, max_len), dict(attributes=tuple(_t(a) for a in att), **kw, **S.HOW[how])
    got = fill_holes_nicely(*args, **kw)
    _same_all(got, fill_holes_nicely(*args, **kw))
    v, t, a, n_filled, info = got
    (rv, rt, ra, rn, rinfo), _ = S.fill_reference(name, how)
    print(name, how, {k: info[k] for k in COUNTS}, "restated", {k: rinfo[k] for k in COUNTS})
    assert n_filled == rn and sorted(info) == sorted(rinfo)
    for k in COUNTS:
        assert info[k] == rinfo[k], k
    for k in ARRAYS:
        if k in rinfo:
            assert np.array_equal(info[k].cpu().numpy(), rinfo[k]), k
    assert info["iterations"].shape[0] == n_filled                  # one patch of created vertices per hole
    assert np.array_equal(t.cpu().numpy(), rt)
    _same_bits(v, rv)
    _same_bits(a[0], ra[0])
    assert np.array_equal(_bits(v[:len(V)]), V.view(np.int32)) and np.array_equal(t.cpu().numpy()[:len(T)], T)      # the prefix
    assert np.array_equal(_bits(a[0][:len(V)]), att[0].view(np.int32))
    before, after = S.boundary_edges(T), S.boundary_edges(t.cpu().numpy())
    assert np.array_equal(after, S.boundary_edges(rt)) and np.isin(after, before).all() and len(after) < len(before)


def test_finish_mesh_smooth_with_several_holes():
    import tsdf_scenes
    centre = (0.1, -0.05, 0.2)
    V, T = S.capped_sphere(3, 0.3, centre)
    v, t, c = _t(V), _t(T), _t(S.colour_ramp(V))
    model = tsdf_scenes.sphere_gaussians(2000).to(DEV)
    model.eval()
    out = model.finish_mesh(v, t, c, align=False, fill="smooth")
    _same_all(out, model.finish_mesh(v, t, c, align=False, fill="smooth"))
    info = out["fill_info"]
    assert out["n_filled"] == 4 and info["n_triangulated"] == 4 and info["n_fans"] == 0
    assert info["iterations"].shape == info["curvature_iterations"].shape == (4,) and info["curvature_code"].tolist() == [0] * 4
    m, created = out["vertices"].shape[0], info["n_new_vertices"]
    assert created == info["n_splits"] > 0 and m == len(np.unique(T)) + created     # the triangulation itself creates no vertex
    index = out["vertex_index"]
    assert index.shape == (m,) and torch.equal(index == -1, torch.arange(m, device=DEV) >= m - created)
    assert torch.equal(index[:m - created], _t(np.unique(T)))       # the cut-off caps' vertices are gone, the rest in order
    assert len(S.boundary_edges(out["triangles"].cpu().numpy())) == 0
