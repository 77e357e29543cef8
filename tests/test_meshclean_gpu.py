"""GPU: mesh finishing (csrc/meshclean.hip, collab_splats_amd/meshclean.py) against the restatement
(tests/meshclean_restatement.py) and closed forms.  Integer results (labels, sizes, edge lists, loops, inlier counts, inlier
sets, winning hypotheses) are compared for equality; fp64 sums of N terms are allowed N 2^-53 relative (the order of a sum is
fixed on the device but is not numpy's); the refit and the alignment are allowed the issue's 1e-6."""
import math

import numpy as np
import pytest
import torch

import meshclean_restatement as R
import meshclean_scenes as Q
import tsdf_scenes as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _v(x):
    return torch.as_tensor(np.ascontiguousarray(x, np.float32)).to(DEV)


def _i(x, dtype=torch.int64):
    return torch.as_tensor(np.ascontiguousarray(x, np.int64)).to(DEV).to(dtype)


def _np(x):
    return x.cpu().numpy()


def _components(V, tri, dtype=torch.int64):
    import collab_splats_amd as m
    labels, sizes = m.mesh_components(_v(V), _i(tri, dtype))
    assert labels.dtype == torch.int32 and sizes.dtype == torch.int32 and labels.is_cuda and labels.shape == (len(tri),)
    ref_labels, ref_sizes = R.mesh_components(V, tri)
    assert np.array_equal(_np(sizes), ref_sizes) and np.array_equal(_np(labels), ref_labels)
    return _np(labels), _np(sizes)


def _stats(V, tri):
    """mesh_edge_stats, checked against the restatement: counts equal, the mean within n_edges 2^-53 relative."""
    import collab_splats_amd as m
    st = m.mesh_edge_stats(_v(V), _i(tri))
    ref = R.mesh_edge_stats(V, tri)
    for k in ("n_edges", "n_boundary", "n_nonmanifold"):
        assert st[k] == ref[k], k
    assert abs(st["mean_edge_length"] - ref["mean_edge_length"]) <= max(1, ref["n_edges"]) * 2.0 ** -53 * ref["mean_edge_length"]
    return st


# ------------------------------------------------------------------------------------------------------- components
def test_tetrahedra_sharing_a_vertex_are_two_components():
    V, tri = Q.tetra_pair(1)
    labels, sizes = _components(V, tri)
    assert sizes.tolist() == [4, 4] and labels.tolist() == [0] * 4 + [1] * 4     # vertex adjacency would give 1
    assert _stats(V, tri)["n_nonmanifold"] == 0


def test_tetrahedra_sharing_an_edge_are_one_component():
    V, tri = Q.tetra_pair(2)
    labels, sizes = _components(V, tri, torch.int32)
    assert sizes.tolist() == [8]
    st = _stats(V, tri)
    assert st["n_nonmanifold"] == 1 and st["n_boundary"] == 0 and st["n_edges"] == 11       # the shared edge has 4 faces


def test_long_strips():
    """A 1 x 20 000-quad strip (find paths as long as the strip) and a second one with no shared vertex."""
    V, tri = Q.merge(Q.strip(20000), Q.strip(20000, y0=5.0))
    labels, sizes = _components(V, tri)
    assert sizes.tolist() == [40000, 40000]
    assert (labels[:40000] == 0).all() and (labels[40000:] == 1).all()
    assert _stats(V, tri)["n_boundary"] == 2 * 40002


def _filter(V, tri, use_largest=False, attributes=()):
    import collab_splats_amd as m
    out = m.filter_mesh_components(_v(V), _i(tri), use_largest, tuple(attributes))
    v2, t2, index, att, n_removed = out
    rv, rt, rindex, rn = R.filter_mesh_components(V, tri, use_largest)
    assert index.dtype == torch.int64 and t2.dtype == torch.int64
    assert np.array_equal(_np(index), rindex) and np.array_equal(_np(t2), rt) and np.array_equal(_np(v2), rv) and n_removed == rn
    return out


def test_bounding_box_rule():
    V, tri, faces = Q.aabb_scene()
    big, inside, touch, straddle = faces
    _, t2, _, _, n_removed = _filter(V, tri)
    assert n_removed == 1 and t2.shape[0] == big + inside + touch   # on the face at exact equality: kept (the rule is closed)
    _, t2, index, _, n_removed = _filter(V, tri, use_largest=True)
    assert n_removed == 3 and t2.shape[0] == big
    assert index.shape[0] == len(Q.icosphere(3)[0])


def test_equal_sizes_the_lower_face_index_wins():
    a, b = Q.icosphere(1, 0.5, (0, 0, 0)), Q.icosphere(1, 0.5, (3, 0, 0))
    V, tri = Q.merge(a, b)
    v2, t2, index, _, n_removed = _filter(V, tri)
    assert n_removed == 1 and np.array_equal(_np(index), np.arange(len(a[0])))
    V, tri = Q.merge(b, a)
    v2, _, _, _, _ = _filter(V, tri)
    assert np.array_equal(_np(v2), b[0])


def test_permuted_faces_same_partition_and_attributes():
    V, tri, _ = Q.aabb_scene()
    rng = np.random.default_rng(4)
    perm = rng.permutation(len(tri))
    lab, sizes = _components(V, tri)
    lab_p, sizes_p = _components(V, tri[perm])
    pairs = {(a, b) for a, b in zip(lab[perm].tolist(), lab_p.tolist())}     # a bijection between the two numberings
    assert len(pairs) == len(sizes) == len(sizes_p)
    assert sorted(sizes.tolist()) == sorted(sizes_p.tolist())
    colour = rng.random((len(V), 3)).astype(np.float32)
    ident = np.arange(len(V))
    v2, t2, index, (c2, i2), _ = _filter(V, tri[perm], attributes=(_v(colour), _i(ident, torch.int32)))
    assert i2.dtype == torch.int32 and np.array_equal(_np(i2), _np(index))
    assert np.array_equal(_np(c2), colour[_np(index)]) and np.array_equal(_np(v2), V[_np(index)])
    kept = np.isin(tri[perm], _np(index)).all(1)
    assert np.array_equal(_np(v2)[_np(t2)], V[tri[perm][kept]])     # the kept faces, in their order, keep their corners


def test_unreferenced_vertices_are_dropped():
    V, tri = Q.icosphere(1)
    V2 = np.concatenate([np.full((5, 3), 9, np.float32), V, np.full((3, 3), -9, np.float32)])
    v2, t2, index, _, n_removed = _filter(V2, tri + 5)
    assert n_removed == 0 and np.array_equal(_np(index), 5 + np.arange(len(V))) and np.array_equal(_np(t2), tri)


def test_empty_inputs():
    import collab_splats_amd as m
    e3 = torch.zeros((0, 3), device=DEV)
    t0 = torch.zeros((0, 3), dtype=torch.int32, device=DEV)
    for v in (e3, _v(Q.icosphere(0)[0])):
        labels, sizes = m.mesh_components(v, t0)
        assert labels.shape == (0,) and sizes.shape == (0,)
        st = m.mesh_edge_stats(v, t0)
        assert st == {"n_edges": 0, "n_boundary": 0, "n_nonmanifold": 0, "mean_edge_length": 0.0}
        v2, t2, index, att, n_removed = m.filter_mesh_components(v, t0, attributes=(v,))
        assert v2.shape == (0, 3) and t2.shape == (0, 3) and index.shape == (0,) and att[0].shape == (0, 3) and n_removed == 0
        loop, edges, n_edges, perimeter = m.mesh_holes(v, t0)
        assert loop.shape == (0,) and edges.shape == (0, 2) and n_edges.shape == (0,) and perimeter.shape == (0,)
        v2, t2, _, n = m.fill_holes(v, t0)
        assert v2.shape == v.shape and t2.shape == (0, 3) and n == 0
    with pytest.raises(ValueError, match="indices"):
        m.mesh_components(e3, torch.zeros((1, 3), dtype=torch.int32, device=DEV))


def test_repeated_corner_is_ignored():
    V, tri = Q.icosphere(0)
    tri = np.concatenate([tri, [[0, 0, 5], [3, 3, 3]]])             # a sliver on an existing edge, and a point
    labels, sizes = _components(V, tri)
    assert sizes.tolist() == [21, 1]
    assert _stats(V, tri)["n_edges"] == 30


def test_two_runs_bitwise_equal():
    import collab_splats_amd as m
    V, tri, _ = Q.aabb_scene()
    Vs, ts = Q.sheet(64, Q.THREE_HOLES)
    P, _ = Q.planted_plane(20000)

    def run():
        out = list(m.mesh_components(_v(V), _i(tri))) + list(m.filter_mesh_components(_v(V), _i(tri))[:3])
        out += list(m.mesh_holes(_v(Vs), _i(ts))) + list(m.fill_holes(_v(Vs), _i(ts), 1.0)[:2])
        st = m.mesh_edge_stats(_v(V), _i(tri))
        plane, inl = m.segment_plane(_v(P), 0.02, 3, 300, 5)
        a, Rm, tr = m.align_floor(_v(P), num_iterations=200)
        return [_np(x) for x in out] + [np.array(list(st.values())), plane.numpy(), _np(inl), _np(a), Rm.numpy(), tr.numpy()]

    for a, b in zip(run(), run()):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------ holes
def _holes(V, tri):
    import collab_splats_amd as m
    loop, edges, n_edges, perimeter = m.mesh_holes(_v(V), _i(tri))
    assert loop.dtype == torch.int32 and edges.dtype == torch.int32 and n_edges.dtype == torch.int32
    assert perimeter.dtype == torch.float64
    rl, re, rn, rp = R.mesh_holes(V, tri)
    assert np.array_equal(_np(edges), re) and np.array_equal(_np(loop), rl) and np.array_equal(_np(n_edges), rn)
    assert np.all(np.abs(_np(perimeter) - rp) <= rn * 2.0 ** -53 * rp)
    return _np(loop), _np(edges), _np(n_edges), _np(perimeter)


def test_closed_sphere_has_no_loop():
    V, tri = Q.icosphere(3)
    loop, edges, n_edges, perimeter = _holes(V, tri)
    assert len(n_edges) == 0 and len(edges) == 0
    st = _stats(V, tri)
    assert st["n_edges"] == 3 * len(tri) // 2 and st["n_boundary"] == 0 and st["n_nonmanifold"] == 0


def test_sheet_with_three_holes():
    V, tri = Q.sheet(64, Q.THREE_HOLES)
    loop, edges, n_edges, perimeter = _holes(V, tri)
    # loops in ascending order of their smallest vertex j 65 + i: the rim (vertex 0), then the holes by their lower-left corner
    order = sorted(Q.THREE_HOLES, key=lambda h: h[2] * 65 + h[0])
    expect = [256] + [2 * ((i1 - i0) + (j1 - j0)) for i0, i1, j0, j1 in order]
    assert n_edges.tolist() == expect
    assert np.array_equal(perimeter, np.array(expect) / 64.0)       # sums of equal fp32 lengths 1 / 64: exact in fp64
    assert _stats(V, tri)["n_boundary"] == sum(expect)


def test_bow_tie_is_one_loop():
    V, tri = Q.sheet(64, Q.BOW_TIE)
    loop, edges, n_edges, perimeter = _holes(V, tri)
    assert n_edges.tolist() == [256, 32]                            # two 4 x 4 holes pinched at one vertex: one loop


def _directed(tri):
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    return e[:, 0] * (1 << 32) + e[:, 1], e[:, 1] * (1 << 32) + e[:, 0]


def test_fill_holes_below_the_rim():
    import collab_splats_amd as m
    V, tri = Q.sheet(64, Q.THREE_HOLES)
    colour = np.random.default_rng(1).random((len(V), 3)).astype(np.float32)
    v2, t2, (c2,), n = m.fill_holes(_v(V), _i(tri), 1.0, (_v(colour),))          # largest hole 40 / 64, the rim 4
    rv, rt, rn = R.fill_holes(V, tri, 1.0)
    assert n == rn == 3 and np.array_equal(_np(v2), rv) and np.array_equal(_np(t2), rt) and t2.dtype == torch.int64
    v2, t2, c2 = _np(v2), _np(t2), _np(c2)
    assert np.array_equal(v2[:len(V)], V) and np.array_equal(c2[:len(V)], colour) and np.array_equal(t2[:len(tri)], tri)
    loop, edges, n_edges, perimeter = _holes(v2, t2)
    assert n_edges.tolist() == [256]                                # only the rim is a boundary
    fwd, back = _directed(t2)
    assert len(np.unique(fwd)) == len(fwd)                          # no directed edge twice
    assert (~np.isin(fwd, back)).sum() == 256                       # every edge but the rim's runs once each way
    st = _stats(v2, t2)
    assert len(np.unique(t2)) - st["n_edges"] + len(t2) == 1        # V - E + F of a disc
    order = sorted(Q.THREE_HOLES, key=lambda h: h[2] * 65 + h[0])
    start = len(tri)
    for k, (i0, i1, j0, j1) in enumerate(order):
        count = 2 * ((i1 - i0) + (j1 - j0))
        fan = v2[t2[start:start + count]].astype(np.float64)
        start += count
        assert (t2[start - count:start, 2] == len(V) + k).all()
        area = 0.5 * np.cross(fan[:, 1] - fan[:, 0], fan[:, 2] - fan[:, 0])
        assert np.abs(area[:, :2]).max() == 0 and (area[:, 2] > 0).all()          # planar, oriented as the sheet
        want = (i1 - i0) * (j1 - j0) / 64.0 ** 2
        assert abs(area[:, 2].sum() - want) <= 1e-6 * want
        ring = np.unique(t2[start - count:start, :2])
        assert np.array_equal(v2[len(V) + k], V[ring].astype(np.float64).mean(0).astype(np.float32))
        assert np.array_equal(c2[len(V) + k], colour[ring].astype(np.float64).mean(0).astype(np.float32))
    assert start == len(t2)


def test_fill_holes_below_every_perimeter_changes_nothing():
    import collab_splats_amd as m
    V, tri = Q.sheet(64, Q.THREE_HOLES)
    v2, t2, att, n = m.fill_holes(_v(V), _i(tri, torch.int32), 0.4)
    assert n == 0 and t2.dtype == torch.int32 and np.array_equal(_np(v2), V) and np.array_equal(_np(t2), tri) and att == ()


# ------------------------------------------------------------------------------------------------------------ plane
@pytest.fixture(scope="module")
def cloud():
    P, nrm = Q.planted_plane(20001, seed=0)
    triples = R.ransac_triples(len(P), 100, 3)
    planes = R.planes_from_triples(P, triples)
    return P, nrm, triples, planes, R.plane_inlier_counts(P, planes, 0.02)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 20001])
def test_plane_inlier_counts(cloud, n):
    import collab_splats_amd as m
    from collab_splats_amd import meshclean
    P, _, _, planes, ref = cloud
    ref = ref if n == len(P) else R.plane_inlier_counts(P[:n], planes, 0.02)
    tile = meshclean.PLANE_TILE
    for h in (1, tile - 1, tile, tile + 1, 100):
        got = m.plane_inlier_counts(_v(P[:n]), _v(planes[:h]), 0.02)
        assert got.dtype == torch.int32 and np.array_equal(_np(got), ref[:h])
    if n == len(P):
        assert ref.max() > 0.55 * n > ref.min()
        for other in (8, 16, 32):                                   # the tile changes no result
            try:
                meshclean.PLANE_TILE = other
                assert np.array_equal(_np(m.plane_inlier_counts(_v(P), _v(planes), 0.02)), ref)
            finally:
                meshclean.PLANE_TILE = tile


def test_hypotheses_match_the_restatement(cloud):
    import collab_splats_amd as m
    P, _, triples, planes, _ = cloud
    got_t, got_p = m.ransac_planes(_v(P), 100, 3)
    assert np.array_equal(_np(got_t), triples) and _np(got_p).tobytes() == planes.tobytes()
    again_t, _ = m.ransac_planes(_v(P), 100, 3)
    other_t, _ = m.ransac_planes(_v(P), 100, 4)
    assert np.array_equal(_np(again_t), triples) and not np.array_equal(_np(other_t), triples)
    small = np.random.default_rng(0).random((3, 3)).astype(np.float32)
    t3, _ = m.ransac_planes(_v(small), 50, 1)                       # N = 3: every triple is a permutation of all points
    assert np.array_equal(_np(t3), R.ransac_triples(3, 50, 1)) and (np.sort(_np(t3), 1) == [0, 1, 2]).all()


def test_threshold_is_strict():
    import collab_splats_amd as m
    t = 0.015625                                                    # 2^-6
    rng = np.random.default_rng(2)
    P = np.concatenate([rng.uniform(-1, 1, (300, 2)), np.repeat([[t], [-t], [t / 2], [np.nextafter(np.float32(t), 0)]], 75, 0)], 1)
    got = m.plane_inlier_counts(_v(P), _v([[0, 0, 1, 0]]), t)
    assert _np(got).tolist() == [150]                               # the points at distance exactly t are out
    assert R.plane_inlier_counts(P, [[0, 0, 1, 0]], t).tolist() == [150]


def test_segment_plane():
    _segment_plane(20000)


def test_segment_plane_refit_sums_more_partials_than_the_final_workgroup_has_threads():
    _segment_plane(65800)                                           # 258 workgroup partials of 256 points through 256 threads


def _segment_plane(n):
    import collab_splats_amd as m
    P, nrm = Q.planted_plane(n, seed=0)                             # 60 % on the plane (+- t / 4), 40 % uniform clutter
    plane, inliers, index = m.segment_plane(_v(P), 0.02, 3, 300, 11, return_index=True)
    rplane, rinl, rindex = R.segment_plane(P, 0.02, 300, 11)
    assert plane.dtype == torch.float64 and not plane.is_cuda and inliers.dtype == torch.int64 and inliers.is_cuda
    assert index == rindex and np.array_equal(_np(inliers), rinl)
    assert len(rinl) >= 0.6 * len(P) - 1
    extent = np.abs(P).max()
    assert np.abs(plane.numpy()[:3] - rplane[:3]).max() <= 1e-6 and abs(plane.numpy()[3] - rplane[3]) / extent <= 1e-6
    assert abs(np.linalg.norm(plane.numpy()[:3]) - 1) < 1e-12
    assert abs(abs(plane.numpy()[:3] @ nrm) - 1) < 1e-4 and abs(abs(plane.numpy()[3]) - 0.4) < 1e-3   # the planted plane


def test_duplicate_and_collinear_hypotheses():
    import collab_splats_amd as m
    P = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 0], [0, 0, 1]], np.float32)
    triples = [[0, 1, 2], [0, 3, 4], [0, 3, 4], [4, 0, 5]]
    _, planes = m.ransac_planes(_v(P), triples=_i(triples))
    assert _np(planes).tobytes() == R.planes_from_triples(P, triples).tobytes() and np.isnan(_np(planes)[0]).all()
    counts = _np(m.plane_inlier_counts(_v(P), planes, 0.01))
    assert counts.tolist() == [0, 4, 4, 4]                          # a collinear triple scores 0
    plane, inliers, index = m.segment_plane(_v(P), 0.01, triples=_i(triples, torch.int32), return_index=True)
    assert index == 1 and _np(inliers).tolist() == [0, 3, 4, 5]     # equal scores: the lowest index wins
    assert np.abs(np.abs(plane.numpy()) - [0, 0, 1, 0]).max() < 1e-12
    with pytest.raises(ValueError, match="no hypothesis"):
        m.segment_plane(_v(P), 0.01, triples=_i(triples[:1]))


# ------------------------------------------------------------------------------------------------------- sampling
def test_sample_surface_lies_in_its_triangles():
    import collab_splats_amd as m
    V, tri = Q.icosphere(2, 0.7, (0.2, 0.1, -0.3))
    pts, face = m.sample_surface(_v(V), _i(tri), 5000, 3)
    assert pts.shape == (5000, 3) and pts.dtype == torch.float32 and face.dtype == torch.int64
    c = V[tri[_np(face)]].astype(np.float64)
    A = np.stack([c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]], 2)          # [n,3,2]
    rhs = _np(pts).astype(np.float64) - c[:, 0]
    uv = np.stack([np.linalg.lstsq(a, r, rcond=None)[0] for a, r in zip(A, rhs)])
    resid = np.abs(np.einsum("nij,nj->ni", A, uv) - rhs).max()
    assert resid < 1e-6 and uv.min() > -1e-5 and uv.sum(1).max() < 1 + 1e-5     # fp32 rounding of a point of size ~1
    again, face2 = m.sample_surface(_v(V), _i(tri), 5000, 3)
    assert torch.equal(again, pts) and torch.equal(face2, face)
    assert not torch.equal(m.sample_surface(_v(V), _i(tri), 5000, 4)[1], face)


def test_sample_surface_is_area_weighted():
    import collab_splats_amd as m
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [5, 0, 0], [8, 0, 0], [5, 2, 0]], np.float32)     # areas 1 and 3
    _, face = m.sample_surface(_v(V), _i([[0, 1, 2], [3, 4, 5]]), 40000, 0)
    assert abs(int((face == 0).sum()) - 10000) <= 433               # 5 sigma, sigma = sqrt(40000 * 0.25 * 0.75)


# ------------------------------------------------------------------------------------------------------ alignment
@pytest.mark.parametrize("normal", [(0.3, -0.2, 0.9), (0.3, -0.2, -0.9), (-0.6, 0.1, 0.5)])
def test_align_floor_cloud(normal):
    import collab_splats_amd as m
    t = 0.02
    P, nrm = Q.planted_plane(20000, 0.7, normal=normal, offset=0.4, t=t, seed=7, clutter_gap=0.1)
    aligned, Rm, tr = m.align_floor(_v(P), t, 3, 300, seed=1)
    ra, rR, rtr = R.align_floor_cloud(P, t, 300, 1)
    Rn, trn = Rm.numpy(), tr.numpy()
    assert Rm.dtype == torch.float64 and aligned.dtype == torch.float32 and aligned.is_cuda
    assert np.abs(Rn @ Rn.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rn) - 1) < 1e-12
    up = nrm if nrm[2] >= 0 else -nrm
    assert np.abs(Rn @ up - [0, 0, 1]).max() < 1e-3                 # the fitted normal is the planted one to the noise
    on = np.abs(P.astype(np.float64) @ nrm - 0.4) < t / 4 + 1e-6
    assert on.sum() >= 14000 and np.abs(_np(aligned)[on, 2]).max() <= t
    assert np.abs(Rn - rR).max() <= 1e-6 and np.abs(trn - rtr).max() <= 1e-6 and trn[0] == 0 and trn[1] == 0
    assert np.abs(_np(aligned) - ra).max() <= 1e-6 * (3 * np.abs(P).max() + 1) + 2.4e-7    # R and t to 1e-6, one fp32 rounding


def test_align_floor_already_aligned_is_the_identity():
    import collab_splats_amd as m
    rng = np.random.default_rng(3)
    floor = np.concatenate([rng.uniform(-1, 1, (6000, 2)), np.full((6000, 1), 0.5)], 1)
    above = np.concatenate([rng.uniform(-1, 1, (2000, 2)), rng.uniform(0.7, 1.5, (2000, 1))], 1)
    P = np.concatenate([floor, above]).astype(np.float32)
    aligned, Rm, tr = m.align_floor(_v(P), num_iterations=200)
    assert np.array_equal(Rm.numpy(), np.eye(3)) and tr.numpy().tolist() == [0.0, 0.0, -0.5]
    assert np.array_equal(_np(aligned)[:, :2], P[:, :2]) and (_np(aligned)[:6000, 2] == 0).all()


def test_align_floor_mesh():
    import collab_splats_amd as m
    V, tri = Q.sheet(64)
    a = 0.4
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    V = (V.astype(np.float64) @ Rx.T + [0.1, 0.2, 0.7]).astype(np.float32)
    bump, btri = Q.icosphere(1, 0.1, (0.5, 0.3, 1.4))               # something above the floor, a tenth of its area
    V, tri = Q.merge((V, tri), (bump, btri))
    aligned, Rm, tr = m.align_floor((_v(V), _i(tri)), num_iterations=200, num_sample_points=5000)
    z = _np(aligned)[:65 * 65, 2]
    assert np.abs(z).max() < 1e-5 and np.abs(Rm.numpy() @ Rx[:, 2] - [0, 0, 1]).max() < 1e-5
    assert _np(aligned)[65 * 65:, 2].min() > 0.3


# ------------------------------------------------------------------------------------------------------ end to end
def _fused_sphere():
    """The sphere of tests/tsdf_scenes.py fused at voxel 0.01 from 24 views in which no pixel sees the cap within 0.3 rad of
    +y (a hole), and a detached blob of radius 0.05 m 1.2 m away along +x from 8 views of its own."""
    from collab_splats_amd import TSDFVolume
    W, H = 160, 120
    centre, radius = np.array([0.1, -0.05, 0.2]), 0.3
    deps, vms, Ks, rgbs = S.sphere_views(24, W, H)
    masks = []
    for M, K, dep in zip(vms, Ks, deps[..., 0]):
        o, d = S._rays(M.astype(np.float64), K.astype(np.float64), W, H)
        p = o + d * dep[..., None]
        masks.append(~((dep > 0) & ((p - centre)[..., 1] / radius > math.cos(0.3))))
    blob = S.sphere_views(8, W, H, centre=tuple(centre + [1.2, 0, 0]), radius=0.05, dist=0.4)
    vol = TSDFVolume(0.01, 0.03, 1.0, device=DEV)
    vol.integrate(_v(deps), _v(vms), _v(Ks), rgbs=_v(rgbs), masks=torch.as_tensor(np.stack(masks)).to(DEV))
    vol.integrate(_v(blob[0]), _v(blob[1]), _v(blob[2]), rgbs=_v(blob[3]))
    return vol.extract_mesh(), centre, radius


def test_finish_mesh_end_to_end():
    import collab_splats_amd as m
    (v, f, c), centre, radius = _fused_sphere()
    r0 = (v.double().cpu() - torch.from_numpy(centre)).norm(dim=1)
    assert int((r0 > 1.0).sum()) > 100                              # the blob is in the extracted mesh
    st0 = m.mesh_edge_stats(v, f)
    assert st0["n_boundary"] > 30                                   # and so is the hole
    model = S.sphere_gaussians(20000).to(DEV)
    model.eval()
    plain = model.finish_mesh(v, f, c, align=False)
    v1, f1, c1, index = plain["vertices"], plain["triangles"], plain["colors"], plain["vertex_index"]
    assert plain["n_removed"] >= 1 and plain["n_filled"] >= 1
    r1 = (v1.double().cpu() - torch.from_numpy(centre)).norm(dim=1)
    assert float(r1.max()) < radius + 0.02                          # the blob is gone
    st1 = m.mesh_edge_stats(v1, f1)
    assert st1["n_boundary"] == 0                                   # the hole is closed
    d1 = (v1.double().cpu() - torch.from_numpy(centre)) / radius
    fan = (index.cpu() < 0) & (d1[:, 1] / d1.norm(dim=1) > math.cos(0.1)) & (d1.norm(dim=1) > 0.8)
    assert int(fan.sum()) >= 1                                      # a fan's centre sits in the middle of the masked cap
    old = index >= 0
    assert int((~old).sum()) == plain["n_filled"] and bool(old[:int(old.sum())].all())
    assert torch.equal(c1[old], c[index[old]]) and torch.equal(v1[old], v[index[old]])       # carried bit for bit
    m_new = v1.shape[0]
    assert c1.shape == (m_new, 3) and plain["normals"].shape == (m_new, 3) and int(f1.max()) == m_new - 1
    assert torch.equal(plain["mesh_transform"], torch.eye(4, dtype=torch.float64))
    assert torch.equal(plain["means"], model.means.detach())
    full = model.finish_mesh(v, f, c)
    T = full["mesh_transform"].numpy()
    assert T.shape == (4, 4) and np.array_equal(T[3], [0, 0, 0, 1]) and np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-12
    moved = _np(v1).astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    assert np.abs(_np(full["vertices"]) - moved).max() < 1e-6      # mesh_transform maps the old vertices onto the new ones
    means = _np(model.means.detach()).astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    assert np.abs(_np(full["means"]) - means).max() < 1e-6
    assert torch.equal(full["triangles"], f1) and torch.equal(full["colors"], c1)
    turned = _np(plain["normals"]).astype(np.float64) @ T[:3, :3].T
    assert np.abs(_np(full["normals"]) - turned).max() < 1e-6
