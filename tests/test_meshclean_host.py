"""CPU: the numpy restatement of the mesh-finishing kernels (tests/meshclean_restatement.py) against independent forms
(scipy's connected_components over the face-adjacency graph, a brute-force fp64 inlier count, closed forms of small meshes), and
the argument checks of collab_splats_amd.meshclean, which run before anything touches the GPU."""
import numpy as np
import pytest
import torch

import meshclean_restatement as R
import meshclean_scenes as Q


def _face_adjacency_components(tri):
    """scipy: faces are nodes, two faces are adjacent iff they share an undirected edge."""
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    T = len(tri)
    owners = {}
    for f, (a, b, c) in enumerate(tri):
        for x, y in ((a, b), (b, c), (c, a)):
            if x != y:
                owners.setdefault((min(x, y), max(x, y)), []).append(f)
    rows, cols = [], []
    for fs in owners.values():
        rows += [fs[0]] * (len(fs) - 1)
        cols += fs[1:]
    g = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(T, T))
    n, lab = connected_components(g, directed=False)
    first = np.full(n, T)
    np.minimum.at(first, lab, np.arange(T))
    rank = np.argsort(np.argsort(first))                            # numbered by smallest face
    return rank[lab]


@pytest.mark.parametrize("scene", ["tetra_vertex", "tetra_edge", "aabb", "strips", "shuffled"])
def test_components_match_scipy(scene):
    if scene == "tetra_vertex":
        V, tri = Q.tetra_pair(1)
    elif scene == "tetra_edge":
        V, tri = Q.tetra_pair(2)
    elif scene == "aabb":
        V, tri, _ = Q.aabb_scene()
    elif scene == "strips":
        V, tri = Q.merge(Q.strip(300), Q.strip(200, y0=5.0))
    else:
        V, tri, _ = Q.aabb_scene()
        tri = tri[np.random.default_rng(3).permutation(len(tri))]
    labels, sizes = R.mesh_components(V, tri)
    ref = _face_adjacency_components(tri)
    assert np.array_equal(labels, ref)
    assert np.array_equal(sizes, np.bincount(ref))


def test_small_mesh_closed_forms():
    V, tri = Q.tetra_pair(1)
    assert len(R.mesh_components(V, tri)[1]) == 2                   # vertex adjacency would give 1
    V, tri = Q.tetra_pair(2)
    st = R.mesh_edge_stats(V, tri)
    assert len(R.mesh_components(V, tri)[1]) == 1 and st["n_nonmanifold"] == 1 and st["n_boundary"] == 0 and st["n_edges"] == 11
    V, tri = Q.icosphere(2)
    st = R.mesh_edge_stats(V, tri)
    assert st["n_edges"] == 3 * len(tri) // 2 and st["n_boundary"] == 0 and len(R.mesh_holes(V, tri)[2]) == 0
    V, tri = Q.sheet(64, Q.THREE_HOLES)
    loop, edges, n_edges, perimeter = R.mesh_holes(V, tri)
    assert sorted(n_edges.tolist()) == sorted([256] + [2 * ((i1 - i0) + (j1 - j0)) for i0, i1, j0, j1 in Q.THREE_HOLES])
    assert np.array_equal(perimeter, n_edges / 64.0)
    assert len(R.mesh_holes(*Q.sheet(64, Q.BOW_TIE))[2]) == 2       # the rim, and the pinched pair as one loop
    V2, tri2, n = R.fill_holes(V, tri, 3.0)
    assert n == 3 and R.mesh_edge_stats(V2, tri2)["n_boundary"] == 256


def test_inlier_counts_match_brute_force_fp64():
    P, _ = Q.planted_plane(4000, seed=5)
    triples = R.ransac_triples(len(P), 50, 7)
    assert all(len(set(t)) == 3 for t in triples.tolist()) and triples.min() >= 0 and triples.max() < len(P)
    planes = R.planes_from_triples(P, triples)
    t = 0.02
    counts = R.plane_inlier_counts(P, planes, t)
    dist = np.abs(P.astype(np.float64) @ planes[:, :3].astype(np.float64).T + planes[:, 3].astype(np.float64))     # [N,H]
    sure_in = (dist < t - 1e-5).sum(0)                              # beyond fp32 rounding of the residual (|x| <= 1.5: ~ 4e-7)
    sure_out = (dist < t + 1e-5).sum(0)
    assert (sure_in <= counts).all() and (counts <= sure_out).all()
    assert np.allclose(np.linalg.norm(planes[:, :3].astype(np.float64), axis=1), 1, atol=1e-6)
    for pl, tr in zip(planes, triples):                             # the plane passes through its three points
        assert np.abs(P[tr].astype(np.float64) @ pl[:3].astype(np.float64) + float(pl[3])).max() < 1e-5


def test_restatement_plane_rules():
    P = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 0]], np.float32)
    planes = R.planes_from_triples(P, [[0, 1, 2], [0, 3, 4], [0, 3, 4]])
    counts = R.plane_inlier_counts(P, planes, 0.01)
    assert np.isnan(planes[0]).all() and counts[0] == 0             # collinear: scores 0
    assert counts[1] == counts[2] == 4
    assert R.segment_plane(P, 0.01, triples=[[0, 1, 2], [0, 3, 4], [0, 3, 4]])[2] == 1     # a tie: the lowest index
    assert not np.array_equal(R.ransac_triples(1000, 20, 0), R.ransac_triples(1000, 20, 1))
    assert np.array_equal(R.ransac_triples(1000, 20, 0), R.ransac_triples(1000, 20, 0))
    assert all(sorted(t) == [0, 1, 2] for t in R.ransac_triples(3, 40, 9).tolist())        # N = 3: redraws until distinct


def test_restatement_alignment():
    P, nrm = Q.planted_plane(3000, 0.7, normal=(0.3, -0.2, -0.9), offset=0.4, seed=2, clutter_gap=0.1)
    aligned, Rm, tr = R.align_floor_cloud(P, 0.02, 200, 0)
    assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(Rm) - 1) < 1e-12
    assert np.allclose(Rm @ -nrm, [0, 0, 1], atol=2e-3)             # the upward normal (n_z was negative) goes to +z
    on = np.abs(P.astype(np.float64) @ nrm - 0.4) < 0.02 / 4 + 1e-6
    assert np.abs(aligned[on, 2]).max() <= 0.02


def _mesh():
    V, tri = Q.tetra_pair(2)
    return torch.from_numpy(V), torch.from_numpy(tri)


def test_argument_checks():
    import collab_splats_amd as m
    from collab_splats_amd import meshclean
    v, t = _mesh()
    mesh_calls = [m.mesh_edge_stats, m.mesh_components, m.filter_mesh_components, m.mesh_holes, m.fill_holes,
                  lambda a, b: m.sample_surface(a, b, 10), lambda a, b: m.align_floor((a, b))]
    for call in mesh_calls:
        bad = t.clone()
        bad[3, 1] = v.shape[0]
        with pytest.raises(ValueError, match="indices"):
            call(v, bad)
        bad[3, 1] = -1
        with pytest.raises(ValueError, match="indices"):
            call(v, bad)
        with pytest.raises(ValueError, match=r"\[T,3\]"):
            call(v, torch.zeros((2, 4), dtype=torch.int64))
        with pytest.raises(ValueError, match="int32 or int64"):
            call(v, t.float())
        with pytest.raises(ValueError, match=r"\[N,3\]"):
            call(v[:, :2], t)
        with pytest.raises(m.MisplatError, match="CPU tensor"):     # everything is in order: there is no CPU fallback
            call(v, t)
    with pytest.raises(ValueError, match="one row per vertex"):
        m.filter_mesh_components(v, t, attributes=(torch.zeros(3, 2),))
    with pytest.raises(ValueError, match="float32"):
        m.fill_holes(v, t, attributes=(torch.zeros(v.shape[0], 2, dtype=torch.float64),))
    p = torch.rand(10, 3)
    with pytest.raises(ValueError, match="ransac_n"):
        m.segment_plane(p, ransac_n=4)
    with pytest.raises(ValueError, match="at least 3"):
        m.segment_plane(p[:2])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="distance_threshold"):
            m.segment_plane(p, distance_threshold=bad)
        with pytest.raises(ValueError, match="distance_threshold"):
            m.plane_inlier_counts(p, torch.zeros(2, 4), bad)
    with pytest.raises(ValueError, match="hypotheses"):
        m.segment_plane(p, num_iterations=0)
    with pytest.raises(ValueError, match="seed"):
        m.segment_plane(p, seed=-1)
    with pytest.raises(ValueError, match="triples must index"):
        m.segment_plane(p, triples=torch.tensor([[0, 1, 10]]))
    with pytest.raises(ValueError, match=r"\[H,4\]"):
        m.plane_inlier_counts(p, torch.zeros(2, 3), 0.1)
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        m.align_floor(torch.zeros(5, 2))
    with pytest.raises(m.MisplatError, match="CPU tensor"):
        m.segment_plane(p)
    with pytest.raises(m.MisplatError, match="CPU tensor"):
        m.plane_inlier_counts(p, torch.zeros(2, 4), 0.1)
    with pytest.raises(m.MisplatError, match="CPU tensor"):
        m.align_floor(p)
    monkey = meshclean.PLANE_TILE
    try:
        meshclean.PLANE_TILE = 12
        with pytest.raises(ValueError, match="PLANE_TILE"):
            m.plane_inlier_counts(p, torch.zeros(2, 4), 0.1)
    finally:
        meshclean.PLANE_TILE = monkey


def test_floor_rotation_matches_restatement():
    from collab_splats_amd.meshclean import floor_rotation
    for plane in ([0.3, -0.2, 0.9, 0.4], [0.3, -0.2, -0.9, 0.4], [0, 0, 2, 1], [0, 0, -1, 1], [1e-7, 0, 1, 0], [1, 0, 0, -2]):
        Rm, d = floor_rotation(plane)
        Rr, dr = R.floor_rotation(plane)
        assert np.allclose(Rm.numpy(), Rr, atol=1e-15) and d == dr
        n = np.array(plane[:3]) / np.linalg.norm(plane[:3])
        n = -n if n[2] < 0 else n
        if np.linalg.norm(np.cross(n, [0, 0, 1])) < 1e-6:
            assert np.array_equal(Rm.numpy(), np.eye(3))
        else:
            assert np.allclose(Rm.numpy() @ n, [0, 0, 1], atol=1e-12)
