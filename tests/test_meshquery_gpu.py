"""GPU: radius-graph clustering (csrc/cluster.hip) against the restatement (tests/meshquery_restatement.py): labels and
sizes EQUAL (integers: no tolerance) on blobs on a sphere, clouds, duplicated positions, long chains, the strictness grid, the
small-cluster rule, empty inputs, vertices far from the origin; two runs bitwise equal; a permuted input gives the same
partition; mesh_clustering's lists; a full-size mesh; and extract_mesh -> mesh_attributes -> query_similarity ->
mesh_clustering end to end."""
import numpy as np
import pytest
import torch

import meshquery_restatement as R
import meshquery_scenes as Q
import tsdf_scenes as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x, np.float32)).to(DEV)


def _gpu(V, mask, r, min_size=10):
    import collab_splats_amd as m
    labels, sizes = m.cluster_labels(_t(V), torch.as_tensor(np.ascontiguousarray(mask, bool)).to(DEV), r, min_size)
    assert labels.dtype == torch.int32 and sizes.dtype == torch.int32 and labels.is_cuda and sizes.is_cuda
    assert labels.shape == (len(V),)
    return labels.cpu().numpy(), sizes.cpu().numpy()


def _check(V, mask, r, min_size=10):
    """The device's labels and sizes equal the restatement's; returns them."""
    labels, sizes = _gpu(V, mask, r, min_size)
    ref_labels, ref_sizes = R.cluster_labels(V, mask, r, min_size)
    assert np.array_equal(sizes, ref_sizes)
    assert np.array_equal(labels, ref_labels)
    return labels, sizes


@pytest.mark.parametrize("n,thr,seed", [(45000, 0.8, 0), (45000, 0.5, 1), (200000, 0.8, 2)])
def test_sphere_blobs(n, thr, seed):
    """The inputs of the host test (where the restatement equals the reference's algorithm), through mesh_clustering."""
    import collab_splats_amd as m
    V, sim = Q.sphere_blobs(n, seed)
    labels, sizes = _check(V, sim > np.float32(thr), 0.03)
    assert len(sizes) >= 3
    ref = R.mesh_clustering(V, sim, thr, 0.03)
    for shape in ((n,), (n, 1)):
        got = m.mesh_clustering(_t(V), _t(sim).reshape(shape), thr, 0.03)
        assert len(got) == len(ref)
        for a, b in zip(got, ref):
            assert a.dtype == torch.int64 and a.is_cuda and np.array_equal(a.cpu().numpy(), b)


@pytest.mark.parametrize("r", [0.012, 0.02])
def test_uniform_cloud_random_mask(r):
    rng = np.random.default_rng(11)
    V = (rng.random((30000, 3)) * 0.4).astype(np.float32)
    mask = rng.random(30000) < 0.5
    for min_size in (0, 1, 10):
        labels, sizes = _check(V, mask, r, min_size)
        assert len(sizes) >= 1 and np.all(labels[~mask] == -1)


def test_clustered_cloud():
    from test_meshmap_gpu import _cloud
    V, P = _cloud("clustered", 20000, 10, seed=12)
    rng = np.random.default_rng(13)
    labels, sizes = _check(V, rng.random(len(V)) < 0.7, 0.004)
    assert len(sizes) >= 20


def test_duplicated_positions():
    """Every position three times, shuffled: distance 0, and equal positions with different indices in one cell."""
    rng = np.random.default_rng(14)
    base = (rng.random((8000, 3)) * 0.25).astype(np.float32)
    V = np.concatenate([base, base, base])[rng.permutation(24000)]
    mask = rng.random(24000) < 0.6
    labels, sizes = _check(V, mask, 0.01)
    assert len(sizes) > 5
    labels, sizes = _check(V, mask, 1e-4, min_size=1)             # only the coincident vertices are joined
    assert sizes.max() <= 3


def test_long_chains():
    """One component of 50 000 vertices and a diameter of 50 000 edges (long find paths, contended hooks) and a second
    chain 1.5 r beside it that must stay separate."""
    V, ids = Q.chains(50000, 0.01, seed=15)
    labels, sizes = _check(V, np.ones(len(V), bool), 0.01)
    assert sorted(sizes.tolist()) == [25000, 50000]
    assert np.array_equal(labels, np.where(ids == ids[0], 0, 1))
    again = _gpu(V, np.ones(len(V), bool), 0.01)
    assert np.array_equal(again[0], labels) and np.array_equal(again[1], sizes)


def test_edge_rule_is_strict():
    V = Q.strict_grid(6)
    r = np.float32(2.0 ** -5)
    every = np.ones(len(V), bool)
    labels, sizes = _check(V, every, float(r))
    assert len(sizes) == 0 and np.all(labels == -1)                # d2 == r2 exactly in fp32: no edge, no cluster
    labels, sizes = _check(V, every, float(r), min_size=0)
    assert np.array_equal(labels, np.arange(216))
    labels, sizes = _check(V, every, float(np.nextafter(r, np.float32(1))))
    assert sizes.tolist() == [216] and np.all(labels == 0)


def test_small_cluster_rule():
    V = Q.ten_and_eleven(0.03)
    labels, sizes = _check(V, np.ones(21, bool), 0.03, min_size=10)
    assert sizes.tolist() == [11] and int((labels == 0).sum()) == 11
    labels, sizes = _check(V, np.ones(21, bool), 0.03, min_size=9)
    assert sizes.tolist() == [10, 11]


def test_empty_inputs():
    import collab_splats_amd as m
    V, sim = Q.sphere_blobs(5000, 16)
    labels, sizes = _check(V, np.zeros(5000, bool), 0.03)
    assert np.all(labels == -1) and len(sizes) == 0
    assert m.mesh_clustering(_t(V), _t(sim), 1e9, 0.03) == []
    labels, sizes = m.cluster_labels(torch.zeros((0, 3), device=DEV), torch.zeros(0, dtype=torch.bool, device=DEV), 0.03)
    assert labels.shape == (0,) and sizes.shape == (0,) and labels.dtype == torch.int32
    assert m.mesh_clustering(torch.zeros((0, 3), device=DEV), torch.zeros(0, device=DEV)) == []


def test_every_vertex_selected():
    V, _ = Q.sphere_blobs(40000, 17)
    labels, sizes = _check(V, np.ones(len(V), bool), 0.01)
    assert sizes.tolist() == [40000] and np.all(labels == 0)       # spacing 0.005: one component
    rng = np.random.default_rng(18)
    V = (rng.random((30000, 3)) * 0.5).astype(np.float32)
    labels, sizes = _check(V, np.ones(len(V), bool), 0.012, min_size=2)
    assert len(sizes) > 10


def test_far_from_the_origin():
    """|x| / r up to 2.5e5 (the bound is 2^18 = 262 144) with r = 0.01: one float step is r / 40 there."""
    rng = np.random.default_rng(19)
    V = (np.array([2000.0, -1500.0, 2500.0]) + rng.random((30000, 3)) * 0.3).astype(np.float32)
    labels, sizes = _check(V, rng.random(len(V)) < 0.8, 0.01, min_size=3)
    assert len(sizes) > 10


def test_two_runs_bitwise_equal():
    import collab_splats_amd as m
    V, sim = Q.sphere_blobs(200000, 20)
    v, mask = _t(V), torch.as_tensor(sim > 0.5).to(DEV)
    a = m.cluster_labels(v, mask, 0.03)
    b = m.cluster_labels(v, mask, 0.03)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and len(a[1]) >= 3


def test_permuted_input_gives_the_same_partition():
    V, sim = Q.sphere_blobs(60000, 21)
    mask = sim > np.float32(0.6)
    labels, sizes = _gpu(V, mask, 0.03)
    p = np.random.default_rng(22).permutation(len(V))              # new vertex i is old vertex p[i]
    labels_p, sizes_p = _gpu(V[p], mask[p], 0.03)
    part = {frozenset(np.nonzero(labels == c)[0].tolist()) for c in range(len(sizes))}
    part_p = {frozenset(p[np.nonzero(labels_p == c)[0]].tolist()) for c in range(len(sizes_p))}
    assert len(part) == len(sizes) >= 3 and part == part_p
    assert np.array_equal((labels >= 0), (labels_p >= 0)[np.argsort(p)])


def test_mesh_clustering_lists_follow_labels_and_sizes():
    import collab_splats_amd as m
    V, sim = Q.sphere_blobs(60000, 23)
    thr = 0.55
    lists = m.mesh_clustering(_t(V), _t(sim), thr, 0.03, min_cluster_size=4)
    labels, sizes = _gpu(V, sim > np.float32(thr), 0.03, 4)
    assert len(lists) == len(sizes) >= 3
    firsts = []
    for c, members in enumerate(lists):
        mem = members.cpu().numpy()
        assert len(mem) == sizes[c] > 4 and np.all(np.diff(mem) > 0)           # ascending members
        assert np.array_equal(mem, np.nonzero(labels == c)[0])
        firsts.append(mem[0])
    assert firsts == sorted(firsts)                                             # clusters by smallest member


def _sphere_mesh(voxel_size, n_views, W, H):
    from collab_splats_amd import TSDFVolume
    d, vm, K, rgb = S.sphere_views(n_views, W, H)
    vol = TSDFVolume(voxel_size, 3 * voxel_size if voxel_size > 0.005 else 0.02, 3.0, device=DEV)
    for b in range(0, n_views, 32):
        sl = slice(b, b + 32)
        vol.integrate(_t(d[sl]), _t(vm[sl]), _t(K[sl]), _t(rgb[sl]))
    return vol.extract_mesh()[0].cpu().numpy()


def test_full_size():
    """The 0.004 TSDF mesh of the sphere (106 494 vertices, as test_meshmap_gpu.test_full_size builds it) with the 30 % of
    its vertices of highest blob similarity selected (about 32 000; millions of edges at r = 0.03), and a cloud of
    1 000 000 points on the sphere with 30 % selected at r = 0.004, both against the restatement in full (a few seconds of
    numpy each on one core)."""
    V = _sphere_mesh(0.004, n_views=100, W=320, H=240)
    assert len(V) > 80000
    d = V.astype(np.float64) - np.array([0.1, -0.05, 0.2])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rng = np.random.default_rng(24)
    c = rng.standard_normal((12, 3))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    sim = np.exp(-((d[:, None, :] - c[None]) ** 2).sum(-1) / (2 * 0.15 ** 2)).max(1) + 0.05 * rng.standard_normal(len(V))
    mask = sim > np.quantile(sim, 0.7)
    assert 0.29 < mask.mean() < 0.31
    labels, sizes = _check(V, mask, 0.03)
    assert len(sizes) >= 1 and sizes.sum() > 0.9 * mask.sum()
    labels, sizes = _check(V, mask, 0.01)
    assert len(sizes) >= 3
    V, sim = Q.sphere_blobs(1_000_000, 25)
    mask = sim > np.quantile(sim, 0.7)
    labels, sizes = _check(V, mask, 0.004)
    assert len(sizes) >= 3 and sizes.max() > 10000


def test_end_to_end_three_caps():
    """extract_mesh -> mesh_attributes -> query_similarity -> mesh_clustering: the 60 k-Gaussian sphere whose Gaussians carry
    latent a inside three disjoint caps (arc radius 0.12 m on the r = 0.3 m sphere) and latent b (orthogonal) elsewhere; query
    a against b.  Exactly three clusters; a vertex more than 0.06 m (the kNN map's sdf_trunc plus r) inside a cap is in that
    cap's cluster, a vertex more than 0.06 m outside every cap is in none.  The views are fused inside the silhouette of a
    sphere of radius 0.28 only (extract_mesh's masks): without them the rendered depth at the sphere's rim leaves sheets of
    vertices up to 0.3 m off the surface, which no Gaussian has among its k nearest and which lie inside no cap."""
    import collab_splats_amd as m
    from collab_splats_amd import radegs
    centre, radius, latent = np.array([0.1, -0.05, 0.2]), 0.3, 13
    caps = np.eye(3)                                               # cap centres: the +x, +y, +z directions from the centre
    base = S.sphere_gaussians(60000)
    p = base.gauss_params
    dirs = (p["means"].data.double().numpy() - centre) / radius
    arc = radius * np.arccos(np.clip(dirs @ caps.T, -1, 1))        # [N,3] arc distance to each cap centre
    inside = (arc < 0.12).any(1)
    a, b = np.zeros(latent, np.float32), np.zeros(latent, np.float32)
    a[0], b[1] = 1.0, 1.0
    feats = torch.from_numpy(np.where(inside[:, None], a[None], b[None]))
    model = radegs.RadegsFeaturesModel(radegs.RadegsFeaturesModelConfig(features_latent_dim=latent), p["means"].data,
                                       p["scales"].data, p["quats"].data, p["opacities"].data, p["features_dc"].data,
                                       p["features_rest"].data, feats).to(DEV)
    model.step = 10 ** 6
    model.eval()
    W, H = 160, 120
    _, vms, _, _ = S.sphere_views(24, 8, 8)
    K = S.intrinsics(W, H, 60.0)
    cams = [S.pinhole_camera(M, K, W, H) for M in vms]
    masks = np.stack([S.render_sphere(M, K, W, H, centre, 0.28)[0] > 0 for M in vms])
    v, f, c = model.extract_mesh(cams, voxel_size=0.01, sdf_trunc=0.03, depth_trunc=1.0, batch_size=4, masks=masks)
    assert v.shape[0] > 10000
    assert float(((v.double().cpu() - torch.from_numpy(centre)).norm(dim=1) - radius).abs().max()) < 0.01   # a sphere, no sheets
    att = model.mesh_attributes(v)
    emb = torch.from_numpy(np.stack([a, b])).to(DEV)
    sim = m.query_similarity(att["distill_features"], emb, 1, method="pairwise", decoder=None)
    assert sim.shape == (v.shape[0],) and sim.is_cuda
    clusters = m.mesh_clustering(v, sim, similarity_threshold=0.8, spatial_radius=0.03)
    assert len(clusters) == 3
    vd = v.double().cpu().numpy() - centre
    varc = radius * np.arccos(np.clip((vd / np.linalg.norm(vd, axis=1, keepdims=True)) @ caps.T, -1, 1))
    label = np.full(v.shape[0], -1)
    for k, members in enumerate(clusters):
        label[members.cpu().numpy()] = k
    owners = set()
    for cap in range(3):
        deep = varc[:, cap] < 0.12 - 0.06
        assert deep.sum() > 50
        ks = np.unique(label[deep])
        assert len(ks) == 1 and ks[0] >= 0                          # all of them in one cluster
        owners.add(int(ks[0]))
    assert len(owners) == 3                                         # one cluster per cap
    outside = (varc > 0.12 + 0.06).all(1)
    assert outside.sum() > 1000 and np.all(label[outside] == -1)
    colors = m.similarity_colors(sim)
    assert colors.shape == (v.shape[0], 3) and float(colors[:, 0].max()) == 1.0 and torch.all(colors[:, 1:] == 0)
