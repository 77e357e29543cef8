"""GPU: the point-cloud cleaning (csrc/pointcloud.hip) against the restatement (tests/pointcloud_restatement.py), bit for bit:
mean and nearest of the kNN, the outlier masks and indices, the radius counts, the density filter and every output of the voxel
reduction, on the host test's shells (with their far outliers), a uniform cloud, duplicated positions, tight clusters and a
cloud far from the origin; nearest against cKDTree in fp64 within the derived bound; the tuning values change nothing; two
runs are bitwise equal; a permuted input gives the permuted result; a million points; clean_pcd end to end."""
import functools

import numpy as np
import pytest
import torch

import meshquery_scenes as MS
import pointcloud_restatement as R
import pointcloud_scenes as S

pytest.importorskip("scipy")
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SCENES = {
    "shell50k": lambda: S.shell(50000, 0),
    "shell200k": lambda: S.shell(200000, 1),
    "uniform": lambda: S.uniform(30000, 11),
    "duplicates": lambda: S.duplicates(8000, 3, 14),
    "clustered": lambda: S.clustered(20000, 10, 12),
    "far": lambda: S.far(30000, 19),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    P = SCENES[name]()
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def ref_knn(name, k):
    return R.knn_mean_distance(scene(name), k)


def _t(x):
    return torch.from_numpy(np.array(x, np.float32)).to(DEV)       # (a copy: the cached scenes are read-only)


def _eq(got: torch.Tensor, ref: np.ndarray):
    """Bitwise: the same dtype, shape and bytes."""
    g = got.cpu().numpy()
    assert g.dtype == ref.dtype and g.shape == ref.shape, (g.dtype, ref.dtype, g.shape, ref.shape)
    assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(ref).view(np.uint8))


# -------------------------------------------------------------------------------------------------------------- kNN
@pytest.mark.parametrize("name", list(SCENES))
def test_knn_and_outlier_mask_equal_restatement(name):
    import collab_splats_amd as m
    P = scene(name)
    mean, nearest = m.knn_mean_distance(_t(P), 20)
    ref_mean, ref_nearest = ref_knn(name, 20)
    _eq(mean, ref_mean)
    _eq(nearest, ref_nearest)
    assert not nearest.any()                                        # every point finds itself
    keep, avg = m.statistical_outlier_mask(_t(P), 20, 2.0)
    thr, n_valid = R.outlier_threshold(ref_mean, 2.0)
    ref_keep = (ref_mean > 0) & (ref_mean.astype(np.float64) < thr)
    _eq(avg, ref_mean)
    assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), ref_keep)
    pts, ind = m.remove_statistical_outlier(_t(P), 20, 2.0)
    assert ind.dtype == torch.int64 and np.array_equal(ind.cpu().numpy(), np.nonzero(ref_keep)[0])
    _eq(pts, P[ref_keep])
    if name.startswith("shell"):
        assert 0.985 * len(P) < ref_keep.sum() < 0.995 * len(P)    # the far 1 % goes
    if name == "duplicates":
        assert ref_keep.sum() > 0.9 * len(P) and n_valid == len(P)


@pytest.mark.parametrize("k", [1, 3, 4, 5, 8, 9, 16, 17, 32])
def test_every_k_class_and_separate_queries(k):
    """k at both ends of each compiled list size (4, 8, 16, 32); queries inside, beside and far outside the cloud."""
    import collab_splats_amd as m
    P = scene("uniform")
    rng = np.random.default_rng(30 + k)
    Q = np.concatenate([P[:300], (rng.random((300, 3)) * 0.4).astype(np.float32),
                        (rng.uniform(-3, 3, (100, 3))).astype(np.float32), np.float32([[40.0, -7.0, 0.2], [0.2, 0.2, 900.0]])])
    mean, nearest = m.knn_mean_distance(_t(P), k, queries=_t(Q))
    ref_mean, ref_nearest = R.knn_mean_distance(P, k, Q)
    _eq(mean, ref_mean)
    _eq(nearest, ref_nearest)
    mean, nearest = m.knn_mean_distance(_t(P[:2000]), k)
    ref_mean, ref_nearest = R.knn_mean_distance(P[:2000], k)
    _eq(mean, ref_mean)
    _eq(nearest, ref_nearest)


def test_duplicates_fewer_points_than_k_and_few_valid():
    import collab_splats_amd as m
    rng = np.random.default_rng(4)
    P = np.concatenate([np.repeat(rng.random((3, 3)), 5, 0), rng.random((200, 3))]).astype(np.float32)
    keep, avg = m.statistical_outlier_mask(_t(P), 5)
    ref_keep, ref_avg = R.statistical_outlier(P, 5)
    _eq(avg, ref_avg)
    assert np.array_equal(keep.cpu().numpy(), ref_keep) and not keep[:15].any() and not avg[:15].any()
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)     # N < k: k_eff = 3
    mean, nearest = m.knn_mean_distance(_t(P), 20)
    ref = R.knn_mean_distance(P, 20)
    _eq(mean, ref[0])
    _eq(nearest, ref[1])
    for cloud, nb in ((np.zeros((4, 3), np.float32), 3), (np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0]], np.float32), 2),
                      (np.zeros((1, 3), np.float32), 20)):         # n_valid = 0, 1, 0
        keep, avg = m.statistical_outlier_mask(_t(cloud), nb)
        ref_keep, ref_avg = R.statistical_outlier(cloud, nb)
        _eq(avg, ref_avg)
        assert np.array_equal(keep.cpu().numpy(), ref_keep)


def test_empty_cloud():
    import collab_splats_amd as m
    E = torch.zeros((0, 3), device=DEV)
    mean, nearest = m.knn_mean_distance(E, 5)
    assert mean.shape == nearest.shape == (0,) and mean.dtype == torch.float32 and mean.is_cuda
    keep, avg = m.statistical_outlier_mask(E)
    assert keep.shape == (0,) and keep.dtype == torch.bool
    pts, ind = m.remove_statistical_outlier(E)
    assert pts.shape == (0, 3) and ind.shape == (0,) and ind.dtype == torch.int64
    assert m.radius_count(E, 0.1).shape == (0,)
    assert m.radius_count(E, 0.1, queries=torch.ones((2, 3), device=DEV)).tolist() == [0, 0]
    pts, ind = m.density_filter(E)
    assert pts.shape == (0, 3) and ind.shape == (0,)
    pts, att, first, counts = m.voxel_down_sample(E, 0.1, [torch.zeros((0, 2), device=DEV)])
    assert pts.shape == (0, 3) and att[0].shape == (0, 2) and first.dtype == torch.int64 and counts.dtype == torch.int32
    pts, ind = m.clean_pcd(E)
    assert pts.shape == (0, 3) and ind.shape == (0,)
    assert m.knn_mean_distance(torch.ones((5, 3), device=DEV), 3, queries=E)[0].shape == (0,)


def test_nearest_against_ckdtree_within_the_derived_bound():
    """k = 1, separate queries, against cKDTree in fp64 on the same fp32 inputs.  With u = 2^-24: dx = fl(q - x) errs by at
    most u |dx| (the inputs are the same floats on both sides), its square by 2 u + u, the two sums of non-negative terms add
    u each: every fp32 d2 is within 5 u of its true value, relatively, so the smallest of them is within 5 u of the true
    smallest; its square root is within 2.5 u, and sqrtf adds u / 2: |nearest - d| <= 3 u d.  The assertion allows the
    8 u d plus one fp32 ulp of the coordinates' magnitude that the feature's specification sets."""
    from scipy.spatial import cKDTree
    import collab_splats_amd as m
    for name, seed in (("shell50k", 40), ("far", 41)):
        P = scene(name)
        rng = np.random.default_rng(seed)
        Q = (P[rng.integers(0, len(P), 20000)] + rng.normal(0, 0.01, (20000, 3))).astype(np.float32)
        _, nearest = m.knn_mean_distance(_t(P), 1, queries=_t(Q))
        d64, _ = cKDTree(P.astype(np.float64)).query(Q.astype(np.float64))
        bound = 8 * 2.0 ** -24 * d64 + float(np.spacing(np.float32(max(np.abs(P).max(), np.abs(Q).max()))))
        err = np.abs(nearest.double().cpu().numpy() - d64)
        print(f"{name}: max |nearest - d64| = {err.max():.3e}, max of error / bound = {(err / bound).max():.3f}, "
              f"max relative error = {(err / np.maximum(d64, 1e-30)).max():.3e}")
        assert np.all(err <= bound)
        import collab_splats_amd.pointcloud as pc
        acc = pc.calculate_accuracy(_t(Q), _t(P), 90)
        assert abs(acc - np.percentile(d64, 90)) <= bound.max()
        comp = pc.calculate_completeness(_t(P), _t(Q), 0.01)
        assert abs(comp - 100 * np.mean(d64 < 0.01)) <= 100 * np.mean(np.abs(d64 - 0.01) <= bound)


def test_tuning_values_runs_and_permutation_change_nothing():
    import collab_splats_amd as m
    import collab_splats_amd.pointcloud as pc
    P = scene("shell50k")
    p = _t(P)
    base = m.statistical_outlier_mask(p, 20, 2.0)
    again = m.statistical_outlier_mask(p, 20, 2.0)
    assert torch.equal(base[0], again[0]) and torch.equal(base[1].view(torch.int32), again[1].view(torch.int32))
    try:
        for edge, lanes in ((0.002, 1), (0.05, 8), (None, 1), (0.011, 8)):
            pc.CELL_EDGE, pc.LANES_PER_QUERY = edge, lanes
            keep, avg = m.statistical_outlier_mask(p, 20, 2.0)
            assert torch.equal(keep, base[0]) and torch.equal(avg.view(torch.int32), base[1].view(torch.int32)), (edge, lanes)
            for k in (1, 7, 32):
                _eq(m.knn_mean_distance(p[:5000], k)[0], R.knn_mean_distance(P[:5000], k)[0])
    finally:
        pc.CELL_EDGE, pc.LANES_PER_QUERY = None, 8
    perm = np.random.default_rng(42).permutation(len(P))           # new point i is old point perm[i]
    keep_p, avg_p = m.statistical_outlier_mask(_t(P[perm]), 20, 2.0)
    assert torch.equal(avg_p.view(torch.int32).cpu(), base[1].view(torch.int32).cpu()[perm])
    assert torch.equal(keep_p.cpu(), base[0].cpu()[perm])
    cnt = m.radius_count(p, 0.03)
    assert torch.equal(m.radius_count(p, 0.03), cnt) and torch.equal(m.radius_count(_t(P[perm]), 0.03).cpu(), cnt.cpu()[perm])
    a = m.voxel_down_sample(p, 0.01, [p])
    b = m.voxel_down_sample(p, 0.01, [p])
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip((a[0], a[1][0]), (b[0], b[1][0])))
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


# ----------------------------------------------------------------------------------------------------- radius count
@pytest.mark.parametrize("name,r", [("shell50k", 0.03), ("shell200k", 0.01), ("uniform", 0.02), ("duplicates", 0.01),
                                    ("duplicates", 1e-4), ("clustered", 0.004), ("far", 0.01)])
def test_radius_count_and_density_filter_equal_restatement(name, r):
    import collab_splats_amd as m
    P = scene(name)
    ref = R.radius_count(P, r)
    cnt = m.radius_count(_t(P), r)
    _eq(cnt, ref)
    assert ref.min() >= 1 and ref.max() > 1
    for pct in (0, 10, 55.5, 100):
        pts, ind = m.density_filter(_t(P), r, pct)
        ref_ind = np.nonzero(ref >= np.percentile(ref, pct))[0]
        assert ind.dtype == torch.int64 and np.array_equal(ind.cpu().numpy(), ref_ind)
        _eq(pts, P[ref_ind])
    Q = np.concatenate([P[:500], P[:500] + np.float32(0.5 * r), np.float32([[1e6, 0, 0], [3e9, -3e9, 3e9]])]).astype(np.float32)
    _eq(m.radius_count(_t(P), r, queries=_t(Q)), R.radius_count(P, r, Q))


def test_radius_rule_is_strict():
    import collab_splats_amd as m
    V = MS.strict_grid(6)
    r = np.float32(2.0 ** -5)
    assert torch.all(m.radius_count(_t(V), float(r)) == 1)         # d2 == r2 exactly in fp32: not counted
    up = float(np.nextafter(r, np.float32(1)))
    _eq(m.radius_count(_t(V), up), R.radius_count(V, up))
    assert int(m.radius_count(_t(V), up).sum()) == 216 + 2 * 3 * 6 * 6 * 5


# ------------------------------------------------------------------------------------------------------------ voxel
def _check_voxel(P, voxel, attributes=(), min_bound=None):
    import collab_splats_amd as m
    pts, att, first, counts = m.voxel_down_sample(_t(P), voxel, [_t(a) for a in attributes], min_bound)
    ref_pts, ref_att, ref_first, ref_counts = R.voxel_down_sample(P, voxel, attributes, min_bound)
    _eq(pts, ref_pts)
    assert len(att) == len(ref_att)
    for a, b in zip(att, ref_att):
        _eq(a, b)
    _eq(first, ref_first)
    _eq(counts, ref_counts)
    return ref_counts


@pytest.mark.parametrize("name,voxel", [("shell200k", 0.01), ("shell200k", 0.015), ("shell50k", 0.004), ("uniform", 0.013),
                                        ("duplicates", 0.003), ("clustered", 0.002), ("far", 0.01), ("uniform", 5.0)])
def test_voxel_down_sample_equals_fp64_evaluation(name, voxel):
    P = scene(name)
    rng = np.random.default_rng(50)
    normals = rng.standard_normal((len(P), 3)).astype(np.float32)
    feats = rng.random((len(P), 7)).astype(np.float32)
    counts = _check_voxel(P, voxel, [normals, feats])
    assert counts.sum() == len(P) and (len(counts) == 1) == (voxel == 5.0)
    _check_voxel(P, voxel, [], min_bound=(P.min(0).astype(np.float64) - np.array([0.3, 0.001, 7.0])).tolist())


@pytest.mark.parametrize("n", [256, 257, 65537])
def test_voxel_down_sample_at_the_sort_pass_counts(n):
    """The points are sorted by voxel number, 0 .. N - 1, 8 bits a pass: one pass at N = 256, two at 257, three at 65 537.  A
    voxel holds 4 points on average, so the order of the fp64 sums shows whether the sort kept the points of a voxel in
    ascending index."""
    P = S.uniform(n, 60 + n % 7)
    voxel = 0.4 / round((n / 4) ** (1 / 3))
    feats = np.random.default_rng(n).random((n, 5)).astype(np.float32)
    counts = _check_voxel(P, voxel, [feats])
    assert counts.sum() == n and counts.max() >= 4 and n / 8 < len(counts) < n / 2


# ---------------------------------------------------------------------------------------------- full size, end to end
def test_full_size():
    """10^6 points (a shell with its far 1 %): the kNN and the radius count against the restatement at 3000 sampled points
    (queried separately there: the same candidate set, the point itself included), the mask against the restated threshold
    of the device's own means, the voxel reduction's invariants."""
    import collab_splats_amd as m
    n = 1_000_000
    P = S.shell(n, 60)
    p = _t(P)
    keep, avg = m.statistical_outlier_mask(p, 20, 2.0)
    sample = np.random.default_rng(61).choice(n, 3000, replace=False)
    far = np.nonzero(np.abs(np.linalg.norm(P, axis=1) - 0.3) > 0.05)[0][:500]      # outliers: the coarse levels' path
    sample = np.concatenate([sample, far])
    avg_h = avg.cpu().numpy()
    ref_mean, _ = R.knn_mean_distance(P, 20, P[sample])
    assert np.array_equal(avg_h[sample].view(np.uint32), ref_mean.view(np.uint32))
    thr, n_valid = R.outlier_threshold(avg_h, 2.0)
    assert n_valid == n
    assert np.array_equal(keep.cpu().numpy(), avg_h.astype(np.float64) < thr)
    assert 0.985 * n < int(keep.sum()) < 0.995 * n
    cnt = m.radius_count(p, 0.01)
    assert np.array_equal(cnt.cpu().numpy()[sample], R.radius_count(P, 0.01, P[sample]))
    pts, _, first, counts = m.voxel_down_sample(p, 0.01)
    assert int(counts.sum()) == n and bool((first[1:] > first[:-1]).all()) and first[0] == 0
    origin = P.astype(np.float64).min(0) - 0.005
    cells = np.floor((P[first.cpu().numpy()].astype(np.float64) - origin) / 0.01).astype(np.int64)
    assert len(np.unique(cells, axis=0)) == len(cells) == pts.shape[0]
    assert np.array_equal(np.floor((pts.double().cpu().numpy() - origin) / 0.01).astype(np.int64)[counts.cpu().numpy() == 1],
                          cells[counts.cpu().numpy() == 1])


def test_clean_pcd_end_to_end():
    """The Gaussian means of the synthetic scene plus far strays, through clean_pcd and RadegsModel.clean_gaussians: the stages
    equal the restatement's, the indices reproduce the returned points, the strays go."""
    import collab_splats_amd as m
    import tsdf_scenes as T
    from collab_splats_amd.synthetic import random_scene
    means = random_scene(40000, 64, 64, seed=5)["means"].float().cpu().numpy()
    rng = np.random.default_rng(70)
    P = np.concatenate([means, means.mean(0) + rng.uniform(-30, 30, (200, 3))]).astype(np.float32)[rng.permutation(40200)]
    pts, idx = m.clean_pcd(_t(P), outlier_removal=True, downsample=False, max_distance=1e9)
    ref_keep, _ = R.statistical_outlier(P, 20, 2.0)
    assert np.array_equal(idx.cpu().numpy(), np.nonzero(ref_keep)[0])
    _eq(pts, P[ref_keep])                                           # without the voxel stage: points == input[indices]
    pts, idx = m.clean_pcd(_t(P), voxel_size=0.5, radius=0.4, max_distance=6.0)
    avg = float(R.radius_count(P, 2.0 * float(np.float32(0.4)), P[:1000]).astype(np.float64).mean())
    vs = 0.5 * max(0.5, min(2.0, 50.0 / max(1e-6, avg)))
    v_pts, _, v_first, _ = R.voxel_down_sample(P, vs)
    keep, _ = R.statistical_outlier(v_pts, 20, 2.0)
    s_pts, s_idx = v_pts[keep], v_first[keep]
    near = np.linalg.norm(s_pts - s_pts.mean(0, dtype=np.float32), axis=1) <= 6.0
    assert idx.dtype == torch.int64 and 100 < len(idx) < len(P)
    assert np.array_equal(idx.cpu().numpy()[:50], s_idx[near][:50]) and abs(len(idx) - near.sum()) <= 2
    model = T.sphere_gaussians(20000).to(DEV)
    model.gauss_params["means"].data[::1000] += 25.0                # 20 strays
    kept = model.clean_gaussians(downsample=False, max_distance=1.0)
    assert kept.dtype == torch.int64 and kept.is_cuda and 19000 < len(kept) <= 19980
    assert not np.isin(np.arange(0, 20000, 1000), kept.cpu().numpy()).any()
    pts, idx = m.clean_pcd(model.means.detach(), downsample=False, max_distance=1.0)
    assert torch.equal(idx, kept) and torch.equal(pts, model.means.detach()[idx])
