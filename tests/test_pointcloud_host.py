"""CPU: the point-cloud restatement (tests/pointcloud_restatement.py) against Open3D's algorithms written independently here
(cKDTree in fp64), its edge cases, the percentile rule, and the argument checks of every public name of
collab_splats_amd.pointcloud.  No GPU."""
import math

import numpy as np
import pytest
import torch

import meshquery_scenes as MS
import pointcloud_restatement as R
import pointcloud_scenes as S

pytest.importorskip("scipy")

SHELLS = [(50000, 0), (200000, 1)]


# ---------------------------------------------------------------------------------------------------- outlier mask
def _open3d_outlier_mask(P, nb_neighbors=20, std_ratio=2.0):
    """Open3D's remove_statistical_outlier as recalled, in fp64: (keep, avg, threshold)."""
    from scipy.spatial import cKDTree
    P64 = P.astype(np.float64)
    dist, _ = cKDTree(P64).query(P64, k=nb_neighbors)
    avg = dist.mean(1)
    valid = avg > 0
    mu = avg[valid].sum() / valid.sum()
    sigma = math.sqrt(((avg[valid] - mu) ** 2).sum() / (valid.sum() - 1))
    thr = mu + std_ratio * sigma
    return valid & (avg < thr), avg, thr


@pytest.mark.parametrize("n,seed", SHELLS)
def test_restated_outlier_mask_equals_open3d_algorithm(n, seed):
    """The masks may differ only at points with |avg64 - thr64| <= 1e-5 thr64, and at most 1e-4 N points may be that close
    (measured on these seeds: none is, and the masks are equal)."""
    P = S.shell(n, seed)
    keep64, avg64, thr64 = _open3d_outlier_mask(P)
    keep32, avg32 = R.statistical_outlier(P)
    close = np.abs(avg64 - thr64) <= 1e-5 * thr64
    differ = keep64 != keep32
    print(f"shell n={n}: kept {int(keep64.sum())} (fp64) / {int(keep32.sum())} (restatement), {int(close.sum())} within 1e-5 of "
          f"the threshold {thr64:.6g}, masks differ at {int(differ.sum())}, max |avg32 - avg64| / mean = "
          f"{np.abs(avg32 - avg64).max() / avg64.mean():.3g}")
    assert close.sum() <= 1e-4 * n                                  # (the reference side alone stays inside the cap)
    assert not np.any(differ & ~close)
    assert 0.985 * n < keep32.sum() < 0.995 * n                    # the 1 % far points go, the shell stays
    assert np.abs(avg32 - avg64).max() <= 1e-4 * avg64.mean()


def test_fixed_sum_is_a_sum():
    rng = np.random.default_rng(2)
    for n in (0, 1, 255, 256, 257, 70000):
        v = rng.random(n)
        assert abs(R.fixed_sum(v) - math.fsum(v)) <= 1e-12 * max(1.0, n)


# ---------------------------------------------------------------------------------------------------- radius count
@pytest.mark.parametrize("n,seed", SHELLS)
def test_restated_radius_count_equals_ckdtree(n, seed):
    """The fp32 strict rule against cKDTree's fp64 <= rule at r = 0.03: equal, except where a pair's distance lies within the
    fp32 rule's own rounding of r.  With u = 2^-24 an fp32 d2 is within 5 u of its true value (dx = fl(xi - xj) errs by
    u |dx|, the square by 3 u, two sums of non-negative terms by u each) and r2 = fl(r r) within u of float32(r)^2, float32(r)
    within u of r: the two rules can disagree on a pair only if | d - r | <= 4 u r; the test allows 8 u r, the bound of the
    nearest-distance test.  A point whose counts differ must therefore see the fp64 count change between r (1 - 8 u) and
    r (1 + 8 u), and the fp32 count must lie between those two.  Measured: at n = 50 000 (3 10^6 pairs within r) the counts
    are equal; at n = 200 000 (5 10^7 pairs) 2 points differ (one pair), and every seed 1 .. 50 of that scene leaves between
    2 and 16 such points: at that many pairs a rounding coincidence of the input is the rule, so equality is asserted outside
    the band, not inside it."""
    from scipy.spatial import cKDTree
    P = S.shell(n, seed)
    P64 = P.astype(np.float64)
    tree = cKDTree(P64)
    ref = tree.query_ball_point(P64, 0.03, return_length=True)
    got = R.radius_count(P, 0.03)
    assert got.dtype == np.int32 and got.min() == 1 and got.max() > 50              # lone far points count themselves
    differ = np.nonzero(got != ref)[0]
    print(f"shell n={n}: {len(differ)} of {n} counts differ from cKDTree's, {int((ref.sum() - n) // 2)} pairs within r")
    eps = 8 * 2.0 ** -24
    lo = tree.query_ball_point(P64[differ], 0.03 * (1 - eps), return_length=True)
    hi = tree.query_ball_point(P64[differ], 0.03 * (1 + eps), return_length=True)
    assert np.all(lo < hi) and np.all(lo <= got[differ]) and np.all(got[differ] <= hi)
    assert len(differ) <= 1e-4 * n
    if n == 50000:
        assert len(differ) == 0


def test_radius_rule_is_strict():
    V = MS.strict_grid(6)
    r = np.float32(2.0 ** -5)
    assert np.all(R.radius_count(V, float(r)) == 1)                # neighbours at d2 == r2 exactly: not counted
    up = R.radius_count(V, float(np.nextafter(r, np.float32(1))))
    assert up.min() == 4 and up.max() == 7 and up.sum() == 216 + 2 * 3 * 6 * 6 * 5
    assert np.array_equal(R.radius_count(V, float(r), queries=V[:10]), np.ones(10, np.int32))


# ----------------------------------------------------------------------------------------------------------- voxel
def _voxel_by_dictionary(P, voxel, min_bound=None):
    """Open3D's accumulation: a map from the fp64 cell to (sum, count), filled in point order."""
    P64 = P.astype(np.float64)
    origin = (P64.min(0) if min_bound is None else np.asarray(min_bound, np.float64)) - voxel / 2
    acc = {}
    for i, p in enumerate(P64):
        key = tuple(np.floor((p - origin) / voxel).astype(np.int64).tolist())
        if key not in acc:
            acc[key] = [np.zeros(3), 0, i]
        acc[key][0] += p
        acc[key][1] += 1
    rows = sorted(acc.values(), key=lambda e: e[2])
    return (np.array([(s / c) for s, c, _ in rows]).astype(np.float32), np.array([i for _, _, i in rows], np.int64),
            np.array([c for _, c, _ in rows], np.int32))


@pytest.mark.parametrize("voxel,min_bound", [(0.01, None), (0.015, None), (0.05, (-2.0, -2.0, -2.0))])
def test_restated_voxel_equals_dictionary_evaluation(voxel, min_bound):
    P = S.shell(3000, 3)
    pts, (att,), first, counts = R.voxel_down_sample(P, voxel, [P[:, ::-1] * 2], min_bound)
    ref_pts, ref_first, ref_counts = _voxel_by_dictionary(P, voxel, min_bound)
    assert np.array_equal(pts, ref_pts) and np.array_equal(first, ref_first) and np.array_equal(counts, ref_counts)
    assert np.all(np.diff(first) > 0) and counts.sum() == 3000 and len(first) < 3000
    assert np.array_equal(att, pts[:, ::-1] * 2)                   # (a permuted, doubled copy: the same sums, exactly)


# ------------------------------------------------------------------------------------------------------ edge cases
def test_coincident_points_have_zero_mean_and_are_dropped():
    rng = np.random.default_rng(4)
    P = np.concatenate([np.repeat(rng.random((3, 3)), 5, 0), rng.random((200, 3))]).astype(np.float32)
    keep, avg = R.statistical_outlier(P, nb_neighbors=5)
    assert np.all(avg[:15] == 0) and not keep[:15].any() and np.all(avg[15:] > 0) and keep[15:].sum() > 150
    keep, avg = R.statistical_outlier(P, nb_neighbors=6)           # a sixth neighbour: no longer zero
    assert np.all(avg[:15] > 0)


def test_fewer_points_than_k_and_single_valid_point():
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)
    mean, nearest = R.knn_mean_distance(P, 20)                     # k_eff = 3
    assert np.array_equal(nearest, np.zeros(3, np.float32))
    assert np.array_equal(mean, (np.float32([1, 1, 2]) + np.sqrt(np.float32([4, 5, 5]))) / np.float32(3))
    keep, avg = R.statistical_outlier(np.zeros((4, 3), np.float32), 3)
    assert not keep.any() and np.all(avg == 0)                     # n_valid = 0
    P = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0]], np.float32)
    keep, avg = R.statistical_outlier(P, 2)                        # n_valid = 1: no threshold, keep = avg > 0
    assert keep.tolist() == [False, False, True] and R.outlier_threshold(avg)[0] == np.inf
    keep, avg = R.statistical_outlier(np.zeros((1, 3), np.float32), 20)
    assert keep.tolist() == [False]


def test_empty_cloud():
    E = np.zeros((0, 3), np.float32)
    mean, nearest = R.knn_mean_distance(E, 5)
    assert mean.shape == nearest.shape == (0,)
    assert R.radius_count(E, 0.1).shape == (0,) and R.density_filter(E).shape == (0,)
    assert np.array_equal(R.radius_count(E, 0.1, queries=np.ones((2, 3), np.float32)), [0, 0])
    pts, _, first, counts = R.voxel_down_sample(E, 0.1)
    assert pts.shape == (0, 3) and first.shape == counts.shape == (0,)


def test_density_filter_percentiles():
    P = S.shell(4000, 5)
    cnt = R.radius_count(P, 0.03)
    assert np.array_equal(R.density_filter(P, 0.03, 0), np.arange(4000))                      # >= the minimum: everything
    assert np.array_equal(R.density_filter(P, 0.03, 100), np.nonzero(cnt == cnt.max())[0])
    ten = R.density_filter(P, 0.03, 10)
    assert 0.85 * 4000 < len(ten) < 4000 and not np.isin(np.nonzero(cnt == 1)[0], ten).any()


@pytest.mark.parametrize("n", [1, 2, 7, 1000])
def test_percentile_rule_is_numpys(n):
    from collab_splats_amd.pointcloud import _percentile
    v = np.sort(np.random.default_rng(n).integers(0, 50, n)).astype(np.int32)
    for pct in (0, 10, 33.3, 50, 90, 99.9, 100):
        assert _percentile(torch.from_numpy(v), float(pct)) == float(np.percentile(v, pct))
    f = np.sort(np.random.default_rng(n + 1).random(n).astype(np.float32))
    for pct in (0, 25, 90, 100):
        assert _percentile(torch.from_numpy(f), float(pct)) == float(np.percentile(f.astype(np.float64), pct))


# -------------------------------------------------------------------------------------------------- argument checks
def test_public_names():
    import collab_splats_amd as m
    from collab_splats_amd import pointcloud, radegs
    for name in pointcloud.__all__:
        assert getattr(m, name) is getattr(pointcloud, name)
    assert pointcloud.CELL_EDGE is None and pointcloud.LANES_PER_QUERY in (1, 8)
    assert callable(radegs.RadegsModel.clean_gaussians)


def test_no_cpu_fallback_for_any_public_name():
    import collab_splats_amd as m
    P = torch.rand(50, 3)
    calls = [lambda: m.knn_mean_distance(P, 5), lambda: m.knn_mean_distance(P, 1, queries=P[:3]),
             lambda: m.statistical_outlier_mask(P), lambda: m.remove_statistical_outlier(P),
             lambda: m.radius_count(P, 0.1), lambda: m.radius_count(P, 0.1, queries=P[:3]), lambda: m.density_filter(P),
             lambda: m.voxel_down_sample(P, 0.1), lambda: m.voxel_down_sample(P, 0.1, [P]),
             lambda: m.remove_far_points(P, max_distance=1.0), lambda: m.clean_pcd(P),
             lambda: m.calculate_accuracy(P, P), lambda: m.calculate_completeness(P, P),
             lambda: m.knn_mean_distance(P[:0], 5), lambda: m.voxel_down_sample(P[:0], 0.1)]
    for call in calls:
        with pytest.raises(m.MisplatError, match="no CPU fallback"):
            call()


def test_argument_checks():
    import collab_splats_amd as m
    from collab_splats_amd import pointcloud
    P = torch.rand(50, 3)
    nan = P.clone()
    nan[7, 2] = float("nan")
    inf = P.clone()
    inf[0, 0] = float("inf")
    for fn in (lambda x: m.knn_mean_distance(x, 3), lambda x: m.statistical_outlier_mask(x), lambda x: m.radius_count(x, 0.1),
               lambda x: m.voxel_down_sample(x, 0.1), lambda x: m.clean_pcd(x), lambda x: m.density_filter(x),
               lambda x: m.remove_far_points(x, 1.0), lambda x: m.calculate_accuracy(x, P), lambda x: m.calculate_completeness(P, x)):
        for bad in (torch.rand(50, 2), torch.rand(50), torch.rand(2, 50, 3)):
            with pytest.raises(ValueError, match=r"\[N,3\]"):
                fn(bad)
    for fn in (lambda x: m.knn_mean_distance(x, 3), lambda x: m.knn_mean_distance(P, 3, queries=x), lambda x: m.statistical_outlier_mask(x),
               lambda x: m.remove_statistical_outlier(x), lambda x: m.radius_count(x, 0.1), lambda x: m.radius_count(P, 0.1, queries=x),
               lambda x: m.density_filter(x), lambda x: m.voxel_down_sample(x, 0.1), lambda x: m.clean_pcd(x),
               lambda x: m.calculate_accuracy(x, P), lambda x: m.calculate_completeness(x, P)):
        for bad in (nan, inf):
            with pytest.raises(ValueError, match="finite"):
                fn(bad)
    for k in (0, 33, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="k must be"):
            m.knn_mean_distance(P, k)
        with pytest.raises(ValueError, match="nb_neighbors"):
            m.statistical_outlier_mask(P, k)
    with pytest.raises(ValueError, match="empty cloud"):
        m.knn_mean_distance(P[:0], 3, queries=P)
    with pytest.raises(ValueError, match="beyond the index's range"):
        m.knn_mean_distance(P * 1e31, 3)
    for ratio in (float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="std_ratio"):
            m.statistical_outlier_mask(P, 20, ratio)
    for r in (0.0, -1.0, float("inf"), float("nan"), 1e-45, 1e39, "r"):
        with pytest.raises(ValueError, match="radius"):
            m.radius_count(P, r)
        with pytest.raises(ValueError, match="radius"):
            m.density_filter(P, r)
        with pytest.raises(ValueError, match="radius"):
            m.clean_pcd(P, radius=r)
    with pytest.raises(ValueError, match="2\\^18"):
        m.radius_count(P + 1.01 * 0.03 * 2.0 ** 18, 0.03)
    for v in (0.0, -0.1, float("inf"), float("nan"), None):
        with pytest.raises(ValueError, match="voxel_size"):
            m.voxel_down_sample(P, v)
        with pytest.raises(ValueError, match="voxel_size"):
            m.clean_pcd(P, voxel_size=v)
    with pytest.raises(ValueError, match="2\\^20 voxels"):
        m.voxel_down_sample(P, 1e-7)
    with pytest.raises(ValueError, match="2\\^20 voxels"):
        m.voxel_down_sample(P, 0.1, min_bound=(-1e6, 0.0, 0.0))
    with pytest.raises(ValueError, match="min_bound"):
        m.voxel_down_sample(P, 0.1, min_bound=(0.0, 0.0))
    with pytest.raises(ValueError, match="min_bound"):
        m.voxel_down_sample(P, 0.1, min_bound=(0.0, float("nan"), 0.0))
    for att in (torch.rand(49, 3), torch.rand(50), torch.rand(50, 0)):
        with pytest.raises(ValueError, match="attribute"):
            m.voxel_down_sample(P, 0.1, [att])
    for pct in (-1, 101, float("nan"), "p"):
        with pytest.raises(ValueError, match="percentile"):
            m.density_filter(P, 0.03, pct)
        with pytest.raises(ValueError, match="percentile"):
            m.calculate_accuracy(P, P, pct)
    with pytest.raises(ValueError, match="max_distance or n_points"):
        m.remove_far_points(P)
    with pytest.raises(ValueError, match="reference"):
        m.remove_far_points(P, 1.0, reference="camera")
    with pytest.raises(ValueError, match="reference"):
        m.clean_pcd(P, reference="camera")
    for n_points in (-1, 51, 2.5):
        with pytest.raises(ValueError, match="n_points"):
            m.remove_far_points(P, n_points=n_points)
    with pytest.raises(ValueError, match="max_distance"):
        m.remove_far_points(P, max_distance=-1.0)
    for edge in (0.0, -1.0, float("nan"), 1e-45):
        pointcloud.CELL_EDGE = edge
        try:
            with pytest.raises(ValueError, match="CELL_EDGE"):
                m.knn_mean_distance(P, 3)
        finally:
            pointcloud.CELL_EDGE = None
    pointcloud.LANES_PER_QUERY = 4
    try:
        with pytest.raises(ValueError, match="LANES_PER_QUERY"):
            m.knn_mean_distance(P, 3)
    finally:
        pointcloud.LANES_PER_QUERY = 8


def test_library_refuses_bad_sizes(built_lib):
    """The C entry points return MISPLAT_EINVAL before touching the device (null pointers: nothing is launched)."""
    import ctypes as C
    from collab_splats_amd import _lib
    lib = _lib.load()
    z = C.c_void_p(0)
    i64 = C.c_int64
    assert lib.misplat_pointcloud_workspace(i64(-1), 1) == -1 and lib.misplat_pointcloud_workspace(i64(1 << 30), 1) == -1
    assert lib.misplat_pointcloud_workspace(i64(10), 5) == -1 and lib.misplat_pointcloud_workspace(i64(10), -1) == -1
    sizes = [lib.misplat_pointcloud_workspace(i64(1000), kind) for kind in range(5)]
    assert all(s > 0 for s in sizes) and sizes[1] > sizes[2]       # three hash levels against one
    assert lib.misplat_pointcloud_knn(z, i64(10), z, i64(0), 33, C.c_float(0.1), 1, z, i64(0), z, z, z) == -1
    assert lib.misplat_pointcloud_knn(z, i64(10), z, i64(0), 3, C.c_float(0.0), 1, z, i64(0), z, z, z) == -1
    assert lib.misplat_pointcloud_cells(z, i64(0), C.c_float(0.1), z, i64(0), z, z) == -1
    assert lib.misplat_pointcloud_radius_count(z, i64(10), z, i64(0), C.c_float(-1.0), z, i64(0), z, z) == -1
    assert lib.misplat_pointcloud_outlier_mask(z, i64(-5), C.c_double(2.0), z, i64(0), z, z) == -1
    assert lib.misplat_pointcloud_voxel_group(z, i64(10), C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0.0), z, i64(0),
                                              z, z, z, z) == -1
    assert lib.misplat_pointcloud_voxel_mean(z, i64(10), 0, z, z, i64(1), z, z) == -1
