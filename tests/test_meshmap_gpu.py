"""GPU: the kNN vertex map (csrc/meshmap.hip) against the restatement (tests/meshmap_restatement.py): neighbour indices and
distance bits equal on every valid row, validity equal; the map's values within 1e-5 max|F| of the fp64 aggregation fed the
same neighbours; two runs bitwise equal with lists of thousands of contributions; the edge cases; the model's
mesh_attributes equal to the two public maps, and outward normals on a fused sphere."""
import numpy as np
import pytest
import torch

import meshmap_restatement as R
import tsdf_scenes as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x, np.float32)).to(DEV)


def _knn_gpu(V, P, k, tr):
    from collab_splats_amd.meshmap import _knn
    idx, d, valid = _knn(_t(V), _t(P), k=k, sdf_trunc=tr)
    return idx.cpu().numpy().astype(np.int64), d.cpu().numpy(), valid.cpu().numpy()


def _check_knn(V, P, k, tr, rows=None):
    idx, d, valid = _knn_gpu(V, P, k, tr)
    Pr = P if rows is None else P[rows]
    ri, rd, _, rv = R.knn(V, Pr, k, tr)
    if rows is not None:
        idx, d, valid = idx[rows], d[rows], valid[rows]
    assert np.array_equal(valid, rv)
    assert np.array_equal(idx[valid], ri[rv])
    assert np.array_equal(d[valid].view(np.uint32), rd[rv].view(np.uint32))
    assert np.all(idx[~valid] == -1)
    return valid


def _sphere_mesh(voxel_size, n_views=60, W=160, H=120):
    from collab_splats_amd import TSDFVolume
    d, vm, K, rgb = S.sphere_views(n_views, W, H)
    vol = TSDFVolume(voxel_size, 3 * voxel_size if voxel_size > 0.005 else 0.02, 3.0, device=DEV)
    for b in range(0, n_views, 32):
        sl = slice(b, b + 32)
        vol.integrate(_t(d[sl]), _t(vm[sl]), _t(K[sl]), _t(rgb[sl]))
    return vol.extract_mesh()[0].cpu().numpy()


def _cloud(kind, n_v, n_p, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        V = rng.random((n_v, 3)) * 0.4
        P = rng.random((n_p, 3)) * 0.44 - 0.02
    else:                                                       # clustered: 20 blobs of vertices, points around them
        c = rng.random((20, 3)) * 0.5
        V = c[rng.integers(0, 20, n_v)] + 0.01 * rng.standard_normal((n_v, 3))
        P = c[rng.integers(0, 20, n_p)] + 0.02 * rng.standard_normal((n_p, 3))
    return V.astype(np.float32), P.astype(np.float32)


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_knn_exact_clouds(kind, k):
    V, P = _cloud(kind, 5000, 20000, seed=k)
    valid = _check_knn(V, P, k, 0.03)
    assert 0.05 < valid.mean() < 1.0


@pytest.mark.parametrize("k", [1, 5, 16])
def test_knn_exact_sphere_mesh(k):
    V = _sphere_mesh(0.01)
    m = S.sphere_gaussians(30000, seed=1)
    P = m.means.detach().numpy()
    assert len(V) > 10000
    valid = _check_knn(V, P, k, 0.03)
    assert valid.mean() > 0.99


@pytest.mark.parametrize("k", [5, 16])
def test_knn_exact_sparse_vertices_several_rings(k):
    """Vertices on a grid of spacing 2.5 sdf_trunc: every valid point's k-th neighbour lies one or more rings out."""
    rng = np.random.default_rng(7)
    tr = 0.01
    g = np.arange(8) * 2.5 * tr
    V = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + 1e-4 * rng.standard_normal((512, 3))
    P = V[rng.integers(0, len(V), 4000)] + 0.004 * rng.standard_normal((4000, 3))
    valid = _check_knn(V.astype(np.float32), P.astype(np.float32), k, tr)
    assert valid.mean() > 0.5
    _, d, _ = _knn_gpu(V, P, k, tr)
    assert np.max(d[valid][:, -1]) > 2.5 * tr                     # (the k-th neighbours are rings away)


def test_knn_exact_far_neighbours_fall_back_to_a_full_scan():
    """One vertex near the points, the others metres away: beyond the ring limit the query scans every vertex."""
    rng = np.random.default_rng(8)
    V = np.concatenate([[[0.0, 0.0, 0.0]], 2.0 + rng.random((300, 3))]).astype(np.float32)
    P = (0.005 * rng.standard_normal((500, 3))).astype(np.float32)
    valid = _check_knn(V, P, 5, 0.03)
    assert valid.all()


def test_knn_exact_duplicated_vertices():
    """Every vertex position three times: equal distances, ordered by vertex index."""
    rng = np.random.default_rng(9)
    base = (rng.random((1500, 3)) * 0.2).astype(np.float32)
    V = np.concatenate([base, base, base])[rng.permutation(4500)]
    P = base[rng.integers(0, 1500, 3000)] + np.float32(0.003) * rng.standard_normal((3000, 3)).astype(np.float32)
    P[:500] = base[:500]                                       # exact hits: three vertices at distance 0
    for k in (1, 5, 16):
        _check_knn(V, P, k, 0.02)


def test_knn_exact_points_outside_the_aabb():
    rng = np.random.default_rng(10)
    V = (rng.random((3000, 3)) * 0.3).astype(np.float32)
    P = (rng.random((6000, 3)) * 0.6 - 0.15).astype(np.float32)
    P[:10] = [[1e6, 0, 0], [-3e5, 2, 1]] * 5
    valid = _check_knn(V, P, 5, 0.03)
    assert 0.05 < valid.mean() < 0.6 and not valid[:10].any()


def _check_map(V, P, F, k, tr, normals=False):
    import collab_splats_amd as m
    fn = m.normals2vertex if normals else m.features2vertex
    out = fn(_t(V), _t(P), _t(F), k=k, sdf_trunc=tr).cpu().numpy()
    idx, d, valid = _knn_gpu(V, P, k, tr)
    ref = R.aggregate(len(V), idx, d, valid, F, normalise=normals)
    tol = 1e-5 * np.abs(F).max()
    assert out.shape == ref.shape and np.abs(out - ref).max() <= tol
    covered = np.zeros(len(V), bool)
    covered[idx[valid].reshape(-1)] = True
    assert np.all(out[~covered] == 0)
    if normals:
        nrm = np.linalg.norm(out[covered].astype(np.float64), axis=1)
        assert np.all(np.abs(nrm - 1) <= 1e-6)
    return out, covered


@pytest.mark.parametrize("k", [1, 5, 16])
def test_map_values(k):
    V, P = _cloud("clustered", 4000, 30000, seed=20 + k)
    rng = np.random.default_rng(k)
    F = rng.standard_normal((len(P), 13)).astype(np.float32) * 3
    out, covered = _check_map(V, P, F, k, 0.03)
    assert covered.mean() > 0.5
    N3 = rng.standard_normal((len(P), 3)).astype(np.float32)
    N3 /= np.linalg.norm(N3, axis=1, keepdims=True)
    N3 = N3 * 0.2 + np.float32([0, 0, 1])                      # mostly +z: the means do not cancel
    _check_map(V, P, N3, k, 0.03, normals=True)


@pytest.mark.parametrize("n_v", [255, 256, 257, 65537])
def test_map_values_at_the_sort_pass_counts(n_v):
    """The contributions are sorted by vertex with keys 0 .. M (M for an invalid row), 8 bits a pass: one pass up to M = 255,
    two from 256 on, three at 65 537.  Points sit on vertices from the first to the last index, so every digit of the key
    decides some list, and a few far points bring the key M."""
    rng = np.random.default_rng(n_v)
    V = (rng.random((n_v, 3)) * 0.4).astype(np.float32)
    at = np.concatenate([[0, 1, n_v - 2, n_v - 1], rng.integers(0, n_v, 296)])
    P = V[at] + np.float32(0.002) * rng.standard_normal((300, 3)).astype(np.float32)
    P[7::25] += 5.0                                            # 12 invalid rows
    F = rng.standard_normal((300, 3)).astype(np.float32)
    out, covered = _check_map(V, P, F, 5, 0.03)
    assert covered[0] and covered[n_v - 1]
    _, _, valid = _knn_gpu(V, P, 5, 0.03)
    assert not valid[7::25].any() and valid.sum() == 300 - 12


def test_long_lists_deterministic():
    """1 M points near a sphere onto 2 k vertices on it: about 2 500 contributions per vertex, split into chunks."""
    import collab_splats_amd as m
    V = S.fibonacci_dirs(2000) * 0.3
    rng = np.random.default_rng(30)
    d = rng.standard_normal((1_000_000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    P = d * (0.3 + 0.005 * rng.standard_normal((len(d), 1)))
    V, P = V.astype(np.float32), P.astype(np.float32)
    F = rng.standard_normal((len(P), 16)).astype(np.float32)
    a = m.features2vertex(_t(V), _t(P), _t(F), k=5, sdf_trunc=0.05)
    b = m.features2vertex(_t(V), _t(P), _t(F), k=5, sdf_trunc=0.05)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    idx, dd, valid = _knn_gpu(V, P, 5, 0.05)
    assert valid.mean() > 0.99
    counts = np.bincount(idx[valid].reshape(-1), minlength=len(V))
    assert counts.mean() > 2000 and counts.max() > 2048
    ref = R.aggregate(len(V), idx, dd, valid, F)
    assert np.abs(a.cpu().numpy() - ref).max() <= 1e-5 * np.abs(F).max()


def test_edge_cases():
    import collab_splats_amd as m
    rng = np.random.default_rng(40)
    V = (rng.random((50, 3)) * 0.1).astype(np.float32)
    F = rng.standard_normal((30, 4)).astype(np.float32)
    # no valid point: zeros [M, D]
    far = (rng.random((30, 3)) + 5).astype(np.float32)
    out = m.features2vertex(_t(V), _t(far), _t(F))
    assert out.shape == (50, 4) and torch.all(out == 0)
    assert torch.all(m.normals2vertex(_t(V), _t(far), _t(F[:, :3])) == 0)
    # N = 0: zeros
    out = m.features2vertex(_t(V), _t(np.zeros((0, 3))), _t(np.zeros((0, 4))))
    assert out.shape == (50, 4) and torch.all(out == 0)
    # sigma = 0: every valid distance 0 (each point on k coincident vertices) -> weights 1/k
    Vd = np.repeat(V[:10], 3, 0)
    P = V[:5]
    Fp = rng.standard_normal((5, 2)).astype(np.float32)
    out = m.features2vertex(_t(Vd), _t(P), _t(Fp), k=3).cpu().numpy()
    assert np.all(np.isfinite(out))
    for i in range(5):
        np.testing.assert_allclose(out[3 * i:3 * i + 3], np.repeat(Fp[i:i + 1], 3, 0), rtol=1e-6)
    assert np.all(out[15:] == 0)
    # a row whose unshifted exps all underflow: sigma tiny against that row's distances
    Vs = np.array([[0, 0, 0], [1e-6, 0, 0], [0, 0.5, 0], [0.0, 0.5, 1e-6], [0, 0.0, 0.9]], np.float32)
    Ps = np.array([[0, 0, 0]] * 50 + [[0, 0.52, 0]], np.float32)
    Fs = np.arange(len(Ps) * 2, dtype=np.float32).reshape(-1, 2)
    out = m.features2vertex(_t(Vs), _t(Ps), _t(Fs), k=2, sdf_trunc=0.03).cpu().numpy()
    assert np.all(np.isfinite(out))
    np.testing.assert_allclose(out[2], Fs[-1], rtol=1e-6)


def _features_model(n, latent=13, seed=0):
    from collab_splats_amd import radegs
    base = S.sphere_gaussians(n, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    feats = torch.randn(n, latent, generator=g)
    cfg = radegs.RadegsFeaturesModelConfig(features_latent_dim=latent)
    p = base.gauss_params
    return radegs.RadegsFeaturesModel(cfg, p["means"].data, p["scales"].data, p["quats"].data, p["opacities"].data,
                                      p["features_dc"].data, p["features_rest"].data, feats)


def test_model_mesh_attributes_equal_the_two_maps():
    import collab_splats_amd as m
    model = _features_model(40000).to(DEV)
    V = torch.as_tensor(_sphere_mesh(0.01)).to(DEV)
    att = model.mesh_attributes(V)
    assert sorted(att) == ["distill_features", "normals"]
    n = m.normals2vertex(V, model.means.detach(), model.normals)
    f = m.features2vertex(V, model.means.detach(), model.distill_features.detach())
    assert torch.equal(att["normals"].view(torch.int32), n.view(torch.int32))
    assert torch.equal(att["distill_features"].view(torch.int32), f.view(torch.int32))
    plain = S.sphere_gaussians(40000).to(DEV).mesh_attributes(V)
    assert list(plain) == ["normals"] and torch.equal(plain["normals"].view(torch.int32), n.view(torch.int32))


def test_model_mesh_normals_point_outward():
    """The 60 k-Gaussian sphere of test_radegs_extract_mesh_equals_per_view_loop: extract, then map the normals."""
    model = S.sphere_gaussians(60000).to(DEV)
    model.eval()
    W, H = 160, 120
    _, vms, _, _ = S.sphere_views(10, 8, 8)
    K = S.intrinsics(W, H, 60.0)
    cams = [S.pinhole_camera(M, K, W, H) for M in vms]
    v, f, c = model.extract_mesh(cams, voxel_size=0.01, sdf_trunc=0.03, depth_trunc=1.0, batch_size=4)
    att = model.mesh_attributes(v)
    n = att["normals"].cpu().numpy().astype(np.float64)
    radial = v.cpu().numpy().astype(np.float64) - np.array([0.1, -0.05, 0.2])
    covered = np.linalg.norm(n, axis=1) > 0
    assert covered.sum() > 5000
    out = np.sum(n[covered] * radial[covered], 1) > 0
    assert out.mean() >= 0.99


def test_full_size():
    """1 M sphere_gaussians onto the 0.004 mesh of the same sphere: 4 096 sampled kNN rows against the brute force, the
    aggregation in full from the GPU's own neighbour lists."""
    import collab_splats_amd as m
    V = _sphere_mesh(0.004, n_views=100, W=320, H=240)
    assert len(V) > 80000
    P = S.sphere_gaussians(1_000_000, seed=2).means.detach().numpy()
    rows = np.random.default_rng(50).choice(len(P), 4096, replace=False)
    _check_knn(V, P, 5, 0.03, rows=rows)
    F = np.random.default_rng(51).standard_normal((len(P), 16)).astype(np.float32)
    out = m.features2vertex(_t(V), _t(P), _t(F), k=5, sdf_trunc=0.03).cpu().numpy()
    idx, d, valid = _knn_gpu(V, P, 5, 0.03)
    ref = R.aggregate(len(V), idx, d, valid, F)
    assert np.abs(out - ref).max() <= 1e-5 * np.abs(F).max()
