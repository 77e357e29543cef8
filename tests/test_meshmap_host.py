"""CPU: the kNN vertex map's restatement (tests/meshmap_restatement.py) against scipy's cKDTree and the reference's algorithm
(cKDTree query + np.add.at in fp64), the argument checks of features2vertex / normals2vertex, and write_ply with normals.
No GPU."""
import numpy as np
import pytest
import torch

import meshmap_restatement as R


def _cloud(n_v, n_p, seed, spread=0.02):
    rng = np.random.default_rng(seed)
    V = rng.random((n_v, 3)).astype(np.float32) * 0.5
    P = (V[rng.integers(0, n_v, n_p)] + spread * rng.standard_normal((n_p, 3))).astype(np.float32)
    return V, P


def _reference_map(V, P, F, k, sdf_trunc, normalise=False):
    """The reference's algorithm as the issue states it: cKDTree over the vertices, k nearest in fp64, rows with d[:,0] >
    sdf_trunc dropped, sigma = mean distance of the kept rows, exp(-d^2 / (2 sigma^2)) normalised per row, np.add.at."""
    from scipy.spatial import cKDTree
    d, idx = cKDTree(np.asarray(V, np.float64)).query(np.asarray(P, np.float64), k=k)
    d, idx = d.reshape(len(P), k), idx.reshape(len(P), k)
    keep = d[:, 0] <= sdf_trunc
    d, idx, F = d[keep], idx[keep], np.asarray(F, np.float64)[keep]
    sigma = d.mean()
    w = np.exp(-d ** 2 / (2 * sigma ** 2))
    w = w / w.sum(1, keepdims=True)
    num = np.zeros((len(V), F.shape[1]))
    den = np.zeros(len(V))
    for j in range(k):
        np.add.at(num, idx[:, j], w[:, j:j + 1] * F)
        np.add.at(den, idx[:, j], w[:, j])
    out = np.where(den[:, None] > 0, num / np.maximum(den, 1e-300)[:, None], 0.0)
    if normalise:
        out = out / (np.linalg.norm(out, axis=1, keepdims=True) + 1e-8)
    return out


@pytest.mark.parametrize("k", [1, 5, 16])
def test_restated_knn_equals_ckdtree(k):
    spatial = pytest.importorskip("scipy.spatial")
    V, P = _cloud(3000, 4000, seed=k)
    idx, d, _, valid = R.knn(V, P, k, 0.03)
    dt, it = spatial.cKDTree(V.astype(np.float64)).query(P.astype(np.float64), k=k)
    dt, it = dt.reshape(len(P), k), it.reshape(len(P), k)
    # exact fp64 distances of the restatement's choice: a row may differ only where the k-th and (k+1)-th are near-tied
    full = np.sort(np.linalg.norm(P[:, None, :].astype(np.float64) - V[None].astype(np.float64), axis=2), axis=1)
    tie = np.zeros(len(P), bool)
    for j in range(k):
        tie |= np.abs(full[:, j + 1] - full[:, j]) <= 1e-6 * np.maximum(full[:, j + 1], 1e-30)
    same = np.all(np.sort(idx, 1) == np.sort(it, 1), 1)
    assert np.all(same | tie) and same.mean() > 0.99
    assert np.allclose(d.astype(np.float64), dt, rtol=1e-6, atol=1e-7)
    assert np.array_equal(valid, d[:, 0] <= np.float32(0.03)) and 0.2 < valid.mean() < 1.0


@pytest.mark.parametrize("k", [1, 5])
def test_restated_aggregation_equals_reference_algorithm(k):
    pytest.importorskip("scipy.spatial")
    V, P = _cloud(2000, 6000, seed=10 + k)
    rng = np.random.default_rng(k)
    F = rng.standard_normal((len(P), 13)).astype(np.float32)
    Nn = rng.standard_normal((len(P), 3)).astype(np.float32)
    for vals, norm in ((F, False), (Nn, True)):
        ref = _reference_map(V, P, vals, k, 0.03, normalise=norm)
        got = R.map_values(V, P, vals, k, 0.03, normalise=norm)
        assert np.abs(got - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max())     # (fp32 distances against fp64)
        assert np.array_equal(got == 0, ref == 0)


def test_restated_divergences():
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    # sigma = 0 (every valid distance is 0): weights 1/k, where the reference's formula gives 0 / 0
    P = np.array([[0, 0, 0]], np.float32)
    idx = np.array([[0, 1]])
    d = np.zeros((1, 2), np.float32)
    w, sigma = R.weights(d, np.array([True]))
    assert sigma == 0.0 and np.all(w == 0.5)
    # a row whose unshifted exps all underflow stays finite (row-shifted form)
    d = np.array([[0.0, 0.0], [40.0, 41.0]], np.float32)
    w, _ = R.weights(d, np.array([True, True]))
    assert np.all(np.isfinite(w)) and np.allclose(w.sum(1), 1.0)
    out = R.aggregate(3, np.array([[0, 1], [1, 2]]), d, np.array([True, True]), np.array([[1.0], [2.0]]))
    assert np.all(np.isfinite(out))
    # nothing valid: zeros
    out = R.map_values(V, P + 5, np.ones((1, 4), np.float32), k=2, sdf_trunc=0.03)
    assert out.shape == (3, 4) and np.all(out == 0)


def test_argument_checks():
    import collab_splats_amd as m
    z = torch.zeros
    V, P, F = z(10, 3), z(20, 3), z(20, 13)
    with pytest.raises(ValueError, match="fewer than k"):
        m.features2vertex(z(4, 3), P, F, k=5)                           # M < k (the reference crashes in np.add.at)
    for k in (0, 17, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            m.features2vertex(V, P, F, k=k)
    with pytest.raises(ValueError, match="sdf_trunc"):
        m.features2vertex(V, P, F, sdf_trunc=0.0)
    with pytest.raises(ValueError, match="mesh_vertices"):
        m.features2vertex(z(10, 2), P, F)
    with pytest.raises(ValueError, match="points"):
        m.features2vertex(V, z(20, 4), F)
    with pytest.raises(ValueError, match="values"):
        m.features2vertex(V, P, z(19, 13))
    with pytest.raises(ValueError, match="normals"):
        m.normals2vertex(V, P, z(20, 4))
    with pytest.raises(m.MisplatError, match="no CPU fallback"):
        m.features2vertex(V, P, F)
    with pytest.raises(m.MisplatError, match="no CPU fallback"):
        m.normals2vertex(V, P, z(20, 3))


def _ply(path):
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    return head.decode("ascii").split("\n"), body


def test_write_ply_with_normals_round_trips(tmp_path):
    from collab_splats_amd import write_ply
    rng = np.random.default_rng(3)
    v = rng.standard_normal((11, 3)).astype(np.float32)
    n = rng.standard_normal((11, 3)).astype(np.float32)
    f = rng.integers(0, 11, (7, 3)).astype(np.int32)
    c = rng.random((11, 3)).astype(np.float32)
    p = str(tmp_path / "n.ply")
    write_ply(p, torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c), normals=torch.from_numpy(n))
    lines, body = _ply(p)
    props = [x.split()[-1] for x in lines if x.startswith("property float")]
    assert props == ["x", "y", "z", "nx", "ny", "nz"]
    vt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                   ("r", "u1"), ("g", "u1"), ("b", "u1")])
    ft = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    assert len(body) == 11 * vt.itemsize + 7 * ft.itemsize
    vr = np.frombuffer(body[:11 * vt.itemsize], vt)
    fr = np.frombuffer(body[11 * vt.itemsize:], ft)
    assert np.array_equal(np.stack([vr["x"], vr["y"], vr["z"]], 1), v)
    assert np.array_equal(np.stack([vr["nx"], vr["ny"], vr["nz"]], 1), n)
    assert np.array_equal(np.stack([vr["r"], vr["g"], vr["b"]], 1), np.round(c * 255).astype(np.uint8))
    assert np.array_equal(fr["i"], f)
    with pytest.raises(ValueError, match="normals"):
        write_ply(p, v, f, c, normals=n[:5])


def test_write_ply_without_normals_is_unchanged(tmp_path):
    """The bytes of the format written before normals existed, assembled here independently."""
    from collab_splats_amd import write_ply
    rng = np.random.default_rng(4)
    v = rng.standard_normal((5, 3)).astype(np.float32)
    f = np.array([[0, 1, 2], [2, 3, 4]], np.int32)
    c = rng.random((5, 3)).astype(np.float32)
    p = str(tmp_path / "plain.ply")
    write_ply(p, v, f, c)
    expect = (b"ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\n"
              b"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face 2\n"
              b"property list uchar int vertex_indices\nend_header\n")
    cu = np.round(np.clip(c, 0, 1) * 255).astype(np.uint8)
    for i in range(5):
        expect += v[i].astype("<f4").tobytes() + cu[i].tobytes()
    for t in f:
        expect += bytes([3]) + t.astype("<i4").tobytes()
    assert open(p, "rb").read() == expect
    write_ply(p, v, f)                                                   # no colours: black, as before
    assert _ply(p)[1][12:15] == b"\0\0\0"
