"""CPU: the mesh queries' restatement (tests/meshquery_restatement.py) against the reference's algorithm written independently
here (cKDTree radius pairs in fp64, scipy connected_components, the > 10 filter), the strictness of the edge rule, the
small-cluster rule, query_similarity on CPU tensors against the fp64 restatement and the closed form, similarity_colors, and
the argument checks of cluster_labels / mesh_clustering.  No GPU."""
import numpy as np
import pytest
import torch

import meshquery_restatement as R
import meshquery_scenes as S


# ------------------------------------------------------------------------------------------------------ clustering
def _reference_clusters(V, sim, thr, r):
    """The reference's mesh_clustering with its dense adjacency held sparse: mask -> radius pairs (fp64, d <= r) ->
    adjacency -> connected_components -> clusters of more than 10, in label order."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    valid = np.where(sim > thr)[0]
    if len(valid) == 0:
        return [], valid, np.zeros((0, 2), np.int64)
    pairs = cKDTree(V[valid].astype(np.float64)).query_pairs(r, output_type="ndarray")
    n = len(valid)
    adj = csr_matrix((np.ones(len(pairs), bool), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    n_comp, lab = connected_components(adj, directed=False)
    out = []
    for c in range(n_comp):
        members = valid[lab == c]
        if len(members) > 10:
            out.append(members)
    return out, valid, pairs


def _edge_set(a, b, n):
    lo, hi = np.minimum(a, b).astype(np.int64), np.maximum(a, b).astype(np.int64)
    return np.unique(lo * n + hi)


@pytest.mark.parametrize("n,thr,seed", [(45000, 0.8, 0), (45000, 0.5, 1), (200000, 0.8, 2)])
def test_restated_clusters_equal_reference_algorithm(n, thr, seed):
    pytest.importorskip("scipy")
    V, sim = S.sphere_blobs(n, seed)
    r = 0.03
    ref, valid, pairs = _reference_clusters(V, sim, thr, r)
    sel, ea, eb = R.edges(V, sim > np.float32(thr), r)
    assert np.array_equal(sel, valid) and len(sel) > n // 50
    # the fp32 strict rule and the fp64 <= rule select the same edges on these inputs (a difference here is a rounding
    # coincidence of the input, not an error of either side)
    assert np.array_equal(_edge_set(ea, eb, len(sel)), _edge_set(pairs[:, 0], pairs[:, 1], len(sel)))
    got = R.mesh_clustering(V, sim, thr, r)
    assert len(got) == len(ref) >= 3
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)
    labels, sizes = R.cluster_labels(V, sim > np.float32(thr), r)
    assert [len(c) for c in ref] == sizes.tolist() and int((labels >= 0).sum()) == int(sizes.sum())


def test_restated_components_on_a_long_chain():
    """Root = smallest member, also for a component whose diameter is thousands of edges."""
    V, ids = S.chains(20000, 0.01, seed=3)
    labels, sizes = R.cluster_labels(V, np.ones(len(V), bool), 0.01)
    assert sizes.tolist() in ([20000, 10000], [10000, 20000])
    first = int(ids[0])
    assert np.array_equal(labels, np.where(ids == first, 0, 1))


def test_edge_rule_is_strict():
    V = S.strict_grid(6)
    r = np.float32(2.0 ** -5)
    every = np.ones(len(V), bool)
    labels, sizes = R.cluster_labels(V, every, float(r))
    assert len(sizes) == 0 and np.all(labels == -1)                # d2 == r2 exactly: no edge, no cluster
    labels, sizes = R.cluster_labels(V, every, float(r), min_cluster_size=0)
    assert np.all(sizes == 1) and np.array_equal(labels, np.arange(216))       # (216 singletons, kept only at size 0)
    labels, sizes = R.cluster_labels(V, every, float(np.nextafter(r, np.float32(1))))
    assert sizes.tolist() == [216] and np.all(labels == 0)


def test_small_cluster_rule():
    V = S.ten_and_eleven(0.03)
    labels, sizes = R.cluster_labels(V, np.ones(21, bool), 0.03, min_cluster_size=10)
    assert sizes.tolist() == [11]
    eleven = np.r_[np.arange(1, 20, 2), 20]
    assert np.array_equal(np.nonzero(labels == 0)[0], eleven) and np.all(np.delete(labels, eleven) == -1)
    labels, sizes = R.cluster_labels(V, np.ones(21, bool), 0.03, min_cluster_size=9)
    assert sizes.tolist() == [10, 11] and labels[0] == 0 and labels[1] == 1   # ordered by smallest member


# ------------------------------------------------------------------------------------------------------ similarity
C_DIM, Q_DIM, TEMP = 512, 4, 0.05
TOL = 2 * C_DIM * 2.0 ** -24 / TEMP + 1e-6                          # see the module docstring of the bound below


def _query_inputs(seed, c_in=C_DIM, m=3000):
    g = torch.Generator().manual_seed(seed)
    emb = torch.nn.functional.normalize(torch.randn(Q_DIM, C_DIM, generator=g), dim=1)
    f = torch.nn.functional.normalize(torch.randn(m, c_in, generator=g), dim=1)
    # rows near each embedding, so the probabilities span 0..1 instead of sitting at 1/Q
    if c_in == C_DIM:
        f = torch.nn.functional.normalize(f + 0.6 * emb[torch.randint(0, Q_DIM, (m,), generator=g)], dim=1)
    return f, emb


def _decoder(seed, c_in, hidden):
    g = torch.Generator().manual_seed(seed)
    w_h = torch.randn(hidden, c_in, generator=g) / c_in ** 0.5
    b_h = 0.1 * torch.randn(hidden, generator=g)
    w_o = torch.randn(C_DIM, hidden, generator=g) / (hidden * C_DIM) ** 0.5 * 2.0
    b_o = 0.01 * torch.randn(C_DIM, generator=g)
    return w_h, b_h, w_o, b_o


@pytest.mark.parametrize("with_decoder", [False, True])
@pytest.mark.parametrize("n_pos", [1, 2])
@pytest.mark.parametrize("method", ["standard", "pairwise"])
def test_query_similarity_equals_fp64_restatement(method, n_pos, with_decoder):
    """An fp32 dot of C terms of unit vectors errs by at most C 2^-24; a logit by at most C 2^-24 / T; a softmax probability
    by at most about twice that: |delta| <= 2 C 2^-24 / T + 1e-6 = 1.2e-3 at C = 512, T = 0.05."""
    import collab_splats_amd as m
    if with_decoder:
        f, emb = _query_inputs(5, c_in=13)
        dec = _decoder(6, 13, 64)
    else:
        f, emb = _query_inputs(4)
        dec = None
    got = m.query_similarity(f, emb, n_pos, method=method, softmax_temp=TEMP, decoder=dec)
    assert got.dtype == torch.float32 and got.shape == (len(f),)
    ref = R.similarity(f.numpy(), emb.numpy(), n_pos, method, TEMP, None if dec is None else [t.numpy() for t in dec])
    err = float(np.abs(got.double().numpy() - ref).max())
    print(f"query_similarity {method} n_pos={n_pos} decoder={with_decoder}: max |delta| = {err:.3e} (bound {TOL:.3e}), "
          f"range {ref.min():.3g} .. {ref.max():.3g}")
    assert err <= TOL
    assert ref.max() - ref.min() > 0.05                             # (the inputs exercise the softmax)


def test_pairwise_similarity_closed_form():
    """The reference's pairwise form is ONE softmax over n_neg copies of p and the negatives: e^{p/T} / (n_neg e^{p/T} +
    sum_j e^{n_j/T})."""
    import collab_splats_amd as m
    f, emb = _query_inputs(7)
    for n_pos in (1, 2, 3):
        raw = f.double().numpy() @ emb.double().numpy().T
        p = raw[:, :n_pos].mean(1) / TEMP
        neg = raw[:, n_pos:] / TEMP
        top = np.maximum(p, neg.max(1))
        closed = np.exp(p - top) / (neg.shape[1] * np.exp(p - top) + np.exp(neg - top[:, None]).sum(1))
        assert np.abs(R.similarity(f.numpy(), emb.numpy(), n_pos, "pairwise", TEMP) - closed).max() <= 1e-12
        got = m.query_similarity(f, emb, n_pos, method="pairwise", softmax_temp=TEMP)
        assert np.abs(got.double().numpy() - closed).max() <= TOL


def test_query_similarity_nan_row_and_extreme_logits():
    import collab_splats_amd as m
    f, emb = _query_inputs(8, m=16)
    f[3] = float("nan")
    got = m.query_similarity(f, emb, 2, method="pairwise")
    assert got[3] == 0 and torch.isfinite(got).all()
    # max-shifted: logits of +-2000 / T neither overflow nor give 0 / 0
    big = torch.cat([2000 * emb[:1], -2000 * emb[:1]])
    got = m.query_similarity(big, emb, 1, method="pairwise")
    assert torch.isfinite(got).all() and abs(float(got[0]) - 1 / 3) < 1e-6 and float(got[1]) == 0


def test_query_similarity_argument_checks():
    import collab_splats_amd as m
    f, emb = _query_inputs(9, m=8)
    with pytest.raises(ValueError, match="method"):
        m.query_similarity(f, emb, 1, method="cosine")
    for n_pos in (0, Q_DIM, -1, 1.5):
        with pytest.raises(ValueError, match="n_positive"):
            m.query_similarity(f, emb, n_pos)
    with pytest.raises(ValueError, match="width"):
        m.query_similarity(f[:, :100], emb, 1)
    with pytest.raises(ValueError, match="decoder"):
        m.query_similarity(f, emb, 1, decoder=_decoder(1, 13, 8))   # decoder for 13-wide features, 512-wide given
    with pytest.raises(ValueError, match="features"):
        m.query_similarity(f[0], emb, 1)
    with pytest.raises(ValueError, match="softmax_temp"):
        m.query_similarity(f, emb, 1, softmax_temp=0.0)


def test_similarity_colors():
    import collab_splats_amd as m
    s = torch.tensor([0.1, 0.4, 0.0, 0.2])
    c = m.similarity_colors(s)
    assert c.dtype == torch.float32 and c.shape == (4, 3)
    assert torch.equal(c[:, 0], s / 0.4) and torch.all(c[:, 1:] == 0)
    assert torch.equal(m.similarity_colors(s[:, None]), c)
    z = m.similarity_colors(torch.zeros(5))
    assert z.shape == (5, 3) and torch.all(z == 0)                  # all-zero stays zero (no 0 / 0)
    assert m.similarity_colors(torch.zeros(0)).shape == (0, 3)


# -------------------------------------------------------------------------------------------------- argument checks
def test_clustering_argument_checks():
    import collab_splats_amd as m
    z = torch.zeros
    V, sim, mask = z(10, 3), z(10), z(10, dtype=torch.bool)
    for fn, per_vertex in ((m.cluster_labels, mask), (m.mesh_clustering, sim)):
        extra = () if fn is m.cluster_labels else (0.8,)
        with pytest.raises(ValueError, match="vertices must be"):
            fn(z(10, 2), per_vertex, *extra, 0.03)
        with pytest.raises(ValueError, match=r"must be \[M\]"):
            fn(V, per_vertex[:9], *extra, 0.03)
        for r in (0.0, -1.0, float("inf"), float("nan"), 1e-45, 1e39):
            with pytest.raises(ValueError, match="radius"):
                fn(V, per_vertex, *extra, r)
        with pytest.raises(ValueError, match="min_cluster_size"):
            fn(V, per_vertex, *extra, 0.03, -1)
        bad = V.clone()
        bad[3, 1] = float("nan")
        with pytest.raises(ValueError, match="finite"):
            fn(bad, per_vertex, *extra, 0.03)
        bad[3, 1] = 1.01 * 0.03 * 2.0 ** 18
        with pytest.raises(ValueError, match="2\\^18"):
            fn(bad, per_vertex, *extra, 0.03)
        with pytest.raises(m.MisplatError, match="no CPU fallback"):
            fn(V, per_vertex, *extra, 0.03)
        with pytest.raises(m.MisplatError, match="no CPU fallback"):
            fn(V, per_vertex[:, None], *extra, 0.03)
    with pytest.raises(ValueError, match="mask must be"):
        m.cluster_labels(V, sim, 0.03)
