"""CPU: the text-query restatement (tests/textquery_restatement.py) against the folded algorithm the kernels run, against
``meshquery.query_similarity`` (the route the new entry points replace) and against its own closed form; what the scenes
promise; every argument error of the new entry points; the model's plumbing that needs no GPU.  No kernel runs here."""
import pytest
import torch

import textquery_restatement as R
import textquery_scenes as S

FLOOR, CAP = 2.0 ** -23, 1e-4


def bound(yard: float) -> float:
    """The project's rule (tests/test_featureloss_gpu.py): 8 x the fp32 restatement's own error, floored at one rounding."""
    return min(8.0 * max(yard, FLOOR), CAP)


@pytest.mark.parametrize("method", S.METHODS)
@pytest.mark.parametrize("name", list(S.SCENES))
def test_the_fold_is_exact_in_fp64(name, method):
    """A = E w_out, c = E b_out, z = (A hid + c) / T and the closed form of "pairwise", in fp64, against the reference's
    order (decode [C, h, w], einsum, softmax): 1e-12 on every pixel of every scene (measured: <= 1e-14)."""
    sc = S.make(name)
    assert S.abs_err(R.folded(sc, torch.float64, method), S.oracle(name, method)) <= 1e-12
    assert S.abs_err(R.folded(sc, torch.float64, method, out_hw=None), S.oracle(name, method, True)) <= 1e-12


@pytest.mark.parametrize("method", S.METHODS)
def test_the_fold_is_exact_on_rows(method):
    sc = S.make(S.ROWS_SCENE)
    got = R.folded(sc, torch.float64, method, latents=S.row_latents())
    assert got.shape == (max(S.ROW_COUNTS),) and S.abs_err(got, S.row_oracle(method)) <= 1e-12


@pytest.mark.parametrize("method", S.METHODS)
@pytest.mark.parametrize("name", list(S.SCENES))
def test_restatement_at_working_resolution_equals_query_similarity(name, method):
    """``query_similarity`` (fp32 torch, ``decoder=None``) on the rows of the decoded main branch against the fp32 restatement
    at the working resolution, fp32 against fp32 on the same decoded tensor, every scene.  The two are not the same arithmetic
    -- a GEMM over [pixels, C] against an einsum over [C, h, w]; "pairwise" as the closed form against the stacked softmax and
    min -- so the sums over C run in different orders and each logit carries its own roundings, times 1 / T = 20 before the
    exp.  What two fp32 evaluations of one quantity can be asked is that they differ by no more than the project's bound on a
    single one, 8 x the fp32 restatement's own error against the fp64 oracle (floored at 2^-23, capped at 1e-4); the
    ``saturated`` scene, where no rounding can matter, must agree bit for bit.  ``query_similarity`` is held to the oracle by
    the same bound."""
    import collab_splats_amd as m
    sc = S.make(name)
    p = R.decode_main(sc["features"], sc["w_hidden"], sc["b_hidden"], sc["w_out"], sc["b_out"], sc["work"])      # [C, h, w] fp32
    got = m.query_similarity(p.reshape(p.shape[0], -1).t(), sc["embeddings"], sc["n_pos"], method=method)
    ora, y32 = S.oracle(name, method, True), S.yardstick(name, method, True)
    assert got.shape == (sc["work"][0] * sc["work"][1],) and got.dtype == torch.float32
    got = got.reshape(ora.shape)
    b = bound(S.abs_err(y32, ora))
    print(f"textquery {name:10s} {method:9s} query_similarity vs fp32 restatement {S.abs_err(got, y32):.3e}  vs oracle "
          f"{S.abs_err(got, ora):.3e}  bound {b:.3e}")
    assert S.abs_err(got, y32) <= b and S.abs_err(got, ora) <= b
    if name == "saturated":
        assert torch.equal(got, y32)


def test_pairwise_closed_form_equals_the_literal_code():
    """exp(p) / (n_neg exp(p) + sum_j exp(n_j)) against the reference's cat / softmax / min on random logits, wide ones
    (differences of hundreds) among them, and NaN -> 0 in both."""
    g = torch.Generator().manual_seed(7)
    for Q, n_pos, scale in ((2, 1, 1.0), (5, 2, 1.0), (9, 8, 30.0), (64, 1, 300.0)):
        raw = scale * torch.randn(Q, 50, generator=g, dtype=torch.float64)                    # [Q, pixels]
        raw[:, 3] = float("nan")
        lit = R.compute_similarity(raw.reshape(Q, 50, 1), torch.eye(Q, dtype=torch.float64), n_pos, 0.05, "pairwise")
        got = R.pairwise_closed_form(raw.t() / 0.05, n_pos)
        assert float(lit[3, 0, 0]) == 0.0 and float(got[3]) == 0.0
        assert bool(torch.isfinite(got).all()) and float((got - lit.reshape(-1)).abs().max()) <= 1e-15


def test_scenes_hold_what_they_promise():
    for name, ((H, W), L, Hd, C, Q, n_pos, work, out) in S.SCENES.items():
        sc = S.make(name)
        assert sc["features"].shape == (H, W, L) and sc["w_out"].shape == (C, Hd) and sc["embeddings"].shape == (Q, C)
        assert float((sc["embeddings"].double().norm(dim=1) - 1).abs().max()) < 1e-6
        for method in S.METHODS:
            ora = S.oracle(name, method)
            assert ora.shape == (out[0], out[1], 1) and bool(torch.isfinite(ora).all())
            assert float(ora.min()) >= 0.0 and float(ora.max()) <= 1.0
    # saturated: the aligned embedding's logit is more than 200 above the others on every pixel (fp64) ...
    sc = S.make("saturated")
    p = R.decode_main(*(sc[k].double() for k in ("features", "w_hidden", "b_hidden", "w_out", "b_out")), sc["work"])
    z = torch.einsum("chw,nc->nhw", p, sc["embeddings"].double()) / 0.05
    assert float((z[0] - z[1:].max(0).values).min()) > 200.0
    # ... so in fp32 every exp of a difference is 0 or 1: "standard" is exactly 1, "pairwise" exactly 1 / n_neg = 0.5 (the
    # reference's softmax over n_neg copies of p and the negatives gives each copy at most 1 / n_neg), and with the aligned
    # embedding among the negatives both are exactly 0 once rounded to fp32
    assert bool((S.oracle("saturated", "standard").float() == 1.0).all())
    assert bool((S.oracle("saturated", "pairwise").float() == 0.5).all())
    for method in S.METHODS:
        neg = R.similarity_map(S.saturated_negative(), torch.float64, method)
        assert float(neg.max()) < 1e-80 and bool((neg.float() == 0.0).all())
    # the scenes cover a shrinking and an enlarging resize, an identity one, and a final resize each way
    assert S.SCENES["shrink"][6][0] < S.SCENES["shrink"][0][0] and S.SCENES["enlarge"][6][0] > S.SCENES["enlarge"][0][0]
    assert S.SCENES["generic"][6] == S.SCENES["generic"][0] == S.SCENES["generic"][7]


# ------------------------------------------------------------------------------------------------ argument errors
def _decoder(L=13, Hd=64, C=16):
    z = torch.zeros
    return (z(Hd, L), z(Hd), {"main": (z(C, Hd), z(C))})


def _query(L=13, Hd=64, Q=3, n_pos=1):
    import collab_splats_amd as m
    z = torch.zeros
    return m.TextQuery(z(Q, Hd), z(Q), z(Hd, L), z(Hd), n_pos, Q)


def test_exports_and_no_cpu_fallback():
    import collab_splats_amd as m
    from collab_splats_amd import ops, textquery
    assert ops.fold_text_queries is m.fold_text_queries is textquery.fold_text_queries
    assert ops.similarity_map is m.similarity_map and ops.gaussian_similarity is m.gaussian_similarity
    z = torch.zeros
    with pytest.raises(m.MisplatError):
        m.fold_text_queries(_decoder(), "main", z(3, 16), 1)
    with pytest.raises(m.MisplatError):
        m.similarity_map(z(6, 6, 13), _query(), (4, 4))
    with pytest.raises(m.MisplatError):
        m.gaussian_similarity(z(10, 13), _query())
    q = _query()
    with pytest.raises(AttributeError):                                 # an immutable record
        q.n_positive = 2


def test_fold_argument_errors():
    import collab_splats_amd as m
    z = torch.zeros
    for L, Hd in ((33, 64), (13, 257)):
        with pytest.raises(ValueError, match="width must be"):
            m.fold_text_queries(_decoder(L, Hd), "main", z(3, 16), 1)
    for Q in (1, 65):
        with pytest.raises(ValueError, match="text embeddings"):
            m.fold_text_queries(_decoder(), "main", z(Q, 16), 1)
    for n_pos in (0, 3, -1, 1.0, True):
        with pytest.raises(ValueError, match="n_positive"):
            m.fold_text_queries(_decoder(), "main", z(3, 16), n_pos)
    with pytest.raises(KeyError):
        m.fold_text_queries(_decoder(), "aux", z(3, 16), 1)
    with pytest.raises(ValueError, match="channels"):
        m.fold_text_queries(_decoder(), "main", z(3, 17), 1)
    with pytest.raises(ValueError, match=r"\[Q, C\]"):
        m.fold_text_queries(_decoder(), "main", z(16), 1)
    with pytest.raises(ValueError, match="float32"):
        m.fold_text_queries(_decoder(), "main", z(3, 16, dtype=torch.float64), 1)
    with pytest.raises(ValueError, match="decoder must be"):
        m.fold_text_queries((z(64, 13), z(64)), "main", z(3, 16), 1)
    with pytest.raises(ValueError, match="do not fit"):
        m.fold_text_queries((z(64, 13), z(64), {"main": (z(16, 63), z(16))}), "main", z(3, 16), 1)


def test_similarity_argument_errors():
    import collab_splats_amd as m
    z = torch.zeros
    f, rows = z(6, 6, 13), z(10, 13)
    for T in (0.0, -0.05, float("inf"), float("nan"), 1e-60, "0.05"):
        with pytest.raises(ValueError, match="softmax_temp"):
            m.similarity_map(f, _query(), (4, 4), softmax_temp=T)
        with pytest.raises(ValueError, match="softmax_temp"):
            m.gaussian_similarity(rows, _query(), softmax_temp=T)
    with pytest.raises(ValueError, match="unknown method"):
        m.similarity_map(f, _query(), (4, 4), method="softmax")
    with pytest.raises(ValueError, match="unknown method"):
        m.gaussian_similarity(rows, _query(), method="softmax")
    with pytest.raises(ValueError, match="TextQuery"):
        m.similarity_map(f, (z(3, 64), z(3)), (4, 4))
    for bad in (_query(Q=1, n_pos=1), _query(Q=65)):
        with pytest.raises(ValueError, match="text embeddings"):
            m.similarity_map(f, bad, (4, 4))
    for bad in (_query(Q=3, n_pos=3), _query(Q=3, n_pos=0)):
        with pytest.raises(ValueError, match="n_positive"):
            m.gaussian_similarity(rows, bad)
    with pytest.raises(ValueError, match="L 1..32"):
        m.similarity_map(z(6, 6, 33), _query(L=33), (4, 4))
    with pytest.raises(ValueError, match="Hd 1..256"):
        m.gaussian_similarity(rows, _query(Hd=257))
    with pytest.raises(ValueError, match="do not fit each other"):
        m.similarity_map(f, m.TextQuery(z(3, 64), z(4), z(64, 13), z(64), 1, 3), (4, 4))
    for dt in (torch.float16, torch.float64):                           # a hand-made record of another dtype would be misread
        for i in range(4):
            q = list(_query())
            q[i] = q[i].to(dt)
            with pytest.raises(ValueError, match="must be float32"):
                m.similarity_map(f, m.TextQuery(*q), (4, 4))
            with pytest.raises(ValueError, match="must be float32"):
                m.gaussian_similarity(rows, m.TextQuery(*q))
    with pytest.raises(ValueError, match="latent width"):
        m.similarity_map(z(6, 6, 12), _query(), (4, 4))
    with pytest.raises(ValueError, match="latent width"):
        m.gaussian_similarity(z(10, 12), _query())
    with pytest.raises(ValueError, match=r"\[H, W, L\]"):
        m.similarity_map(z(6, 13), _query(), (4, 4))
    with pytest.raises(ValueError, match="float32"):
        m.similarity_map(z(6, 6, 13, dtype=torch.float64), _query(), (4, 4))
    with pytest.raises(ValueError, match="empty"):
        m.similarity_map(z(0, 6, 13), _query(), (4, 4))
    for hw in ((0, 4), (4,), (2 ** 14, 2 ** 14 + 1)):
        with pytest.raises(ValueError, match="work_hw"):
            m.similarity_map(f, _query(), hw)
        with pytest.raises(ValueError, match="out_hw"):
            m.similarity_map(f, _query(), (4, 4), out_hw=hw)
    with pytest.raises(ValueError, match=r"\[N, L\]"):
        m.gaussian_similarity(z(10), _query())
    with pytest.raises(ValueError, match="float32"):
        m.gaussian_similarity(rows.double(), _query())


# ------------------------------------------------------------------------------------------------ the model
def _model(metadata=None, **cfg):
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    sc = random_scene(50, 64, 48, seed=1)
    feats = torch.rand(50, 13, generator=torch.Generator().manual_seed(2))
    return radegs.RadegsFeaturesModel(radegs.RadegsFeaturesModelConfig(**cfg), sc["means"], sc["log_scales"], sc["quats"],
                                      sc["opacity_logits"], sc["sh"][:, 0], sc["sh"][:, 1:], feats,
                                      **({} if metadata is None else {"metadata": metadata}))


def test_model_plumbing_without_a_gpu():
    import collab_splats_amd as m
    from collab_splats_amd import radegs
    assert radegs.RadegsFeaturesModelConfig().similarity_method == "pairwise"
    plain = _model()
    assert plain.text_query is None
    with pytest.raises(ValueError, match="metadata"):
        plain.set_text_queries(torch.zeros(3, 32), 1)
    plain.set_text_queries(None)                                        # clearing needs no decoder
    with pytest.raises(ValueError, match="no text queries"):
        plain.gaussian_similarity()
    model = _model({"feature_type": "clip", "feature_dims": {"clip": (32, 6, 8), "dino": (16, 5, 7)}})
    with pytest.raises(ValueError, match="n_positive"):
        model.set_text_queries(torch.zeros(3, 32), 3)
    with pytest.raises(ValueError, match="channels"):
        model.set_text_queries(torch.zeros(3, 16), 1)                   # the main branch has 32 channels, not dino's 16
    with pytest.raises(m.MisplatError):                                 # sizes are right, tensors on the CPU: no fallback
        model.set_text_queries(torch.zeros(3, 32), 1)
    assert model.text_query is None
    assert "text_query" not in model.state_dict() and not any("text_query" in k for k in model.state_dict())
