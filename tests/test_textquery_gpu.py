"""GPU: the text-query similarity kernels (csrc/textquery.hip, collab_splats_amd/textquery.py) against the fp64 restatement
(tests/textquery_restatement.py: the reference's own order, nothing folded) on the scenes of tests/textquery_scenes.py.

Error measure: max |got - oracle| over every pixel (absolute: the value lies in 0..1).  The bound is the project's rule from
tests/test_featureloss_gpu.py: 8 x the error the fp32 restatement itself makes on the same scene against the same oracle
(computed here from the restatement, never from the code under test), floored at 2^-23 and capped at 1e-4.  The reasoning for
8 carries over: the kernels sum a logit's Hd products in one chain where the restatement sums C products per channel and C
more per query in another order; the softmax at T = 0.05 multiplies either's logit error by 20 before the exp.

``saturated``: the logits are hundreds apart, so every exp of a difference is exactly 0 or 1 in fp32.  "standard" is then exactly
1 or 0.  "pairwise" is a softmax over n_neg copies of the positive logit and the n_neg negatives, so a copy's probability is at
most 1 / n_neg: exactly 0.5 with the scene's two negatives where the aligned embedding is positive, exactly 0 where it is
negative.  Each is held bit for bit, and to the oracle rounded to fp32.
(The figures of a GPU run belong in DESIGN.md section 23; this test prints them.)"""
import pytest
import torch

import textquery_restatement as R
import textquery_scenes as S

pytestmark = pytest.mark.gpu

MULTIPLE = 8.0
FLOOR = 2.0 ** -23
CAP = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def bound(yard: float) -> float:
    return min(MULTIPLE * max(yard, FLOOR), CAP)


def fold(scene, dev):
    import collab_splats_amd as m
    dec = (scene["w_hidden"].to(dev), scene["b_hidden"].to(dev), {"main": (scene["w_out"].to(dev), scene["b_out"].to(dev))})
    return m.fold_text_queries(dec, "main", scene["embeddings"].to(dev), scene["n_pos"])


def run_gpu(scene, dev, method, out_hw="scene", features=None):
    import collab_splats_amd as m
    f = scene["features"].to(dev) if features is None else features
    out = m.similarity_map(f, fold(scene, dev), scene["work"], scene["out"] if out_hw == "scene" else out_hw, method=method)
    torch.cuda.synchronize()
    return out


def in_range(t: torch.Tensor) -> bool:
    return bool(torch.isfinite(t).all()) and float(t.min()) >= 0.0 and float(t.max()) <= 1.0


@pytest.mark.parametrize("method", S.METHODS)
@pytest.mark.parametrize("name", list(S.SCENES))
def test_similarity_map_against_the_fp64_oracle(dev, name, method):
    scene, ora = S.make(name), S.oracle(name, method)
    got = run_gpu(scene, dev, method)
    assert got.shape == ora.shape == (scene["out"][0], scene["out"][1], 1) and got.dtype == torch.float32
    e_gpu, e_32 = S.abs_err(got, ora), S.abs_err(S.yardstick(name, method), ora)
    print(f"textquery {name:10s} {method:9s} gpu {e_gpu:.3e}  fp32 restatement {e_32:.3e}  bound {bound(e_32):.3e}")
    assert in_range(got), (name, method)
    assert e_gpu <= bound(e_32), (name, method, e_gpu, e_32)


def test_fold_is_the_fp64_sum_rounded_once(dev):
    """A and c of every scene equal the fp64 products rounded to fp32, bit for bit (a sum of exact products in fp64 carries
    2^-53 per term: far below half an fp32 rounding step for these sizes; the same on any device)."""
    for name in S.SCENES:
        scene = S.make(name)
        q = fold(scene, dev)
        A, c = R.fold(scene["embeddings"].double(), scene["w_out"].double(), scene["b_out"].double())
        assert q.Q == scene["embeddings"].shape[0] and q.n_positive == scene["n_pos"]
        assert torch.equal(q.A.cpu(), A.float()) and torch.equal(q.c.cpu(), c.float()), name


@pytest.mark.parametrize("method", S.METHODS)
def test_saturated_is_exact(dev, method):
    top = 1.0 if method == "standard" else 0.5                          # 1 / n_neg for "pairwise": see the module docstring
    got = run_gpu(S.make("saturated"), dev, method)
    assert in_range(got) and bool((got == top).all())
    assert torch.equal(got.cpu(), S.oracle("saturated", method).float())
    neg = S.saturated_negative()
    got = run_gpu(neg, dev, method)
    assert in_range(got) and bool((got == 0.0).all())
    assert torch.equal(got.cpu(), R.similarity_map(neg, torch.float64, method).float())


@pytest.mark.parametrize("method", S.METHODS)
def test_a_nan_latent_gives_zero_and_touches_nothing_else(dev, method):
    """A NaN in one pixel's features (``generic``: no resize, so no other pixel reads it) and in one row of the row form:
    that similarity is 0 for either method (the relu keeps the NaN as torch's does, every logit is NaN, and the NaN result is
    written as 0: the reference's nan_to_num for "pairwise", applied to "standard" too); every other
    value keeps its bits."""
    import collab_splats_amd as m
    scene = S.make("generic")
    clean = run_gpu(scene, dev, method)
    f = scene["features"].clone()
    f[3, 4, 2] = float("nan")
    got = run_gpu(scene, dev, method, features=f.to(dev))
    assert float(got[3, 4, 0]) == 0.0 and in_range(got)
    keep = torch.ones(got.shape, dtype=torch.bool, device=dev)
    keep[3, 4] = False
    assert torch.equal(got[keep], clean[keep]) and float(clean[3, 4, 0]) > 0.0
    if method == "pairwise":                                            # the reference's own answer there
        sc = dict(scene, features=f)
        assert float(R.similarity_map(sc, torch.float64, method)[3, 4, 0]) == 0.0
    rows_scene, rows = S.make(S.ROWS_SCENE), S.row_latents()[:64].clone()
    base = m.gaussian_similarity(rows.to(dev), fold(rows_scene, dev), method=method)
    rows[17, 0] = float("nan")
    got = m.gaussian_similarity(rows.to(dev), fold(rows_scene, dev), method=method)
    assert float(got[17]) == 0.0 and in_range(got)
    assert torch.equal(torch.cat([got[:17], got[18:]]), torch.cat([base[:17], base[18:]]))


@pytest.mark.parametrize("name", ["shrink", "ragged"])
def test_two_runs_are_equal_bit_for_bit(dev, name):
    scene = S.make(name)
    for method in S.METHODS:
        assert torch.equal(run_gpu(scene, dev, method), run_gpu(scene, dev, method)), method


def test_strided_features_equal_the_contiguous_run(dev):
    """``features`` as the [..., 3:16] slice of a [24, 40, 17] tensor (what ``outputs["features"]`` is): read in place through
    the pixel stride, the result equal to the contiguous run's bit for bit."""
    from collab_splats_amd import featureloss
    scene = S.make("shrink")
    wide = torch.randn(24, 40, 17, generator=torch.Generator().manual_seed(5))
    wide[..., 3:16] = scene["features"]
    view = wide.to(dev)[..., 3:16]
    assert not view.is_contiguous()
    kept, stride = featureloss._features_view(view, "test")
    assert kept.data_ptr() == view.data_ptr() and stride == 17                      # no copy
    for method in S.METHODS:
        assert torch.equal(run_gpu(scene, dev, method), run_gpu(scene, dev, method, features=view)), method


@pytest.mark.parametrize("method", S.METHODS)
@pytest.mark.parametrize("name", list(S.SCENES))
def test_map_at_working_size_equals_the_route_it_replaces(dev, name, method):
    """``similarity_map`` at ``work_hw`` against ``query_similarity`` on ``feature_decode``'s output (the decoded main branch,
    [h w, C]) for the same scene: within the scene's bound of each other, and the new route within it of the oracle."""
    import collab_splats_amd as m
    scene = S.make(name)
    h, w = scene["work"]
    new = run_gpu(scene, dev, method, out_hw=None)
    dec = (scene["w_hidden"].to(dev), scene["b_hidden"].to(dev), {"main": (scene["w_out"].to(dev), scene["b_out"].to(dev))})
    decoded = m.feature_decode(scene["features"].to(dev), dec, {"main": (scene["w_out"].shape[0], h, w)}, (h, w),
                               channels_last=True)["main"]
    old = m.query_similarity(decoded, scene["embeddings"].to(dev), scene["n_pos"], method=method).reshape(h, w, 1)
    ora = S.oracle(name, method, True)
    b = bound(S.abs_err(S.yardstick(name, method, True), ora))
    print(f"textquery {name:10s} {method:9s} at work: new {S.abs_err(new, ora):.3e}  decode + query_similarity "
          f"{S.abs_err(old, ora):.3e}  between them {S.abs_err(new, old):.3e}  bound {b:.3e}")
    assert new.shape == (h, w, 1) and in_range(new)
    assert S.abs_err(new, ora) <= b and S.abs_err(new, old) <= b, (name, method)


@pytest.mark.parametrize("method", S.METHODS)
@pytest.mark.parametrize("n", S.ROW_COUNTS)
def test_gaussian_similarity_against_the_restatement(dev, n, method):
    import collab_splats_amd as m
    scene = S.make(S.ROWS_SCENE)
    rows = S.row_latents()[:n].to(dev)
    got = m.gaussian_similarity(rows, fold(scene, dev), method=method)
    again = m.gaussian_similarity(rows, fold(scene, dev), method=method)
    torch.cuda.synchronize()
    ora = S.row_oracle(method)[:n]
    e_gpu, e_32 = S.abs_err(got, ora), S.abs_err(S.row_oracle(method, torch.float32)[:n], ora)
    print(f"textquery rows {n:5d} {method:9s} gpu {e_gpu:.3e}  fp32 restatement {e_32:.3e}  bound {bound(e_32):.3e}")
    assert got.shape == (n,) and got.dtype == torch.float32 and in_range(got) and torch.equal(got, again)
    assert e_gpu <= bound(e_32), (n, method, e_gpu, e_32)


def test_model_similarity_output(dev):
    """``RadegsFeaturesModel`` on a synthetic scene: no ``"similarity"`` before ``set_text_queries``; afterwards [H, W, 1] equal
    to ``similarity_map`` applied to the view's own ``outputs["features"]`` -- also for a view already at the working size,
    where the reference sets none; the fold is a snapshot of the decoder; ``set_text_queries(None)`` removes the map again."""
    import collab_splats_amd as m
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 72, 56, 3000
    sc = random_scene(N, W, H, seed=8)
    feats = torch.rand(N, 13, generator=torch.Generator().manual_seed(2))
    dims = {"clip": (48, 4, 6), "dino": (24, 5, 7)}
    work = (32, 48)                                                     # (int(4 * 8.0), int(6 * 8.0))
    torch.manual_seed(11)
    model = radegs.RadegsFeaturesModel(radegs.RadegsFeaturesModelConfig(), sc["means"], sc["log_scales"], sc["quats"],
                                       sc["opacity_logits"], sc["sh"][:, 0], sc["sh"][:, 1:], feats,
                                       metadata={"feature_type": "clip", "feature_dims": dims}).to(dev)
    model.eval()
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 0]])
    cam = radegs.PinholeCamera.make(c2w, 0.9 * W, 0.9 * W, W, H)
    assert "similarity" not in model.get_outputs_for_camera(cam)
    emb = torch.nn.functional.normalize(torch.randn(4, 48, generator=torch.Generator().manual_seed(3)), dim=1).to(dev)
    model.set_text_queries(emb, 1)
    q = model.text_query
    out = model.get_outputs_for_camera(cam)
    sim = out["similarity"]
    assert sim.shape == (H, W, 1) and in_range(sim) and float(sim.max()) > float(sim.min())
    assert torch.equal(sim, m.similarity_map(out["features"], q, work, (H, W), method="pairwise"))
    ref = {}
    for dt in (torch.float64, torch.float32):                           # the restatement on the view's own features
        dec = [t.detach().to(dt).cpu() for t in model.decoder.query_decoder("clip")]
        ref[dt] = R.resize_map(R.compute_similarity(R.decode_main(out["features"].to(dt).cpu(), *dec, work), emb.to(dt).cpu(), 1,
                                                    0.05, "pairwise"), (H, W))
    assert S.abs_err(sim, ref[torch.float64]) <= bound(S.abs_err(ref[torch.float32], ref[torch.float64]))
    small = model.get_outputs_for_camera(radegs.PinholeCamera.make(c2w, 0.9 * work[1], 0.9 * work[1], work[1], work[0]))
    assert small["similarity"].shape == (work[0], work[1], 1) and in_range(small["similarity"])
    gs = model.gaussian_similarity()
    assert gs.shape == (N,) and in_range(gs)
    assert torch.equal(gs, m.gaussian_similarity(model.distill_features.detach(), q, "pairwise"))
    with torch.no_grad():                                               # the fold is a snapshot: training on does not move it
        model.decoder.feature_branch_dict["clip"].bias.add_(emb[0])
    assert model.text_query is q and torch.equal(model.get_outputs_for_camera(cam)["similarity"], sim)
    model.set_text_queries(emb, 1)
    assert not torch.equal(model.text_query.c, q.c)
    assert not torch.equal(model.get_outputs_for_camera(cam)["similarity"], sim)
    model.set_text_queries(None)
    assert "similarity" not in model.get_outputs_for_camera(cam)
