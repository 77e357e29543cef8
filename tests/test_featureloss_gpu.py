"""GPU: the fused decoder + cosine feature loss (csrc/featloss.hip, collab_splats_amd/featureloss.py) against the fp64
restatement (tests/featureloss_restatement.py) on the scenes of tests/featureloss_scenes.py.

Error measure, per tensor: max |got - oracle| / max |oracle|, no row or pixel left out (the analytically zero gradients of
a one-channel branch's own parameters: ``featureloss_scenes.grad_err``).  The bound of a tensor is
``MULTIPLE`` times the error the fp32 restatement itself makes on the same scene against the same oracle (computed here from
the restatement, never from the code under test), and never above the project's standing 1e-4 for gradients.  The fp32
restatement's error is floored at 2^-23: a tensor of a handful of entries can come out of the fp32 run correct to the last
bit by chance, but no fp32 result can be asked to carry less than one rounding of its own.

MULTIPLE = 8: the kernels sum a prediction's 64 products in two chains, a pixel's channel sums in up to 8 splits x 4 waves and
the pixel sums in tiles, where the restatement's einsum / sum use yet another order; different orders over n terms differ by
about sqrt(n) roundings relative to the terms' size, which for the largest sums here (768 channels, 660 pixels) is some 25
roundings against the restatement's own few.  (The figures of a GPU run belong in DESIGN.md section 21; this test prints them.)

LAUNCH_SCENES (featureloss_scenes.py) go on to 2 064 channels and 17 820 pixels under the same rule: there the kernels' sums
over pixels are partial sums per 256 pixels and per pixel split that meet in fp64, chains no longer than above, while the
restatement's own error grows with its longer sums.  Their inputs are built so that no hidden pre-activation lies within fp32
rounding of zero (asserted in test_featureloss_host.py); without that the restatement's error, and with it the bound, would
measure one flipped relu and not rounding."""
import pytest
import torch

import featureloss_restatement as R
import featureloss_scenes as S

pytestmark = pytest.mark.gpu

MULTIPLE = 8.0
FLOOR = 2.0 ** -23
CAP = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def run_gpu(scene, dev, features=None, gt=None):
    """Loss, per-branch sums and all gradients of a scene through ``feature_loss``; ``features`` / ``gt`` override the
    scene's (device tensors)."""
    import collab_splats_amd as m
    f = (scene["features"].to(dev) if features is None else features).detach().requires_grad_(True)
    wh, bh = scene["w_hidden"].to(dev).requires_grad_(True), scene["b_hidden"].to(dev).requires_grad_(True)
    br = {n: (w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)) for n, (w, b) in scene["branches"].items()}
    gts = {n: t.to(dev) for n, t in scene["gt"].items()} if gt is None else gt
    loss = m.feature_loss(f, (wh, bh, br), gts, scene["main"], scene["regularization_lambda"], scene["loss_lambda"])
    sums = loss.grad_fn.branch_sums
    loss.backward()
    torch.cuda.synchronize()
    grads = {"features": f.grad, "w_hidden": wh.grad, "b_hidden": bh.grad}
    for n, (w, b) in br.items():
        grads["w_out." + n], grads["b_out." + n] = w.grad, b.grad
    names = list(scene["gt"]) if gt is None else list(gt)
    return {"loss": loss.detach(), "sums": dict(zip(names, sums)), "grads": grads}


def bound(yard: float) -> float:
    return min(MULTIPLE * max(yard, FLOOR), CAP)


@pytest.mark.parametrize("name", list(S.SCENES) + list(S.LAUNCH_SCENES))
def test_loss_and_gradients_against_the_fp64_oracle(dev, name):
    scene, ora, y32 = S.make(name), S.oracle(name), S.yardstick(name)
    got = run_gpu(scene, dev)
    rows = [("loss", S.rel_err(got["loss"], ora["loss"]), S.rel_err(y32["loss"], ora["loss"]))]
    for n in ora["sums"]:
        rows.append(("sum." + n, S.rel_err(got["sums"][n], ora["sums"][n]), S.rel_err(y32["sums"][n], ora["sums"][n])))
    for k, ref in ora["grads"].items():
        assert got["grads"][k].shape == ref.shape and bool(torch.isfinite(got["grads"][k]).all()), k
        rows.append((k, S.grad_err(got["grads"][k], ora["grads"], k), S.grad_err(y32["grads"][k], ora["grads"], k)))
    for k, e_gpu, e_32 in rows:
        print(f"featureloss {name:16s} {k:14s} gpu {e_gpu:.3e}  fp32 restatement {e_32:.3e}  bound {bound(e_32):.3e}")
    for k, e_gpu, e_32 in rows:
        assert e_gpu <= bound(e_32), (name, k, e_gpu, e_32)
        assert e_gpu <= CAP, (name, k, e_gpu)


def test_dead_hidden_layer(dev):
    """``dead``: h = 0 and p = 0 everywhere.  The loss is features_loss_lambda * 1 up to one rounding; the gradients of
    ``features``, ``w_hidden``, ``b_hidden`` and ``w_out`` are exact zeros.  ``b_out`` is the one parameter an all-zero
    prediction still moves under the stated cosine (a clamped norm is a constant: d/dp = -g / (1e-8 |g|), restated and
    checked against torch on the CPU in test_featureloss_host.py): its gradient is finite and equals the oracle's.  With the
    ground truth zero as well, every gradient is an exact zero."""
    scene, ora = S.make("dead"), S.oracle("dead")
    got = run_gpu(scene, dev)
    assert abs(float(got["loss"]) - 1e-3) <= 1e-3 * 2.0 ** -23
    assert float(got["sums"]["main"]) == 16.0
    for k in ("features", "w_hidden", "b_hidden", "w_out.main"):
        assert bool((got["grads"][k] == 0).all()), k
    assert bool(torch.isfinite(got["grads"]["b_out.main"]).all())
    assert S.rel_err(got["grads"]["b_out.main"], ora["grads"]["b_out.main"]) <= bound(
        S.rel_err(S.yardstick("dead")["grads"]["b_out.main"], ora["grads"]["b_out.main"]))
    blank = run_gpu(scene, dev, gt={"main": torch.zeros(16, 4, 4, device=dev)})
    assert abs(float(blank["loss"]) - 1e-3) <= 1e-3 * 2.0 ** -23
    for k, v in blank["grads"].items():
        assert bool(torch.isfinite(v).all()) and bool((v == 0).all()), k


def test_all_zero_ground_truth_pixel_adds_one_and_no_gradient(dev):
    """The all-zero ground-truth pixel of ``same_dims`` (both branches are at the main map's resolution, so the pixel's
    predictions depend on one main-map pixel alone): the per-pixel term is exactly 1 -- the branch sum with the pixel's
    ground truth zero equals, bit for bit, the sum with every OTHER pixel unchanged and the features under that pixel
    replaced, which changes that pixel's prediction only -- and no gradient changes."""
    scene = S.make("same_dims")
    base = run_gpu(scene, dev)
    H, W = scene["features"].shape[:2]
    hm, wm = scene["dims"]["main"][1:]
    y, x = S.ZERO_GT_PIXEL
    # the render pixels only main-map pixel (y, x) reads: its four taps (scale 7.5: taps of neighbours are 7 pixels away)
    ty = R._axis(H, hm, torch.float64)
    tx = R._axis(W, wm, torch.float64)
    rows, cols = {int(ty[0][y]), int(ty[1][y])}, {int(tx[0][x]), int(tx[1][x])}
    for other in range(hm):
        if other != y:
            assert not ({int(ty[0][other]), int(ty[1][other])} & rows)
    f2 = scene["features"].clone()
    g = torch.Generator().manual_seed(77)
    for r in rows:
        for c in cols:
            f2[r, c] = 3.0 * torch.randn(f2.shape[2], generator=g)
    moved = run_gpu(scene, dev, features=f2.to(dev))
    for n in base["sums"]:
        assert float(base["sums"][n]) == float(moved["sums"][n]), n
    assert float(base["loss"]) == float(moved["loss"])
    # the pixel's own term is 1: the sum over the other 15 pixels plus exactly 1, in the oracle's arithmetic
    ora = S.oracle("same_dims")
    pred = R.decode(scene["features"].double(), scene["w_hidden"].double(), scene["b_hidden"].double(),
                    {n: (w.double(), b.double()) for n, (w, b) in scene["branches"].items()}, scene["dims"], scene["main"])
    for n, p in pred.items():
        terms = 1.0 - R.cosine(p, scene["gt"][n].double())
        assert float(terms[y, x]) == 1.0
        assert abs(float(base["sums"][n]) - float(terms.sum())) <= 16 * 2.0 ** -22, n
    # no gradient through the pixel: the features under it get none, and the parameters' gradients do not see its prediction
    for r in rows:
        for c in cols:
            assert bool((base["grads"]["features"][r, c] == 0).all()) and bool((moved["grads"]["features"][r, c] == 0).all())
    for k in base["grads"]:
        if k != "features":
            assert torch.equal(base["grads"][k], moved["grads"][k]), k
    mask = torch.ones(H, W, dtype=torch.bool)
    for r in rows:
        for c in cols:
            mask[r, c] = False
    assert torch.equal(base["grads"]["features"].cpu()[mask], moved["grads"]["features"].cpu()[mask])
    assert float(ora["grads"]["features"][sorted(rows)[0], sorted(cols)[0]].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["down_int", "wide", "pixel_splits", "hidden_256_split"])
def test_two_runs_are_equal_bit_for_bit(dev, name):
    """``pixel_splits`` / ``hidden_256_split``: the partial sums per pixel split and per channel split, and the passes over 64
    hidden units, are in the sums as well."""
    scene = S.make(name)
    a, b = run_gpu(scene, dev), run_gpu(scene, dev)
    assert torch.equal(a["loss"], b["loss"])
    for n in a["sums"]:
        assert torch.equal(a["sums"][n], b["sums"][n]), n
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


def test_strided_features_equal_the_contiguous_run(dev):
    """``features`` as the [..., 3:16] slice of a [45, 80, 17] tensor (what ``outputs["features"]`` is): read in place through
    the pixel stride, every result equal to the contiguous run's bit for bit."""
    _strided_equals_contiguous(dev, "down_int")


def test_strided_features_equal_the_contiguous_run_under_pixel_splits(dev):
    """The same on ``pixel_splits`` ([33, 67, 17]): thousands of main-map pixels, each reading its own render pixel."""
    _strided_equals_contiguous(dev, "pixel_splits")


def _strided_equals_contiguous(dev, name):
    from collab_splats_amd import featureloss
    scene = S.make(name)
    H, W, L = scene["features"].shape
    assert L == 13
    wide = torch.randn(H, W, 17, generator=torch.Generator().manual_seed(5))
    wide[..., 3:16] = scene["features"]
    view = wide.to(dev)[..., 3:16]
    assert not view.is_contiguous()
    kept, stride = featureloss._features_view(view, "test")
    assert kept.data_ptr() == view.data_ptr() and stride == 17                      # no copy
    a, b = run_gpu(scene, dev), run_gpu(scene, dev, features=view)
    assert torch.equal(a["loss"], b["loss"])
    for n in a["sums"]:
        assert torch.equal(a["sums"][n], b["sums"][n]), n
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


@pytest.mark.parametrize("name", ["down_int", "enlarge", "hidden_200", "mixed_axes"])
def test_v_features_is_written_whole(dev, name):
    """Two runs whose gradient buffers start from different garbage (NaN, then a large number, left in the allocator's
    freed blocks): equal results, all finite, and exact zeros on the render rows no tap of the resize touches."""
    scene, ora = S.make(name), S.oracle(name)
    H, W, L = scene["features"].shape
    outs = []
    for fill in (float("nan"), 1e30):
        junk = [torch.full((H, W, L), fill, device=dev) for _ in range(4)]
        del junk
        outs.append(run_gpu(scene, dev)["grads"]["features"])
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])
    untouched = (ora["grads"]["features"] == 0).all(-1).all(-1)                       # rows the oracle leaves at zero
    if name in ("down_int", "mixed_axes"):
        assert int(untouched.sum()) >= H // 2
    assert bool((outs[0].cpu()[untouched] == 0).all())


@pytest.mark.parametrize("name", ["down_int", "branch_up"])
@pytest.mark.parametrize("resize_factor", [1.0, 8.0])
def test_decode_features_against_the_restatement(dev, name, resize_factor):
    """``RadegsFeaturesModel.decode_features``: name -> [C_b, h, w] with the model's sizes (the main branch at
    int(dim * resize_factor), the others at their own dims), values against the fp64 restatement's decode, bounded by the fp32
    restatement's own error as above."""
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    scene = S.make(name)
    sc = random_scene(20, 64, 48, seed=1)
    meta = {"feature_type": scene["main"], "feature_dims": scene["dims"]}
    model = radegs.RadegsFeaturesModel(radegs.RadegsFeaturesModelConfig(), sc["means"], sc["log_scales"], sc["quats"],
                                       sc["opacity_logits"], sc["sh"][:, 0], sc["sh"][:, 1:], torch.zeros(20, 13), metadata=meta)
    state = {"hidden_conv.weight": scene["w_hidden"][:, :, None, None], "hidden_conv.bias": scene["b_hidden"]}
    for n, (w, b) in scene["branches"].items():
        state[f"feature_branch_dict.{n}.weight"], state[f"feature_branch_dict.{n}.bias"] = w[:, :, None, None], b
    model.decoder.load_state_dict(state)
    model = model.to(dev)
    got = model.decode_features(scene["features"].to(dev), resize_factor=resize_factor)
    res = {}
    for dt in (torch.float64, torch.float32):
        res[dt] = R.decode(scene["features"].to(dt), scene["w_hidden"].to(dt), scene["b_hidden"].to(dt),
                           {n: (w.to(dt), b.to(dt)) for n, (w, b) in scene["branches"].items()}, scene["dims"], scene["main"],
                           resize_factor)
    C, Hm, Wm = scene["dims"]["main"]
    assert got["main"].shape == (C, int(Hm * resize_factor), int(Wm * resize_factor))
    assert got["aux0"].shape == scene["dims"]["aux0"]
    for n in got:
        e_gpu, e_32 = S.rel_err(got[n], res[torch.float64][n]), S.rel_err(res[torch.float32][n], res[torch.float64][n])
        print(f"decode {name} x{resize_factor} {n}: gpu {e_gpu:.3e} fp32 restatement {e_32:.3e}")
        assert e_gpu <= bound(e_32), (n, e_gpu, e_32)


@pytest.mark.parametrize("name", ["hidden_200", "channel_cap", "four_branches", "pixel_splits"])
def test_feature_decode_in_both_layouts(dev, name):
    """``feature_decode`` itself (the generic path with a ragged chunk, 8 channel splits, four branches, thousands of pixels)
    against the fp64 restatement's decode, the bound as above; ``channels_last`` equals the transposed default bit for bit."""
    import collab_splats_amd as m
    scene = S.make(name)
    dec = (scene["w_hidden"].to(dev), scene["b_hidden"].to(dev), {n: (w.to(dev), b.to(dev)) for n, (w, b) in scene["branches"].items()})
    main_hw = scene["dims"][scene["main"]][1:]
    got = m.feature_decode(scene["features"].to(dev), dec, scene["dims"], main_hw)
    last = m.feature_decode(scene["features"].to(dev), dec, scene["dims"], main_hw, channels_last=True)
    torch.cuda.synchronize()
    res = {dt: R.decode(scene["features"].to(dt), scene["w_hidden"].to(dt), scene["b_hidden"].to(dt),
                        {n: (w.to(dt), b.to(dt)) for n, (w, b) in scene["branches"].items()}, scene["dims"], scene["main"])
           for dt in (torch.float64, torch.float32)}
    assert list(got) == list(scene["dims"]) and list(last) == list(scene["dims"])
    for n, (C, Hb, Wb) in scene["dims"].items():
        assert got[n].shape == (C, Hb, Wb) and last[n].shape == (Hb * Wb, C)
        assert bool(torch.isfinite(got[n]).all())
        assert torch.equal(last[n], got[n].reshape(C, Hb * Wb).t()), n
        e_gpu, e_32 = S.rel_err(got[n], res[torch.float64][n]), S.rel_err(res[torch.float32][n], res[torch.float64][n])
        print(f"decode {name:16s} {n:5s} gpu {e_gpu:.3e}  fp32 restatement {e_32:.3e}  bound {bound(e_32):.3e}")
        assert e_gpu <= bound(e_32), (name, n, e_gpu, e_32)


def test_per_gaussian_forward_against_the_linear_form(dev):
    import collab_splats_amd as m
    scene = S.make("odd_dims")
    mlp = m.TwoLayerMLP(5, 33, scene["dims"])
    state = {"hidden_conv.weight": scene["w_hidden"][:, :, None, None], "hidden_conv.bias": scene["b_hidden"]}
    for n, (w, b) in scene["branches"].items():
        state[f"feature_branch_dict.{n}.weight"], state[f"feature_branch_dict.{n}.bias"] = w[:, :, None, None], b
    mlp.load_state_dict(state)
    x = torch.randn(1000, 5, generator=torch.Generator().manual_seed(9))
    got = mlp.to(dev).per_gaussian_forward(x.to(dev))
    for dt in (torch.float64, torch.float32):
        ref = R.per_gaussian(x.to(dt), scene["w_hidden"].to(dt), scene["b_hidden"].to(dt),
                             {n: (w.to(dt), b.to(dt)) for n, (w, b) in scene["branches"].items()})
        if dt == torch.float64:
            ref64 = ref
    for n, (w, _) in scene["branches"].items():
        assert got[n].shape == (1000, w.shape[0]) and not got[n].requires_grad
        assert S.rel_err(got[n], ref64[n]) <= bound(S.rel_err(ref[n], ref64[n])), n
    # and as the decoder of query_similarity: the helper's 4-tuple gives the same decoded features
    q = mlp.query_decoder("main")
    emb = torch.nn.functional.normalize(torch.randn(3, 67, generator=torch.Generator().manual_seed(10)), dim=1).to(dev)
    a = m.query_similarity(x.to(dev), emb, 1, decoder=q)
    b = m.query_similarity(got["main"], emb, 1)
    assert float((a - b).abs().max()) < 1e-5


def test_one_features_model_step(dev):
    """One training step of the features model on a synthetic scene: ``get_outputs`` -> ``get_loss_dict`` -> ``backward``.
    ``features_loss`` equals the restatement evaluated (fp64) on the model's own rendered features; ``distill_features`` and
    every decoder parameter receive a finite, non-zero gradient; a ``FusedAdam`` step over every group, ``decoder`` among
    them, changes the decoder's weights."""
    from collab_splats_amd import FusedAdam, fused_adam_step_all, radegs
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 208, 128, 5000
    sc = random_scene(N, W, H, seed=8)
    feats = torch.rand(N, 13, generator=torch.Generator().manual_seed(2))
    dims = {"clip": (48, 8, 13), "dino": (24, 6, 9)}
    cfg = radegs.RadegsFeaturesModelConfig(rasterize_mode="antialiased", regularization_from_iter=0,
                                           output_depth_during_training=True)
    torch.manual_seed(11)
    model = radegs.RadegsFeaturesModel(cfg, sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0],
                                       sc["sh"][:, 1:], feats, metadata={"feature_type": "clip", "feature_dims": dims}).to(dev)
    model.train()
    model.step = 5000
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 0]])
    cam = radegs.PinholeCamera.make(c2w, 0.9 * W, 0.9 * W, W, H)
    g = torch.Generator().manual_seed(12)
    batch = {"image": torch.rand(H, W, 3, generator=g),
             "features_dict": {n: torch.randn(*d, generator=g) for n, d in dims.items()}}       # on the CPU: any device
    batch["features_dict"]["clip"][:, 0, 0] = 0.0
    opts = {name: FusedAdam(params, lr=1e-3, eps=1e-15) for name, params in model.get_param_groups().items()}
    assert "decoder" in opts and "distill_features" in opts
    out = model.get_outputs(cam)
    assert not out["features"].is_contiguous()                                      # the channel slice of the render, as is
    loss = model.get_loss_dict(out, batch)
    assert set(loss) >= {"main_loss", "depth_normal_loss", "features_loss"}
    w_h, b_h, br = model.decoder.flat()
    ref, _ = R.feature_loss(out["features"].detach().double().cpu(), w_h.detach().double().cpu(), b_h.detach().double().cpu(),
                            {n: (w.detach().double().cpu(), b.detach().double().cpu()) for n, (w, b) in br.items()},
                            {n: t.double() for n, t in batch["features_dict"].items()}, "clip",
                            cfg.features_regularization_lambda, cfg.features_loss_lambda)
    assert abs(float(loss["features_loss"]) - float(ref)) <= 1e-5 * abs(float(ref))
    sum(loss.values()).backward()
    gf = model.distill_features.grad
    assert gf is not None and bool(torch.isfinite(gf).all()) and float(gf.abs().sum()) > 0
    before = {k: p.detach().clone() for k, p in model.decoder.named_parameters()}
    for k, p in model.decoder.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), k
        assert float(p.grad.abs().sum()) > 0, k
    fused_adam_step_all(opts)
    torch.cuda.synchronize()
    for k, p in model.decoder.named_parameters():
        assert not torch.equal(p.detach(), before[k]), k
        assert bool(torch.isfinite(p).all()), k
