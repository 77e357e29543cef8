"""CPU: the feature-loss restatement (tests/featureloss_restatement.py) against torch's own operators and against finite
differences, the resize-the-hidden-layer identity the kernels rely on, ``TwoLayerMLP``'s checkpoint layout, the features
model's parameter groups and every argument error of the new entry points.  No kernel runs here."""
import pytest
import torch
import torch.nn.functional as F

import featureloss_restatement as R
import featureloss_scenes as S


def test_bilinear_restatement_matches_interpolate():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 9, 16, generator=g, dtype=torch.float64)
    for size in ((4, 5), (9, 16), (20, 33), (7, 11), (1, 1), (72, 128)):
        ref = F.interpolate(x[None], size=size, mode="bilinear", align_corners=False)[0]
        assert float((R.bilinear(x, size) - ref).abs().max()) < 1e-13, size


def test_cosine_restatement_matches_torch_at_its_edges():
    """Values and gradients of the restated cosine equal ``F.cosine_similarity(dim=0)`` on ordinary pixels, an all-zero
    ground-truth pixel (cos = 0, no gradient), an all-zero prediction (cos = 0, gradient g / (1e-8 |g|): the clamped norm is
    a constant) and both zero.  A non-zero prediction of norm below 1e-8 has the same VALUE in both; there the restatement
    differentiates the stated formula (the clamped norm is a constant: -g / (1e-8 |g|)), while torch clamps in place outside
    autograd and lets the norm's own gradient through -- a case no decoder output reaches, kept out of the comparison."""
    g = torch.Generator().manual_seed(2)
    p0 = torch.randn(6, 1, 5, generator=g, dtype=torch.float64)
    gt = torch.randn(6, 1, 5, generator=g, dtype=torch.float64)
    gt[:, 0, 1] = 0.0
    p0[:, 0, 2] = 0.0
    p0[:, 0, 3] = 0.0
    gt[:, 0, 3] = 0.0
    res = []
    for fn in (R.cosine, lambda a, b: F.cosine_similarity(a, b, dim=0)):
        p = p0.clone().requires_grad_(True)
        c = fn(p, gt)
        (1.0 - c).sum().backward()
        res.append((c.detach(), p.grad))
    assert torch.allclose(res[0][0], res[1][0], rtol=1e-13, atol=0.0)
    assert torch.allclose(res[0][1], res[1][1], rtol=1e-12, atol=0.0)
    c, grad = res[0]
    assert float(c[0, 1]) == 0.0 and float(grad[:, 0, 1].abs().max()) == 0.0             # all-zero ground truth
    assert float(c[0, 2]) == 0.0 and float(grad[:, 0, 2].abs().max()) > 1e6              # all-zero prediction
    assert float(c[0, 3]) == 0.0 and float(grad[:, 0, 3].abs().max()) == 0.0             # both
    tiny = (p0[:, :, :1] * 1e-10).requires_grad_(True)                                    # 0 < |p| < 1e-8
    c_tiny = R.cosine(tiny, gt[:, :, :1])
    assert torch.allclose(c_tiny, F.cosine_similarity(tiny, gt[:, :, :1], dim=0), rtol=1e-13, atol=0.0)
    (1.0 - c_tiny).sum().backward()
    want = -gt[:, :, :1] / (1e-8 * torch.linalg.vector_norm(gt[:, :, :1], dim=0))
    assert torch.allclose(tiny.grad, want, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("name", ["down_int", "branch_up", "odd_dims", "four_branches", "mixed_axes"])
def test_resizing_the_hidden_layer_equals_resizing_the_predictions(name):
    """fp64: the loss and every gradient agree to 1e-12 (relative to the largest entry) between the model's order (resize
    p_b) and the kernels' (apply branch b's layer to the resized h).  ``four_branches`` and ``mixed_axes`` hold resizes that
    shrink one axis and enlarge the other."""
    a, b = S.oracle(name), R.run(S.make(name), torch.float64, resized_hidden=True)
    assert S.rel_err(b["loss"], a["loss"]) <= 1e-12
    for k in a["grads"]:
        assert S.rel_err(b["grads"][k], a["grads"][k]) <= 1e-12, k


def test_oracle_gradients_against_finite_differences():
    """Central differences of the fp64 loss along random directions, every parameter of ``odd_dims`` at once and one by one."""
    sc = S.make("odd_dims")
    ora = S.oracle("odd_dims")
    keys = list(ora["grads"])

    def tensors():
        t = {"features": sc["features"].double(), "w_hidden": sc["w_hidden"].double(), "b_hidden": sc["b_hidden"].double()}
        for n, (w, b) in sc["branches"].items():
            t["w_out." + n], t["b_out." + n] = w.double(), b.double()
        return t

    def loss_at(t):
        br = {n: (t["w_out." + n], t["b_out." + n]) for n in sc["branches"]}
        gt = {n: v.double() for n, v in sc["gt"].items()}
        return float(R.feature_loss(t["features"], t["w_hidden"], t["b_hidden"], br, gt, sc["main"], sc["regularization_lambda"],
                                    sc["loss_lambda"])[0])

    g = torch.Generator().manual_seed(3)
    base = tensors()
    for moved in [keys] + [[k] for k in keys]:
        dirs = {k: torch.randn(base[k].shape, generator=g, dtype=torch.float64) for k in moved}
        # (the exact-zero pre-activations sit on the relu's kink: keep the zero block of features and the zero biases fixed)
        if "features" in dirs:
            dirs["features"][sc["features"] == 0] = 0.0
        if "b_hidden" in dirs:
            dirs["b_hidden"][sc["b_hidden"] == 0] = 0.0
        want = sum(float((ora["grads"][k] * dirs[k]).sum()) for k in moved)
        eps = 1e-6
        plus = {k: v + eps * dirs[k] if k in dirs else v for k, v in base.items()}
        minus = {k: v - eps * dirs[k] if k in dirs else v for k, v in base.items()}
        got = (loss_at(plus) - loss_at(minus)) / (2 * eps)
        assert abs(got - want) <= 1e-6 * max(abs(want), 1e-9) + 1e-12, (moved, got, want)


def test_scenes_hold_what_they_promise():
    for name in S.SCENES:
        sc = S.make(name)
        for n, t in sc["gt"].items():
            zero = (t == 0).all(0)
            assert bool(zero[S.ZERO_GT_PIXEL]) and int(zero.sum()) == 1, (name, n)
        if name in S.ZERO_PREACT:
            assert S.zero_preactivations(name) > 0, name
    assert len(S.ZERO_PREACT) * 2 >= len(S.SCENES)
    dead = S.oracle("dead")
    assert abs(float(dead["loss"]) - 1e-3) < 1e-15
    for k in ("features", "w_hidden", "b_hidden", "w_out.main"):
        assert float(dead["grads"][k].abs().max()) == 0.0, k
    # the all-zero prediction is the clamped case: d/dp = -g / (1e-8 |g|), which reaches b_out (and only b_out)
    assert float(dead["grads"]["b_out.main"].abs().max()) > 1.0


def test_launch_scenes_hold_their_input_conditions():
    """What makes the fp32 yardstick of a launch scene mean something: no hidden pre-activation on which fp32 and fp64 can
    disagree about the relu.  Exact-grid scenes: the fp32 pre-activations equal the fp64 ones bit for bit, and some are exact
    zeros.  Random scenes: every non-zero fp64 pre-activation is at least 2^-18 of the largest (fp32's 2^-24 per operation
    over the few terms of a dot product stays well inside that), and fp32 agrees on every sign."""
    assert set(S.EXACT_GRID) <= set(S.LAUNCH_SCENES) and not set(S.LAUNCH_SCENES) & set(S.SCENES)
    for name in S.LAUNCH_SCENES:
        sc = S.make(name)
        for n, t in sc["gt"].items():
            assert t.shape[1] >= 2 and t.shape[2] >= 3, (name, n)
            zero = (t == 0).all(0)
            assert bool(zero[S.ZERO_GT_PIXEL]) and int(zero.sum()) == 1, (name, n)
        p64, p32 = S.preactivations(name, torch.float64), S.preactivations(name, torch.float32)
        if name in S.EXACT_GRID:
            f, wh, bh = sc["features"], sc["w_hidden"], sc["b_hidden"]
            assert torch.equal(f * 16, (f * 16).round()) and float(f.abs().max()) <= 4.0, name
            for t in (wh, bh):
                assert torch.equal(t * 256, (t * 256).round()) and float(t.abs().max()) <= 1.0, name
            assert torch.equal(p32.double(), p64), name
            assert int((p64 == 0).sum()) > 0, name
        else:
            nonzero = p64[p64 != 0].abs()
            assert float(nonzero.min()) >= S.PREACT_MARGIN * float(nonzero.max()), (name, float(nonzero.min() / nonzero.max()))
            assert torch.equal(torch.sign(p32).double(), torch.sign(p64)), name


def _plan(name):
    """The launch shape ``make_plan`` (csrc/featloss.hip) derives from a scene's sizes, restated: per branch the 16-channel
    units, the channel splits S, the 64-pixel tiles of the per-pixel kernels, the 256-pixel tiles and the pixel splits PS of
    the weight-gradient kernel, and whether the branch is at the main map's resolution; then the chunks of 64 hidden units.
    A change of ``make_plan`` has to be restated here, and the regimes below looked at again."""
    (_, _), L, Hd, main, others, _ = S.ALL_SCENES[name]
    rows = {}
    for n, (C, Hb, Wb) in zip(S.branch_names(len(others)), [main] + list(others)):
        P, units = Hb * Wb, -(-C // 16)
        tiles256 = -(-P // 256)
        rows[n] = {"C": C, "P": P, "units": units, "S": min(max(units // 8, 1), 8), "tiles64": -(-P // 64), "tiles256": tiles256,
                   "PS": min(max(tiles256 // 4, 1), 16), "identity": (Hb, Wb) == tuple(main[1:])}
    return L, Hd, -(-Hd // 64), rows


def _tiles_of_split(row, split):
    return len(range(split, row["tiles256"], row["PS"]))


def test_plan_restatement_on_the_production_shape():
    """The shape every training step runs (render 1080 x 1920, clip 768 x 64 x 114, dino 384): 7 pixel splits, 6 and 3
    channel splits -- what LAUNCH_SCENES stands in for at a size a test can afford."""
    for C, S_want in ((768, 6), (384, 3), (1024, 8)):
        units = -(-C // 16)
        assert min(max(units // 8, 1), 8) == S_want
    assert min(max(-(-64 * 114 // 256) // 4, 1), 16) == 7


def test_launch_scenes_reach_their_regimes():
    """Each row of LAUNCH_SCENES reaches the launch regime it is there for (a later change of ``make_plan`` or of a scene must
    not un-cover one silently)."""
    old = [_plan(n) for n in S.SCENES]
    assert all(r["PS"] == 1 for _, _, _, rows in old for r in rows.values())                 # what SCENES never reaches
    assert all(Hd <= 64 for _, Hd, _, _ in old) and max(len(rows) for _, _, _, rows in old) == 3

    L, Hd, chunks, rows = _plan("pixel_splits")
    m, a = rows["main"], rows["aux0"]
    assert Hd == 64 and (m["P"], m["tiles256"], m["PS"]) == (2211, 9, 2)
    assert (_tiles_of_split(m, 0), _tiles_of_split(m, 1)) == (5, 4)                          # unequal splits
    assert m["P"] - 8 * 256 == 163 and 2 * 64 < 163 < 3 * 64                                 # last tile: one wave partial, one empty
    assert (a["P"], a["tiles256"], a["PS"]) == (3100, 13, 3) and not a["identity"]           # another PS: early exit of blockIdx.y == 2

    L, Hd, chunks, rows = _plan("split_cap")
    m = rows["main"]
    assert Hd == 64 and len(rows) == 1 and m["C"] < 16 and (m["P"], m["tiles256"], m["PS"]) == (17820, 70, 16)
    assert m["tiles256"] // 4 > 16                                                           # the cap binds
    assert sorted({_tiles_of_split(m, s) for s in range(16)}) == [4, 5]
    H, W = S.ALL_SCENES["split_cap"][0]
    assert (2 * H, W) == S.ALL_SCENES["split_cap"][3][1:]                                    # rows enlarge by 2: taps 1/4, 3/4

    L, Hd, chunks, rows = _plan("hidden_256_split")
    m = rows["main"]
    assert (L, Hd, chunks) == (32, 256, 4) and (m["units"], m["S"], m["PS"]) == (17, 2, 2) and m["units"] % 8 != 0
    assert not rows["aux0"]["identity"] and rows["aux0"]["C"] % 16 != 0

    L, Hd, chunks, rows = _plan("hidden_200_split")
    assert (Hd, chunks, Hd % 64) == (200, 4, 8) and rows["main"]["PS"] == 2
    assert (rows["aux0"]["tiles256"], rows["aux0"]["PS"]) == (14, 3) and not rows["aux0"]["identity"]

    for name in ("pixel_splits", "hidden_256_split", "hidden_200_split"):                    # exact taps (1, 0)
        assert S.ALL_SCENES[name][0] == S.ALL_SCENES[name][3][1:], name

    L, Hd, chunks, rows = _plan("hidden_65")
    assert (Hd, chunks, Hd % 64) == (65, 2, 1)

    L, Hd, chunks, rows = _plan("hidden_200")
    assert (Hd, chunks, Hd % 64) == (200, 4, 8)
    (_, hm, wm), (_, hb, wb) = S.ALL_SCENES["hidden_200"][3], S.ALL_SCENES["hidden_200"][4][0]
    assert hb > hm and wb > wm                                                               # an enlarging branch

    L, Hd, chunks, rows = _plan("hidden_1")
    assert (L, Hd, chunks) == (1, 1, 1)

    L, Hd, chunks, rows = _plan("channel_cap")
    assert Hd == 64 and [r["units"] for r in rows.values()] == [73, 129]
    for r in rows.values():
        assert r["units"] // 8 > 8 and r["S"] == 8                                           # the cap binds
        assert r["units"] % 32 != 0 and r["P"] < 64                                          # uneven units a wave, one partial wave
    assert rows["main"]["C"] % 16 != 0 and rows["aux0"]["C"] % 16 == 0                       # a ragged last unit, and a whole one

    L, Hd, chunks, rows = _plan("four_branches")
    assert len(rows) == 4 and Hd < 64
    assert [r["identity"] for r in rows.values()] == [True, True, False, False]
    assert sorted({r["S"] for r in rows.values()}) == [1, 2]
    (_, hm, wm), others = S.ALL_SCENES["four_branches"][3], S.ALL_SCENES["four_branches"][4]
    assert others[1][1] > hm and others[1][2] < wm and others[2][1] < hm and others[2][2] > wm   # one axis each way, both ways

    (H, W), (_, hm, wm), (_, hb, wb) = S.ALL_SCENES["mixed_axes"][0], S.ALL_SCENES["mixed_axes"][3], S.ALL_SCENES["mixed_axes"][4][0]
    assert H > hm and W < wm and hb > hm and wb < wm


def test_two_layer_mlp_has_the_checkpoint_layout():
    import collab_splats_amd as m
    dims = {"clip": (768, 64, 114), "dino": (384, 64, 114)}
    mlp = m.TwoLayerMLP(13, 64, dims)
    shapes = {k: tuple(v.shape) for k, v in mlp.state_dict().items()}
    assert shapes == {"hidden_conv.weight": (64, 13, 1, 1), "hidden_conv.bias": (64,),
                      "feature_branch_dict.clip.weight": (768, 64, 1, 1), "feature_branch_dict.clip.bias": (768,),
                      "feature_branch_dict.dino.weight": (384, 64, 1, 1), "feature_branch_dict.dino.bias": (384,)}
    g = torch.Generator().manual_seed(4)
    ckpt = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
    mlp.load_state_dict(ckpt)
    w_h, b_h, br = mlp.flat()
    assert w_h.shape == (64, 13) and torch.equal(w_h, ckpt["hidden_conv.weight"][:, :, 0, 0])
    assert torch.equal(br["dino"][0], ckpt["feature_branch_dict.dino.weight"][:, :, 0, 0]) and br["clip"][1].shape == (768,)
    assert w_h.data_ptr() == mlp.hidden_conv.weight.data_ptr()                              # views: gradients reach the module
    q = mlp.query_decoder("clip")
    assert [tuple(t.shape) for t in q] == [(64, 13), (64,), (768, 64), (768,)] and not any(t.requires_grad for t in q)
    with pytest.raises(KeyError):
        mlp.query_decoder("siglip")
    # forward: the module as defined, [B, L, H, W] -> dict, equal to the restatement's decode without any resize
    x = torch.randn(2, 13, 3, 5, generator=g)
    out = mlp(x)
    assert set(out) == set(dims) and out["clip"].shape == (2, 768, 3, 5)
    ref = R.decode(x[1].permute(1, 2, 0), w_h, b_h, br, {"clip": (768, 3, 5), "dino": (384, 3, 5)}, "clip")
    assert S.rel_err(out["dino"][1], ref["dino"]) < 1e-5 and S.rel_err(out["clip"][1], ref["clip"]) < 1e-5


def _model(metadata=None, n=50, **cfg):
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    sc = random_scene(n, 64, 48, seed=1)
    feats = torch.rand(n, 13, generator=torch.Generator().manual_seed(2))
    return radegs.RadegsFeaturesModel(radegs.RadegsFeaturesModelConfig(**cfg), sc["means"], sc["log_scales"], sc["quats"],
                                      sc["opacity_logits"], sc["sh"][:, 0], sc["sh"][:, 1:], feats, **(
                                          {} if metadata is None else {"metadata": metadata}))


META = {"feature_type": "clip", "feature_dims": {"clip": (32, 6, 8), "dino": (16, 5, 7)}}


def test_features_model_config_and_param_groups():
    from collab_splats_amd import radegs
    cfg = radegs.RadegsFeaturesModelConfig()
    assert (cfg.features_latent_dim, cfg.mlp_hidden_dim, cfg.features_loss_lambda, cfg.features_regularization_lambda) == \
        (13, 64, 1e-3, 0.1)
    model = _model(META)
    groups = model.get_param_groups()
    assert set(groups) == {"means", "scales", "quats", "opacities", "features_dc", "features_rest", "distill_features", "decoder"}
    assert len(groups["decoder"]) == 6 and all(p.requires_grad for p in groups["decoder"])
    assert {id(p) for p in groups["decoder"]} == {id(p) for p in model.decoder.parameters()}
    assert model.main_features_name == "clip" and model.main_features_dims == (32, 6, 8)
    assert any(k.startswith("decoder.hidden_conv") for k in model.state_dict())
    # without metadata the model is what it was: no decoder, the same state dict, the Gaussian groups only
    plain = _model()
    assert not hasattr(plain, "decoder") and "decoder" not in plain.get_param_groups()
    assert not any(k.startswith("decoder") for k in plain.state_dict())
    with pytest.raises(ValueError, match="metadata"):
        plain.decode_features(torch.zeros(4, 4, 13))
    with pytest.raises(ValueError, match="feature_type"):
        _model({"feature_type": "siglip", "feature_dims": META["feature_dims"]})
    with pytest.raises(ValueError, match="metadata needs"):
        _model({"feature_dims": META["feature_dims"]})


def _flat(L=13, Hd=64, dims=None):
    dims = dims or {"a": (8, 4, 4)}
    z = torch.zeros
    return (z(Hd, L), z(Hd), {n: (z(d[0], Hd), z(d[0])) for n, d in dims.items()}), {n: z(*d) for n, d in dims.items()}


def test_no_cpu_fallback_and_argument_errors():
    import collab_splats_amd as m
    from collab_splats_amd import ops
    assert ops.feature_loss is m.feature_loss and ops.feature_decode is m.feature_decode
    z = torch.zeros
    dec, gt = _flat()
    # sizes are right, tensors on the CPU: no fallback
    with pytest.raises(m.MisplatError):
        m.feature_loss(z(6, 6, 13), dec, gt, "a")
    with pytest.raises(m.MisplatError):
        m.feature_decode(z(6, 6, 13), dec, {"a": (8, 4, 4)}, (4, 4))
    with pytest.raises(m.MisplatError):
        m.TwoLayerMLP(13, 64, {"a": (8, 4, 4)}).per_gaussian_forward(z(10, 13))
    # the limits: L 1..32, Hd 1..256, 1..4 branches -- ValueError before any launch
    for L, Hd in ((33, 64), (13, 257)):
        d2, g2 = _flat(L, Hd)
        with pytest.raises(ValueError, match="width must be"):
            m.feature_loss(z(6, 6, L), d2, g2, "a")
        with pytest.raises(ValueError, match="width must be"):
            m.TwoLayerMLP(L, Hd, {"a": (8, 4, 4)})
    five = {f"b{i}": (4, 2, 2) for i in range(5)}
    d5, g5 = _flat(dims=five)
    with pytest.raises(ValueError, match="branches"):
        m.feature_loss(z(6, 6, 13), d5, g5, "b0")
    with pytest.raises(ValueError, match="main branch"):
        m.feature_loss(z(6, 6, 13), dec, gt, "nope")
    with pytest.raises(ValueError, match=r"\[C, H, W\]"):
        m.feature_loss(z(6, 6, 13), dec, {"a": z(8, 16)}, "a")
    with pytest.raises(ValueError, match="float32"):
        m.feature_loss(z(6, 6, 13), dec, {"a": z(8, 4, 4, dtype=torch.float64)}, "a")
    with pytest.raises(ValueError, match="float32"):
        m.feature_loss(z(6, 6, 13, dtype=torch.float64), dec, gt, "a")
    with pytest.raises(ValueError, match=r"\[H, W, L\]"):
        m.feature_loss(z(6, 13), dec, gt, "a")
    with pytest.raises(ValueError, match="latent width"):
        m.feature_loss(z(6, 6, 12), dec, gt, "a")
    with pytest.raises(ValueError, match="differ"):
        m.feature_loss(z(6, 6, 13), dec, {"a": z(8, 4, 4), "b": z(8, 4, 4)}, "a")
    with pytest.raises(ValueError, match="do not fit"):
        m.feature_loss(z(6, 6, 13), dec, {"a": z(9, 4, 4)}, "a")
    with pytest.raises(ValueError, match="decoder must be"):
        m.feature_loss(z(6, 6, 13), (dec[0], dec[1]), gt, "a")
    with pytest.raises(ValueError, match="empty"):
        m.feature_loss(z(0, 6, 13), dec, gt, "a")
    with pytest.raises(ValueError, match=r"\(C, H, W\)"):
        m.feature_decode(z(6, 6, 13), dec, {"a": (8, 0, 4)}, (4, 4))
    with pytest.raises(ValueError, match="main map"):
        m.feature_decode(z(6, 6, 13), dec, {"a": (8, 4, 4)}, (0, 4))
    with pytest.raises(ValueError, match=r"\[N, L\]"):
        m.TwoLayerMLP(13, 64, {"a": (8, 4, 4)}).per_gaussian_forward(z(10))


def test_features_model_entry_points_fail_loudly_on_the_cpu():
    import collab_splats_amd as m
    model = _model(META, ssim_lambda=0.0, use_depth_normal_loss=False)
    out = {"rgb": torch.rand(48, 64, 3), "features": torch.rand(48, 64, 13)}
    fd = {n: torch.rand(*d) for n, d in META["feature_dims"].items()}
    with pytest.raises(m.MisplatError):
        model.get_loss_dict(out, {"image": torch.rand(48, 64, 3), "features_dict": fd})
    with pytest.raises(m.MisplatError):
        model.decode_features(torch.rand(48, 64, 13))
    with pytest.raises(ValueError, match="features_dict"):
        model.get_loss_dict(out, {"image": torch.rand(48, 64, 3)})
    with pytest.raises(ValueError, match="feature_dims say"):
        model.get_loss_dict(out, {"image": torch.rand(48, 64, 3), "features_dict": {**fd, "dino": torch.rand(16, 5, 8)}})
    with pytest.raises(ValueError, match="resize_factor"):
        model.decode_features(torch.rand(48, 64, 13), resize_factor=0.01)
    # a model without metadata keeps the base dict
    plain = _model(ssim_lambda=0.0, use_depth_normal_loss=False)
    assert set(plain.get_loss_dict(out, {"image": torch.rand(48, 64, 3)})) == {"main_loss", "scale_reg"}
