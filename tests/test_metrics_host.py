"""CPU: the restatement of the evaluation metrics (tests/metrics_restatement.py) against what pins it -- the reference's own
``mean_angular_error`` (tests/golden/metrics_goldens.npz), ``oracle/ssim_oracle.py`` and the PSNR formula -- and every condition
the scenes of tests/metrics_scenes.py state, which the GPU tests rely on for their exact comparisons."""
import math
import os

import numpy as np
import pytest
import torch

import metrics_restatement as R
import metrics_scenes as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_goldens.npz")
IMAGE_CASES = [(s, b, c) for s in S.SHAPES for b in S.BATCHES for c in S.CONTENTS]


def test_angle_map_equals_the_reference_golden():
    z = np.load(GOLDEN)
    pred, gt, ref = (torch.from_numpy(z[k]) for k in ("pred", "gt", "angles"))
    assert pred.shape == (2, 3, 5, 7) and ref.shape == (2, 5, 7)
    dots = (pred * gt).sum(1)
    assert int((dots > 1).sum()) >= 1 and int((dots < -1).sum()) >= 1       # the clamp is exercised on both sides
    got = R.mean_angular_error(pred, gt)                                     # float32, as the reference ran it
    assert got.dtype == torch.float32 and torch.equal(got, ref)
    assert float((R.mean_angular_error(pred.double(), gt.double()) - ref.double()).abs().max()) < 1e-3


def test_window_is_the_kernels_window():
    """The restated taps are what ``make_window`` (csrc/ssimwin.h) yields, printed with 9 digits -- enough to name a float32
    -- and they need not be the taps of ``ssim_oracle.gauss_window``: ``torch.sum`` may add the same eleven numbers in another
    order (where this was written its sum lands one float32 step lower and seven of the eleven taps move by one step)."""
    from oracle import ssim_oracle
    half = [0.00102838036, 0.00759875868, 0.0360007733, 0.109360695, 0.213005543, 0.266011745]
    want = torch.tensor(half + half[-2::-1], dtype=torch.float32)
    w, w_torch = R.gauss_window(), ssim_oracle.gauss_window()
    assert w.dtype == torch.float32 and torch.equal(w, want) and torch.equal(w, w.flip(0))
    step = torch.abs(w.double() - w_torch.double()) / (w_torch.double() * 2.0 ** -23)
    assert float(step.max()) <= 1.0                                          # one float32 step or none, tap by tap


@pytest.mark.parametrize("shape", S.SHAPES)
def test_ssim_equals_the_loss_oracle(shape):
    """Given ``ssim_oracle``'s window the restatement IS ``ssim_oracle.ssim``.  With the kernels' window it differs by what a
    float32 step per tap does to a variance: every 2-D weight moves by at most 2^-22 of itself, so each window mean of
    values in 0..1 moves by at most 2^-22, a variance E[xx] - mx^2 by three times that, and the contrast factor -- numerator
    and denominator each two such terms over at least C2 -- by at most 12 * 2^-22 / C2 = 3.5e-3 (the luminance factor's means
    move together and cancel to first order).  That is the worst case, a bright patch without texture; the smooth scenes
    measure about 1e-5, which is why the GPU tests' oracle has to carry the kernels' window."""
    from oracle import ssim_oracle
    pred, gt = S.image_scene(shape, 3, "smooth")
    same = R.ssim(pred.double(), gt.double(), ssim_oracle.gauss_window())
    own = R.ssim(pred.double(), gt.double())
    for b in range(3):
        ref = float(ssim_oracle.ssim(gt[b].double(), pred[b].double()))
        assert abs(float(same[b]) - ref) <= 1e-13, (shape, b)
        print(f"ssim {shape[0]}x{shape[1]} view {b}: the kernels' window against ssim_oracle's {abs(float(own[b]) - ref):.3e}")
        assert abs(float(own[b]) - ref) <= 12 * 2.0 ** -22 / R.C2, (shape, b)


def test_psnr_follows_its_formula():
    pred, gt = S.image_scene((27, 43), 3, "random")
    out = R.image_metrics(pred, gt)
    mse = ((pred.double() - gt.double()) ** 2).reshape(3, -1).mean(-1)
    assert torch.allclose(out["mse"], mse, rtol=1e-14, atol=0)
    assert torch.allclose(out["psnr"], -10.0 * torch.log(mse) / math.log(10.0), rtol=1e-13, atol=0)
    same = R.image_metrics(gt, gt)
    assert bool((same["mse"] == 0).all()) and bool(torch.isposinf(same["psnr"]).all())
    assert float(R.image_metrics(torch.full((1, 11, 11, 3), 0.5), torch.full((1, 11, 11, 3), 0.4))["psnr"]) == pytest.approx(20.0, abs=1e-5)


@pytest.mark.parametrize("shape,B,content", IMAGE_CASES)
def test_image_scenes_meet_their_conditions(shape, B, content):
    pred, gt = S.image_scene(shape, B, content)
    assert pred.shape == (B, shape[0], shape[1], 3) and pred.dtype == torch.float32 and gt.shape == pred.shape
    for t in (pred, gt):
        assert float(t.min()) >= 0.0 and float(t.max()) <= 1.0
        assert float(t.reshape(B, -1).std(-1).min()) > 0.05                  # no constant image (see the scene file)
    for b in range(1, B):
        assert not torch.equal(gt[b], gt[0])                                 # different content per view
    ora, y32 = S.image_oracle(shape, B, content), S.image_yardstick(shape, B, content)
    if content == "identical":
        assert torch.equal(pred, gt) and bool((ora["mse"] == 0).all()) and bool(torch.isposinf(ora["psnr"]).all())
        assert float((ora["ssim"] - 1).abs().max()) < 1e-12
    else:
        assert bool((ora["mse"] > 0).all())
        if content == "near":
            assert 57.0 < float(ora["psnr"].min()) and float(ora["psnr"].max()) < 63.0
        # the fp32 restatement's own error is a usable yardstick: 8 x it stays under the bound's cap of 1e-4
        assert S.view_err(y32["mse"], ora["mse"], True) <= 1e-6 and S.view_err(y32["l1"], ora["l1"], True) <= 1e-6
    # (on SSIM it reaches 1.2e-5 where ONE window position sees a smooth image: E[xx] - mx^2 cancels most of its digits)
    assert S.view_err(y32["ssim"], ora["ssim"], False) <= 2e-5
    assert bool(((ora["ssim"] > -1) & (ora["ssim"] <= 1)).all())


def test_image_shapes_are_the_listed_ones():
    assert S.SHAPES == [(11, 11), (26, 26), (27, 43), (12, 37), (135, 240)] and S.BATCHES == [1, 3]
    assert S.PIXEL_SHAPES == [(5, 7), (17, 33), (64, 64)] and S.PIXEL_B == 3


def test_constant_images_are_no_yardstick():
    """Why the parity scenes hold no constant image: the fp32 restatement itself is ~1e-4 off there."""
    a, b = torch.full((1, 27, 43, 3), 0.25), torch.full((1, 27, 43, 3), 0.75)
    e = S.view_err(R.image_metrics(a, b, torch.float32)["ssim"], R.image_metrics(a, b)["ssim"], False)
    assert e > 1e-5


@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("shape", S.PIXEL_SHAPES)
def test_normal_scenes_keep_away_from_the_thresholds(shape, quantised):
    sc = S.normal_scene(shape, quantised)
    assert sc["pred"].shape == (S.PIXEL_B, shape[0], shape[1], 3)
    assert float(sc["angles_deg"].min()) >= 1.0 and float(sc["angles_deg"].max()) <= 179.0
    excluded = 1.0 - float(sc["valid"].float().mean())
    assert 0.2 < excluded < 0.47                                              # "about a third"
    for kw in (dict(), dict(valid=sc["valid"]), dict(normalize=False)):
        ora = R.normal_metrics(sc["pred"], sc["gt"], **kw)
        assert S.threshold_margin_deg(ora["map"]) >= 0.05
        assert S.threshold_margin_deg(R.normal_metrics(sc["pred"], sc["gt"], dtype=torch.float32, **kw)["map"]) >= 0.04
        for k in ("a11.25", "a22.5", "a30"):                                  # pixels on both sides of every threshold
            assert bool((ora[k] < 1).all()) and bool((ora[k] > 0).any())
    if quantised:
        enc_p, enc_g = (sc["pred"] + 1) / 2, (sc["gt"] + 1) / 2
        assert torch.equal(2 * enc_p - 1, sc["pred"]) and torch.equal(2 * enc_g - 1, sc["gt"])     # exact in float32
        assert float(enc_p.min()) >= 0 and float(enc_p.max()) <= 1


def test_aligned_scene_is_identical_and_opposite():
    p, q = S.aligned_scene()
    assert torch.equal(p[:, :, :8], q[:, :, :8]) and torch.equal(p[:, :, 8:], -q[:, :, 8:])
    assert float(((p * p).sum(-1) - 1).abs().max()) < 1e-6
    ora = R.normal_metrics(p, q, normalize=False)["map"]
    assert bool(torch.isfinite(ora).all()) and float(ora.min()) >= 0 and float(ora.max()) <= math.pi


@pytest.mark.parametrize("shape", S.PIXEL_SHAPES)
def test_depth_scenes_keep_away_from_the_ratios(shape):
    sc = S.depth_scene(shape)
    assert sc["pred"].shape == (S.PIXEL_B, shape[0], shape[1]) and bool((sc["gt"] > 0).all()) and bool((sc["pred"] > 0).all())
    assert S.ratio_margin(sc["pred"], sc["gt"]) >= S.RATIO_GAP
    ora = R.depth_metrics(sc["pred"], sc["gt"])
    for k in ("delta1", "delta2", "delta3"):
        assert bool(((ora[k] > 0) & (ora[k] < 1)).all())
    assert bool((ora["delta1"] < ora["delta2"]).all()) and bool((ora["delta2"] < ora["delta3"]).all())
    assert 0.3 < float((sc["gt"] <= 5.0).float().mean()) < 0.7                # max_depth = 5 removes about half
    ex = S.depth_scene_excluded(shape)
    assert S.ratio_margin(ex["pred"], ex["gt"]) >= S.RATIO_GAP
    n = R.depth_metrics(ex["pred"], ex["gt"])["count"]
    assert n.tolist() == [shape[0] * shape[1] - ex["n_bad"]] * 2 + [0]
    both = R.depth_metrics(ex["pred"], ex["gt"])
    assert bool(torch.isfinite(both["rmse"][:2]).all()) and bool(torch.isnan(both["rmse"][2]))
    y32 = R.depth_metrics(ex["pred"], ex["gt"], dtype=torch.float32)
    assert bool(torch.isfinite(y32["rmse_log"][:2]).all())
