"""GPU: the evaluation metrics (csrc/evalmetrics.hip, collab_splats_amd/metrics.py, the model's evaluation methods) against the
fp64 restatement (tests/metrics_restatement.py) on the scenes of tests/metrics_scenes.py.

Bounds are the rule of test_identity_gpu.py and test_featureloss_gpu.py: ``min(8 x max(e32, 2^-23), 1e-4)`` with e32 the error
the fp32 run of the restatement makes on the same scene against the same oracle -- never a figure of the code under test.
Errors are per view, the largest view counts: relative for mse and l1, absolute for ssim (the index is bounded by 1); psnr is
held to (10 / ln 10) x the mse bound in dB (d psnr = -(10 / ln 10) d mse / mse: derived, not measured).  Fractions and counts
are compared exactly: the host test asserts that no oracle angle or depth ratio of these scenes is near a threshold.  The
SSIM oracle carries the kernels' own float32 window (``metrics_restatement.gauss_window``, pinned to ``make_window()`` by the
host test): ``torch.sum``'s window differs in the last bit of seven taps, which alone moves a smooth image's SSIM by 1e-5.
(The figures of a GPU run belong in DESIGN.md section 34; these tests print them.)"""
import math

import pytest
import torch

import metrics_restatement as R
import metrics_scenes as S

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


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.int32),
                                                                      b.reshape(-1).contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------- images
@pytest.mark.parametrize("content", S.CONTENTS)
@pytest.mark.parametrize("B", S.BATCHES)
@pytest.mark.parametrize("shape", S.SHAPES)
def test_image_metrics_against_the_fp64_oracle(dev, shape, B, content):
    import collab_splats_amd as m
    pred, gt = S.image_scene(shape, B, content)
    got = m.image_metrics(pred.to(dev), gt.to(dev))
    ora, y32 = S.image_oracle(shape, B, content), S.image_yardstick(shape, B, content)
    assert sorted(got) == ["l1", "mse", "psnr", "ssim"]
    for k in got:
        assert got[k].shape == (B,) and got[k].dtype == torch.float32 and got[k].is_cuda
    tag = f"image {shape[0]}x{shape[1]} B={B} {content:9s}"
    e_ssim, y_ssim = S.view_err(got["ssim"], ora["ssim"], False), S.view_err(y32["ssim"], ora["ssim"], False)
    print(f"{tag} ssim gpu {e_ssim:.3e}  fp32 restatement {y_ssim:.3e}  bound {bound(y_ssim):.3e}")
    if content == "identical":
        assert bool((got["mse"] == 0).all()) and bool((got["l1"] == 0).all()) and bool(torch.isposinf(got["psnr"]).all())
        assert float((got["ssim"].double().cpu() - 1.0).abs().max()) <= bound(y_ssim)
        return
    rows = []
    for k in ("mse", "l1"):
        rows.append((k, S.view_err(got[k], ora[k], True), S.view_err(y32[k], ora[k], True)))
        print(f"{tag} {k:4s} gpu {rows[-1][1]:.3e}  fp32 restatement {rows[-1][2]:.3e}  bound {bound(rows[-1][2]):.3e}")
    e_psnr, b_psnr = S.view_err(got["psnr"], ora["psnr"], False), (10.0 / math.log(10.0)) * bound(rows[0][2])
    print(f"{tag} psnr gpu {e_psnr:.3e} dB  bound {b_psnr:.3e} dB")
    for k, e_gpu, e_32 in rows:
        assert e_gpu <= bound(e_32), (k, e_gpu, e_32)
    assert e_ssim <= bound(y_ssim), (e_ssim, y_ssim)
    assert e_psnr <= b_psnr, (e_psnr, b_psnr)


@pytest.mark.parametrize("shape", S.SHAPES)
def test_image_metrics_bits(dev, shape):
    """Two runs agree bit for bit; view b of a B = 3 call is the B = 1 call on that view; ssim=False leaves mse, l1 and psnr
    as they are; the wrappers return the same tensors."""
    import collab_splats_amd as m
    for content in ("random", "smooth"):
        pred, gt = (t.to(dev) for t in S.image_scene(shape, 3, content))
        a, b = m.image_metrics(pred, gt), m.image_metrics(pred, gt)
        lean = m.image_metrics(pred, gt, ssim=False)
        assert sorted(lean) == ["l1", "mse", "psnr"]
        for k in a:
            assert _bits_equal(a[k], b[k]), k
            if k != "ssim":
                assert _bits_equal(a[k], lean[k]), k
        for v in range(3):
            one = m.image_metrics(pred[v], gt[v])                      # [H, W, 3]
            for k in a:
                assert _bits_equal(a[k][v:v + 1], one[k]), (k, v)
        assert _bits_equal(m.psnr(pred, gt), a["psnr"]) and _bits_equal(m.ssim(pred, gt), a["ssim"])


# ------------------------------------------------------------------------------------------------------------ normals
def _check_normals(tag, got, ora, y32):
    for k in ("a11.25", "a22.5", "a30", "count"):
        assert torch.equal(torch.nan_to_num(got[k].double().cpu(), nan=-1.0),                         # exact counts over a count
                           torch.nan_to_num(ora[k].to(torch.float32).double(), nan=-1.0)), (tag, k)
    finite = torch.isfinite(ora["mean"])
    assert torch.equal(torch.isnan(got["mean"]).cpu(), ~finite)
    assert torch.equal(torch.isnan(got["map"]).cpu(), torch.isnan(ora["map"]))
    if bool(finite.any()):
        e, y = S.view_err(got["mean"].cpu()[finite], ora["mean"][finite], True), S.view_err(y32["mean"][finite], ora["mean"][finite], True)
        print(f"{tag} mean gpu {e:.3e}  fp32 restatement {y:.3e}  bound {bound(y):.3e}")
        assert e <= bound(y), (tag, e, y)
        keep = torch.isfinite(ora["map"])
        top = float(ora["map"][keep].abs().max())
        e = float((got["map"].double().cpu()[keep] - ora["map"][keep]).abs().max()) / top
        y = float((y32["map"].double()[keep] - ora["map"][keep]).abs().max()) / top
        print(f"{tag} map  gpu {e:.3e}  fp32 restatement {y:.3e}  bound {bound(y):.3e}")
        assert e <= bound(y), (tag, e, y)


@pytest.mark.parametrize("shape", S.PIXEL_SHAPES)
def test_normal_metrics_against_the_fp64_oracle(dev, shape):
    import collab_splats_amd as m
    sc = S.normal_scene(shape)
    pred, gt, valid = sc["pred"].to(dev), sc["gt"].to(dev), sc["valid"].to(dev)
    for name, kw in (("plain", {}), ("masked", {"valid": sc["valid"]}), ("raw", {"normalize": False})):
        gkw = dict(kw, valid=valid) if "valid" in kw else kw
        got = m.normal_metrics(pred, gt, return_map=True, **gkw)
        assert got["map"].shape == pred.shape[:3] and all(got[k].shape == (S.PIXEL_B,) for k in got if k != "map")
        _check_normals(f"normals {shape[0]}x{shape[1]} {name:6s}", got, R.normal_metrics(sc["pred"], sc["gt"], **kw),
                       R.normal_metrics(sc["pred"], sc["gt"], dtype=torch.float32, **kw))
        again = m.normal_metrics(pred, gt, return_map=True, **gkw)
        assert all(_bits_equal(got[k], again[k]) for k in got if k != "map")
        assert "map" not in m.normal_metrics(pred, gt, **gkw)
        one = m.normal_metrics(pred[1], gt[1], **({"valid": valid[1]} if "valid" in kw else kw))
        assert all(_bits_equal(got[k][1:2], one[k]) for k in one)      # a view's sums do not depend on B or b


@pytest.mark.parametrize("shape", S.PIXEL_SHAPES)
def test_normal_metrics_exclusions(dev, shape):
    """Zero-length vectors are excluded under ``normalize``; a view with nothing left gives NaN and count 0."""
    import collab_splats_amd as m
    sc = S.normal_scene(shape)
    pred, gt, valid = sc["pred"].clone(), sc["gt"].clone(), sc["valid"].clone()
    pred[0, 0, :3] = 0.0
    gt[0, 1, 1:4] = 0.0
    gt[1] = 0.0                                                         # view 1: no vector at all
    valid[2] = False                                                    # view 2: masked out
    got = m.normal_metrics(pred.to(dev), gt.to(dev), valid.to(dev), return_map=True)
    ora = R.normal_metrics(pred, gt, valid)
    assert ora["count"][1:].tolist() == [0.0, 0.0] and got["count"].cpu()[1:].tolist() == [0.0, 0.0]
    for k in ("mean", "a11.25", "a22.5", "a30"):
        assert bool(torch.isnan(got[k][1:]).all()) and bool(torch.isfinite(got[k][0]))
    assert bool(torch.isnan(got["map"][0, 0, :3]).all()) and bool(torch.isnan(got["map"][0, 1, 1:4]).all())
    _check_normals(f"normals {shape[0]}x{shape[1]} excluded", got, ora, R.normal_metrics(pred, gt, valid, dtype=torch.float32))


@pytest.mark.parametrize("shape", S.PIXEL_SHAPES)
def test_encoded_normals_equal_decoding_by_hand(dev, shape):
    """The quantised scene's 0..1 encoding decodes exactly in float32 (asserted by the host test): both calls see the same
    vectors and must agree bit for bit, and with the oracle as the plain scene does."""
    import collab_splats_amd as m
    sc = S.normal_scene(shape, True)
    pred, gt, valid = sc["pred"].to(dev), sc["gt"].to(dev), sc["valid"].to(dev)
    enc = m.normal_metrics((pred + 1) / 2, (gt + 1) / 2, valid, encoded=True, return_map=True)
    dec = m.normal_metrics(pred, gt, valid, return_map=True)
    for k in enc:
        assert torch.equal(torch.nan_to_num(enc[k], nan=-1.0), torch.nan_to_num(dec[k], nan=-1.0)), k
    _check_normals(f"normals {shape[0]}x{shape[1]} encoded", enc, R.normal_metrics((sc["pred"] + 1) / 2, (sc["gt"] + 1) / 2, sc["valid"], encoded=True),
                   R.normal_metrics((sc["pred"] + 1) / 2, (sc["gt"] + 1) / 2, sc["valid"], encoded=True, dtype=torch.float32))


def test_aligned_normals_stay_in_range(dev):
    """Identical and opposite unit vectors: the clamp keeps acos finite.  For identical unit vectors the dot product is within
    4 roundings of 1 (three products, two sums, less one shared), and acos(1 - e) ~ sqrt(2 e): theta <= sqrt(2 * 4 * 2^-23)."""
    import collab_splats_amd as m
    p, q = S.aligned_scene()
    for normalize in (False, True):
        amap = m.normal_metrics(p.to(dev), q.to(dev), normalize=normalize, return_map=True)["map"].cpu()
        pi32 = float(torch.tensor(math.pi, dtype=torch.float32))       # (the map is float32: pi rounds up by 8.7e-8)
        assert bool(torch.isfinite(amap).all()) and float(amap.min()) >= 0.0 and float(amap.max()) <= pi32
        limit = math.sqrt(2 * 4 * 2.0 ** -23)
        assert float(amap[:, :, :8].max()) <= limit and float((math.pi - amap[:, :, 8:]).max()) <= limit + 2.0 ** -22


def test_mean_angular_error_equals_the_map(dev):
    """The reference's signature and layout ([B, C, H, W] -> [B, H, W]) on the golden's input, against the golden itself."""
    import os
    import numpy as np
    import collab_splats_amd as m
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_goldens.npz"))
    pred, gt, ref = (torch.from_numpy(z[k]) for k in ("pred", "gt", "angles"))
    got = m.mean_angular_error(pred.to(dev), gt.to(dev))
    assert got.shape == (2, 5, 7) and got.dtype == torch.float32
    ora = R.mean_angular_error(pred.double(), gt.double())
    e, y = S.view_err(got, ora, False) / math.pi, S.view_err(ref, ora, False) / math.pi
    print(f"mean_angular_error gpu {e:.3e}  reference (fp32) {y:.3e}  bound {bound(y):.3e}")
    assert e <= bound(y)
    assert bool((got.cpu()[(pred.double() * gt.double()).sum(1) > 1] == 0).all())        # clamped: exactly 0


# -------------------------------------------------------------------------------------------------------------- depth
DEPTH_VALUES = ("abs_rel", "sq_rel", "rmse", "rmse_log")


def _check_depth(tag, got, ora, y32):
    assert sorted(got) == sorted(DEPTH_VALUES + ("delta1", "delta2", "delta3", "count"))
    for k in ("delta1", "delta2", "delta3", "count"):
        assert torch.equal(torch.nan_to_num(got[k].double().cpu(), nan=-1.0),
                           torch.nan_to_num(ora[k].to(torch.float32).double(), nan=-1.0)), (tag, k)
    finite = ora["count"] > 0
    for k in DEPTH_VALUES:
        assert torch.equal(torch.isnan(got[k]).cpu(), ~finite), (tag, k)
        if bool(finite.any()):
            e, y = S.view_err(got[k].cpu()[finite], ora[k][finite], True), S.view_err(y32[k][finite], ora[k][finite], True)
            print(f"{tag} {k:8s} gpu {e:.3e}  fp32 restatement {y:.3e}  bound {bound(y):.3e}")
            assert e <= bound(y), (tag, k, e, y)


@pytest.mark.parametrize("shape", S.PIXEL_SHAPES)
def test_depth_metrics_against_the_fp64_oracle(dev, shape):
    import collab_splats_amd as m
    sc = S.depth_scene(shape)
    pred, gt, valid = sc["pred"].to(dev), sc["gt"].to(dev), sc["valid"].to(dev)
    for name, kw in (("plain", {}), ("masked", {"valid": sc["valid"]}), ("max 5", {"max_depth": 5.0}), ("max 0", {"max_depth": 0.0})):
        gkw = dict(kw, valid=valid) if "valid" in kw else kw
        got = m.depth_metrics(pred, gt, **gkw)
        _check_depth(f"depth {shape[0]}x{shape[1]} {name:6s}", got, R.depth_metrics(sc["pred"], sc["gt"], **kw),
                     R.depth_metrics(sc["pred"], sc["gt"], dtype=torch.float32, **kw))
        again = m.depth_metrics(pred[..., None], gt[..., None], **gkw)                  # [B, H, W, 1], and a second run
        assert all(_bits_equal(got[k], again[k]) for k in got)
        one = m.depth_metrics(pred[2:3], gt[2:3], **({"valid": valid[2:3]} if "valid" in kw else kw))
        assert all(_bits_equal(got[k][2:3], one[k]) for k in got)
    assert float(m.depth_metrics(pred, gt, max_depth=5.0)["count"].sum()) < float(m.depth_metrics(pred, gt)["count"].sum())


@pytest.mark.parametrize("shape", S.PIXEL_SHAPES)
def test_depth_metrics_exclusions(dev, shape):
    """Zeros, negatives, infinities and NaN in either map do not count; a view with nothing left gives NaN and count 0."""
    import collab_splats_amd as m
    ex = S.depth_scene_excluded(shape)
    got = m.depth_metrics(ex["pred"].to(dev), ex["gt"].to(dev))
    assert got["count"].cpu().tolist() == [shape[0] * shape[1] - ex["n_bad"]] * 2 + [0]
    _check_depth(f"depth {shape[0]}x{shape[1]} excluded", got, R.depth_metrics(ex["pred"], ex["gt"]),
                 R.depth_metrics(ex["pred"], ex["gt"], dtype=torch.float32))
    masked = m.depth_metrics(ex["pred"].to(dev), ex["gt"].to(dev), ex["valid"].to(dev), max_depth=5.0)
    _check_depth(f"depth {shape[0]}x{shape[1]} all rules", masked, R.depth_metrics(ex["pred"], ex["gt"], ex["valid"], 5.0),
                 R.depth_metrics(ex["pred"], ex["gt"], ex["valid"], 5.0, dtype=torch.float32))


# -------------------------------------------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def model_and_cams(dev):
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene, view_matrix
    W, H, N = 64, 48, 8000
    sc = random_scene(N, W, H, seed=9)
    model = radegs.RadegsModel(radegs.RadegsModelConfig(rasterize_mode="antialiased"), sc["means"], sc["log_scales"], sc["quats"],
                               sc["opacity_logits"], sc["sh"][:, 0], sc["sh"][:, 1:]).to(dev).eval()
    model.step = 10_000
    flip = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0]))
    cams = [radegs.PinholeCamera.make((torch.linalg.inv(view_matrix(i)[0]) @ flip)[:3, :4], 0.9 * W, 0.9 * W, W, H) for i in range(5)]
    g = torch.Generator().manual_seed(3)
    images = [torch.rand(H, W, 3, generator=g) for _ in range(5)]
    return model, cams, images, N


def test_model_metrics_dict_and_eval_images(dev, model_and_cams):
    import collab_splats_amd as m
    model, cams, images, N = model_and_cams
    out = model.get_outputs_for_camera(cams[0])
    H, W = out["rgb"].shape[:2]
    md = model.get_metrics_dict(out, {"image": images[0]})
    direct = m.image_metrics(out["rgb"].contiguous(), images[0].to(dev), ssim=False)["psnr"][0]
    assert sorted(md) == ["gaussian_count", "psnr"] and md["gaussian_count"] == N == model.num_points
    assert md["psnr"].is_cuda and md["psnr"].shape == () and _bits_equal(md["psnr"], direct)
    u8 = (images[0] * 255).round().to(torch.uint8)                       # a uint8 batch image: 0..1 floats first (get_gt_img)
    assert _bits_equal(model.get_metrics_dict(out, {"image": u8})["psnr"], m.psnr(out["rgb"].contiguous(), model.get_gt_img(u8.to(dev)))[0])
    assert float((model.get_gt_img(u8.to(dev)).cpu() - images[0]).abs().max()) <= 0.5 / 255 + 1e-6
    scores, pics = model.get_image_metrics_and_images(out, {"image": images[0]})
    assert sorted(scores) == ["psnr", "ssim"] and all(isinstance(v, float) for v in scores.values())
    both = m.image_metrics(out["rgb"].contiguous(), images[0].to(dev))
    assert scores["psnr"] == float(both["psnr"][0]) and scores["ssim"] == float(both["ssim"][0])
    assert sorted(pics) == ["img"] and pics["img"].shape == (H, 2 * W, 3)
    assert torch.equal(pics["img"][:, :W], images[0].to(dev)) and torch.equal(pics["img"][:, W:], out["rgb"])
    # an RGBA ground truth goes over the render's background
    alpha = (torch.rand(H, W, 1, generator=torch.Generator().manual_seed(4)) > 0.5).float()
    rgba = torch.cat([images[0], alpha], dim=-1)
    over = alpha * images[0] + (1 - alpha) * out["background"].cpu()
    assert torch.equal(model.composite_with_background(rgba.to(dev), out["background"]).cpu(), over)
    assert model.composite_with_background(images[0], out["background"]) is images[0]
    assert _bits_equal(model.get_metrics_dict(out, {"image": rgba})["psnr"], m.psnr(out["rgb"].contiguous(), over.to(dev))[0])
    assert torch.equal(model.get_image_metrics_and_images(out, {"image": rgba})[1]["img"][:, :W].cpu(), over)


def test_model_evaluate_views_does_not_depend_on_the_batches(dev, model_and_cams):
    import collab_splats_amd as m
    model, cams, images, _ = model_and_cams
    maps = model.render_views(cams, batch_size=1)
    g = torch.Generator().manual_seed(5)
    normals = [(maps["normals"][i].cpu() + 0.05 * torch.rand(maps["normals"][i].shape, generator=g)).clamp(0, 1) for i in range(5)]
    depths = [maps["depth"][i].cpu() * (0.8 + 0.4 * torch.rand(maps["depth"][i].shape, generator=g)) for i in range(5)]
    valid = [torch.rand(maps["depth"][i].shape[:2], generator=g) > 1.0 / 3.0 for i in range(5)]
    two = model.evaluate_views(cams, images, normals, depths, valid, batch_size=2)
    one = model.evaluate_views(cams, images, normals, depths, valid, batch_size=1)
    assert sorted(two) == ["mean", "per_view"] and len(two["per_view"]) == 4 + 5 + 8 and sorted(two["mean"]) == sorted(two["per_view"])
    for k, v in two["per_view"].items():
        assert v.shape == (5,) and v.is_cuda and _bits_equal(v, one["per_view"][k]), k
        assert two["mean"][k] == float(v.mean()) or (math.isnan(two["mean"][k]) and bool(torch.isnan(v).any())), k
    for i in range(5):                                                  # and equals scoring the views one at a time
        im = m.image_metrics(maps["rgb"][i], images[i].to(dev))
        nm = m.normal_metrics(maps["normals"][i], normals[i].to(dev), valid[i].to(dev), encoded=True)
        dm = m.depth_metrics(maps["depth"][i:i + 1], depths[i][None].to(dev), valid[i][None].to(dev))
        for k in im:
            assert _bits_equal(two["per_view"][k][i:i + 1], im[k]), (k, i)
        for k in nm:
            assert _bits_equal(two["per_view"]["normal_" + k][i:i + 1], nm[k]), (k, i)
        for k in dm:
            assert _bits_equal(two["per_view"]["depth_" + k][i:i + 1], dm[k]), (k, i)
    assert float(two["per_view"]["depth_count"].sum()) > 0 and float(two["per_view"]["normal_count"].sum()) > 0
    only = model.evaluate_views(cams[:3], images[:3], batch_size=4)
    assert sorted(only["per_view"]) == ["l1", "mse", "psnr", "ssim"] and only["per_view"]["psnr"].shape == (3,)


# ---------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_come_before_any_launch(dev):
    import collab_splats_amd as m
    z = lambda *s: torch.zeros(*s, device=dev)                                           # noqa: E731
    with pytest.raises(ValueError, match="SSIM needs"):
        m.image_metrics(z(1, 10, 40, 3), z(1, 10, 40, 3))
    with pytest.raises(ValueError, match="SSIM needs"):
        m.ssim(z(40, 10, 3), z(40, 10, 3))
    assert bool((m.image_metrics(z(1, 10, 40, 3), z(1, 10, 40, 3), ssim=False)["mse"] == 0).all())   # fine without SSIM
    with pytest.raises(m.MisplatError, match="CPU tensor"):
        m.image_metrics(torch.zeros(1, 11, 11, 3), torch.zeros(1, 11, 11, 3))
    with pytest.raises(m.MisplatError, match="CPU tensor"):
        m.normal_metrics(z(1, 4, 4, 3), torch.zeros(1, 4, 4, 3))
    with pytest.raises(m.MisplatError, match="CPU tensor"):
        m.depth_metrics(z(1, 4, 4), z(1, 4, 4), valid=torch.ones(1, 4, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="differ in shape"):
        m.image_metrics(z(1, 12, 12, 3), z(1, 12, 13, 3))
    with pytest.raises(ValueError, match="differ in shape"):
        m.depth_metrics(z(2, 4, 4), z(1, 4, 4))
    with pytest.raises(ValueError, match="float32"):
        m.image_metrics(z(1, 12, 12, 3).double(), z(1, 12, 12, 3).double())
    with pytest.raises(ValueError, match=r"\[B, H, W, 3\]"):
        m.normal_metrics(z(1, 4, 4, 2), z(1, 4, 4, 2))
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        m.mean_angular_error(z(1, 4, 4, 3), z(1, 4, 4, 3))
    with pytest.raises(ValueError, match="valid must be"):
        m.depth_metrics(z(1, 4, 4), z(1, 4, 4), valid=torch.ones(1, 4, 5, dtype=torch.bool, device=dev))
    many = z(1, 11, 11, 3).expand(65536, 11, 11, 3)                                      # (a view: no 95 MB allocation)
    with pytest.raises(ValueError, match="65535 views"):
        m.image_metrics(many, many)
    with pytest.raises(ValueError, match="65535 views"):
        m.depth_metrics(many[..., 0], many[..., 0])
    from collab_splats_amd import _lib
    import ctypes as C
    lib = _lib.load()
    assert lib.misplat_eval_image_scratch_floats(C.c_int32(65536), C.c_int32(11), C.c_int32(11)) == -1
    assert lib.misplat_eval_image_scratch_floats(C.c_int32(1), C.c_int32(46341), C.c_int32(46341)) == -1     # H W >= 2^31
    assert lib.misplat_eval_image_scratch_floats(C.c_int32(3), C.c_int32(27), C.c_int32(43)) == 3 * 3 * 2 * 3
    buf = z(64)
    p = C.c_void_p(buf.data_ptr())
    null = C.c_void_p(0)
    s = _lib.stream_ptr()
    assert lib.misplat_eval_image(C.c_int32(65536), C.c_int32(11), C.c_int32(11), p, p, C.c_int32(1), p, p, s) == -1
    assert lib.misplat_eval_image(C.c_int32(1), C.c_int32(10), C.c_int32(11), p, p, C.c_int32(1), p, p, s) == -1
    assert lib.misplat_eval_image(C.c_int32(1), C.c_int32(11), C.c_int32(11), null, p, C.c_int32(1), p, p, s) == -1
    assert lib.misplat_eval_normals(C.c_int32(1), C.c_int32(4), C.c_int32(4), p, null, null, C.c_int32(0), C.c_int32(1), null, p, p, s) == -1
    assert lib.misplat_eval_depth(C.c_int32(0), C.c_int32(4), C.c_int32(4), p, p, null, C.c_float(0.0), p, p, s) == -1
