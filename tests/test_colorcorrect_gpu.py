"""GPU: the colour correction (csrc/colorcorrect.hip, ``color_correct`` / ``color_corrected_metrics``, the model's
``color_corrected_metrics`` flag) against the fp64 restatement (tests/colorcorrect_restatement.py) on the scenes of
tests/colorcorrect_scenes.py.

Image parity: 2^-22 absolute per element, every element.  The bound is four times what re-ordering the restatement's own
fp64 sums moves its output (2^-24, one float32 step of a value in [0.5, 1)); tests/test_colorcorrect_host.py repeats that
measurement on every scene, and asserts the conditions under which no mask and no rank decision can differ between device and
restatement -- which is why the mask counts are compared exactly.  The apply is held to bits: the restatement's apply, driven
by the DEVICE's warps, must reproduce the device's image bit for bit through the whole chain of iterations.
(The figures of a GPU run belong in DESIGN.md section 35; these tests print them.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import colorcorrect_restatement as R
import colorcorrect_scenes as S

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -22


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.int32),
                                                                      b.reshape(-1).contiguous().view(torch.int32))


def _np_bits_equal(a: np.ndarray, b: np.ndarray) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _run(dev, pred: np.ndarray, gt: np.ndarray, **kw):
    import collab_splats_amd as m
    img, fit = m.color_correct(torch.from_numpy(np.array(pred)).to(dev), torch.from_numpy(np.array(gt)).to(dev), return_fit=True, **kw)
    return img.cpu().numpy(), fit["warps"].cpu().numpy(), fit["counts"].cpu().numpy()


def _dev_max(a: np.ndarray, b: np.ndarray) -> float:
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


def _check_view(tag, family, pred, gt, img, warps, counts, ref):
    e = _dev_max(img, ref["image"])
    print(f"{tag} image gpu - restatement {e:.3e}  bound {BOUND:.3e}")
    assert np.isfinite(img).all() and np.isfinite(warps).all()
    assert np.array_equal(counts, ref["counts"]), (tag, counts, ref["counts"])
    assert _np_bits_equal(R.apply_chain(pred, warps), img), tag           # the apply, from the device's own fit: bit for bit
    assert e <= BOUND, (tag, e)
    if family in ("identical", "exactwarp"):
        assert _dev_max(img, gt) <= BOUND, tag
    if family == "allmasked":
        assert not img.any() and not warps.any() and not counts.any(), tag
    if family == "gray":
        assert np.array_equal(img[..., 0].view(np.int32), img[..., 1].view(np.int32)), tag
        assert np.array_equal(img[..., 0].view(np.int32), img[..., 2].view(np.int32)), tag


@pytest.mark.parametrize("family,size", S.scenes())
def test_color_correct_against_the_restatement(dev, family, size):
    pred, gt = S.scene(family, size)
    img, warps, counts = _run(dev, pred, gt)
    assert img.shape == pred.shape and img.dtype == np.float32 and warps.shape == (1, 5, 10, 3) and warps.dtype == np.float64
    assert counts.shape == (1, 5, 3) and counts.dtype == np.int64
    _check_view(f"{family:9s} {size[0]}x{size[1]}", family, pred, gt, img, warps[0], counts[0], S.restated(family, size))


@pytest.mark.parametrize("families,size", S.stacks())
def test_stacked_views_equal_the_single_calls_bit_for_bit(dev, families, size):
    """B = 3 with three different families: every view against its restatement, two runs equal, and view b equal to the B = 1
    call on that view (image, warps and counts)."""
    pred, gt = S.stacked(families, size)
    img, warps, counts = _run(dev, pred, gt)
    again = _run(dev, pred, gt)
    assert _np_bits_equal(img, again[0]) and np.array_equal(warps.view(np.int64), again[1].view(np.int64))
    assert np.array_equal(counts, again[2])
    for b, family in enumerate(families):
        _check_view(f"{family:9s} {size[0]}x{size[1]} (view {b} of 3)", family, pred[b], gt[b], img[b], warps[b], counts[b],
                    S.restated(family, size))
        one = _run(dev, pred[b], gt[b])                                    # [H, W, 3]
        assert one[0].shape == pred[b].shape and _np_bits_equal(one[0], img[b]), (family, b)
        assert np.array_equal(one[1][0].view(np.int64), warps[b].view(np.int64)) and np.array_equal(one[2][0], counts[b])


def test_number_of_iterations(dev):
    import collab_splats_amd as m
    pred, gt = S.scene("saturated", (17, 33))
    p, g = torch.from_numpy(np.array(pred)).to(dev), torch.from_numpy(np.array(gt)).to(dev)
    zero, fit = m.color_correct(p, g, num_iters=0, return_fit=True)
    assert zero.data_ptr() != p.data_ptr() and _bits_equal(zero, p)
    assert fit["warps"].shape == (1, 0, 10, 3) and fit["counts"].shape == (1, 0, 3)
    one, five = m.color_correct(p, g, num_iters=1), m.color_correct(p, g)
    assert not torch.equal(one, five)
    for n, got in ((1, one), (5, five)):
        ref = R.color_correct(pred, gt, num_iters=n)["image"]
        assert _dev_max(got.cpu().numpy(), ref) <= BOUND, n
    three, f3 = m.color_correct(p, g, num_iters=3, return_fit=True)
    _, f5 = m.color_correct(p, g, return_fit=True)
    assert torch.equal(f3["warps"], f5["warps"][:, :3]) and torch.equal(f3["counts"], f5["counts"][:, :3])   # a prefix of the chain
    wide = m.color_correct(p, g, eps=0.04)                                 # another eps: other masks, and the restatement's
    assert _dev_max(wide.cpu().numpy(), R.color_correct(pred, gt, eps=0.04)["image"]) <= BOUND
    assert not torch.equal(wide, five)


def test_color_corrected_metrics_are_the_metrics_of_the_corrected_image(dev):
    import collab_splats_amd as m
    pred, gt = (torch.from_numpy(np.array(a)).to(dev) for a in S.stacked(S.STACKS[0], (17, 33)))
    got = m.color_corrected_metrics(pred, gt)
    direct = m.image_metrics(m.color_correct(pred, gt), gt)
    assert sorted(got) == ["cc_l1", "cc_mse", "cc_psnr", "cc_ssim"]
    for k, v in direct.items():
        assert got["cc_" + k].shape == (3,) and got["cc_" + k].is_cuda and _bits_equal(got["cc_" + k], v), k
    lean = m.color_corrected_metrics(pred, gt, ssim=False)
    assert sorted(lean) == ["cc_l1", "cc_mse", "cc_psnr"] and _bits_equal(lean["cc_psnr"], got["cc_psnr"])
    one = m.color_corrected_metrics(pred, gt, num_iters=1)
    assert _bits_equal(one["cc_mse"], m.image_metrics(m.color_correct(pred, gt, num_iters=1), gt)["mse"])
    plain = m.image_metrics(pred, gt)
    assert float(got["cc_mse"][0]) < float(plain["mse"][0])               # the rand view: the correction helps


# -------------------------------------------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def model_and_cams(dev):
    """The 8 000-Gaussian, 64 x 48 model of test_metrics_gpu.py."""
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
    return model, cams, images


def test_model_flag_adds_the_colour_corrected_scores(dev, model_and_cams):
    import dataclasses
    import collab_splats_amd as m
    model, cams, images = model_and_cams
    out = model.get_outputs_for_camera(cams[0])
    off, pics_off = model.get_image_metrics_and_images(out, {"image": images[0]})
    assert sorted(off) == ["psnr", "ssim"]                                # the flag is off: the keys of before
    config = model.config
    try:
        model.config = dataclasses.replace(config, color_corrected_metrics=True)
        on, pics_on = model.get_image_metrics_and_images(out, {"image": images[0]})
    finally:
        model.config = config
    assert sorted(on) == ["cc_psnr", "cc_ssim", "psnr", "ssim"] and all(isinstance(v, float) for v in on.values())
    assert on["psnr"] == off["psnr"] and on["ssim"] == off["ssim"] and torch.equal(pics_on["img"], pics_off["img"])
    direct = m.color_corrected_metrics(out["rgb"].contiguous(), images[0].to(dev))
    assert on["cc_psnr"] == float(direct["cc_psnr"][0]) and on["cc_ssim"] == float(direct["cc_ssim"][0])
    assert sorted(model.get_metrics_dict(out, {"image": images[0]})) == ["gaussian_count", "psnr"]


def test_model_evaluate_views_colour_corrected(dev, model_and_cams):
    import dataclasses
    import collab_splats_amd as m
    model, cams, images = model_and_cams
    plain = model.evaluate_views(cams, images, batch_size=2)
    assert sorted(plain["per_view"]) == ["l1", "mse", "psnr", "ssim"]     # the flag is off and nothing was asked for
    assert sorted(model.evaluate_views(cams, images, batch_size=2, color_correct=False)["per_view"]) == ["l1", "mse", "psnr", "ssim"]
    two = model.evaluate_views(cams, images, batch_size=2, color_correct=True)
    one = model.evaluate_views(cams, images, batch_size=1, color_correct=True)
    names = ["cc_l1", "cc_mse", "cc_psnr", "cc_ssim", "l1", "mse", "psnr", "ssim"]
    assert sorted(two["per_view"]) == names and sorted(two["mean"]) == names
    maps = model.render_views(cams, batch_size=1)
    for k in names:
        assert two["per_view"][k].shape == (5,) and _bits_equal(two["per_view"][k], one["per_view"][k]), k
        if not k.startswith("cc_"):
            assert _bits_equal(two["per_view"][k], plain["per_view"][k]), k
    for i in range(5):
        direct = m.color_corrected_metrics(maps["rgb"][i], images[i].to(dev))
        for k, v in direct.items():
            assert _bits_equal(two["per_view"][k][i:i + 1], v), (k, i)
    config = model.config
    try:                                                                   # None follows the config
        model.config = dataclasses.replace(config, color_corrected_metrics=True)
        follows = model.evaluate_views(cams[:2], images[:2], batch_size=2)
        refuses = model.evaluate_views(cams[:2], images[:2], batch_size=2, color_correct=False)
    finally:
        model.config = config
    assert sorted(follows["per_view"]) == names and sorted(refuses["per_view"]) == ["l1", "mse", "psnr", "ssim"]
    assert _bits_equal(follows["per_view"]["cc_psnr"], two["per_view"]["cc_psnr"][:2])


# ---------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_come_before_any_launch(dev):
    import collab_splats_amd as m
    from collab_splats_amd import _lib
    z = lambda *s: torch.zeros(*s, device=dev)                                           # noqa: E731
    with pytest.raises(ValueError, match="differ in shape"):
        m.color_correct(z(1, 12, 12, 3), z(1, 12, 13, 3))
    with pytest.raises(ValueError, match="float32"):
        m.color_correct(z(1, 12, 12, 3).double(), z(1, 12, 12, 3).double())
    with pytest.raises(ValueError, match=r"\[B, H, W, 3\]"):
        m.color_correct(z(1, 4, 4, 4), z(1, 4, 4, 4))
    with pytest.raises(ValueError, match="num_iters"):
        m.color_correct(z(1, 4, 4, 3), z(1, 4, 4, 3), num_iters=65)
    with pytest.raises(ValueError, match="num_iters"):
        m.color_correct(z(1, 4, 4, 3), z(1, 4, 4, 3), num_iters=2.0)
    with pytest.raises(ValueError, match="eps"):
        m.color_correct(z(1, 4, 4, 3), z(1, 4, 4, 3), eps=-1e-3)
    with pytest.raises(m.MisplatError, match="CPU tensor"):
        m.color_correct(z(1, 4, 4, 3), torch.zeros(1, 4, 4, 3))
    with pytest.raises(ValueError, match="SSIM needs"):
        m.color_corrected_metrics(z(1, 10, 40, 3), z(1, 10, 40, 3))
    many = z(1, 2, 2, 3).expand(65536, 2, 2, 3)
    with pytest.raises(ValueError, match="65535 views"):
        m.color_correct(many, many)
    lib = _lib.load()
    buf = torch.zeros(4096, device=dev, dtype=torch.float64)
    p, null, s = C.c_void_p(buf.data_ptr()), C.c_void_p(0), _lib.stream_ptr()
    q = C.c_void_p(buf.data_ptr() + 8192)
    i32 = C.c_int32
    assert lib.misplat_colorcorrect_scratch_floats(i32(65536), i32(4), i32(4)) == -1
    assert lib.misplat_colorcorrect(i32(0), i32(4), i32(4), p, p, i32(5), C.c_float(0.002), p, q, p, p, s) == -1
    assert lib.misplat_colorcorrect(i32(1), i32(4), i32(4), p, p, i32(65), C.c_float(0.002), p, q, p, p, s) == -1
    assert lib.misplat_colorcorrect(i32(1), i32(4), i32(4), p, p, i32(5), C.c_float(0.5), p, q, p, p, s) == -1
    assert lib.misplat_colorcorrect(i32(1), i32(4), i32(4), p, p, i32(5), C.c_float(0.002), null, q, p, p, s) == -1
    assert lib.misplat_colorcorrect(i32(1), i32(4), i32(4), p, p, i32(5), C.c_float(0.002), p, p, p, p, s) == -1   # in place
    assert not buf.any()
