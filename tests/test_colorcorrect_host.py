"""CPU: the scenes of tests/colorcorrect_scenes.py meet the conditions the GPU tests rest on, and the restatement
(tests/colorcorrect_restatement.py) agrees with an independent oracle.  Nothing here runs the library's kernels.

Conditions (on the inputs, met by the choice of seeds; the restatement alone decides them):
  * in every iteration no value of x or gt other than exact 0 or 1 lies within 2^-20 of eps or 1 - eps: no mask can flip
    between the device and the restatement, whose iterates differ by 2^-22 at most;
  * no eigenvalue of any Gram matrix has a ratio to the largest inside [2^-50, 2^-42]: the cut at 2^-46 is unambiguous;
  * ``saturated``: the three masks of the first iteration differ pairwise;
  * ``rand``, ``smooth``, ``saturated``: the corrected MSE is below the uncorrected.
The GPU tests' image bound 2^-22 is four times what re-ordering the restatement's own fp64 sums moves its output (one float32
step of a value in [0.5, 1): 2^-24); this test repeats that measurement on every scene with a permutation of the pixels and
asserts that four times it stays within the bound.

Oracle: the published formulation, the same loop with ``torch.linalg.lstsq(rcond=2^-23, driver="gelsd")`` in fp64 on the masked
design matrix.  ``gelsd`` on purpose: the default ``gelsy`` is no minimum-norm solver and is 0.37 off on ``gray`` and ``clipch``."""
import numpy as np
import pytest

import colorcorrect_restatement as R
import colorcorrect_scenes as S

BOUND = 2.0 ** -22


def _dev(a, b) -> float:
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


@pytest.mark.parametrize("family,size", S.scenes())
def test_scene_conditions(family, size):
    c = S.conditions(family, size)
    print(f"{family:9s} {size[0]}x{size[1]} margin {c['margin']:.3e} mse {c['mse_before']:.3e} -> {c['mse_after']:.3e}")
    assert c["margin"] >= S.GUARD, c
    assert c["rank_gap_clear"], c
    if family == "saturated":
        assert c["masks_differ"], c
    if family in ("rand", "smooth", "saturated"):
        assert c["mse_after"] < c["mse_before"], c
    pred, gt = S.scene(family, size)
    assert pred.dtype == np.float32 and gt.dtype == np.float32 and pred.shape == size + (3,)
    assert float(min(pred.min(), gt.min())) >= 0.0 and float(max(pred.max(), gt.max())) <= 1.0
    if family == "gray":
        assert np.array_equal(pred[..., 0], pred[..., 1]) and np.array_equal(pred[..., 0], pred[..., 2])
        assert np.array_equal(gt[..., 0], gt[..., 1]) and np.array_equal(gt[..., 0], gt[..., 2])
        ranks = [int((lam > R.CUT).sum()) for rat in S.restated(family, size)["ratios"] for lam in rat if lam is not None]
        assert ranks and max(ranks) <= 3, ranks
    if family == "clipch":
        assert not pred[..., 1].any() and not S.restated(family, size)["counts"][:, 1].any()
    if family == "allmasked":
        assert not pred.any()


@pytest.mark.parametrize("family,size", S.scenes())
def test_restatement_against_the_lstsq_oracle_and_reordered_sums(family, size):
    pred, gt = S.scene(family, size)
    ref = S.restated(family, size)
    oracle = R.color_correct(pred, gt, solver=R.solve_lstsq)
    e = _dev(oracle["image"], ref["image"])
    P = size[0] * size[1]
    moved = R.color_correct(pred, gt, order=np.random.default_rng(5).permutation(P))
    y = _dev(moved["image"], ref["image"])
    print(f"{family:9s} {size[0]}x{size[1]} lstsq oracle {e:.3e}  re-ordered sums {y:.3e}  bound {BOUND:.3e}")
    assert e <= BOUND, (family, size, e)
    assert 4.0 * y <= BOUND, (family, size, y)
    assert np.array_equal(oracle["counts"], ref["counts"]) and np.array_equal(moved["counts"], ref["counts"])


def test_restatement_known_answers():
    for size in S.SIZES:
        for family in ("identical", "exactwarp"):
            _, gt = S.scene(family, size)
            assert _dev(S.restated(family, size)["image"], gt) <= BOUND, (family, size)
        res = S.restated("allmasked", size)
        assert not res["image"].any() and not res["warps"].any() and not res["counts"].any()
        g = S.restated("gray", size)["image"]
        assert np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 0], g[..., 2]) and np.isfinite(g).all()
    pred, gt = S.scene("saturated", (17, 33))
    one, five = R.color_correct(pred, gt, num_iters=1), S.restated("saturated", (17, 33))
    assert not np.array_equal(one["image"], five["image"])
    assert np.array_equal(R.color_correct(pred, gt, num_iters=0)["image"].view(np.int32), pred.view(np.int32))
    # (the GPU test also runs this scene with one iteration and with eps = 0.04: the same guard for those thresholds)
    wide = R.color_correct(pred, gt, eps=0.04)
    assert S.threshold_margin(wide, gt, 0.04) >= S.GUARD and S.rank_gap_clear(wide) and S.rank_gap_clear(one)
    assert not np.array_equal(wide["image"], five["image"])
    # the apply alone, driven by the warps, is the image: what the GPU test does with the device's warps
    assert np.array_equal(R.apply_chain(pred, five["warps"]).view(np.int32), five["image"].view(np.int32))


def test_thresholds_are_float32():
    lo, hi = R.thresholds()
    assert lo.dtype == np.float32 and hi.dtype == np.float32 and hi == np.float32(1.0) - np.float32(0.5 / 255)
    z = np.array([lo, np.nextafter(lo, np.float32(0)), hi, np.nextafter(hi, np.float32(2)), 0.0, 1.0], dtype=np.float32)
    assert R.unclipped(z).tolist() == [True, False, True, False, False, False]


def test_binding_and_config():
    """The wrappers validate before any launch and fail loudly on CPU tensors; the config carries Splatfacto's flag, off."""
    import torch
    import collab_splats_amd as m
    from collab_splats_amd import radegs
    assert radegs.RadegsModelConfig().color_corrected_metrics is False
    assert radegs.RadegsFeaturesModelConfig().color_corrected_metrics is False
    z = torch.zeros
    with pytest.raises(ValueError, match="differ in shape"):
        m.color_correct(z(1, 4, 4, 3), z(1, 4, 5, 3))
    with pytest.raises(ValueError, match="float32"):
        m.color_correct(z(1, 4, 4, 3).double(), z(1, 4, 4, 3).double())
    with pytest.raises(ValueError, match=r"\[B, H, W, 3\]"):
        m.color_correct(z(1, 4, 4, 2), z(1, 4, 4, 2))
    with pytest.raises(ValueError, match="num_iters"):
        m.color_correct(z(1, 4, 4, 3), z(1, 4, 4, 3), num_iters=65)
    with pytest.raises(ValueError, match="num_iters"):
        m.color_correct(z(1, 4, 4, 3), z(1, 4, 4, 3), num_iters=-1)
    with pytest.raises(ValueError, match="eps"):
        m.color_correct(z(1, 4, 4, 3), z(1, 4, 4, 3), eps=0.5)
    with pytest.raises(ValueError, match="eps"):
        m.color_correct(z(1, 4, 4, 3), z(1, 4, 4, 3), eps=float("nan"))
    with pytest.raises(m.MisplatError, match="CPU tensor"):
        m.color_correct(z(1, 4, 4, 3), z(1, 4, 4, 3))
    with pytest.raises(m.MisplatError, match="CPU tensor"):
        m.color_corrected_metrics(z(12, 12, 3), z(12, 12, 3))


def test_entry_point_rejects_bad_sizes_before_any_launch(built_lib):
    """MISPLAT_EINVAL comes back before anything is launched or dereferenced: this runs without a GPU, on made-up pointers."""
    import ctypes as C
    from collab_splats_amd import _lib
    lib = _lib.load()
    i32, f32 = C.c_int32, C.c_float
    size = lib.misplat_colorcorrect_scratch_floats
    assert size(i32(0), i32(4), i32(4)) == -1 and size(i32(65536), i32(4), i32(4)) == -1
    assert size(i32(1), i32(46341), i32(46341)) == -1 and size(i32(1), i32(0), i32(4)) == -1
    assert size(i32(1), i32(1), i32(1)) == 2 * 65 * 3 and size(i32(3), i32(17), i32(33)) == 2 * 65 * 3 * 3 * 3
    assert size(i32(2), i32(1080), i32(1920)) == 2 * 65 * 3 * 256 * 2                # at most 256 workgroups per view and channel
    a, b, o, w = (C.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000))
    null, eps = C.c_void_p(0), f32(0.5 / 255)

    def call(B=1, H=4, W=4, pred=a, gt=b, iters=5, eps=eps, scratch=w, out=o, warps=w, counts=w):
        return lib.misplat_colorcorrect(i32(B), i32(H), i32(W), pred, gt, i32(iters), eps, scratch, out, warps, counts, null)

    for kw in (dict(B=0), dict(B=65536), dict(H=0), dict(H=46341, W=46341), dict(iters=-1), dict(iters=65), dict(eps=f32(0.5)),
               dict(eps=f32(-1e-3)), dict(eps=f32(float("nan"))), dict(pred=null), dict(gt=null), dict(out=null), dict(out=a),
               dict(scratch=null), dict(scratch=C.c_void_p(0x4004)), dict(warps=null), dict(counts=null)):
        assert call(**kw) == -1, kw
