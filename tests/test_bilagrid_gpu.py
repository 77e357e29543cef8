"""GPU: the bilateral-grid slice and TV loss (csrc/bilagrid.hip, collab_splats_amd/bilagrid.py) against the fp64
restatement (tests/bilagrid_restatement.py) on the scenes of tests/bilagrid_scenes.py, and the model wiring.

Error measure, per tensor, as in test_featureloss_gpu.py: max |got - oracle| / max |oracle|, no pixel or cell left out.  The
bound of a tensor is ``MULTIPLE`` times the error the fp32 restatement itself makes on the same scene against the same
oracle (computed here from the restatement, never from the code under test), that error floored at 2^-23 (no fp32 result
can be asked to carry less than one rounding of its own), and never above the project's standing 1e-4.

MULTIPLE = 8.  The slice's output and the image-side gradient are per-pixel expressions of fixed length (seven lerps per
channel, a 4-term and a 24-term sum) that the kernels evaluate in the restatement's order, so they sit at the yardstick
itself.  The grid-side gradient of a cell is a sum over the pixels of its support -- up to some 300 in ``blocks``, 42 000 in
``split`` -- which the restatement adds one pixel at a time in index order, and the kernels as strided private sums per lane, a
shuffle tree over 64 lanes, four waves and up to 16 row slices: two different orders over n terms differ by about sqrt(n)
roundings of the sum's size relative to each other, which for n = 42 000 spread over 256 lanes x 11 slices (chains of ~15) is
a handful of roundings against the restatement's own chain of n; 8 covers it with the margin the feature loss uses.  The TV
sums meet in fp64 in the kernels, which can only be closer to the oracle than the fp32 restatement's fp32 sum.  (The
figures of a GPU run belong in DESIGN.md section 24; this test prints them.)

``S.REGIME_SCENES`` / ``S.REGIME_TV_SHAPES`` take the same tests, under the same bound, to the launch regimes a training run
reaches: several trips of the three grid-stride loops, a middle camera among 23, empty row slices, the sizes at the header's
limits, a 1 x 1 image and colours outside 0..1 (test_bilagrid_host.py asserts from the launch arithmetic what each reaches)."""
import pytest
import torch

import bilagrid_scenes as S

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


def run_gpu(scene, cam, dev, grids=None):
    import collab_splats_amd as m
    rgb = scene["rgb"].to(dev).requires_grad_(True)
    g = (scene["grids"] if grids is None else grids).to(dev).requires_grad_(True)
    out = m.bilagrid_slice(rgb, g, cam)
    out.backward(scene["v_out"].to(dev))
    torch.cuda.synchronize()
    return {"out": out.detach(), "v_rgb": rgb.grad, "v_grids": g.grad}


def run_tv_gpu(grids, dev):
    import collab_splats_amd as m
    g = grids.to(dev).requires_grad_(True)
    loss = m.bilagrid_tv_loss(g)
    loss.backward()
    torch.cuda.synchronize()
    return {"loss": loss.detach(), "v_grids": g.grad}


@pytest.mark.parametrize("name", S.ALL_SCENES)
def test_slice_and_gradients_against_the_fp64_oracle(dev, name):
    scene = S.make(name)
    for cam in S.cameras(name):
        ora, y32 = S.oracle(name, cam), S.yardstick(name, cam)
        got = run_gpu(scene, cam, dev)
        rows = [(k, S.rel_err(got[k], ora[k]), S.rel_err(y32[k], ora[k])) for k in ("out", "v_rgb", "v_grids")]
        for k, e_gpu, e_32 in rows:
            print(f"bilagrid {name:10s} cam {cam} {k:8s} gpu {e_gpu:.3e}  fp32 restatement {e_32:.3e}  bound {bound(e_32):.3e}")
        for k, e_gpu, e_32 in rows:
            assert got[k].shape == ora[k].shape and bool(torch.isfinite(got[k]).all()), (name, cam, k)
            assert e_gpu <= bound(e_32), (name, cam, k, e_gpu, e_32)
        others = [c for c in range(scene["num"]) if c != cam]
        assert bool((got["v_grids"][others] == 0).all()), (name, cam)


@pytest.mark.parametrize("name", ["tiny", "one_row", "one_col", "blocks", "flat_z", "saturated", "deep"])
def test_identity_grid_returns_rgb_bit_for_bit(dev, name):
    import collab_splats_amd as m
    scene = S.make(name)
    grids = m.BilateralGrid(scene["num"], *scene["shape"]).grids.detach()
    for cam in (0, scene["num"] - 1):
        got = run_gpu(scene, cam, dev, grids=grids)
        assert torch.equal(got["out"].cpu(), scene["rgb"]), (name, cam)
    batched = m.bilagrid_slice(scene["rgb"][None].to(dev), grids.to(dev), 0)           # [1, H, W, 3] comes back as such
    assert batched.shape == (1,) + tuple(scene["rgb"].shape) and torch.equal(batched[0].cpu(), scene["rgb"])


@pytest.mark.parametrize("name", S.ALL_TV_SHAPES)
def test_tv_loss_and_gradient_against_the_fp64_oracle(dev, name):
    ora, y32 = S.tv_oracle(name), S.tv_yardstick(name)
    got = run_tv_gpu(S.tv_grids(name), dev)
    rows = [(k, S.rel_err(got[k], ora[k]), S.rel_err(y32[k], ora[k])) for k in ("loss", "v_grids")]
    for k, e_gpu, e_32 in rows:
        print(f"bilagrid tv {name:10s} {k:8s} gpu {e_gpu:.3e}  fp32 restatement {e_32:.3e}  bound {bound(e_32):.3e}")
    for k, e_gpu, e_32 in rows:
        assert got[k].shape == ora[k].shape and e_gpu <= bound(e_32), (name, k, e_gpu, e_32)


def test_tv_gradient_scales_with_the_incoming_scalar(dev):
    import collab_splats_amd as m
    g = S.tv_grids("odd_3").to(dev).requires_grad_(True)
    (10 * m.bilagrid_tv_loss(g)).backward()
    ten = g.grad.clone()
    assert S.rel_err(ten, 10 * S.tv_oracle("odd_3")["v_grids"]) <= bound(
        S.rel_err(S.tv_yardstick("odd_3")["v_grids"], S.tv_oracle("odd_3")["v_grids"]))


@pytest.mark.parametrize("name", ["blocks", "split", "deep"] + list(S.REGIME_SCENES))
def test_two_runs_are_equal_bit_for_bit(dev, name):
    """``split`` / ``deep``: the row slices of a support and the two level chunks are in the sums as well.  The regime scenes:
    the cameras they list beyond camera 0 (``many_cams``: 11 and 22, with the finish kernel's second trip in the result)."""
    scene = S.make(name)
    for cam in S.cameras(name)[1:]:
        a, b = run_gpu(scene, cam, dev), run_gpu(scene, cam, dev)
        for k in a:
            assert torch.equal(a[k], b[k]), (cam, k)
    ta, tb = run_tv_gpu(scene["grids"], dev), run_tv_gpu(scene["grids"], dev)
    assert torch.equal(ta["loss"], tb["loss"]) and torch.equal(ta["v_grids"], tb["v_grids"])


def test_empty_row_slices_write_their_zeros_into_dirty_scratch(dev):
    """The grid-side backward's scratch comes from ``torch.empty``: a row slice without rows must still write its zeros, or
    the second pass adds whatever lay there.  Fresh device memory is often zero, so the comparison on ``empty_slices`` alone
    can pass by luck; here the block the scratch will take is filled with NaN first (freed blocks of the caching allocator
    are handed out again for a request of the same size -- checked with a probe, so the test cannot pass without its premise)."""
    import ctypes as C
    import collab_splats_amd as m
    from collab_splats_amd import _lib
    scene = S.make("empty_slices")
    (H, W), (GW, GH, L) = scene["rgb"].shape[:2], scene["shape"]
    n = int(_lib.load().misplat_bilagrid_scratch_floats(C.c_int32(H), C.c_int32(W), C.c_int32(GW), C.c_int32(GH), C.c_int32(L)))
    assert n == 11 * GW * GH * 8 * 12                                                  # 11 row slices, L padded to 8 levels
    for cam in S.cameras("empty_slices"):
        ora, y32 = S.oracle("empty_slices", cam), S.yardstick("empty_slices", cam)
        torch.cuda.empty_cache()
        rgb = scene["rgb"].to(dev).requires_grad_(True)
        g = scene["grids"].to(dev).requires_grad_(True)
        out = m.bilagrid_slice(rgb, g, cam)
        v_out = scene["v_out"].to(dev)
        junk = [torch.full((n,), float("nan"), device=dev) for _ in range(3)]
        torch.cuda.synchronize()
        del junk
        probe = torch.empty(n, device=dev)
        assert bool(torch.isnan(probe).all()), "the allocator did not hand the dirtied block out again: the test has no premise"
        del probe
        out.backward(v_out)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(g.grad).all()), cam
        e_gpu, e_32 = S.rel_err(g.grad, ora["v_grids"]), S.rel_err(y32["v_grids"], ora["v_grids"])
        assert e_gpu <= bound(e_32), (cam, e_gpu, e_32)
        assert bool((g.grad[1 - cam] == 0).all())


@pytest.mark.parametrize("name", list(S.REGIME_TV_SHAPES))
def test_two_tv_runs_are_equal_bit_for_bit(dev, name):
    """The partials of several trips and all 1024 of them in tv_finish_kernel meet in a fixed order."""
    ta, tb = run_tv_gpu(S.tv_grids(name), dev), run_tv_gpu(S.tv_grids(name), dev)
    assert torch.equal(ta["loss"], tb["loss"]) and torch.equal(ta["v_grids"], tb["v_grids"])


@pytest.mark.parametrize("name,cams", [("one_pixel", (0, 1)), ("max_depth", (0, 1)), ("many_cams", (11,)), ("beyond", (0, 1))])
def test_identity_grid_returns_rgb_bit_for_bit_on_regime_scenes(dev, name, cams):
    """``beyond``: the identity affine is constant along z, so colours outside 0..1 come back bit for bit as well."""
    import collab_splats_amd as m
    scene = S.make(name)
    grids = m.BilateralGrid(scene["num"], *scene["shape"]).grids.detach()
    if name == "beyond":
        assert float(scene["rgb"].min()) < 0.0 and float(scene["rgb"].max()) > 1.0
    for cam in cams:
        got = run_gpu(scene, cam, dev, grids=grids)
        assert torch.equal(got["out"].cpu(), scene["rgb"]), (name, cam)


def test_upstream_gradient_layouts(dev):
    """The layouts of ``v_out`` the autograd node meets: ``sum().backward()`` hands it an expanded, stride-0 tensor of ones, and
    a [1, H, W, 3] image gets its gradient in that shape.  Both must give the gradients of the explicit, dense [H, W, 3] run."""
    import collab_splats_amd as m
    scene = S.make("blocks")
    cam = 1

    def run(batched: bool, how: str):
        rgb = (scene["rgb"][None] if batched else scene["rgb"]).to(dev).requires_grad_(True)
        g = scene["grids"].to(dev).requires_grad_(True)
        out = m.bilagrid_slice(rgb, g, cam)
        if how == "sum":
            out.sum().backward()
        else:
            v = torch.ones_like(out) if how == "ones" else scene["v_out"].to(dev).view(out.shape)
            out.backward(v)
        torch.cuda.synchronize()
        assert rgb.grad.shape == rgb.shape and g.grad.shape == g.shape
        return rgb.grad.reshape(scene["rgb"].shape), g.grad

    ones = run(False, "ones")
    for batched, how in ((False, "sum"), (True, "sum"), (True, "ones")):
        got = run(batched, how)
        assert torch.equal(got[0], ones[0]) and torch.equal(got[1], ones[1]), (batched, how)
    assert float(ones[1][cam].abs().sum()) > 0 and bool((ones[1][0] == 0).all())
    dense, dense_b = run(False, "v_out"), run(True, "v_out")
    assert torch.equal(dense[0], dense_b[0]) and torch.equal(dense[1], dense_b[1])
    ora = S.oracle("blocks", cam)
    y32 = S.yardstick("blocks", cam)
    for k, got in (("v_rgb", dense_b[0]), ("v_grids", dense_b[1])):
        assert S.rel_err(got, ora[k]) <= bound(S.rel_err(y32[k], ora[k])), k


def _model(dev, flag: bool, features: bool = False):
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 240, 136, 6000
    sc = random_scene(N, W, H, seed=2)
    args = (sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0], sc["sh"][:, 1:])
    kw = dict(rasterize_mode="antialiased", regularization_from_iter=0, use_bilateral_grid=flag)
    extra = {"num_train_data": 3} if flag else {}
    if features:
        model = radegs.RadegsFeaturesModel(radegs.RadegsFeaturesModelConfig(**kw), *args,
                                           torch.rand(N, 13, generator=torch.Generator().manual_seed(2)), **extra)
    else:
        model = radegs.RadegsModel(radegs.RadegsModelConfig(**kw), *args, **extra)
    model = model.to(dev).train()
    model.step = 5000
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 0]])
    cam = radegs.PinholeCamera.make(c2w, 0.9 * W, 0.9 * W, W, H)
    return model, cam, (H, W)


@pytest.mark.parametrize("features", [False, True])
def test_model_training_step_with_the_grid(dev, features):
    from collab_splats_amd import FusedAdam, fused_adam_step_all
    plain, cam, (H, W) = _model(dev, False, features)
    model, _, _ = _model(dev, True, features)
    base = plain.get_outputs(cam)["rgb"].detach()
    cam.metadata = {"cam_idx": 1}
    assert torch.equal(plain.get_outputs(cam)["rgb"], base)                            # the flag is off: metadata changes nothing
    # identity grids: the corrected image is the uncorrected one, bit for bit
    assert torch.equal(model.get_outputs(cam)["rgb"].detach(), base)
    with torch.no_grad():
        model.bil_grids.grids.add_(0.05 * torch.randn(model.bil_grids.grids.shape, generator=torch.Generator().manual_seed(4)).to(dev))
    out = model.get_outputs(cam)
    assert out["rgb"].shape == (H, W, 3) and not torch.equal(out["rgb"].detach(), base)
    # without metadata, with metadata that names no camera, and in evaluation: the uncorrected image
    cam.metadata = None
    assert torch.equal(model.get_outputs(cam)["rgb"].detach(), base)
    cam.metadata = {"other": 3}
    assert torch.equal(model.get_outputs(cam)["rgb"].detach(), base)
    cam.metadata = {"cam_idx": 1}
    model.eval()
    plain.eval()
    with torch.no_grad():
        assert torch.equal(model.get_outputs(cam)["rgb"], plain.get_outputs(cam)["rgb"])
        assert "tv_loss" not in model.get_loss_dict(model.get_outputs(cam), {"image": torch.rand(H, W, 3)})
    model.train()
    # one step: main_loss + tv_loss reach the grids and the Gaussians; step_all moves the rendered camera's grid
    groups = model.get_param_groups()
    assert "bilateral_grid" in groups
    opts = {name: FusedAdam(params, lr=1e-3, eps=1e-15) for name, params in groups.items()}
    out = model.get_outputs(cam)
    loss = model.get_loss_dict(out, {"image": torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5))})
    assert {"main_loss", "tv_loss"} <= set(loss)
    from bilagrid_restatement import tv
    ref = 10 * float(tv(model.bil_grids.grids.detach().cpu(), torch.float64))
    assert abs(float(loss["tv_loss"].detach()) - ref) <= 1e-5 * ref
    (loss["main_loss"] + loss["tv_loss"]).backward()
    g = model.bil_grids.grids.grad
    assert g is not None and g.shape == model.bil_grids.grids.shape and bool(torch.isfinite(g).all())
    assert float(g[1].abs().sum()) > 0
    for k, p in model.gauss_params.items():
        if k == "distill_features":
            continue                                                                   # (no feature loss in this step)
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0, k
    before = model.bil_grids.grids.detach().clone()
    fused_adam_step_all(opts)
    torch.cuda.synchronize()
    after = model.bil_grids.grids.detach()
    assert bool(torch.isfinite(after).all()) and not torch.equal(after[1], before[1])
