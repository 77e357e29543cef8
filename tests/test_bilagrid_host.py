"""CPU (no kernel runs): the restatement of the bilateral-grid slice and TV loss (tests/bilagrid_restatement.py) against the
torch composition it restates and against finite differences, the scenes' construction, the fp32 yardstick's own error, and
the argument checks of ``collab_splats_amd.bilagrid`` and of the model wiring."""
import pytest
import torch
import torch.nn.functional as F

import bilagrid_restatement as R
import bilagrid_scenes as S

MULTIPLE = 8.0                                         # test_bilagrid_gpu.py's
CAP = 1e-4


def composition(rgb, grids, cam):
    """``F.grid_sample(grids[cam][None], ((x, y, z) - 0.5) * 2, "bilinear", "border", align_corners=True)`` followed by the
    affine, in the dtype of ``rgb``; z is the restatement's luma (fp32 value, as the definition has it)."""
    H, W = rgb.shape[:2]
    dt = rgb.dtype
    x = torch.arange(W, dtype=dt) / (W - 1) if W > 1 else torch.zeros(W, dtype=dt)
    y = torch.arange(H, dtype=dt) / (H - 1) if H > 1 else torch.zeros(H, dtype=dt)
    z = R._Luma.apply(rgb, torch.float32)
    coords = torch.stack([x[None, :].expand(H, W), y[:, None].expand(H, W), z], dim=-1)
    A = F.grid_sample(grids[cam][None], ((coords - 0.5) * 2)[None, None], mode="bilinear", padding_mode="border",
                      align_corners=True)[0, :, 0]                                       # [12, H, W]
    A = A.reshape(3, 4, H, W)
    ones = torch.ones(H, W, 1, dtype=dt)
    v = torch.cat([rgb, ones], dim=-1).permute(2, 0, 1)                                   # [4, H, W]
    return (A * v[None]).sum(1).permute(1, 2, 0)


def composition_tv(grids):
    num = grids.shape[0]
    total = 0.0
    for axis in (2, 3, 4):
        n = grids.shape[axis]
        if n < 2:
            continue
        hi = grids.index_select(axis, torch.arange(1, n))
        lo = grids.index_select(axis, torch.arange(0, n - 1))
        total = total + ((hi - lo) ** 2).sum() / (hi.numel() // num)
    return total / num


@pytest.mark.parametrize("name", list(S.SCENES))
def test_every_pixel_is_on_a_border_plane_or_clear_of_the_integers(name):
    sc = S.make(name)
    low, high, clear = S.gz_classes(sc["rgb"], sc["shape"][2])
    assert bool((low | high | clear).all())
    assert sc["num"] >= 2 and not torch.equal(sc["grids"][0], sc["grids"][-1])
    assert float(sc["rgb"].min()) >= 0.0 and float(sc["rgb"].max()) <= 1.0
    if name in ("saturated", "deep", "split"):
        black, white = (sc["rgb"] == 0).all(-1), (sc["rgb"] == 1).all(-1)
        assert int(black.sum()) >= 12 and int(white.sum()) >= 12
        assert bool(low[black].all()) and bool(high[white].all())
    if name == "flat_z":
        assert bool(low.all())


def test_luma_of_black_and_white_is_exact():
    assert float(R.luma(torch.zeros(1, 1, 3))) == 0.0
    assert float(R.luma(torch.ones(1, 1, 3))) == 1.0


@pytest.mark.parametrize("name", list(S.SCENES))
def test_fp64_restatement_equals_the_torch_composition(name):
    sc = S.make(name)
    for cam in (0, sc["num"] - 1):
        ora = S.oracle(name, cam)
        rgb = sc["rgb"].double().requires_grad_(True)
        grids = sc["grids"].double().requires_grad_(True)
        out = composition(rgb, grids, cam)
        (out * sc["v_out"].double()).sum().backward()
        for key, got in (("out", out), ("v_rgb", rgb.grad), ("v_grids", grids.grad)):
            assert S.rel_err(ora[key], got) <= 1e-12, (name, cam, key, S.rel_err(ora[key], got))


@pytest.mark.parametrize("name", list(S.TV_SHAPES))
def test_fp64_tv_equals_the_index_select_form(name):
    ora = S.tv_oracle(name)
    g = S.tv_grids(name).double().requires_grad_(True)
    loss = composition_tv(g)
    loss.backward()
    assert abs(float(loss.detach()) - float(ora["loss"])) <= 1e-12 * abs(float(ora["loss"]))
    assert S.rel_err(ora["v_grids"], g.grad) <= 1e-12


def test_oracle_gradients_against_central_differences_on_odd():
    """Central differences of the same lines with the luma in fp64 as well (an fp32-rounded z is a staircase at the scale of a
    step).  The output is quadratic in rgb inside an interval of z and linear in the grid, so the differences are exact up to
    rounding; the step stays inside the interval (GZ_MARGIN)."""
    sc = S.make("odd")
    cam, h = 1, 1e-4
    dt = torch.float64
    ana = R.run_slice(sc["rgb"], sc["grids"], sc["v_out"], cam, dt, luma_dtype=dt)
    # with the fp32 luma the gradients are the same up to the difference of the two z (2^-24 relative)
    ora = S.oracle("odd", cam)
    assert S.rel_err(ana["v_rgb"], ora["v_rgb"]) < 1e-6 and S.rel_err(ana["v_grids"], ora["v_grids"]) < 1e-6

    def value(rgb, grids):
        return float((R.slice_image(rgb, grids, cam, dt, luma_dtype=dt) * sc["v_out"].double()).sum())

    gen = torch.Generator().manual_seed(3)
    rgb, grids = sc["rgb"].double(), sc["grids"].double()
    top_rgb, top_grid = float(ana["v_rgb"].abs().max()), float(ana["v_grids"].abs().max())
    for _ in range(24):
        y, x, c = (int(torch.randint(0, n, (1,), generator=gen)) for n in rgb.shape)
        up, dn = rgb.clone(), rgb.clone()
        up[y, x, c] += h
        dn[y, x, c] -= h
        fd = (value(up, grids) - value(dn, grids)) / (2 * h)
        assert abs(fd - float(ana["v_rgb"][y, x, c])) <= 1e-8 * top_rgb, (y, x, c)
    for _ in range(24):
        idx = tuple(int(torch.randint(0, n, (1,), generator=gen)) for n in grids.shape[1:])
        up, dn = grids.clone(), grids.clone()
        up[(cam,) + idx] += h
        dn[(cam,) + idx] -= h
        fd = (value(rgb, up) - value(rgb, dn)) / (2 * h)
        assert abs(fd - float(ana["v_grids"][(cam,) + idx])) <= 1e-8 * top_grid, idx
    tg = S.tv_grids("odd_3").double()
    tv_ana = S.tv_oracle("odd_3")["v_grids"]
    for _ in range(12):
        idx = tuple(int(torch.randint(0, n, (1,), generator=gen)) for n in tg.shape)
        up, dn = tg.clone(), tg.clone()
        up[idx] += h
        dn[idx] -= h
        fd = (float(R.tv(up, dt)) - float(R.tv(dn, dt))) / (2 * h)
        assert abs(fd - float(tv_ana[idx])) <= 1e-8 * float(tv_ana.abs().max()), idx


@pytest.mark.parametrize("name", list(S.SCENES))
def test_fp32_yardstick_is_well_inside_the_cap(name):
    sc = S.make(name)
    for cam in (0, sc["num"] - 1):
        ora, y32 = S.oracle(name, cam), S.yardstick(name, cam)
        for key in ("out", "v_rgb", "v_grids"):
            assert y32[key].dtype == torch.float32
            e = S.rel_err(y32[key], ora[key])
            assert e < CAP / MULTIPLE, (name, cam, key, e)
        others = [c for c in range(sc["num"]) if c != cam]
        assert bool((ora["v_grids"][others] == 0).all())


@pytest.mark.parametrize("name", list(S.TV_SHAPES))
def test_fp32_tv_yardstick_is_well_inside_the_cap(name):
    ora, y32 = S.tv_oracle(name), S.tv_yardstick(name)
    assert abs(float(y32["loss"]) - float(ora["loss"])) < CAP / MULTIPLE * abs(float(ora["loss"]))
    assert S.rel_err(y32["v_grids"], ora["v_grids"]) < CAP / MULTIPLE


@pytest.mark.parametrize("name", ["blocks", "saturated", "one_row", "one_col", "flat_z"])
def test_identity_grid_returns_rgb_bit_for_bit_in_fp32(name):
    import collab_splats_amd as m
    sc = S.make(name)
    grids = m.BilateralGrid(2, *sc["shape"]).grids.detach()
    out = R.slice_image(sc["rgb"], grids, 1, torch.float32)
    assert out.dtype == torch.float32 and torch.equal(out, sc["rgb"])


def test_bilateral_grid_module_state():
    import collab_splats_amd as m
    mod = m.BilateralGrid(5)
    sd = mod.state_dict()
    assert list(sd) == ["grids"] and sd["grids"].shape == (5, 12, 8, 16, 16) and sd["grids"].dtype == torch.float32
    eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])
    assert bool((sd["grids"] == eye.view(1, 12, 1, 1, 1)).all()) and mod.grids.requires_grad
    assert m.BilateralGrid(2, 4, 3, 2).grids.shape == (2, 12, 2, 3, 4)              # (grid_X, grid_Y, grid_W) = (GW, GH, L)
    other = m.BilateralGrid(5)
    other.load_state_dict({"grids": torch.randn(5, 12, 8, 16, 16)})
    for bad in ((0, 16, 16, 8), (2, 0, 16, 8), (2, 16, 257, 8), (2, 16, 16, 17), (2, 16, 16, 0)):
        with pytest.raises(ValueError, match="BilateralGrid"):
            m.BilateralGrid(*bad)


def test_argument_errors_are_raised_before_any_gpu_call():
    import collab_splats_amd as m
    from collab_splats_amd import ops
    assert ops.bilagrid_slice is m.bilagrid_slice and ops.bilagrid_tv_loss is m.bilagrid_tv_loss
    rgb, grids = torch.rand(6, 8, 3), torch.zeros(2, 12, 8, 16, 16)
    # no CPU fallback; dtype and layout
    with pytest.raises(m.MisplatError, match=r"bilagrid_slice.*cpu"):
        m.bilagrid_slice(rgb, grids, 0)
    with pytest.raises(m.MisplatError, match=r"bilagrid_tv_loss.*cpu"):
        m.bilagrid_tv_loss(grids)
    with pytest.raises(m.MisplatError, match=r"bilagrid_slice: grids must be float32.*float64"):
        m.bilagrid_slice(rgb, grids.double(), 0)
    with pytest.raises(m.MisplatError, match=r"bilagrid_tv_loss: grids must be float32.*float16"):
        m.bilagrid_tv_loss(grids.half())
    with pytest.raises(m.MisplatError, match=r"bilagrid_slice: rgb must be float32.*float64"):
        m.bilagrid_slice(rgb.double(), grids, 0)
    # shapes and indices
    for bad in (torch.rand(6, 8, 4), torch.rand(2, 6, 8, 3), torch.rand(8, 3), torch.rand(1, 1, 6, 8, 3)):
        with pytest.raises(ValueError, match=r"bilagrid_slice: rgb must be \[H, W, 3\]"):
            m.bilagrid_slice(bad, grids, 0)
    with pytest.raises(ValueError, match=r"12 channels.*\(2, 9, 8, 16, 16\)"):
        m.bilagrid_slice(rgb, torch.zeros(2, 9, 8, 16, 16), 0)
    with pytest.raises(ValueError, match=r"bilagrid_tv_loss.*12 channels"):
        m.bilagrid_tv_loss(torch.zeros(2, 9, 8, 16, 16))
    with pytest.raises(ValueError, match=r"grids must be \[num, 12, L, GH, GW\]"):
        m.bilagrid_tv_loss(torch.zeros(12, 8, 16, 16))
    for cam in (-1, 2, 7):
        with pytest.raises(ValueError, match=rf"cam_idx {cam} outside \[0, 2\)"):
            m.bilagrid_slice(rgb, grids, cam)
    with pytest.raises(ValueError, match="host int"):
        m.bilagrid_slice(rgb, grids, torch.tensor(0))
    with pytest.raises(ValueError, match=r"1\.\.256.*\(257, 16\)"):
        m.bilagrid_tv_loss(torch.zeros(1, 12, 8, 16, 257))
    with pytest.raises(ValueError, match=r"1\.\.16.*L = 17"):
        m.bilagrid_slice(rgb, torch.zeros(1, 12, 17, 4, 4), 0)
    with pytest.raises(ValueError, match=r"1\.\.256"):
        m.bilagrid_slice(rgb, torch.zeros(1, 12, 2, 0, 4), 0)
    # (a CPU tensor is refused for its device before its layout is looked at; the layout check itself:)
    from collab_splats_amd import bilagrid

    class _OnGpu(torch.Tensor):
        is_cuda = True

    strided = torch.rand(6, 8, 6)[..., :3].as_subclass(_OnGpu)
    with pytest.raises(m.MisplatError, match=r"bilagrid_slice: rgb must be contiguous.*\(6, 8, 3\)"):
        bilagrid._check_plain("bilagrid_slice", rgb=strided)


def _model(flag: bool, features: bool = False, **kw):
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    sc = random_scene(40, 64, 48, seed=1)
    args = (sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0], sc["sh"][:, 1:])
    if features:
        cfg = radegs.RadegsFeaturesModelConfig(use_bilateral_grid=flag, ssim_lambda=0.0)
        return radegs.RadegsFeaturesModel(cfg, *args, torch.rand(40, 13, generator=torch.Generator().manual_seed(2)), **kw)
    return radegs.RadegsModel(radegs.RadegsModelConfig(use_bilateral_grid=flag, ssim_lambda=0.0), *args, **kw)


GAUSS = {"means", "scales", "quats", "opacities", "features_dc", "features_rest"}


def test_model_wiring_with_the_flag_off_is_unchanged():
    from collab_splats_amd import radegs
    cfg = radegs.RadegsModelConfig()
    assert cfg.use_bilateral_grid is False and cfg.grid_shape == (16, 16, 8)
    assert radegs.RadegsFeaturesModelConfig().use_bilateral_grid is False
    for features in (False, True):
        model = _model(False, features, num_train_data=7)                              # ignored without the flag
        assert not hasattr(model, "bil_grids") and not any("bil_grids" in k for k in model.state_dict())
        assert set(model.get_param_groups()) == GAUSS | ({"distill_features"} if features else set())
    model = _model(False).train()
    rgb = torch.rand(8, 8, 3)
    loss = model.get_loss_dict({"rgb": rgb}, {"image": torch.rand(8, 8, 3)})
    assert set(loss) == {"main_loss", "scale_reg"}


def test_model_wiring_with_the_flag_on():
    import collab_splats_amd as m
    from collab_splats_amd import radegs
    for features in (False, True):
        with pytest.raises(ValueError, match="num_train_data"):
            _model(True, features)
        with pytest.raises(ValueError, match="num_train_data"):
            _model(True, features, num_train_data=0)
        model = _model(True, features, num_train_data=3)
        assert isinstance(model.bil_grids, m.BilateralGrid) and model.bil_grids.grids.shape == (3, 12, 8, 16, 16)
        assert "bil_grids.grids" in model.state_dict()
        groups = model.get_param_groups()
        assert set(groups) == GAUSS | {"bilateral_grid"} | ({"distill_features"} if features else set())
        assert len(groups["bilateral_grid"]) == 1 and groups["bilateral_grid"][0] is model.bil_grids.grids
    cfg = radegs.RadegsModelConfig(use_bilateral_grid=True, grid_shape=(4, 3, 2))
    from collab_splats_amd.synthetic import random_scene
    sc = random_scene(10, 64, 48, seed=1)
    args = (sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0], sc["sh"][:, 1:])
    assert radegs.RadegsModel(cfg, *args, num_train_data=2).bil_grids.grids.shape == (2, 12, 2, 3, 4)
    with pytest.raises(ValueError, match="grid_shape"):
        radegs.RadegsModel(radegs.RadegsModelConfig(use_bilateral_grid=True, grid_shape=(4, 3)), *args, num_train_data=2)
    with pytest.raises(ValueError, match="BilateralGrid"):
        radegs.RadegsModel(radegs.RadegsModelConfig(use_bilateral_grid=True, grid_shape=(4, 3, 40)), *args, num_train_data=2)
    # training: tv_loss is asked of the GPU (no CPU fallback); evaluation: no tv_loss at all
    model = _model(True, num_train_data=3)
    outputs, batch = {"rgb": torch.rand(8, 8, 3)}, {"image": torch.rand(8, 8, 3)}
    with pytest.raises(m.MisplatError, match="bilagrid_tv_loss"):
        model.train().get_loss_dict(outputs, batch)
    assert set(model.eval().get_loss_dict(outputs, batch)) == {"main_loss", "scale_reg"}
