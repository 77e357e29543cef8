"""CPU (no kernel runs): the restatement of the bilateral-grid slice and TV loss (tests/bilagrid_restatement.py) against the
torch composition it restates and against finite differences, the scenes' construction, the fp32 yardstick's own error, and
the argument checks of ``collab_splats_amd.bilagrid`` and of the model wiring; and the launch arithmetic of csrc/bilagrid.hip
restated, from which the regime scenes' reach is asserted."""
import math

import numpy as np
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


@pytest.mark.parametrize("name", S.ALL_SCENES)
def test_every_pixel_is_on_a_border_plane_or_clear_of_the_integers(name):
    sc = S.make(name)
    L = sc["shape"][2]
    low, high, clear = S.gz_classes(sc["rgb"], L)
    assert bool((low | high | clear).all())
    assert sc["num"] >= 2 and not torch.equal(sc["grids"][0], sc["grids"][-1])
    lo, hi = S.RGB_RANGE.get(name, (0.0, 1.0))
    assert float(sc["rgb"].min()) >= lo and float(sc["rgb"].max()) <= hi
    if name in S.RGB_RANGE:                             # colours outside 0..1 on both sides, and pixels beyond both border planes
        assert float(sc["rgb"].min()) < -0.2 and float(sc["rgb"].max()) > 1.2
        raw = R.luma(sc["rgb"]) * (L - 1)
        assert int((raw < 0).sum()) >= 16 and int((raw > L - 1).sum()) >= 16
        assert bool(low[raw < 0].all()) and bool(high[raw > L - 1].all())
    if name in ("saturated", "deep", "split", "max_depth"):
        black, white = (sc["rgb"] == 0).all(-1), (sc["rgb"] == 1).all(-1)
        assert int(black.sum()) >= 12 and int(white.sum()) >= 12
        assert bool(low[black].all()) and bool(high[white].all())
    if name == "flat_z":
        assert bool(low.all())


def test_luma_of_black_and_white_is_exact():
    assert float(R.luma(torch.zeros(1, 1, 3))) == 0.0
    assert float(R.luma(torch.ones(1, 1, 3))) == 1.0


@pytest.mark.parametrize("name", S.ALL_SCENES)
def test_fp64_restatement_equals_the_torch_composition(name):
    sc = S.make(name)
    for cam in S.cameras(name):
        ora = S.oracle(name, cam)
        rgb = sc["rgb"].double().requires_grad_(True)
        grids = sc["grids"].double().requires_grad_(True)
        out = composition(rgb, grids, cam)
        (out * sc["v_out"].double()).sum().backward()
        for key, got in (("out", out), ("v_rgb", rgb.grad), ("v_grids", grids.grad)):
            assert S.rel_err(ora[key], got) <= 1e-12, (name, cam, key, S.rel_err(ora[key], got))


@pytest.mark.parametrize("name", S.ALL_TV_SHAPES)
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


@pytest.mark.parametrize("name", S.ALL_SCENES)
def test_fp32_yardstick_is_well_inside_the_cap(name):
    sc = S.make(name)
    for cam in S.cameras(name):
        ora, y32 = S.oracle(name, cam), S.yardstick(name, cam)
        for key in ("out", "v_rgb", "v_grids"):
            assert y32[key].dtype == torch.float32
            e = S.rel_err(y32[key], ora[key])
            assert e < CAP / MULTIPLE, (name, cam, key, e)
        others = [c for c in range(sc["num"]) if c != cam]
        assert bool((ora["v_grids"][others] == 0).all())


@pytest.mark.parametrize("name", S.ALL_TV_SHAPES)
def test_fp32_tv_yardstick_is_well_inside_the_cap(name):
    ora, y32 = S.tv_oracle(name), S.tv_yardstick(name)
    assert abs(float(y32["loss"]) - float(ora["loss"])) < CAP / MULTIPLE * abs(float(ora["loss"]))
    assert S.rel_err(y32["v_grids"], ora["v_grids"]) < CAP / MULTIPLE


# ---- the launch arithmetic of csrc/bilagrid.hip, restated by hand from its source (nothing is imported from it): if a
# constant there moves, test_regime_scenes_reach_the_regimes_they_name fails and names the scene to resize

K_TILE_W, K_TILE_H = 32, 8                             # kTileW, kTileH
K_STAGE = 4096                                         # kStage
K_LEV = 8                                              # kLev
K_MAX_SPLIT, K_SPLIT_PIXELS = 16, 4096                 # kMaxSplit, kSplitPixels
TV_BLOCKS = 1024                                       # MISPLAT_BILAGRID_TV_BLOCKS
MAX_XY, MAX_L = 256, 16                                # MISPLAT_BILAGRID_MAX_XY, MISPLAT_BILAGRID_MAX_L
F32 = np.float32


def axis_pos(p: int, n: int, g: int):
    """(i0, i1, t) of pixel p of n on a grid axis of g vertices, every operation in fp32."""
    u = F32(p) / F32(n - 1) if n > 1 else F32(0)
    c = min(max(u * F32(g - 1), F32(0)), F32(g - 1))
    f = np.floor(c)
    return int(f), min(int(f) + 1, g - 1), c - f


def support(v: int, n: int, g: int):
    """[lo, hi]: the pixels of an axis that the gather of vertex v visits (a superset of those with a weight)."""
    if g == 1 or n == 1:
        return 0, n - 1
    s = (n - 1) / (g - 1)
    return max(math.floor((v - 1) * s) - 1, 0), min(math.ceil((v + 1) * s) + 1, n - 1)


def split_count(H: int, W: int, GW: int, GH: int) -> int:
    rows = min(H, 2 * (H - 1) // (GH - 1) + 3) if GH > 1 else H
    cols = min(W, 2 * (W - 1) // (GW - 1) + 3) if GW > 1 else W
    s = -(-rows * cols // K_SPLIT_PIXELS)
    return max(min(s, K_MAX_SPLIT, rows), 1)


def stage_sizes(H: int, W: int, shape):
    """n_stage of every workgroup of the slice kernels; a workgroup stages its columns in LDS iff n_stage <= kStage."""
    GW, GH, L = shape
    out = []
    for by in range(0, H, K_TILE_H):
        for bx in range(0, W, K_TILE_W):
            nx = axis_pos(min(bx + K_TILE_W, W) - 1, W, GW)[1] - axis_pos(bx, W, GW)[0] + 1
            ny = axis_pos(min(by + K_TILE_H, H) - 1, H, GH)[1] - axis_pos(by, H, GH)[0] + 1
            out.append(nx * ny * L * 12)
    return out


def slice_rows(H: int, W: int, shape):
    """{vy: rows of each of the n_split row slices of a column of grid row vy} in the grid-side backward (0: empty)."""
    GW, GH, _ = shape
    n_split = split_count(H, W, GW, GH)
    out = {}
    for vy in range(GH):
        r0, r1 = support(vy, H, GH)
        per = (r1 - r0 + 1 + n_split - 1) // n_split
        out[vy] = [max(min(r1, r0 + s * per + per - 1) - (r0 + s * per) + 1, 0) for s in range(n_split)]
    return out


def weighted_vertices(n: int, g: int):
    """The vertices of a grid axis that some pixel gives a non-zero weight."""
    hit = set()
    for p in range(n):
        i0, i1, t = axis_pos(p, n, g)
        hit.add(i0)
        if t > 0:
            hit.add(i1)
    return hit


def level_chunks(L: int) -> int:
    return (L + K_LEV - 1) // K_LEV


def stream_blocks(total: int) -> int:
    return max(1, min((total + 255) // 256, TV_BLOCKS))


def trips(total: int, doubled: bool) -> int:
    """Trips of a grid-stride loop over ``total`` elements: tv_fwd_kernel launches stream_blocks workgroups of 256,
    tv_bwd_kernel and grid_bwd_finish_kernel twice as many."""
    lanes = stream_blocks(total) * (2 if doubled else 1) * 256
    return -(-total // lanes)


def regimes(name: str):
    if name in S.SCENES:
        (H, W), shape, num, _ = S.SCENES[name]
    else:
        (H, W), shape, num = S.REGIME_SCENES[name][:3]
    GW, GH, L = shape
    rows = slice_rows(H, W, shape)
    return {"finish_total": 12 * L * GH * GW * num, "finish_trips": trips(12 * L * GH * GW * num, True),
            "max_stage": max(stage_sizes(H, W, shape)), "columns": GW * GH, "n_split": split_count(H, W, GW, GH),
            "empty_slices": {vy: sum(1 for r in v if r == 0) for vy, v in rows.items()}, "chunks": level_chunks(L),
            "weighted_columns": len(weighted_vertices(W, GW)) * len(weighted_vertices(H, GH)), "num": num, "HW": (H, W), "L": L}


def tv_regimes(name: str):
    num, shape = S.TV_SHAPES[name] if name in S.TV_SHAPES else S.REGIME_TV_SHAPES[name][:2]
    total = 12 * shape[2] * shape[1] * shape[0] * num
    return {"total": total, "wanted": (total + 255) // 256, "partials": stream_blocks(total), "fwd_trips": trips(total, False),
            "bwd_trips": trips(total, True)}


def test_launch_arithmetic_restatement_on_known_values():
    """The restated helpers on values worked out by hand from the kernel's formulas."""
    assert axis_pos(0, 1, 16) == (0, 1, 0) and axis_pos(10, 11, 256)[:2] == (255, 255) and axis_pos(7, 9, 256)[:2] == (223, 224)
    assert support(0, 43, 3) == (0, 22) and support(1, 43, 3) == (0, 42) and support(2, 43, 3) == (20, 42)
    assert support(5, 1, 16) == (0, 0) and support(0, 9, 1) == (0, 8)
    assert split_count(150, 420, 4, 3) == 11 and split_count(43, 1000, 2, 3) == 11 and split_count(1080, 1920, 16, 16) == 10
    assert split_count(1, 1, 16, 16) == 1 and split_count(9, 11, 256, 256) == 1
    assert stream_blocks(1) == 1 and stream_blocks(256 * 1024 + 1) == 1024 and level_chunks(8) == 1 and level_chunks(9) == 2
    # the reference's 300 training cameras at the default grid: 28 full trips and a ragged one forward, 14 and one in
    # the two doubled kernels
    assert trips(300 * 12 * 8 * 16 * 16, False) == 29 and trips(300 * 12 * 8 * 16 * 16, True) == 15


def test_regime_scenes_reach_the_regimes_they_name():
    """What each regime scene is there for, from the launch arithmetic above -- and that no scene of ``SCENES`` /
    ``TV_SHAPES`` reached it.  A failure after a constant of csrc/bilagrid.hip moved names the scene to resize."""
    old = {name: regimes(name) for name in S.SCENES}
    new = {name: regimes(name) for name in S.REGIME_SCENES}
    old_tv = {name: tv_regimes(name) for name in S.TV_SHAPES}
    new_tv = {name: tv_regimes(name) for name in S.REGIME_TV_SHAPES}
    # many_cams: a second trip of grid_bwd_finish_kernel, a camera that is neither the first nor the last, 22 zeroed slices
    r = new["many_cams"]
    assert r["finish_total"] == 565248 > 2 * TV_BLOCKS * 256 and r["finish_trips"] == 2, r
    assert r["num"] == 23 and S.cameras("many_cams") == (0, 11, 22)
    assert all(o["finish_trips"] == 1 and o["num"] <= 3 for o in old.values())
    assert all(set(S.cameras(n)) <= {0, o["num"] - 1} for n, o in old.items())
    # max_grid: both sides at MISPLAT_BILAGRID_MAX_XY; an unstaged workgroup far above kStage, 65 536 columns of which most
    # carry no weight, three trips of the finish kernel
    r = new["max_grid"]
    assert S.REGIME_SCENES["max_grid"][1][:2] == (MAX_XY, MAX_XY) and r["columns"] == 65536
    assert r["max_stage"] == 691200 > 100 * K_STAGE and r["weighted_columns"] * 100 < r["columns"], r
    assert r["finish_total"] == 1572864 and r["finish_trips"] == 3
    assert all(o["max_stage"] <= 8 * K_STAGE and o["columns"] <= 256 for o in old.values())
    # empty_slices: 11 row slices, the last three of a border vertex's 23-row support empty; the middle vertex has none
    r = new["empty_slices"]
    assert r["n_split"] == 11 and r["empty_slices"] == {0: 3, 1: 0, 2: 3}, r
    assert slice_rows(43, 1000, (2, 3, 2))[0] == [3] * 7 + [2, 0, 0, 0]
    assert all(sum(o["empty_slices"].values()) == 0 for o in old.values())
    assert old["split"]["n_split"] == 11                                               # (the scene the issue compares with)
    # max_depth: L = MISPLAT_BILAGRID_MAX_L, two FULL level chunks
    r = new["max_depth"]
    assert r["L"] == MAX_L == 2 * K_LEV and r["chunks"] == 2
    assert all(o["L"] < MAX_L and (o["chunks"] == 1 or o["L"] % K_LEV != 0) for o in old.values())
    # one_pixel: both image sides 1 at once
    assert new["one_pixel"]["HW"] == (1, 1) and all(o["HW"] != (1, 1) for o in old.values())
    # beyond: the only scene with colours outside 0..1 (the counts are asserted with the scene's construction)
    assert set(S.RGB_RANGE) == {"beyond"} and "beyond" in new
    # TV cams_11: more workgroups wanted than the cap, so tv_finish_kernel reads all 1024 partials; a ragged second trip
    t = new_tv["cams_11"]
    assert t["wanted"] == 1056 > TV_BLOCKS == t["partials"] and t["fwd_trips"] == 2 and t["bwd_trips"] == 1, t
    assert 0 < t["total"] - TV_BLOCKS * 256 < TV_BLOCKS * 256
    # cams_45: 4.2 trips forward, 2.1 backward;  wide: 6 and 3 at the longest row
    t = new_tv["cams_45"]
    assert (t["fwd_trips"], t["bwd_trips"]) == (5, 3) and t["total"] % (TV_BLOCKS * 256) != 0, t
    t = new_tv["wide"]
    assert (t["fwd_trips"], t["bwd_trips"]) == (6, 3) and S.REGIME_TV_SHAPES["wide"][1][:2] == (MAX_XY, MAX_XY), t
    assert all(o["fwd_trips"] == 1 and o["bwd_trips"] == 1 and o["partials"] < TV_BLOCKS for o in old_tv.values())


@pytest.mark.parametrize("name", ["blocks", "saturated", "one_row", "one_col", "flat_z", "one_pixel", "max_depth", "beyond"])
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
