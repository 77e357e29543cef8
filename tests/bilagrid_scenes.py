"""Seeded scenes for the bilateral-grid tests (test infrastructure).  Every scene has ``num >= 2`` cameras with DIFFERENT
non-identity grids (the identity plus noise of about 0.1), so a wrong camera index or a swapped axis shows up; an image ``rgb``
in 0..1 and an upstream gradient ``v_out``.  Pixel values are chosen so that every pixel's gz = z (L - 1) is exactly 0,
exactly L - 1, or farther than ``GZ_MARGIN`` from any integer (``gz_classes``; asserted for all scenes in
test_bilagrid_host.py): no arithmetic then picks another interval than the restatement's, and no pixel is left out of any
comparison.

``SCENES`` / ``TV_SHAPES`` are seeded from their position in the sorted dict, so a name added there would re-seed the rest:
the scenes for the launch regimes a training run reaches live in ``REGIME_SCENES`` / ``REGIME_TV_SHAPES`` with a seed of
their own each (what each one reaches is asserted from the launch arithmetic in test_bilagrid_host.py)."""
import functools

import torch

import bilagrid_restatement as R

GZ_MARGIN = 1e-3

# name: (H, W), (GW, GH, L), num, number of saturated patches
SCENES = {
    "tiny": ((5, 7), (16, 16, 8), 2, 0),              # more grid columns than pixels: most columns have an empty support
    "one_row": ((1, 33), (16, 16, 8), 2, 0),          # H - 1 == 0
    "one_col": ((19, 1), (16, 16, 8), 2, 0),          # W - 1 == 0
    "odd": ((37, 53), (4, 3, 2), 3, 0),               # three different sizes, none the default
    "blocks": ((70, 130), (16, 16, 8), 2, 0),         # several cells, workgroup edges in both axes
    "flat_z": ((21, 30), (5, 4, 1), 2, 0),            # L == 1: the z-gradient is identically 0
    "saturated": ((24, 40), (16, 16, 8), 2, 6),       # patches of exact black and exact white: the border rule
    # beyond the stated list: the launch regimes of csrc/bilagrid.hip those do not reach
    "deep": ((20, 24), (3, 2, 11), 2, 2),             # L > 8: two level chunks in the grid-side backward
    "split": ((150, 420), (4, 3, 2), 2, 3),           # a support of > 4096 pixels: row slices met by the second pass
}
STATED = ("tiny", "one_row", "one_col", "odd", "blocks", "flat_z", "saturated")
TV_SHAPES = {                                          # name: num, (GW, GH, L)
    "default_1": (1, (16, 16, 8)), "default_3": (3, (16, 16, 8)), "odd_1": (1, (4, 3, 2)), "odd_3": (3, (4, 3, 2)),
    "flat_1": (1, (5, 4, 1)), "flat_3": (3, (5, 1, 6)),
}

# name: (H, W), (GW, GH, L), num, number of saturated patches, seed, cameras to run
REGIME_SCENES = {
    "many_cams": ((24, 40), (16, 16, 8), 23, 0, 2471, (0, 11, 22)),   # the finish kernel's second trip, a middle camera
    "max_grid": ((9, 11), (256, 256, 1), 2, 0, 2472, (0, 1)),         # 65 536 columns, unstaged far above kStage, 3 trips
    "empty_slices": ((43, 1000), (2, 3, 2), 2, 0, 2473, (0, 1)),      # 11 row slices, 3 of them empty at the border vertices
    "max_depth": ((64, 96), (6, 5, 16), 2, 4, 2474, (0, 1)),          # L = 16: two full level chunks; white reaches level 15
    "one_pixel": ((1, 1), (16, 16, 8), 2, 0, 2475, (0, 1)),           # H - 1 == W - 1 == 0
    "beyond": ((24, 40), (5, 4, 4), 2, 0, 2476, (0, 1)),              # colours from RGB_RANGE: below and above the grid
}
RGB_RANGE = {"beyond": (-0.25, 1.25)}                  # every other scene draws from 0..1
REGIME_TV_SHAPES = {                                   # name: num, (GW, GH, L), seed
    "cams_11": (11, (16, 16, 8), 2481),                # 1056 workgroups wanted: the cap, a ragged second trip, 1024 partials
    "cams_45": (45, (16, 16, 8), 2482),                # 4.2 trips forward, 2.1 backward
    "wide": (1, (256, 256, 2), 2483),                  # 6 trips at the longest row
}
ALL_SCENES = list(SCENES) + list(REGIME_SCENES)
ALL_TV_SHAPES = list(TV_SHAPES) + list(REGIME_TV_SHAPES)


def cameras(name: str):
    """The cameras the tests run of a scene: the first and the last, and for a regime scene the ones it lists."""
    return REGIME_SCENES[name][5] if name in REGIME_SCENES else (0, SCENES[name][2] - 1)


def make_grids(num: int, shape, g: torch.Generator) -> torch.Tensor:
    GW, GH, L = shape
    eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]).view(1, 12, 1, 1, 1)
    return (eye + 0.1 * torch.randn(num, 12, L, GH, GW, generator=g)).contiguous()


def gz_classes(rgb: torch.Tensor, L: int):
    """(exactly 0, exactly L - 1, clear of every integer by GZ_MARGIN) per pixel, from the fp32 luma."""
    gz = (R.luma(rgb, torch.float32) * (L - 1)).clamp(0, L - 1).double()
    low, high = gz == 0, gz == L - 1
    clear = (gz - gz.round()).abs() > GZ_MARGIN
    return low, high, clear


@functools.lru_cache(maxsize=None)
def make(name: str):
    if name in SCENES:
        (H, W), shape, num, patches = SCENES[name]
        seed = 2400 + sorted(SCENES).index(name)
    else:
        (H, W), shape, num, patches, seed, _ = REGIME_SCENES[name]
    g = torch.Generator().manual_seed(seed)
    L = shape[2]
    lo, hi = RGB_RANGE.get(name, (0.0, 1.0))

    def draw(*size):
        u = torch.rand(*size, generator=g)
        return u if name not in RGB_RANGE else lo + (hi - lo) * u

    rgb = draw(H, W, 3)
    for k in range(patches):                           # exact black and exact white, alternating
        y, x = int(torch.randint(0, max(H - 3, 1), (1,), generator=g)), int(torch.randint(0, max(W - 4, 1), (1,), generator=g))
        rgb[y:y + 3, x:x + 4] = float(k % 2)
    for _ in range(64):                                # re-draw the pixels whose gz lies within the margin of an integer
        low, high, clear = gz_classes(rgb, L)
        bad = ~(low | high | clear)
        if not bool(bad.any()):
            break
        rgb[bad] = draw(int(bad.sum()), 3)
    return {"rgb": rgb.contiguous(), "grids": make_grids(num, shape, g), "v_out": torch.randn(H, W, 3, generator=g),
            "shape": shape, "num": num}


@functools.lru_cache(maxsize=None)
def oracle(name: str, cam: int):
    """The fp64 restatement of a scene for one camera: computed once, shared by the tests, never written to."""
    sc = make(name)
    return R.run_slice(sc["rgb"], sc["grids"], sc["v_out"], cam, torch.float64)


@functools.lru_cache(maxsize=None)
def yardstick(name: str, cam: int):
    """The fp32 restatement of the same."""
    sc = make(name)
    return R.run_slice(sc["rgb"], sc["grids"], sc["v_out"], cam, torch.float32)


@functools.lru_cache(maxsize=None)
def tv_grids(name: str) -> torch.Tensor:
    if name in TV_SHAPES:
        num, shape = TV_SHAPES[name]
        seed = 2450 + sorted(TV_SHAPES).index(name)
    else:
        num, shape, seed = REGIME_TV_SHAPES[name]
    return make_grids(num, shape, torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def tv_oracle(name: str):
    return R.run_tv(tv_grids(name), torch.float64)


@functools.lru_cache(maxsize=None)
def tv_yardstick(name: str):
    return R.run_tv(tv_grids(name), torch.float32)


def rel_err(a: torch.Tensor, ref: torch.Tensor) -> float:
    """max |a - ref| / max |ref| over the whole tensor (0 where both are all zero; inf where only the reference is)."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    diff, top = float((a - ref).abs().max()), float(ref.abs().max())
    if not (diff == diff):
        return float("inf")
    if top == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / top
