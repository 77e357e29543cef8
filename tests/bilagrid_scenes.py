"""Seeded scenes for the bilateral-grid tests (test infrastructure).  Every scene has ``num >= 2`` cameras with DIFFERENT
non-identity grids (the identity plus noise of about 0.1), so a wrong camera index or a swapped axis shows up; an image ``rgb``
in 0..1 and an upstream gradient ``v_out``.  Pixel values are chosen so that every pixel's gz = z (L - 1) is exactly 0,
exactly L - 1, or farther than ``GZ_MARGIN`` from any integer (``gz_classes``; asserted for all scenes in
test_bilagrid_host.py): no arithmetic then picks another interval than the restatement's, and no pixel is left out of any
comparison."""
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
    (H, W), shape, num, patches = SCENES[name]
    g = torch.Generator().manual_seed(2400 + sorted(SCENES).index(name))
    L = shape[2]
    rgb = torch.rand(H, W, 3, generator=g)
    for k in range(patches):                           # exact black and exact white, alternating
        y, x = int(torch.randint(0, max(H - 3, 1), (1,), generator=g)), int(torch.randint(0, max(W - 4, 1), (1,), generator=g))
        rgb[y:y + 3, x:x + 4] = float(k % 2)
    for _ in range(64):                                # re-draw the pixels whose gz lies within the margin of an integer
        low, high, clear = gz_classes(rgb, L)
        bad = ~(low | high | clear)
        if not bool(bad.any()):
            break
        rgb[bad] = torch.rand(int(bad.sum()), 3, generator=g)
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
    num, shape = TV_SHAPES[name]
    return make_grids(num, shape, torch.Generator().manual_seed(2450 + sorted(TV_SHAPES).index(name)))


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
