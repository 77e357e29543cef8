"""Seeded scenes of the feature-loss tests.  Every value is drawn in float32 (so the fp64 oracle, the fp32 yardstick and the GPU
see the same numbers).  Every scene gives one ground-truth pixel of each branch the value all-zero (the data manager emits
such pixels on purpose), and ``ZERO_PREACT`` scenes also hold exact zeros among the hidden pre-activations: a block of
``features`` is zero, so x = 0 on the main-map pixels whose four taps lie inside it, and ``b_hidden`` is zero for a few hidden
units -- there w x + b == 0 exactly, whatever the order of the arithmetic (the relu's subgradient at 0).  ``SCENES`` are the
scenes the kernels were written against; ``LAUNCH_SCENES`` reach the launch regimes those never enter."""
import functools

import torch

import featureloss_restatement as R

# name: (render H, W), L, Hd, main (C, H, W), other branches
SCENES = {
    "down_int": ((45, 80), 13, 64, (40, 9, 16), [(24, 7, 11)]),
    "branch_up": ((45, 80), 13, 64, (40, 9, 16), [(24, 20, 33)]),
    "same_dims": ((30, 30), 13, 64, (8, 4, 4), [(8, 4, 4)]),
    "enlarge": ((6, 10), 13, 64, (16, 12, 21), []),
    "wide": ((20, 20), 13, 64, (768, 4, 4), [(384, 3, 5)]),
    "odd_dims": ((17, 23), 5, 33, (67, 5, 7), [(1, 5, 7), (130, 2, 3)]),
    "dead": ((12, 12), 13, 64, (16, 4, 4), []),
}
ZERO_PREACT = ("down_int", "same_dims", "wide", "odd_dims")

# The launch regimes SCENES never reaches (csrc/featloss.hip ``make_plan``: channel splits S, pixel splits PS of the
# weight-gradient kernel, the Hd == 64 switch, the passes / chunks of 64 hidden units of an Hd above 64, kMaxBranch).  Same
# columns, then the seed; tests/test_featureloss_host.py asserts the regime of every row.
LAUNCH_SCENES = {
    # exact-grid scenes (EXACT_GRID): thousands of pixels, pre-activations exact in fp32
    "pixel_splits": ((33, 67), 13, 64, (16, 33, 67), [(8, 50, 62)], 2001),           # PS 2 (5 + 4 tiles, ragged last) and 3
    "split_cap": ((66, 135), 13, 64, (4, 132, 135), [], 2002),                        # PS 16 (the cap), C < 16, rows x 2
    "hidden_256_split": ((33, 67), 32, 256, (272, 33, 67), [(130, 12, 9)], 2003),     # L 32, Hd 256: 4 chunks, S 2, PS 2
    "hidden_200_split": ((33, 67), 5, 200, (24, 33, 67), [(40, 57, 60)], 2004),       # ragged last chunk, PS 2 and 3
    # random scenes, drawn as SCENES are
    "hidden_65": ((17, 23), 13, 65, (40, 9, 16), [(24, 7, 11)], 2015),                # a second pass of one hidden unit
    "hidden_200": ((17, 23), 13, 200, (40, 9, 16), [(24, 20, 33)], 2016),             # ragged chunk, an enlarging branch
    "hidden_1": ((9, 7), 1, 1, (3, 4, 5), [(17, 6, 3)], 2007),                        # both lower limits
    "channel_cap": ((12, 12), 13, 64, (1160, 3, 5), [(2064, 2, 3)], 2008),            # S 8 (the cap), 73 and 129 units
    "four_branches": ((21, 37), 7, 48, (20, 10, 19), [(33, 10, 19), (5, 23, 8), (300, 4, 40)], 2019),   # kMaxBranch
    "mixed_axes": ((50, 6), 13, 64, (16, 7, 31), [(16, 29, 4)], 2010),                # one axis each way, both resizes
}
# Exact-grid scenes: ``features`` are multiples of 2^-4 in [-4, 4], ``w_hidden`` / ``b_hidden`` multiples of 2^-8 in [-1, 1],
# and the render has the main map's size (taps exactly (1, 0)) or half of it along an axis (taps 1/4, 3/4).  Every product is
# then a multiple of 2^-14 at the least and every partial sum is below 2^8: w x + b is exact in fp32 in any order, with or
# without fma.  With plain random inputs some of 10^5 .. 10^6 pre-activations land within fp32 rounding of zero, the fp32 and
# fp64 restatements disagree on that relu, and the yardstick's own gradient error is 1e-3 .. 6e-2: a bound built on it
# means nothing.  Here the two agree bit for bit, and the pre-activations that are exact zeros (a corner of ``features`` and two
# entries of ``b_hidden`` are zero, and a few more fall on zero by chance) are zeros on both sides.
EXACT_GRID = ("pixel_splits", "split_cap", "hidden_256_split", "hidden_200_split")
# Random launch scenes: the seed is chosen so that every non-zero fp64 pre-activation is at least PREACT_MARGIN times the
# largest one, so fp32 in any order lands on the same side of the relu (asserted in the host test).
PREACT_MARGIN = 2.0 ** -18
ALL_SCENES = {**{k: v + (None,) for k, v in SCENES.items()}, **LAUNCH_SCENES}
MAIN = "main"
ZERO_GT_PIXEL = (1, 2)                                  # (row, column) of the all-zero ground-truth pixel, every branch


def branch_names(n_other: int):
    return [MAIN] + [f"aux{i}" for i in range(n_other)]


@functools.lru_cache(maxsize=None)
def make(name: str):
    (H, W), L, Hd, main_dims, others, seed = ALL_SCENES[name]
    g = torch.Generator().manual_seed(1000 + sorted(SCENES).index(name) if seed is None else seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)                 # noqa: E731
    names = branch_names(len(others))
    dims = dict(zip(names, [main_dims] + list(others)))
    features = rn(H, W, L)
    w_hidden, b_hidden = rn(Hd, L) / L ** 0.5, 0.3 * rn(Hd)
    branches = {n: (rn(d[0], Hd) / Hd ** 0.5, 0.1 * rn(d[0])) for n, d in dims.items()}
    gt = {n: rn(*d) for n, d in dims.items()}
    for t in gt.values():
        t[:, ZERO_GT_PIXEL[0], ZERO_GT_PIXEL[1]] = 0.0
    if name in ZERO_PREACT:
        features[: (H * 2) // 3, : (W * 2) // 3] = 0.0
        b_hidden[: max(Hd // 8, 2)] = 0.0
    if name in EXACT_GRID:
        ri = lambda k, *s: torch.randint(-k, k + 1, s, generator=g).to(torch.float32)    # noqa: E731
        features = ri(64, H, W, L) / 16.0
        w_hidden, b_hidden = ri(256, Hd, L) / 256.0, ri(256, Hd) / 256.0
        # exact zeros by construction as well as by chance, as in ZERO_PREACT: x = 0 in a corner, b = 0 for two hidden units
        features[: H // 4, : W // 4] = 0.0
        b_hidden[:2] = 0.0
    if name == "dead":
        w_hidden.zero_()
        b_hidden.fill_(-1.0)
        branches = {n: (w, torch.zeros_like(b)) for n, (w, b) in branches.items()}
    return {"name": name, "features": features, "w_hidden": w_hidden, "b_hidden": b_hidden, "branches": branches, "gt": gt,
            "dims": dims, "main": MAIN, "regularization_lambda": 0.1, "loss_lambda": 1e-3}


@functools.lru_cache(maxsize=None)
def oracle(name: str):
    """The fp64 restatement of a scene: computed once, shared by the tests, never written to."""
    return R.run(make(name), torch.float64)


@functools.lru_cache(maxsize=None)
def yardstick(name: str):
    """The fp32 restatement of the same scene."""
    return R.run(make(name), torch.float32)


def rel_err(a: torch.Tensor, ref: torch.Tensor, top: float = None) -> float:
    """max |a - ref| / max |ref| over the whole tensor (0 where both are all zero; inf where only the reference is).
    ``top``: another denominator (see ``grad_err``)."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    diff, top = float((a - ref).abs().max()), float(ref.abs().max()) if top is None else top
    if not (diff == diff):
        return float("inf")
    if top == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / top


def preactivations(name: str, dtype) -> torch.Tensor:
    """The hidden pre-activations w_hidden x + b_hidden of a scene, [Hd, H_main, W_main], as the restatement forms them."""
    sc = make(name)
    x = R.bilinear(sc["features"].to(dtype).permute(2, 0, 1), sc["dims"][MAIN][1:])
    return torch.einsum("jl,lyx->jyx", sc["w_hidden"].to(dtype), x) + sc["b_hidden"].to(dtype)[:, None, None]


def zero_preactivations(name: str) -> int:
    """How many hidden pre-activations of the scene are exactly zero (fp64)."""
    return int((preactivations(name, torch.float64) == 0).sum())


def grad_err(got: torch.Tensor, ora_grads: dict, key: str) -> float:
    """The error measure of one gradient tensor against the oracle's.  A branch of ONE channel has cos = sign(p g), a constant,
    so the gradients of its own ``w_out`` / ``b_out`` are analytically zero: every arithmetic returns the rounding residue of two
    cancelling sums (1e-21 in the fp64 oracle, 1e-12 in fp32), and a ratio against the oracle's own residue measures nothing.
    Such a tensor -- its oracle below 2^-40 of the scene's largest gradient of the same kind -- is measured against that
    largest gradient instead; every entry still counts.  An oracle that is exactly zero keeps the exact comparison."""
    ref = ora_grads[key]
    top = float(ref.abs().max())
    kind = key.split(".")[0]
    sib = max(float(v.abs().max()) for k, v in ora_grads.items() if k.split(".")[0] == kind)
    return rel_err(got, ref, sib if 0.0 < top < 2.0 ** -40 * sib else None)
