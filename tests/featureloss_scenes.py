"""Seeded scenes of the feature-loss tests.  Every value is drawn in float32 (so the fp64 oracle, the fp32 yardstick and the GPU
see the same numbers).  Every scene gives one ground-truth pixel of each branch the value all-zero (the data manager emits
such pixels on purpose), and ``ZERO_PREACT`` scenes also hold exact zeros among the hidden pre-activations: a block of
``features`` is zero, so x = 0 on the main-map pixels whose four taps lie inside it, and ``b_hidden`` is zero for a few hidden
units -- there w x + b == 0 exactly, whatever the order of the arithmetic (the relu's subgradient at 0)."""
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
MAIN = "main"
ZERO_GT_PIXEL = (1, 2)                                  # (row, column) of the all-zero ground-truth pixel, every branch


def branch_names(n_other: int):
    return [MAIN] + [f"aux{i}" for i in range(n_other)]


@functools.lru_cache(maxsize=None)
def make(name: str):
    (H, W), L, Hd, main_dims, others = SCENES[name]
    g = torch.Generator().manual_seed(1000 + sorted(SCENES).index(name))
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


def zero_preactivations(name: str) -> int:
    """How many hidden pre-activations of the scene are exactly zero (fp64)."""
    sc = make(name)
    x = R.bilinear(sc["features"].double().permute(2, 0, 1), sc["dims"][MAIN][1:])
    pre = torch.einsum("jl,lyx->jyx", sc["w_hidden"].double(), x) + sc["b_hidden"].double()[:, None, None]
    return int((pre == 0).sum())


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
