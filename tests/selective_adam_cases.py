"""Seeded single-step cases for the row-selective Adam tests (test infrastructure), in the style of tests/adam_cases.py.

A case is the six Gaussian groups of ``n`` rows -- means [n, 3], features_dc [n, 3], features_rest [n, 15, 3], opacities
[n, 1], scales [n, 3], quats [n, 4]: 59 floats per row -- with the reference's learning rates, ``eps = 1e-15`` and a
consistent injected state of step t - 1 (``exp_avg_sq = s^2``, ``exp_avg = a s``, |a| <= 1).  Per element about a third is
never touched (s = 0, g = 0), a sixth idle (g = 0, s > 0), the rest has a gradient; the first and the last element of every
tensor always have one.  Gradients and s span 1e-6 .. 1, parameters have the standard deviation ``P_SPREAD`` x lr.

The masks of a size are named; ``masks(n)`` leaves out those a size cannot hold (rows 2047 and 2048 below 2 049 rows, the
random masks -- row 0 forced on and the last row forced off, so neither set is empty -- at one row)."""
import functools

import torch

import adam_cases as A
import adam_restatement as R
import selective_adam_restatement as S

EPS = A.EPS
BETAS = A.BETAS
OTHER_BETAS = A.OTHER_BETAS
NAMES = ("means", "features_dc", "features_rest", "opacities", "scales", "quats")
ROW_SHAPES = ((3,), (3,), (15, 3), (1,), (3,), (4,))
WIDTHS = (3, 3, 45, 1, 3, 4)
LRS = A.LRS[:6]
# one row; a bitmap tail that is no multiple of 8; one wave; both sides of the 2 048-row bitmap block; several blocks
SIZES = (1, 7, 64, 2047, 2048, 2049, 10007)
STEPS = {"t1": (1,), "t1000": (1000,), "mixed": (1, 1000)}
CASES = [(n, s) for n in SIZES for s in ("t1", "t1000")] + [(2049, "mixed")]
MASKS = ("none", "all", "first", "last", "alternating", "rows_2047_2048", "random_2", "random_50")


def tensors(seed: int, shapes, lrs, steps, betas=(BETAS,)):
    """[{"p", "g", "m", "v", "untouched", "idle", "lr", "t", "betas"}], one per shape (the recipe of ``adam_cases.make``)."""
    out = []
    for i, shape in enumerate(shapes):
        g = torch.Generator().manual_seed(seed * 100 + i)
        n = 1
        for d in shape:
            n *= d
        u = torch.rand(n, generator=g)
        if n:
            u[0] = u[-1] = 1.0
        untouched, idle = u < 1 / 3, (u >= 1 / 3) & (u < 1 / 2)
        s = (0.1 + torch.randn(n, generator=g).abs()) * A._decades(n, g)
        a = 2 * torch.rand(n, generator=g) - 1
        grad = torch.randn(n, generator=g) * A._decades(n, g)
        s[untouched] = 0.0
        grad[untouched | idle] = 0.0
        lr = lrs[i % len(lrs)]
        p = torch.randn(n, generator=g) * (A.P_SPREAD * lr)
        t = {"p": p, "g": grad, "m": a * s, "v": s * s, "untouched": untouched, "idle": idle}
        out.append({**{k: x.view(shape).contiguous() for k, x in t.items()}, "lr": lr, "t": steps[i % len(steps)],
                    "betas": betas[i % len(betas)]})
    return out


@functools.lru_cache(maxsize=None)
def make(n: int, steps: str = "t1000"):
    """The six groups of ``n`` rows at the step counts ``STEPS[steps]``."""
    return tensors(4200 + 17 * n + list(STEPS).index(steps), [(n,) + r for r in ROW_SHAPES], LRS, STEPS[steps])


@functools.lru_cache(maxsize=None)
def masks(n: int):
    """{name: [n] bool} of the masks a size can hold."""
    rows = torch.arange(n)
    out = {"none": torch.zeros(n, dtype=torch.bool), "all": torch.ones(n, dtype=torch.bool), "first": rows == 0,
           "last": rows == n - 1, "alternating": rows % 2 == 0}
    if n >= 2049:
        out["rows_2047_2048"] = (rows == 2047) | (rows == 2048)
    if n >= 2:
        for name, density in (("random_2", 0.02), ("random_50", 0.5)):
            m = torch.rand(n, generator=torch.Generator().manual_seed(9000 + n + int(100 * density))) < density
            m[0], m[-1] = True, False
            out[name] = m
    return out


def _run(n: int, steps: str, step, dtype):
    return [dict(zip(("p", "m", "v"), step(c["p"], c["g"], c["m"], c["v"], c["lr"], *c["betas"], EPS, c["t"], dtype)))
            for c in make(n, steps)]


@functools.lru_cache(maxsize=None)
def oracle(n: int, steps: str):
    """The fp64 restatement of the DENSE step of every tensor: computed once, shared, never written to."""
    return _run(n, steps, R.adam_step, torch.float64)


@functools.lru_cache(maxsize=None)
def yardstick(n: int, steps: str):
    """``torch.optim.Adam`` in fp32 on the CPU on the same (dense)."""
    return _run(n, steps, R.torch_adam_step, torch.float32)


def under_mask(dense, cases, mask):
    """A dense result restricted to the rows of ``mask``: the other rows are the inputs, in the result's dtype."""
    out = []
    for res, c in zip(dense, cases):
        rows = mask.view(-1, *([1] * (c["p"].dim() - 1)))
        out.append({k: torch.where(rows, res[k], c[k].to(res[k].dtype)) for k in ("p", "m", "v")})
    return out


def masked_oracle(n: int, steps: str, mask):
    """The fp64 restatement under a row mask (``selective_adam_restatement.selective_adam_step`` of every tensor)."""
    return [dict(zip(("p", "m", "v"), S.selective_adam_step(c["p"], c["g"], c["m"], c["v"], mask, c["lr"], *c["betas"], EPS,
                                                            c["t"], torch.float64))) for c in make(n, steps)]
