"""Seeded single-step cases for the fused-Adam tests (test infrastructure).  A case is a list of tensors that go into ONE
``step_all``; each tensor has its own learning rate, step count t and betas, and a consistent injected state of step t - 1:

    exp_avg_sq = s^2,  exp_avg = a s   with s >= 0 and |a| <= 1

(a second moment of 0 under a first moment that is not 0 cannot arise in training, and at eps = 1e-15 it gives updates of
1e9: it is never generated, which test_adam_host.py asserts).  Per element: about a third has s = 0 and g = 0 (never touched:
a Gaussian no view has reached yet, another camera's grid), a sixth has g = 0 with s > 0 (touched earlier, not now: the
moments decay and p still moves), the rest has a gradient; the first and the last element of every tensor always have one, so
that a dropped head or tail element of even the 1-element tensor shows.  Gradients and s span 1e-6 .. 1 element by element.
Parameters have the standard deviation ``P_SPREAD`` x lr of their tensor, so a one-step update stands above the rounding of
the parameter (the yardstick's update error is asserted in test_adam_host.py)."""
import functools

import torch

import adam_restatement as R

EPS = 1e-15                                            # the reference's, every group
P_SPREAD = 16.0
BETAS = (0.9, 0.999)
OTHER_BETAS = (0.8, 0.99)
# the reference's six groups (means, features_dc, features_rest, opacities, scales, quats) and the means at the end of their
# schedule
LRS = (1.6e-4, 0.0025, 0.0025 / 20, 0.05, 0.005, 0.001, 1.6e-6)
# exactly MISPLAT_ADAM_MAX_TENSORS = 8 tensors, the empty one in the middle: 1, 3 (scalar tail only), 4 (one float4), 5, one
# block of 2048 less one, exactly, plus one
EIGHT = ((1,), (3,), (4,), (5,), (0,), (2047,), (2048,), (2049,))
# more than 8: _launch cuts the list into a launch of 8 and one of 2
TEN = ((4097,), (10007, 3), (7,), (64,), (255,), (256,), (257,), (1000,), (12,), (2050,))
FOUR = ((5,), (2049,), (33,), (4097,))


def _specs(shapes, steps, betas=(BETAS,)):
    return [{"shape": s, "lr": LRS[i % len(LRS)], "t": steps[i % len(steps)], "betas": betas[i % len(betas)]}
            for i, s in enumerate(shapes)]


# name: (seed, [tensor specs])
CASES = {
    "t1": (3101, _specs(EIGHT, (1,))),
    "t2": (3102, _specs(EIGHT, (2,))),
    "t1000": (3103, _specs(EIGHT, (1000,))),
    "t30000": (3104, _specs(EIGHT, (30000,))),
    "mixed_steps": (3105, _specs(EIGHT, (1, 30000))),                  # step counts differ inside one launch
    "chunked": (3106, _specs(TEN, (1000, 2))),                        # a 9th and a 10th tensor
    "two_betas": (3107, _specs(FOUR, (1000,), (BETAS, OTHER_BETAS))),  # one step_all, two launches
}


def _decades(n: int, g: torch.Generator) -> torch.Tensor:
    return 10.0 ** (-6.0 * torch.rand(n, generator=g))


@functools.lru_cache(maxsize=None)
def make(name: str):
    """[{"p", "g", "m", "v" (fp32, CPU), "untouched", "idle" (bool masks), "lr", "t", "betas"}] of a case."""
    seed, specs = CASES[name]
    out = []
    for i, spec in enumerate(specs):
        g = torch.Generator().manual_seed(seed * 100 + i)
        shape = spec["shape"]
        n = 1
        for d in shape:
            n *= d
        u = torch.rand(n, generator=g)
        if n:
            u[0] = u[-1] = 1.0
        untouched, idle = u < 1 / 3, (u >= 1 / 3) & (u < 1 / 2)
        s = (0.1 + torch.randn(n, generator=g).abs()) * _decades(n, g)
        a = 2 * torch.rand(n, generator=g) - 1
        grad = torch.randn(n, generator=g) * _decades(n, g)
        s[untouched] = 0.0
        grad[untouched | idle] = 0.0
        p = torch.randn(n, generator=g) * (P_SPREAD * spec["lr"])
        t = {"p": p, "g": grad, "m": a * s, "v": s * s, "untouched": untouched, "idle": idle}
        out.append({**{k: x.view(shape).contiguous() for k, x in t.items()}, "lr": spec["lr"], "t": spec["t"],
                    "betas": spec["betas"]})
    return out


def _run(name: str, step, dtype):
    return [dict(zip(("p", "m", "v"), step(c["p"], c["g"], c["m"], c["v"], c["lr"], *c["betas"], EPS, c["t"], dtype)))
            for c in make(name)]


@functools.lru_cache(maxsize=None)
def oracle(name: str):
    """The fp64 restatement of every tensor of a case: computed once, shared by the tests, never written to."""
    return _run(name, R.adam_step, torch.float64)


@functools.lru_cache(maxsize=None)
def yardstick(name: str):
    """``torch.optim.Adam`` in fp32 on the CPU on the same."""
    return _run(name, R.torch_adam_step, torch.float32)


def rel_err(a: torch.Tensor, ref: torch.Tensor) -> float:
    """max |a - ref| / max |ref| over the whole tensor (0 for an empty one or where both are all zero)."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    if ref.numel() == 0:
        return 0.0 if a.shape == ref.shape else float("inf")
    diff, top = float((a - ref).abs().max()), float(ref.abs().max())
    if not (diff == diff):
        return float("inf")
    if top == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / top


def errors(got, case, ora):
    """{"p", "m", "v", "update"}: the four measures of one tensor; the update p_after - p_before is formed in fp64."""
    e = {k: rel_err(got[k], ora[k]) for k in ("p", "m", "v")}
    before = case["p"].double()
    e["update"] = rel_err(got["p"].detach().double().cpu() - before, ora["p"] - before)
    return e
