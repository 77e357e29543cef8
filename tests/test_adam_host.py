"""CPU (no kernel runs): the Adam restatement (tests/adam_restatement.py) against ``torch.optim.Adam`` in fp64, the
conditions the case generator (tests/adam_cases.py) promises, and the fp32 yardstick's own error on every case."""
import pytest
import torch

import adam_cases as A
import adam_restatement as R

MULTIPLE = 8.0                                         # test_adam_gpu.py's
CAP = 1e-4


@pytest.mark.parametrize("name", list(A.CASES))
def test_fp64_restatement_equals_torch_adam_in_fp64(name):
    for i, (c, ora) in enumerate(zip(A.make(name), A.oracle(name))):
        ref = dict(zip(("p", "m", "v"), R.torch_adam_step(c["p"], c["g"], c["m"], c["v"], c["lr"], *c["betas"], A.EPS, c["t"],
                                                           torch.float64)))
        for k in ("p", "m", "v"):
            assert ora[k].dtype == ref[k].dtype == torch.float64 and ora[k].shape == c["p"].shape
            assert A.rel_err(ora[k], ref[k]) <= 1e-12, (name, i, k, A.rel_err(ora[k], ref[k]))
        before = c["p"].double()
        assert A.rel_err(ora["p"] - before, ref["p"] - before) <= 1e-12, (name, i)


def test_the_cases_cover_what_they_are_there_for():
    sizes = lambda name: [c["p"].numel() for c in A.make(name)]
    eight = [1, 3, 4, 5, 0, 2047, 2048, 2049]
    for name in ("t1", "t2", "t1000", "t30000", "mixed_steps"):
        assert sizes(name) == eight                                                    # exactly 8, the empty one in the middle
    assert [{c["t"] for c in A.make(n)} for n in ("t1", "t2", "t1000", "t30000")] == [{1}, {2}, {1000}, {30000}]
    assert [c["t"] for c in A.make("mixed_steps")] == [1, 30000] * 4
    assert len(A.make("chunked")) == 10 and {4097, 30021} <= set(sizes("chunked"))
    assert [c["betas"] for c in A.make("two_betas")] == [A.BETAS, A.OTHER_BETAS] * 2 and A.BETAS != A.OTHER_BETAS
    lrs = {c["lr"] for name in A.CASES for c in A.make(name)}
    assert lrs == {1.6e-4, 0.0025, 0.0025 / 20, 0.05, 0.005, 0.001, 1.6e-6}
    assert {c["lr"] for c in A.make("t30000")} == lrs                                  # all seven within one launch


@pytest.mark.parametrize("name", list(A.CASES))
def test_generated_states_are_consistent(name):
    """v = s^2 >= 0, |m| <= sqrt(v) (so never v = 0 under m != 0), untouched rows all zero, idle rows with a zero gradient
    and a state, every other row with a gradient; the shares over the case; gradients over six decades."""
    cases = A.make(name)
    n_all = n_untouched = n_idle = 0
    grads = []
    for i, c in enumerate(cases):
        p, g, m, v, un, idle = (c[k].reshape(-1) for k in ("p", "g", "m", "v", "untouched", "idle"))
        assert all(x.dtype == torch.float32 and x.is_contiguous() for x in (c["p"], c["g"], c["m"], c["v"]))
        assert bool((v >= 0).all()) and bool(torch.isfinite(torch.stack([p, g, m, v])).all())
        assert bool((m.double().abs() <= v.double().sqrt() * (1 + 2.0 ** -22)).all()), (name, i)
        assert not bool(((v == 0) & (m != 0)).any())
        assert not bool((un & idle).any())
        assert bool((g[un] == 0).all() and (m[un] == 0).all() and (v[un] == 0).all())
        assert bool((g[idle] == 0).all() and (v[idle] > 0).all())
        active = ~(un | idle)
        assert bool((g[active] != 0).all() and (v[active] > 0).all())
        if p.numel():
            assert bool(active[0]) and bool(active[-1])
        n_all, n_untouched, n_idle = n_all + p.numel(), n_untouched + int(un.sum()), n_idle + int(idle.sum())
        grads.append(g[active].abs())
    assert 0.30 < n_untouched / n_all < 0.37 and 0.13 < n_idle / n_all < 0.20, (n_untouched / n_all, n_idle / n_all)
    grads = torch.cat(grads)
    assert float(grads.max()) > 0.5 and float(grads.quantile(0.1)) < 1e-5


@pytest.mark.parametrize("name", list(A.CASES))
def test_oracle_leaves_untouched_rows_alone_and_moves_idle_ones(name):
    for c, ora, y32 in zip(A.make(name), A.oracle(name), A.yardstick(name)):
        un, idle = c["untouched"], c["idle"]
        for res in (ora, y32):
            for k in ("p", "m", "v"):
                assert torch.equal(res[k][un], c[k][un].to(res[k].dtype)), (name, k)
        assert bool((ora["v"][idle] < c["v"][idle].double()).all())
        assert bool((ora["m"][idle].abs() <= c["m"][idle].double().abs()).all())
        moving = idle & (c["m"] != 0)
        assert bool((ora["p"][moving] != c["p"][moving].double()).all())


@pytest.mark.parametrize("name", list(A.CASES))
def test_fp32_torch_adam_yardstick_is_well_inside_the_cap(name):
    """The parameters' spread of ``A.P_SPREAD`` = 16 learning rates keeps the update error of fp32 ``torch.optim.Adam`` --
    the rounding of p_after relative to the largest update of the tensor -- at or below CAP / MULTIPLE = 1.25e-5 on every
    tensor of every case, so MULTIPLE x yardstick never meets the cap."""
    for i, (c, ora, y32) in enumerate(zip(A.make(name), A.oracle(name), A.yardstick(name))):
        assert all(y32[k].dtype == torch.float32 for k in y32)
        e = A.errors(y32, c, ora)
        print(f"adam {name:11s} tensor {i} n {c['p'].numel():6d} t {c['t']:5d} lr {c['lr']:.1e} fp32 torch: " +
              "  ".join(f"{k} {v:.2e}" for k, v in e.items()))
        for k, v in e.items():
            assert v <= CAP / MULTIPLE, (name, i, k, v)
        if c["p"].numel():
            assert float((ora["p"] - c["p"].double()).abs().max()) > 0                 # there is an update to measure
