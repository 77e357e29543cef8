"""GPU: the row-selective Adam (csrc/optim.hip ``misplat_adam_step_rows`` / ``misplat_visible_rows``,
``collab_splats_amd.SelectiveAdam``) on the single-step cases of tests/selective_adam_cases.py.

What a step is held to, for every mask of every size: the selected rows carry the bits ``FusedAdam`` gives copies of the same
tensors (under the all-ones mask that is every element of p, m and v); they are within the bound of tests/test_adam_gpu.py of
the fp64 restatement under the mask (tests/selective_adam_restatement.py) -- 8 x the error that fp32 ``torch.optim.Adam`` on
the CPU, the reference's optimizer, makes on the same rows against the same oracle, floored at 2^-23 and capped at 1e-4; the
measures are ``adam_cases.errors`` over the masked tensors, printed before they are asserted --; the unselected rows are
bit-identical to their inputs in all three tensors; and the step count is t for every tensor, the empty mask included."""
import functools
import importlib.util
import os

import pytest
import torch

import adam_cases as A
import selective_adam_cases as SC
import selective_adam_restatement as S

pytestmark = pytest.mark.gpu

MULTIPLE = 8.0
FLOOR = 2.0 ** -23
CAP = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def bound(yard: float) -> float:
    return min(MULTIPLE * max(yard, FLOOR), CAP)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def load(cases, dev, cls):
    """[(optimizer over one tensor of a case, its parameter)] with the state of step t - 1 injected."""
    out = []
    for c in cases:
        p = c["p"].clone().to(dev).requires_grad_(True)
        p.grad = c["g"].clone().to(dev)
        opt = cls([p], lr=c["lr"], betas=c["betas"], eps=SC.EPS)
        opt.state[p] = {"step": torch.tensor(float(c["t"] - 1)), "exp_avg": c["m"].clone().to(dev),
                        "exp_avg_sq": c["v"].clone().to(dev)}
        out.append((opt, p))
    return out


def result(loaded):
    return [{"p": p.detach().cpu(), "m": o.state[p]["exp_avg"].cpu(), "v": o.state[p]["exp_avg_sq"].cpu()} for o, p in loaded]


def steps_of(loaded):
    return [int(o.state[p]["step"]) for o, p in loaded]


def run_dense(cases, dev):
    from collab_splats_amd import FusedAdam, fused_adam_step_all
    loaded = load(cases, dev, FusedAdam)
    fused_adam_step_all([o for o, _ in loaded])
    torch.cuda.synchronize()
    return result(loaded)


def run_selective(cases, dev, mask, as_uint8=False):
    from collab_splats_amd import SelectiveAdam, selective_adam_step_all
    loaded = load(cases, dev, SelectiveAdam)
    vis = mask.to(torch.uint8).to(dev) if as_uint8 else mask.to(dev)
    selective_adam_step_all([o for o, _ in loaded], vis)
    torch.cuda.synchronize()
    return result(loaded), steps_of(loaded)


@functools.lru_cache(maxsize=None)
def dense(n: int, steps: str, dev):
    """``FusedAdam`` on copies of the tensors of a case: run once, shared by its masks, never written to."""
    return run_dense(SC.make(n, steps), dev)


def check_against_dense(got, den, cases, mask, what):
    for i, (g, d, c) in enumerate(zip(got, den, cases)):
        for k in ("p", "m", "v"):
            assert g[k].shape == c["p"].shape and g[k].dtype == torch.float32
            assert same_bits(g[k][mask], d[k][mask]), (what, i, k, "selected rows differ from FusedAdam")
            assert same_bits(g[k][~mask], c[k][~mask]), (what, i, k, "unselected rows moved")


@pytest.mark.parametrize("n,steps,name", [(n, s, m) for n, s in SC.CASES for m in SC.masks(n)])
def test_one_step_under_a_mask(dev, n, steps, name):
    cases, mask = SC.make(n, steps), SC.masks(n)[name]
    got, counts = run_selective(cases, dev, mask, as_uint8=name in ("alternating", "random_2"))
    assert counts == [c["t"] for c in cases]                                           # whatever the mask holds
    den = dense(n, steps, dev)
    ora, y32 = SC.masked_oracle(n, steps, mask), SC.under_mask(SC.yardstick(n, steps), cases, mask)
    rows = [(i, c, A.errors(g, c, o), A.errors(y, c, o)) for i, (c, g, o, y) in enumerate(zip(cases, got, ora, y32))]
    for i, c, e_gpu, e_32 in rows:
        print(f"selective adam n {n:5d} {steps:5s} {name:14s} {SC.NAMES[i]:13s} t {c['t']:4d}  " + "  ".join(
            f"{k} gpu {e_gpu[k]:.2e} torch fp32 {e_32[k]:.2e} bound {bound(e_32[k]):.2e}" for k in e_gpu))
    check_against_dense(got, den, cases, mask, (n, steps, name))
    if name == "all":
        for g, d in zip(got, den):
            assert all(same_bits(g[k], d[k]) for k in ("p", "m", "v"))
    for i, c, e_gpu, e_32 in rows:
        assert all(bool(torch.isfinite(got[i][k]).all()) for k in ("p", "m", "v"))
        for k in e_gpu:
            assert e_gpu[k] <= bound(e_32[k]), (n, steps, name, i, k, e_gpu[k], e_32[k])


def test_poisoned_gradients_of_unselected_rows_change_nothing(dev):
    """NaN and inf in the gradients of the rows the mask leaves out: the result is the unpoisoned one bit for bit."""
    n, steps = 2049, "t1000"
    cases, mask = SC.make(n, steps), SC.masks(n)["random_50"]
    clean, _ = run_selective(cases, dev, mask)
    poisoned = []
    for c in cases:
        g = c["g"].clone()
        out = (~mask).nonzero().flatten()
        g[out[0::3]], g[out[1::3]], g[out[2::3]] = float("nan"), float("inf"), float("-inf")
        poisoned.append({**c, "g": g})
    got, counts = run_selective(poisoned, dev, mask)
    assert counts == [c["t"] for c in cases]
    for i, (g, ref, c) in enumerate(zip(got, clean, cases)):
        for k in ("p", "m", "v"):
            assert same_bits(g[k], ref[k]), (i, k)
            assert bool(torch.isfinite(g[k][mask]).all()) and same_bits(g[k][~mask], c[k][~mask])


def test_more_elements_than_the_grid_holds(dev):
    """The row kernel caps its grid at 16 384 workgroups of 256 lanes = 4 194 304 lanes and sweeps one tensor at a time; 100 000
    rows at full density are 4 500 000 elements of features_rest (width 45), so its last 305 696 are reached only by the
    second trip of the grid-stride loop (5.9 M elements, 94 MB of state in all).  Equal to FusedAdam bit for bit (compared on
    the device)."""
    from collab_splats_amd import FusedAdam, SelectiveAdam, fused_adam_step_all, selective_adam_step_all
    n = 100000
    assert n * max(SC.WIDTHS) > 16384 * 256
    cases = SC.tensors(5100, [(n,) + r for r in SC.ROW_SHAPES], SC.LRS, (1000,))
    a, b = load(cases, dev, FusedAdam), load(cases, dev, SelectiveAdam)
    fused_adam_step_all([o for o, _ in a])
    selective_adam_step_all([o for o, _ in b], torch.ones(n, dtype=torch.bool, device=dev))
    torch.cuda.synchronize()
    for i, ((oa, pa), (ob, pb), c) in enumerate(zip(a, b, cases)):
        assert same_bits(pa.detach(), pb.detach()) and not torch.equal(pb.detach().cpu(), c["p"]), i
        for k in ("exp_avg", "exp_avg_sq"):
            assert same_bits(oa.state[pa][k], ob.state[pb][k]), (i, k)
        assert int(ob.state[pb]["step"]) == 1000


class Calls:
    """Counts the calls of C entries (``_lib.load()`` hands out one object whose attributes are the entries)."""

    def __init__(self, monkeypatch, *names):
        from collab_splats_amd import _lib
        lib = _lib.load()
        self.n = {name: 0 for name in names}
        for name in names:
            monkeypatch.setattr(lib, name, self._counting(name, getattr(lib, name)))

    def _counting(self, name, fn):
        def call(*args):
            self.n[name] += 1
            return fn(*args)
        return call


def test_ten_tensors_are_two_launches_over_one_id_list(dev, monkeypatch):
    n = 2049
    shapes = [(n,) + r for r in SC.ROW_SHAPES] + [(n, 2), (n, 5), (n, 7), (n,)]
    cases, mask = SC.tensors(5200, shapes, A.LRS, (1000, 2)), SC.masks(n)["random_50"]
    den = run_dense(cases, dev)
    calls = Calls(monkeypatch, "misplat_adam_step_rows", "misplat_union_ids", "misplat_touched_bits", "misplat_adam_step")
    got, counts = run_selective(cases, dev, mask)
    assert calls.n == {"misplat_adam_step_rows": 2, "misplat_union_ids": 1, "misplat_touched_bits": 1, "misplat_adam_step": 0}
    assert counts == [c["t"] for c in cases] and len(cases) == 10
    check_against_dense(got, den, cases, mask, "ten tensors")


def test_two_betas_are_two_launches_over_one_id_list(dev, monkeypatch):
    n = 2049
    cases = SC.tensors(5300, [(n,) + r for r in SC.ROW_SHAPES[:4]], SC.LRS, (1000,), (SC.BETAS, SC.OTHER_BETAS))
    assert [c["betas"] for c in cases] == [SC.BETAS, SC.OTHER_BETAS] * 2
    mask = SC.masks(n)["alternating"]
    den = run_dense(cases, dev)
    calls = Calls(monkeypatch, "misplat_adam_step_rows", "misplat_union_ids")
    got, counts = run_selective(cases, dev, mask)
    assert calls.n == {"misplat_adam_step_rows": 2, "misplat_union_ids": 1} and counts == [1000] * 4
    check_against_dense(got, den, cases, mask, "two betas")
    assert not same_bits(den[0]["p"], den[1]["p"])


def test_step_of_one_optimizer_and_a_non_contiguous_gradient(dev):
    """``SelectiveAdam.step(visibility)`` on its own, with a strided gradient: stepped through its contiguous copy."""
    from collab_splats_amd import SelectiveAdam
    n = 2049
    c, mask = SC.make(n, "t1000")[0], SC.masks(n)["random_50"]
    (a_opt, a_p), = load([c], dev, SelectiveAdam)
    (b_opt, b_p), = load([c], dev, SelectiveAdam)
    wide = torch.zeros(n, 6, device=dev)
    wide[:, ::2] = c["g"].to(dev)
    b_p.grad = wide[:, ::2]
    assert not b_p.grad.is_contiguous()
    a_opt.step(mask.to(dev))
    b_opt.step(mask.to(dev))
    torch.cuda.synchronize()
    (a,), (b,) = result([(a_opt, a_p)]), result([(b_opt, b_p)])
    assert all(same_bits(a[k], b[k]) for k in a) and not torch.equal(a["p"], c["p"])
    assert torch.equal(wide[:, ::2].cpu(), c["g"]) and steps_of([(a_opt, a_p), (b_opt, b_p)]) == [1000, 1000]


def test_a_mask_view_that_is_not_8_byte_aligned(dev):
    n = 2047
    cases, mask = SC.make(n, "t1"), SC.masks(n)["random_50"]
    from collab_splats_amd import SelectiveAdam, selective_adam_step_all
    loaded = load(cases, dev, SelectiveAdam)
    storage = torch.zeros(n + 3, dtype=torch.bool, device=dev)
    storage[3:] = mask.to(dev)
    assert storage[3:].data_ptr() % 8 == 3
    selective_adam_step_all({name: o for name, (o, _) in zip(SC.NAMES, loaded)}, storage[3:])
    torch.cuda.synchronize()
    check_against_dense(result(loaded), dense(n, "t1", dev), cases, mask, "misaligned mask")


REFUSALS = ("short_mask", "float_mask", "int32_mask", "cpu_mask", "two_dimensional_mask", "other_row_count", "sparse_gradient",
            "strided_parameter", "strided_exp_avg", "strided_exp_avg_sq")


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_leave_everything_as_it_was(dev, what):
    from collab_splats_amd import MisplatError, SelectiveAdam, selective_adam_step_all
    n = 64
    cases = SC.make(n, "t1000")
    loaded = load(cases, dev, SelectiveAdam)
    mask = SC.masks(n)["all"].to(dev)
    watched = [(p, p.detach().clone(), o.state[p]) for o, p in loaded]
    if what == "short_mask":
        mask = mask[:n - 1]
    elif what == "float_mask":
        mask = mask.float()
    elif what == "int32_mask":
        mask = mask.int()
    elif what == "cpu_mask":
        mask = mask.cpu()
    elif what == "two_dimensional_mask":
        mask = mask.view(n, 1)
    else:
        c = cases[4]                                                                   # scales [n, 3], the last but one entry
        if what == "other_row_count":
            p = c["p"][:32].clone().to(dev).requires_grad_(True)
            p.grad = c["g"][:32].clone().to(dev)
            st = {"exp_avg": c["m"][:32].clone().to(dev), "exp_avg_sq": c["v"][:32].clone().to(dev)}
        elif what == "sparse_gradient":
            p = c["p"].clone().to(dev).requires_grad_(True)
            p.grad = c["g"].clone().to(dev).to_sparse()
            st = {"exp_avg": c["m"].clone().to(dev), "exp_avg_sq": c["v"].clone().to(dev)}
        else:
            strided = lambda x: x.t().contiguous().to(dev).t()                         # [n, 3] with strides (1, n)
            p = (strided(c["p"]) if what == "strided_parameter" else c["p"].clone().to(dev)).detach().requires_grad_(True)
            p.grad = c["g"].clone().to(dev)
            st = {"exp_avg": strided(c["m"]) if what == "strided_exp_avg" else c["m"].clone().to(dev),
                  "exp_avg_sq": strided(c["v"]) if what == "strided_exp_avg_sq" else c["v"].clone().to(dev)}
            assert not all(x.is_contiguous() for x in (p, st["exp_avg"], st["exp_avg_sq"]))
        opt = SelectiveAdam([p], lr=c["lr"], betas=c["betas"], eps=SC.EPS)
        opt.state[p] = {"step": torch.tensor(999.0), **st}
        loaded[4] = (opt, p)
        watched[4] = (p, p.detach().clone(), opt.state[p])
    before = [(ref, st["exp_avg"].clone(), st["exp_avg_sq"].clone()) for _, ref, st in watched]
    with pytest.raises(MisplatError):
        selective_adam_step_all([o for o, _ in loaded], mask)
    torch.cuda.synchronize()
    for (p, _, st), (ref_p, ref_m, ref_v) in zip(watched, before):
        assert same_bits(p.detach(), ref_p) and same_bits(st["exp_avg"], ref_m) and same_bits(st["exp_avg_sq"], ref_v)
        assert int(st["step"]) == 999
    with pytest.raises(TypeError):
        selective_adam_step_all([torch.optim.Adam([loaded[0][1]])], SC.masks(n)["all"].to(dev))


@pytest.mark.parametrize("n_cams,n", [(1, 1), (3, 1), (1, 2049), (3, 2049)])
def test_visibility_from_radii_equals_its_restatement(dev, n_cams, n):
    from collab_splats_amd import MisplatError, visibility_from_radii
    g = torch.Generator().manual_seed(70 + 10 * n_cams + n)
    radii = torch.randint(-2, 4, (n_cams, n, 2), generator=g, dtype=torch.int32)       # zero and negative radii present
    if n == 1:
        radii[0, 0] = torch.tensor([3, 0]) if n_cams == 1 else torch.tensor([0, -1])
        radii[-1, 0, 0] = 2
    else:
        assert bool((radii == 0).any()) and bool((radii < 0).any())
    want = S.visibility_from_radii(radii)
    got = visibility_from_radii(radii.to(dev))
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and got.shape == (n,) and got.is_cuda
    assert torch.equal(got.cpu().bool(), want) and int(got.max()) <= 1
    if n > 1:
        assert 0 < int(want.sum()) < n
        strided = radii.to(dev)[:, ::2]                                                # a non-contiguous view
        assert torch.equal(visibility_from_radii(strided).cpu().bool(), want[::2])
    with pytest.raises(MisplatError):
        visibility_from_radii(radii)                                                   # CPU
    with pytest.raises(MisplatError):
        visibility_from_radii(radii.to(dev).long())


def test_two_runs_are_bitwise_equal(dev):
    n, steps = 10007, "t1000"
    cases, mask = SC.make(n, steps), SC.masks(n)["random_50"]
    a, _ = run_selective(cases, dev, mask)
    b, _ = run_selective(cases, dev, mask)
    assert all(same_bits(x[k], y[k]) for x, y in zip(a, b) for k in ("p", "m", "v"))


@pytest.mark.parametrize("strategy", ["default", "mcmc"])
def test_training_with_visible_adam_and_densification(dev, strategy):
    """The example's loop with ``visible_adam=True`` under both densification strategies: finite parameters at the end, a
    Gaussian count that has moved from 2 000, and a last ``main_loss`` below the first.  Conditions, not a measured rate."""
    spec = importlib.util.spec_from_file_location("train_synthetic", os.path.join(ROOT, "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    built, build_model = [], mod.build_model
    mod.build_model = lambda *a, **k: built.append(build_model(*a, **k)) or built[-1]  # (train() returns its log only)
    log = mod.train(steps=40, n=2000, W=96, H=64, refine_every=10, visible_adam=True, verbose=False, strategy=strategy)
    model = built[-1]
    from collab_splats_amd import SelectiveAdam
    assert len(log) == 40 and all(isinstance(o, SelectiveAdam) for o in model.optimizers.values())
    for name, p in model.gauss_params.items():
        assert bool(torch.isfinite(p).all()), name
        st = model.optimizers[name].state[model.optimizers[name].param_groups[0]["params"][0]]
        assert st["exp_avg"].shape == p.shape and bool(torch.isfinite(st["exp_avg"]).all())
    print(f"visible adam, {strategy}: main_loss {log[0][0]:.5f} -> {log[-1][0]:.5f}, gaussians {log[0][1]} -> {log[-1][1]}")
    assert model.means.shape[0] == log[-1][1] != 2000
    assert log[-1][0] < log[0][0]
