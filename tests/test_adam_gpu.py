"""GPU: the fused multi-tensor Adam (csrc/optim.hip ``misplat_adam_step``, collab_splats_amd/optim.py) against the fp64
restatement (tests/adam_restatement.py) on the single-step cases of tests/adam_cases.py, and its refusals.

Error measures, per tensor: max |got - oracle| / max |oracle| for the parameter and the two moments, and the same for the
update p_after - p_before formed in fp64 (the parameter itself would hide an update that is wrong by a few per cent under
its own size).  The bound of each is the bilateral-grid tests' rule: ``MULTIPLE`` = 8 times the error that fp32
``torch.optim.Adam`` on the CPU -- the reference's optimizer, not the code under test -- makes on the same tensor against
the same oracle, that error floored at 2^-23, and never above the project's standing 1e-4.  Every step is five to ten fp32
operations per element in torch's order, so the kernel sits at the yardstick; 8 is the margin those tests use.  (The
figures of a GPU run belong in DESIGN.md section 11; this test prints them.)"""
import pytest
import torch

import adam_cases as A

pytestmark = pytest.mark.gpu

MULTIPLE = 8.0
FLOOR = 2.0 ** -23
CAP = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def bound(yard: float) -> float:
    return min(MULTIPLE * max(yard, FLOOR), CAP)


def load(case, dev, grad=None):
    """(FusedAdam over one tensor of a case, its parameter) with the state of step t - 1 injected."""
    from collab_splats_amd import FusedAdam
    p = case["p"].clone().to(dev).requires_grad_(True)
    p.grad = case["g"].clone().to(dev) if grad is None else grad
    opt = FusedAdam([p], lr=case["lr"], betas=case["betas"], eps=A.EPS)
    opt.state[p] = {"step": torch.tensor(float(case["t"] - 1)), "exp_avg": case["m"].clone().to(dev),
                    "exp_avg_sq": case["v"].clone().to(dev)}
    return opt, p


def result(opt, p):
    st = opt.state[p]
    return {"p": p.detach().cpu(), "m": st["exp_avg"].cpu(), "v": st["exp_avg_sq"].cpu()}


@pytest.mark.parametrize("name", list(A.CASES))
def test_one_step_against_the_fp64_oracle(dev, name):
    """One ``step_all`` over all tensors of a case (one optimizer each: its own lr, step count and betas)."""
    from collab_splats_amd import fused_adam_step_all
    cases = A.make(name)
    loaded = [load(c, dev) for c in cases]
    fused_adam_step_all([opt for opt, _ in loaded])
    torch.cuda.synchronize()
    rows = []
    for i, (c, (opt, p), ora, y32) in enumerate(zip(cases, loaded, A.oracle(name), A.yardstick(name))):
        got = result(opt, p)
        assert int(opt.state[p]["step"]) == c["t"]
        rows.append((i, c, got, A.errors(got, c, ora), A.errors(y32, c, ora)))
    for i, c, _, e_gpu, e_32 in rows:
        print(f"adam {name:11s} tensor {i} n {c['p'].numel():6d} t {c['t']:5d} lr {c['lr']:.1e}  " + "  ".join(
            f"{k} gpu {e_gpu[k]:.2e} torch fp32 {e_32[k]:.2e} bound {bound(e_32[k]):.2e}" for k in e_gpu))
    for i, c, got, e_gpu, e_32 in rows:
        for k in ("p", "m", "v"):
            assert got[k].shape == c["p"].shape and got[k].dtype == torch.float32 and bool(torch.isfinite(got[k]).all())
        for k in e_gpu:
            assert e_gpu[k] <= bound(e_32[k]), (name, i, k, e_gpu[k], e_32[k])
        # never touched: bit-identical;  touched earlier, not now: the second moment decays
        un, idle = c["untouched"], c["idle"]
        for k in ("p", "m", "v"):
            assert torch.equal(got[k][un], c[k][un]), (name, i, k)
        assert bool((got["v"][idle] < c["v"][idle]).all()), (name, i)


def test_two_betas_split_into_two_launches(dev):
    """The case ``two_betas`` is what it says: ``_launch`` groups its four entries under two (betas, eps) keys."""
    entries = []
    for c in A.make("two_betas"):
        entries += load(c, dev)[0]._entries()
    assert len({e[3:] for e in entries}) == 2 and len(entries) == 4


def test_misaligned_parameter_is_refused_before_any_launch(dev):
    """A contiguous view that starts one float into its storage is 4-byte aligned, not 16: ``misplat_adam_step`` returns
    EINVAL before it launches anything, ``step()`` raises, and p, m, v and the step count are as they were."""
    from collab_splats_amd import FusedAdam, MisplatError
    c = A.make("t1000")[5]                                                             # 2047 elements
    storage = torch.zeros(c["p"].numel() + 1, device=dev)
    storage[1:] = c["p"].to(dev)
    view = storage[1:].detach().requires_grad_(True)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    opt = FusedAdam([view], lr=c["lr"], betas=c["betas"], eps=A.EPS)
    view.grad = c["g"].to(dev)
    opt.state[view] = {"step": torch.tensor(float(c["t"] - 1)), "exp_avg": c["m"].clone().to(dev),
                       "exp_avg_sq": c["v"].clone().to(dev)}
    with pytest.raises(MisplatError, match="misplat_adam_step"):
        opt.step()
    torch.cuda.synchronize()
    st = opt.state[view]
    assert torch.equal(view.detach().cpu(), c["p"]) and torch.equal(st["exp_avg"].cpu(), c["m"])
    assert torch.equal(st["exp_avg_sq"].cpu(), c["v"]) and int(st["step"]) == c["t"] - 1
    # the same tensors at an aligned address are stepped
    opt2, p2 = load(c, dev)
    opt2.step()
    assert not torch.equal(p2.detach().cpu(), c["p"]) and int(opt2.state[p2]["step"]) == c["t"]


def test_non_contiguous_gradient_is_stepped_through_its_contiguous_copy(dev):
    c = A.make("chunked")[1]                                                           # (10007, 3)
    wide = torch.zeros(10007, 6, device=dev)
    wide[:, ::2] = c["g"].to(dev)
    strided = wide[:, ::2]
    assert not strided.is_contiguous() and torch.equal(strided.cpu(), c["g"])
    a_opt, a_p = load(c, dev)
    b_opt, b_p = load(c, dev, grad=strided)
    a_opt.step()
    b_opt.step()
    torch.cuda.synchronize()
    a, b = result(a_opt, a_p), result(b_opt, b_p)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(wide[:, ::2].cpu(), c["g"]) and not torch.equal(a["p"], c["p"])
