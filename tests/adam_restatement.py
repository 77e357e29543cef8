"""One step of Adam restated in plain tensor arithmetic (test infrastructure), parameterised by dtype.  The formula is the
single-tensor path of ``torch.optim.Adam`` (no weight decay, no amsgrad, maximize=False), which csrc/optim.hip's
``misplat_adam_step`` fuses:

    exp_avg.lerp_(g, 1 - b1)                     m = m + (1 - b1) (g - m)
    v = b2 v + (1 - b2) g^2
    denom = sqrt(v) / sqrt(1 - b2^t) + eps
    p -= lr / (1 - b1^t) * m / denom

The scalar bias terms are Python floats (doubles), as in torch.  The fp64 run is the oracle of test_adam_gpu.py.  Its
yardstick is NOT this file in fp32 but ``torch.optim.Adam`` itself in fp32 on the CPU (``torch_adam_step``): the reference's
optimizer, with the state of step t - 1 injected."""
import math

import torch


def adam_step(p, g, m, v, lr: float, b1: float, b2: float, eps: float, t: int, dtype):
    """(p, m, v) after step ``t`` (1-based) in ``dtype``; the inputs are not written to."""
    p, g, m, v = (x.detach().to(dtype) for x in (p, g, m, v))
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * (g * g)
    bias1, bias2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    denom = v.sqrt() / math.sqrt(bias2) + eps
    p = p - (lr / bias1) * (m / denom)
    return p, m, v


def torch_adam_step(p, g, m, v, lr: float, b1: float, b2: float, eps: float, t: int, dtype):
    """The same step by ``torch.optim.Adam`` on the CPU in ``dtype``, from the injected state of step t - 1."""
    param = p.detach().to(dtype).cpu().clone().requires_grad_(True)
    param.grad = g.detach().to(dtype).cpu().clone()
    opt = torch.optim.Adam([param], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    opt.state[param] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.detach().to(dtype).cpu().clone(),
                        "exp_avg_sq": v.detach().to(dtype).cpu().clone()}
    opt.step()
    st = opt.state[param]
    assert int(st["step"]) == t
    return param.detach(), st["exp_avg"], st["exp_avg_sq"]
