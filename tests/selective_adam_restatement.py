"""The row-selective Adam step and the visibility rule restated in plain tensor arithmetic (test infrastructure).

``selective_adam_step`` is ``adam_restatement.adam_step`` under a row mask: a row with flag 1 gets the step -- bias-corrected
with the tensor's global 1-based step count ``t``, whatever the row's own history (the convention of
``torch.optim.SparseAdam``) --, a row with flag 0 keeps p, m and v as they are.  ``visibility_from_radii`` is the rule of
``collab_splats_amd.visibility_from_radii``: a Gaussian is visible when both of its projected radii are positive for some
camera."""
import torch

import adam_restatement as R


def selective_adam_step(p, g, m, v, mask, lr: float, b1: float, b2: float, eps: float, t: int, dtype):
    """(p, m, v) after step ``t`` in ``dtype`` with only the rows ``mask`` ([N] bool) stepped; the inputs are not written to."""
    stepped = R.adam_step(p, g, m, v, lr, b1, b2, eps, t, dtype)
    rows = mask.bool().view(-1, *([1] * (p.dim() - 1)))
    return tuple(torch.where(rows, new, old.detach().to(dtype)) for new, old in zip(stepped, (p, m, v)))


def visibility_from_radii(radii):
    """[N] bool from radii [C, N, 2]."""
    return (radii > 0).all(-1).any(0)
