"""Restatement of the features model's decoder and cosine feature loss, step by step as the model defines them, in torch on
the CPU at a chosen dtype.  The fp64 run (autograd for the gradients) is the oracle of the GPU tests; the fp32 run is their
yardstick for rounding.  Order of operations: the PREDICTIONS of a branch that is not the main one are resized (not the hidden
layer), as the model does.

    1. x   = bilinear(features -> (H_main, W_main))
    2. h   = relu(w_hidden x + b_hidden)                      (subgradient 0 at <= 0)
    3. p_b = w_out[b] h + b_out[b];  not the main branch: p_b = bilinear(p_b -> (H_b, W_b))
    4. loss_b = mean over pixels of 1 - <p_b, g_b> / (max(|p_b|, 1e-8) max(|g_b|, 1e-8))
    5. features_loss = loss_lambda * sum_b weight_b loss_b,  weight_main = 1, others = regularization_lambda
"""
import torch

EPS = 1e-8


def _axis(n_in: int, n_out: int, dtype):
    """Taps of a bilinear resize without corner alignment along one axis: source coordinate (i + 0.5) * n_in / n_out - 0.5,
    clamped at 0; lower index its floor, upper index one more but at most the last; weights (1 - frac, frac)."""
    i = torch.arange(n_out, dtype=dtype)
    src = ((i + 0.5) * (n_in / n_out) - 0.5).clamp_min(0.0)
    i0 = src.floor().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    l1 = src - i0
    return i0.long(), i1.long(), 1.0 - l1, l1


def bilinear(x: torch.Tensor, size) -> torch.Tensor:
    """[C, H, W] -> [C, size[0], size[1]]: the 4-tap rule, the same whether it shrinks or enlarges (no antialiasing)."""
    y0, y1, ly0, ly1 = _axis(x.shape[1], int(size[0]), x.dtype)
    x0, x1, lx0, lx1 = _axis(x.shape[2], int(size[1]), x.dtype)
    top = x[:, y0][:, :, x0] * lx0 + x[:, y0][:, :, x1] * lx1
    bot = x[:, y1][:, :, x0] * lx0 + x[:, y1][:, :, x1] * lx1
    return top * ly0[None, :, None] + bot * ly1[None, :, None]


def hidden(features: torch.Tensor, w_hidden, b_hidden, main_hw) -> torch.Tensor:
    """features [H, W, L] -> h [Hd, H_main, W_main]."""
    x = bilinear(features.permute(2, 0, 1), main_hw)
    return torch.relu(torch.einsum("jl,lyx->jyx", w_hidden, x) + b_hidden[:, None, None])


def decode(features, w_hidden, b_hidden, branches, dims, main, resize_factor: float = 1.0):
    """name -> [C_b, h, w]: the main branch at (int(H_main * resize_factor), int(W_main * resize_factor)), every other branch
    resized from there to its own (H_b, W_b).  ``branches``: name -> (w_out, b_out); ``dims``: name -> (C, H, W)."""
    hw = (int(dims[main][1] * resize_factor), int(dims[main][2] * resize_factor))
    h = hidden(features, w_hidden, b_hidden, hw)
    out = {}
    for name, (w_out, b_out) in branches.items():
        p = torch.einsum("cj,jyx->cyx", w_out, h) + b_out[:, None, None]
        out[name] = p if name == main else bilinear(p, dims[name][1:])
    return out


def decode_resized_hidden(features, w_hidden, b_hidden, branches, dims, main):
    """The same predictions the other way round: the hidden layer is resized to the branch's resolution, then the branch's
    linear layer is applied (bilinear weights sum to 1, so the two orders agree up to rounding)."""
    h = hidden(features, w_hidden, b_hidden, dims[main][1:])
    out = {}
    for name, (w_out, b_out) in branches.items():
        hb = h if name == main else bilinear(h, dims[name][1:])
        out[name] = torch.einsum("cj,jyx->cyx", w_out, hb) + b_out[:, None, None]
    return out


def cosine(p: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """[C, H, W] x 2 -> [H, W]: each norm clamped at 1e-8 on its own (a clamped norm is a constant for the gradient)."""
    num = (p * g).sum(0)
    return num / (torch.linalg.vector_norm(p, dim=0).clamp_min(EPS) * torch.linalg.vector_norm(g, dim=0).clamp_min(EPS))


def loss_from_predictions(pred, gt, main, regularization_lambda, loss_lambda):
    total, sums = 0.0, {}
    for name, p in pred.items():
        terms = 1.0 - cosine(p, gt[name])
        sums[name] = terms.sum()
        total = total + (1.0 if name == main else regularization_lambda) * terms.mean()
    return loss_lambda * total, sums


def feature_loss(features, w_hidden, b_hidden, branches, gt, main, regularization_lambda=0.1, loss_lambda=1e-3,
                 resized_hidden: bool = False):
    """(features_loss, {name: sum over pixels of 1 - cos})."""
    dims = {name: tuple(t.shape) for name, t in gt.items()}
    dec = decode_resized_hidden if resized_hidden else decode
    return loss_from_predictions(dec(features, w_hidden, b_hidden, branches, dims, main), gt, main, regularization_lambda,
                                 loss_lambda)


def per_gaussian(x, w_hidden, b_hidden, branches):
    """[N, L] -> name -> [N, C_b]: the decoder row by row."""
    h = torch.relu(x @ w_hidden.t() + b_hidden)
    return {name: h @ w.t() + b for name, (w, b) in branches.items()}


def run(scene, dtype, resized_hidden: bool = False):
    """Loss and all gradients of a scene (tests/featureloss_scenes.py) at ``dtype``: {"loss", "sums", "grads": {"features",
    "w_hidden", "b_hidden", "w_out.<name>", "b_out.<name>"}}."""
    cast = lambda t: t.detach().to(dtype).clone().requires_grad_(True)                # noqa: E731
    f, wh, bh = cast(scene["features"]), cast(scene["w_hidden"]), cast(scene["b_hidden"])
    br = {n: (cast(w), cast(b)) for n, (w, b) in scene["branches"].items()}
    gt = {n: t.to(dtype) for n, t in scene["gt"].items()}
    loss, sums = feature_loss(f, wh, bh, br, gt, scene["main"], scene["regularization_lambda"], scene["loss_lambda"],
                              resized_hidden=resized_hidden)
    loss.backward()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)            # noqa: E731
    grads = {"features": zero(f), "w_hidden": zero(wh), "b_hidden": zero(bh)}
    for n, (w, b) in br.items():
        grads["w_out." + n], grads["b_out." + n] = zero(w), zero(b)
    return {"loss": loss.detach(), "sums": {n: s.detach() for n, s in sums.items()}, "grads": grads}
