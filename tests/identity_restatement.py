"""The identity losses of DESIGN.md section 33, restated in torch from their definition (not from the kernels): values AND
gradients are written out by hand, so the same code runs in float64 (the oracle) and in float32 (the yardstick of the GPU
tests) without autograd.  tests/test_identity_host.py checks it against autograd through F.conv2d + F.cross_entropy and through
F.log_softmax.

2-D:  z = W x + b per pixel;  ce = logsumexp_k(z) - z[t - 1] (the maximum subtracted before exp);
      loss = sum_labelled ce / max(n_labelled, 1);  target 0 = unlabelled, t in 1..K = class t - 1, anything else unlabelled.
      With r = softmax(z) - onehot at labelled pixels (0 elsewhere) and g = grad_out / max(n_labelled, 1):
      d/dx = g W^T r,  dW = g sum_pix r x^T,  db = g sum_pix r.
3-D:  p_j = softmax(W e_j + b);  loss = sum_j sum_{i valid} KL(p_sample_j || p_table_ji) / max(n_valid, 1), an entry being valid
      unless it is -1 or its own sample;  log-softmax exact (no + 1e-10).
"""
import torch


def logits(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """[..., D] -> [..., K]"""
    return x @ weight.t() + bias


def log_softmax(z: torch.Tensor) -> torch.Tensor:
    m = z.max(dim=-1, keepdim=True)[0]
    return z - (m + torch.log(torch.exp(z - m).sum(dim=-1, keepdim=True)))


def loss_2d(features, weight, bias, target, grad_out: float = 1.0):
    """{"loss", "n", "grads": {"features", "weight", "bias"}} in the dtype of ``features``."""
    H, W, D = features.shape
    K = weight.shape[0]
    x = features.reshape(-1, D)
    t = target.reshape(-1).to(torch.int64)
    lab = (t >= 1) & (t <= K)
    n = int(lab.sum())
    lp = log_softmax(logits(x, weight, bias))                                    # [P, K]
    cls = torch.where(lab, t - 1, torch.zeros_like(t))
    ce = -lp.gather(1, cls[:, None])[:, 0]
    ce = torch.where(lab, ce, torch.zeros_like(ce))
    denom = max(n, 1)
    loss = ce.sum() / denom
    onehot = torch.zeros_like(lp).scatter_(1, cls[:, None], 1.0)
    r = torch.where(lab[:, None], torch.exp(lp) - onehot, torch.zeros_like(lp)) * (grad_out / denom)
    xz = torch.where(lab[:, None], x, torch.zeros_like(x))                       # an unlabelled pixel takes no part at all
    return {"loss": loss, "n": n,
            "grads": {"features": (r @ weight).reshape(H, W, D), "weight": r.t() @ xz, "bias": r.sum(0)}}


def labels(features, weight, bias):
    """(labels [H, W] int64 = argmax class + 1, the first of equal maxima; confidence [H, W]; margin [H, W] = top logit - second
    (inf for K = 1); the largest |logit|)."""
    H, W, D = features.shape
    z = logits(features.reshape(-1, D), weight, bias)
    best = torch.argmax(z, dim=-1)
    conf = torch.exp(log_softmax(z)).max(dim=-1)[0]
    if z.shape[1] > 1:
        top = torch.topk(z, 2, dim=-1)[0]
        margin = top[:, 0] - top[:, 1]
    else:
        margin = torch.full_like(z[:, 0], float("inf"))
    return (best + 1).reshape(H, W), conf.reshape(H, W), margin.reshape(H, W), float(z.abs().max())


def valid_pairs(sample, table, n_rows: int):
    s = sample[:, None].expand_as(table).to(torch.int64)
    t = table.to(torch.int64)
    return s, t, (t >= 0) & (t < n_rows) & (t != s)


def loss_3d(identities, weight, bias, sample, table, grad_out: float = 1.0):
    """{"loss", "n", "grads": {"identities", "weight", "bias"}} in the dtype of ``identities``."""
    N, D = identities.shape
    s, t, ok = valid_pairs(sample, table, N)
    s, t = s[ok], t[ok]                                                          # [Q]
    n = int(ok.sum())
    denom = max(n, 1)
    es, et = identities[s], identities[t]
    lps, lpt = log_softmax(logits(es, weight, bias)), log_softmax(logits(et, weight, bias))
    p, q = torch.exp(lps), torch.exp(lpt)
    kl = (p * (lps - lpt)).sum(-1)                                               # [Q]
    loss = kl.sum() / denom
    g = grad_out / denom
    dzs = p * ((lps - lpt) - kl[:, None]) * g
    dzt = (q - p) * g
    v_e = torch.zeros_like(identities)
    v_e.index_add_(0, s, dzs @ weight)
    v_e.index_add_(0, t, dzt @ weight)
    return {"loss": loss, "n": n,
            "grads": {"identities": v_e, "weight": dzs.t() @ es + dzt.t() @ et, "bias": dzs.sum(0) + dzt.sum(0)}}
