"""Text-query similarity of rendered views and of Gaussians (plumbing around csrc/textquery.hip; no kernels here).

Reference: collab_splats/models/rade_features_model.py:493-539 (``get_outputs_for_camera``: decode at ``resize_factor=8.0``,
``compute_similarity``, resize to the image), :143-147 (the per-Gaussian ``similarity``) and
collab_splats/utils/features.py:237-325 (``compute_similarity``).  The text embeddings E [Q, C] meet a decoded
feature p = w_out h + b_out only through E p = (E w_out) h + E b_out, so a query set is folded ONCE into A [Q, Hd] and c [Q]
(``fold_text_queries``) and a pixel or a Gaussian then costs a few hundred multiply-adds: no [C, h, w] or [N, C] tensor exists.
Reachable as ``ops.fold_text_queries`` / ``ops.similarity_map`` / ``ops.gaussian_similarity`` too.  DESIGN.md section 23.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence

import torch
from torch import Tensor

from ._lib import ptr, require_gpu, run
from .featureloss import MAX_HIDDEN, MAX_LATENT, Decoder, _features_view, _flat

MAX_QUERIES = 64
MAX_CHANNELS = 2 ** 20
MAX_PIXELS = 2 ** 28
METHODS = ("standard", "pairwise")


class TextQuery(NamedTuple):
    """A folded query set: ``A`` [Q, Hd] = E w_out and ``c`` [Q] = E b_out of one decoder branch, the hidden layer they apply
    to (``w_hidden`` [Hd, L], ``b_hidden`` [Hd]: detached copies) and the split of the Q embeddings into the first
    ``n_positive`` positive and the other negative ones.  A snapshot of the decoder's weights at the fold."""
    A: Tensor
    c: Tensor
    w_hidden: Tensor
    b_hidden: Tensor
    n_positive: int
    Q: int


def _check_counts(what: str, Q: int, n_positive) -> None:
    if not 2 <= Q <= MAX_QUERIES:
        raise ValueError(f"{what}: 2..{MAX_QUERIES} text embeddings (at least one positive and one negative), got {Q}")
    if not isinstance(n_positive, int) or isinstance(n_positive, bool) or not 1 <= n_positive <= Q - 1:
        raise ValueError(f"{what}: n_positive must be an integer in 1..Q-1 = {Q - 1} (at least one positive and one negative "
                         f"embedding), got {n_positive!r}")


@torch.no_grad()
def fold_text_queries(decoder: Decoder, name: str, text_embeddings: Tensor, n_positive: int) -> TextQuery:
    """Fold ``text_embeddings`` [Q, C] (unit-norm rows, the first ``n_positive`` positive, the others negative; the caller's
    text encoder made them) into branch ``name`` of ``decoder`` (a ``TwoLayerMLP`` or ``(w_hidden, b_hidden, {name: (w_out,
    b_out)})``): A = E w_out and c = E b_out, each entry one fp64 sum over C in index order, rounded once."""
    w_h, b_h, branches = _flat(decoder)
    if name not in branches:
        raise KeyError(f"fold_text_queries: no branch {name!r} (have {sorted(branches)})")
    w_o, b_o = branches[name]
    if w_h.dim() != 2 or b_h.shape != (w_h.shape[0],):
        raise ValueError(f"fold_text_queries: w_hidden must be [Hd, L] and b_hidden [Hd], got {tuple(w_h.shape)} and {tuple(b_h.shape)}")
    hidden, latent = int(w_h.shape[0]), int(w_h.shape[1])
    if not 1 <= latent <= MAX_LATENT:
        raise ValueError(f"fold_text_queries: the latent width must be 1..{MAX_LATENT}, got {latent}")
    if not 1 <= hidden <= MAX_HIDDEN:
        raise ValueError(f"fold_text_queries: the hidden width must be 1..{MAX_HIDDEN}, got {hidden}")
    if w_o.dim() != 2 or w_o.shape[1] != hidden or b_o.shape != (w_o.shape[0],):
        raise ValueError(f"fold_text_queries: branch {name!r}: w_out {tuple(w_o.shape)} / b_out {tuple(b_o.shape)} do not fit "
                         f"Hd = {hidden}")
    channels = int(w_o.shape[0])
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"fold_text_queries: a branch of 1..2^20 channels, got {channels}")
    if text_embeddings.dim() != 2:
        raise ValueError(f"fold_text_queries: text_embeddings must be [Q, C], got {tuple(text_embeddings.shape)}")
    Q = int(text_embeddings.shape[0])
    _check_counts("fold_text_queries", Q, n_positive)
    if text_embeddings.shape[1] != channels:
        raise ValueError(f"fold_text_queries: text embeddings of width {text_embeddings.shape[1]} against a branch of {channels} "
                         f"channels")
    for t in (text_embeddings, w_h, b_h, w_o, b_o):
        if t.dtype != torch.float32:
            raise ValueError(f"fold_text_queries: embeddings and decoder parameters must be float32, got {t.dtype}")
    require_gpu(text_embeddings, w_h, b_h, w_o, b_o)
    emb, w_o, b_o = text_embeddings.detach().contiguous(), w_o.detach().contiguous(), b_o.detach().contiguous()
    dev = emb.device
    A = torch.empty(Q, hidden, device=dev, dtype=torch.float32)
    c = torch.empty(Q, device=dev, dtype=torch.float32)
    run("misplat_textquery_fold", Q, channels, hidden, ptr(emb), ptr(w_o), ptr(b_o), ptr(A), ptr(c))
    return TextQuery(A, c, w_h.detach().clone().contiguous(), b_h.detach().clone().contiguous(), n_positive, Q)


def _check_query(what: str, query: TextQuery, latent: int, method: str, softmax_temp: float) -> int:
    if not isinstance(query, TextQuery):
        raise ValueError(f"{what}: query must be the TextQuery that fold_text_queries returns")
    if method not in METHODS:
        raise ValueError(f"{what}: unknown method {method!r}: choose 'standard' or 'pairwise'")
    t32 = C.c_float(softmax_temp).value if isinstance(softmax_temp, (int, float)) else float("nan")
    if not (t32 > 0 and math.isfinite(t32)):
        raise ValueError(f"{what}: softmax_temp must be positive and finite (in fp32), got {softmax_temp!r}")
    hidden = int(query.w_hidden.shape[0])
    if not (1 <= int(query.w_hidden.shape[1]) <= MAX_LATENT and 1 <= hidden <= MAX_HIDDEN):
        raise ValueError(f"{what}: a hidden layer of L 1..{MAX_LATENT} and Hd 1..{MAX_HIDDEN}, got {tuple(query.w_hidden.shape)}")
    _check_counts(what, int(query.Q), query.n_positive)
    if (tuple(query.A.shape) != (query.Q, hidden) or tuple(query.c.shape) != (query.Q,)
            or tuple(query.b_hidden.shape) != (hidden,)):
        raise ValueError(f"{what}: the query's tensors do not fit each other (A {tuple(query.A.shape)}, c {tuple(query.c.shape)}, "
                         f"w_hidden {tuple(query.w_hidden.shape)}, b_hidden {tuple(query.b_hidden.shape)}, Q = {query.Q})")
    for t in query[:4]:
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: the query's tensors must be float32, got {t.dtype}")
    if latent != query.w_hidden.shape[1]:
        raise ValueError(f"{what}: features of width {latent} against a query of latent width {query.w_hidden.shape[1]}")
    return hidden


def _hw(what: str, name: str, hw: Sequence[int]):
    if len(hw) != 2 or min(int(v) for v in hw) < 1:
        raise ValueError(f"{what}: {name} must be (H, W) >= 1, got {tuple(hw)}")
    h, w = int(hw[0]), int(hw[1])
    if h * w > MAX_PIXELS:
        raise ValueError(f"{what}: {name} {(h, w)} is a map of more than 2^28 pixels")
    return h, w


@torch.no_grad()
def similarity_map(features: Tensor, query: TextQuery, work_hw: Sequence[int], out_hw: Optional[Sequence[int]] = None,
                   method: str = "pairwise", softmax_temp: float = 0.05) -> Tensor:
    """The similarity of every pixel to the positive queries, [H_out, W_out, 1] fp32 in 0..1 (``compute_similarity`` on the main
    branch decoded at ``work_hw``, then the reference's bilinear resize of the heat map to ``out_hw``; None: it stays at
    ``work_hw``).  ``features`` [H, W, L] float32 on the GPU (a channel slice of a wider image is read in place) is resized
    bilinearly to ``work_hw``, goes through the hidden layer, and z_q = (A_q . hid + c_q) / softmax_temp; "standard":
    softmax(z)[:n_positive].sum(); "pairwise": exp(p) / (n_neg exp(p) + sum_j exp(n_j)) with p the mean positive z (what
    ``query_similarity`` documents); NaN -> 0.  Two launches (one where the sizes agree)."""
    what = "similarity_map"
    feats, stride = _features_view(features, what)
    hidden = _check_query(what, query, int(feats.shape[2]), method, softmax_temp)
    h, w = _hw(what, "work_hw", work_hw)
    Ho, Wo = (h, w) if out_hw is None else _hw(what, "out_hw", out_hw)
    require_gpu(feats, *query[:4])
    H, W, L = (int(v) for v in feats.shape)
    work = torch.empty(h, w, 1, device=feats.device, dtype=torch.float32)
    run("misplat_textquery_map", H, W, L, stride, C.c_void_p(feats.data_ptr()), hidden, ptr(query.w_hidden),
        ptr(query.b_hidden), query.Q, query.n_positive, ptr(query.A), ptr(query.c), METHODS.index(method), softmax_temp, h, w,
        ptr(work))
    if (Ho, Wo) == (h, w):
        return work
    out = torch.empty(Ho, Wo, 1, device=feats.device, dtype=torch.float32)
    run("misplat_textquery_upsample", h, w, ptr(work), Ho, Wo, ptr(out))
    return out


@torch.no_grad()
def gaussian_similarity(latents: Tensor, query: TextQuery, method: str = "pairwise", softmax_temp: float = 0.05) -> Tensor:
    """The same similarity per row of ``latents`` [N, L] float32 on the GPU (the model's ``distill_features``), no resize:
    [N] fp32 in 0..1, without the [N, C] decoded features of ``per_gaussian_forward``."""
    what = "gaussian_similarity"
    if latents.dim() != 2:
        raise ValueError(f"{what}: latents must be [N, L], got {tuple(latents.shape)}")
    if latents.dtype != torch.float32:
        raise ValueError(f"{what}: latents must be float32, got {latents.dtype}")
    N, L = (int(v) for v in latents.shape)
    if N > MAX_PIXELS:
        raise ValueError(f"{what}: more than 2^28 rows ({N})")
    hidden = _check_query(what, query, L, method, softmax_temp)
    rows = latents.detach().contiguous()
    require_gpu(rows, *query[:4])
    out = torch.empty(N, device=rows.device, dtype=torch.float32)
    run("misplat_textquery_rows", N, L, L, ptr(rows), hidden, ptr(query.w_hidden), ptr(query.b_hidden), query.Q,
        query.n_positive, ptr(query.A), ptr(query.c), METHODS.index(method), softmax_temp, ptr(out))
    return out


__all__ = ["TextQuery", "fold_text_queries", "similarity_map", "gaussian_similarity"]
