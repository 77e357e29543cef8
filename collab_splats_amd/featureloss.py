"""The features model's decoder and its cosine feature loss (plumbing around csrc/featloss.hip; no kernels here).

Reference: /root/reference/collab_splats/models/rade_features_model.py:149-189 (``decode_features``), :545-584
(``get_loss_dict``) and /root/reference/collab_splats/utils/features.py:408-478 (``TwoLayerMLP``).  ``feature_loss`` is one
autograd node over ``misplat_featloss_fwd`` / ``misplat_featloss_bwd``; ``decode`` and ``TwoLayerMLP.per_gaussian_forward``
run on ``misplat_feature_decode``.  Reachable as ``ops.feature_loss`` / ``ops.feature_decode`` too.  DESIGN.md section 21.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import _lib
from ._lib import ptr, require_gpu, run

MAX_LATENT = 32
MAX_HIDDEN = 256
MAX_BRANCHES = 4


class TwoLayerMLP(nn.Module):
    """The decoder of the features model: a shared 1 x 1 convolution ``hidden_conv`` (latent -> hidden, then relu) and one
    1 x 1 convolution per feature model in ``feature_branch_dict`` (hidden -> C_b).  Parameter names and shapes are the
    reference's (``hidden_conv.weight`` [Hd, L, 1, 1], ``feature_branch_dict.<name>.weight`` [C_b, Hd, 1, 1], biases), so
    the ``decoder.*`` entries of a reference checkpoint load with ``load_state_dict``.  Only the channel count of each
    ``features_dim_dict`` entry (C_b, H_b, W_b) is used here."""

    def __init__(self, input_dim: int, hidden_dim: int, features_dim_dict: Mapping[str, Sequence[int]]):
        super().__init__()
        _check_sizes(input_dim, hidden_dim, [(int(d[0]), 1, 1) for d in features_dim_dict.values()], "TwoLayerMLP")
        self.hidden_conv = nn.Conv2d(input_dim, hidden_dim, kernel_size=1)
        self.feature_branch_dict = nn.ModuleDict({name: nn.Conv2d(hidden_dim, int(dims[0]), kernel_size=1)
                                                  for name, dims in features_dim_dict.items()})

    def forward(self, x: Tensor) -> Dict[str, Tensor]:
        """[B, L, H, W] -> {name: [B, C_b, H, W]}: the module as the reference defines it (torch convolutions, differentiable).
        The training loss and ``decode_features`` do not come through here: they run on the HIP kernels."""
        h = F.relu(self.hidden_conv(x))
        return {name: conv(h) for name, conv in self.feature_branch_dict.items()}

    def flat(self) -> Tuple[Tensor, Tensor, Dict[str, Tuple[Tensor, Tensor]]]:
        """(w_hidden [Hd, L], b_hidden [Hd], {name: (w_out [C_b, Hd], b_out [C_b])}): views of the parameters (gradients flow)."""
        hc = self.hidden_conv
        return (hc.weight.view(hc.out_channels, hc.in_channels), hc.bias,
                {name: (conv.weight.view(conv.out_channels, conv.in_channels), conv.bias)
                 for name, conv in self.feature_branch_dict.items()})

    def query_decoder(self, name: str) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        """The 4-tuple ``query_similarity(decoder=...)`` takes for one branch: (w_hidden, b_hidden, w_out, b_out), detached."""
        w_h, b_h, branches = self.flat()
        if name not in branches:
            raise KeyError(f"TwoLayerMLP: no branch {name!r} (have {sorted(branches)})")
        return w_h.detach(), b_h.detach(), branches[name][0].detach(), branches[name][1].detach()

    @torch.no_grad()
    def per_gaussian_forward(self, x: Tensor) -> Dict[str, Tensor]:
        """[N, L] -> {name: [N, C_b]}: the decoder applied row by row (``misplat_feature_decode``, channels last)."""
        if x.dim() != 2:
            raise ValueError(f"per_gaussian_forward: x must be [N, L], got {tuple(x.shape)}")
        n = int(x.shape[0])
        dims = {name: (conv.out_channels, n, 1) for name, conv in self.feature_branch_dict.items()}
        out = feature_decode(x.reshape(n, 1, x.shape[1]), self, dims, (n, 1), channels_last=True)
        return {name: t.reshape(n, -1) for name, t in out.items()}


Decoder = Union[TwoLayerMLP, Tuple[Tensor, Tensor, Mapping[str, Tuple[Tensor, Tensor]]]]


def _check_sizes(latent: int, hidden: int, dims: Sequence[Sequence[int]], what: str) -> None:
    if not 1 <= int(latent) <= MAX_LATENT:
        raise ValueError(f"{what}: the latent width must be 1..{MAX_LATENT}, got {latent}")
    if not 1 <= int(hidden) <= MAX_HIDDEN:
        raise ValueError(f"{what}: the hidden width must be 1..{MAX_HIDDEN}, got {hidden}")
    if not 1 <= len(dims) <= MAX_BRANCHES:
        raise ValueError(f"{what}: 1..{MAX_BRANCHES} feature branches, got {len(dims)}")
    for d in dims:
        if len(d) != 3 or min(int(v) for v in d) < 1:
            raise ValueError(f"{what}: a branch's dims must be (C, H, W) with every entry >= 1, got {tuple(d)}")


def _flat(decoder: Decoder):
    if isinstance(decoder, TwoLayerMLP):
        return decoder.flat()
    if not (isinstance(decoder, (tuple, list)) and len(decoder) == 3 and isinstance(decoder[2], Mapping)):
        raise ValueError("decoder must be a TwoLayerMLP or (w_hidden, b_hidden, {name: (w_out, b_out)})")
    return decoder[0], decoder[1], dict(decoder[2])


def _features_view(features: Tensor, what: str) -> Tuple[Tensor, int]:
    """[H, W, L] float32 whose pixels are ``stride`` floats apart and whose channels are adjacent (a channel slice of a
    wider contiguous image is read in place); anything else is copied once."""
    if features.dim() != 3:
        raise ValueError(f"{what}: features must be [H, W, L], got {tuple(features.shape)}")
    if features.dtype != torch.float32:
        raise ValueError(f"{what}: features must be float32, got {features.dtype}")
    H, W, L = features.shape
    if H < 1 or W < 1:
        raise ValueError(f"{what}: empty feature image {tuple(features.shape)}")
    if H * W > 2 ** 28 or W * L >= 2 ** 31:
        raise ValueError(f"{what}: a feature image of more than 2^28 pixels or 2^31 floats a row {tuple(features.shape)}")
    sy, sx, sl = features.stride()
    if L > 0 and (sl == 1 or L == 1) and sx >= L and sy == W * sx:
        return features, int(sx)
    return features.contiguous(), int(L)


def _prepare(features: Tensor, decoder: Decoder, dims: Mapping[str, Sequence[int]], main_hw: Sequence[int], what: str):
    w_h, b_h, branches = _flat(decoder)
    names = list(dims)
    if set(names) != set(branches):
        raise ValueError(f"{what}: the decoder's branches {sorted(branches)} and the feature names {sorted(names)} differ")
    if w_h.dim() != 2 or b_h.shape != (w_h.shape[0],):
        raise ValueError(f"{what}: w_hidden must be [Hd, L] and b_hidden [Hd], got {tuple(w_h.shape)} and {tuple(b_h.shape)}")
    hidden, latent = int(w_h.shape[0]), int(w_h.shape[1])
    dlist = [tuple(int(v) for v in dims[n]) for n in names]
    _check_sizes(latent, hidden, dlist, what)
    if len(main_hw) != 2 or min(int(v) for v in main_hw) < 1:
        raise ValueError(f"{what}: the main map's size must be (H, W) >= 1, got {tuple(main_hw)}")
    if features.dim() == 3 and features.shape[2] != latent:
        raise ValueError(f"{what}: features of width {features.shape[2]} against a decoder of latent width {latent}")
    ws, bs = [], []
    for n, d in zip(names, dlist):
        w_o, b_o = branches[n]
        if tuple(w_o.shape) != (d[0], hidden) or tuple(b_o.shape) != (d[0],):
            raise ValueError(f"{what}: branch {n!r}: w_out {tuple(w_o.shape)} / b_out {tuple(b_o.shape)} do not fit "
                             f"C = {d[0]}, Hd = {hidden}")
        ws.append(w_o)
        bs.append(b_o)
    feats, stride = _features_view(features, what)
    params = [w_h, b_h] + ws + bs
    for t in params:
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: decoder parameters must be float32, got {t.dtype}")
    require_gpu(feats, *params)
    return feats, stride, names, dlist, latent, hidden, w_h, b_h, ws, bs


def _ptr_array(tensors: Sequence[Tensor]):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _dims_array(dlist):
    flat = [v for d in dlist for v in d]
    return (C.c_int32 * len(flat))(*flat)


def _scratch(lib, latent, hidden, main_hw, dlist, decode_only: bool, dev, what: str) -> Tensor:
    n = int(lib.misplat_featloss_scratch_floats(latent, hidden, int(main_hw[0]), int(main_hw[1]), len(dlist), _dims_array(dlist),
                                                int(decode_only)))
    if n < 0:
        raise ValueError(f"{what}: sizes outside the kernels' limits (main map {tuple(main_hw)}, branches {dlist})")
    return torch.empty(n, device=dev, dtype=torch.float32)


class _FeatureLoss(torch.autograd.Function):
    """``get_loss_dict``'s feature term as ONE autograd node: forward = four or five launches, backward = six, instead of
    the ~30 small launches each way of the op chain (interpolate, two convolutions, cosine_similarity, mean, per branch)."""

    @staticmethod
    def forward(ctx, features, stride, meta, w_h, b_h, *rest):
        lib = _lib.load()
        names, dlist, main_hw, weights, lam = meta
        nb = len(names)
        ws, bs, gts = rest[:nb], rest[nb:2 * nb], rest[2 * nb:]
        H, W, L = (int(v) for v in features.shape)
        hidden = int(w_h.shape[0])
        dev = features.device
        # (views of the module's [.., 1, 1] convolution weights are contiguous already; a flat tuple may not be)
        w_h, b_h = w_h.contiguous(), b_h.contiguous()
        ws, bs = [t.contiguous() for t in ws], [t.contiguous() for t in bs]
        scratch = _scratch(lib, L, hidden, main_hw, dlist, False, dev, "feature_loss")
        loss = torch.empty((), device=dev, dtype=torch.float32)
        sums = torch.empty(nb, device=dev, dtype=torch.float32)
        wts = (C.c_float * nb)(*weights)
        run("misplat_featloss_fwd", H, W, L, stride, C.c_void_p(features.data_ptr()), hidden, ptr(w_h), ptr(b_h), main_hw[0],
            main_hw[1], nb, _dims_array(dlist), _ptr_array(ws), _ptr_array(bs), _ptr_array(gts), wts, lam, ptr(scratch),
            ptr(sums), ptr(loss))
        ctx.save_for_backward(w_h, scratch, *ws, *bs, *gts)
        ctx.meta = (H, W, L, hidden, nb, dlist, tuple(main_hw), tuple(weights), float(lam))
        ctx.branch_sums = sums
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, g):
        H, W, L, hidden, nb, dlist, main_hw, weights, lam = ctx.meta
        none = (None,) * (5 + 3 * nb)
        if g is None:
            return none
        saved = ctx.saved_tensors
        w_h, scratch = saved[0], saved[1]
        ws, bs, gts = saved[2:2 + nb], saved[2 + nb:2 + 2 * nb], saved[2 + 2 * nb:]
        dev = w_h.device
        g = g.to(torch.float32).contiguous()
        v_features = torch.empty(H, W, L, device=dev, dtype=torch.float32)
        v_wh, v_bh = torch.empty_like(w_h), torch.empty(hidden, device=dev, dtype=torch.float32)
        v_ws, v_bs = [torch.empty_like(t) for t in ws], [torch.empty_like(t) for t in bs]
        wts = (C.c_float * nb)(*weights)
        run("misplat_featloss_bwd", H, W, L, hidden, ptr(w_h), main_hw[0], main_hw[1], nb, _dims_array(dlist), _ptr_array(ws),
            _ptr_array(bs), _ptr_array(gts), wts, lam, ptr(scratch), ptr(g), ptr(v_features), ptr(v_wh), ptr(v_bh),
            _ptr_array(v_ws), _ptr_array(v_bs))
        return (v_features, None, None, v_wh, v_bh, *v_ws, *v_bs, *((None,) * nb))


def feature_loss(features: Tensor, decoder: Decoder, gt_dict: Mapping[str, Tensor], main: str,
                 features_regularization_lambda: float = 0.1, features_loss_lambda: float = 1e-3) -> Tensor:
    """``features_loss`` of the features model (rade_features_model.py:545-584) as a device scalar with gradients to
    ``features`` and every decoder parameter:

        features_loss_lambda * sum_b weight_b * mean_pixels(1 - cos(p_b, gt_b)),   weight_main = 1, others = regularization

    ``features`` [H, W, L] float32 on the GPU (a channel slice of a wider image is read in place); ``decoder`` a
    ``TwoLayerMLP`` or ``(w_hidden [Hd, L], b_hidden [Hd], {name: (w_out [C_b, Hd], b_out [C_b])})``; ``gt_dict`` name ->
    [C_b, H_b, W_b], channel-major, one entry per branch; ``main`` names the branch whose (H_b, W_b) is the decoder's working
    resolution.  The per-branch sums of 1 - cos of the last call are on the returned tensor's ``grad_fn.branch_sums``."""
    if main not in gt_dict:
        raise ValueError(f"feature_loss: the main branch {main!r} is not among the ground-truth features {sorted(gt_dict)}")
    for n, t in gt_dict.items():
        if t.dim() != 3:
            raise ValueError(f"feature_loss: ground truth {n!r} must be [C, H, W], got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"feature_loss: ground truth {n!r} must be float32, got {t.dtype}")
    dims = {n: tuple(t.shape) for n, t in gt_dict.items()}
    main_hw = dims[main][1:]
    feats, stride, names, dlist, _, _, w_h, b_h, ws, bs = _prepare(features, decoder, dims, main_hw, "feature_loss")
    gts = [gt_dict[n] for n in names]
    require_gpu(*gts)
    gts = [t.contiguous() for t in gts]
    weights = tuple(1.0 if n == main else float(features_regularization_lambda) for n in names)
    meta = (names, dlist, tuple(int(v) for v in main_hw), weights, float(features_loss_lambda))
    return _FeatureLoss.apply(feats, stride, meta, w_h, b_h, *ws, *bs, *gts)


@torch.no_grad()
def feature_decode(features: Tensor, decoder: Decoder, dims: Mapping[str, Sequence[int]], main_hw: Sequence[int],
                   channels_last: bool = False) -> Dict[str, Tensor]:
    """The decoder's predictions (inference, no gradient): ``features`` [H, W, L] is resized bilinearly to ``main_hw``, goes
    through the hidden layer, and every branch of ``dims`` (name -> (C_b, H_b, W_b)) is evaluated at its own (H_b, W_b) --
    what resizing the branch's prediction from ``main_hw`` gives.  Returns name -> [C_b, H_b, W_b] (or [H_b * W_b, C_b] with
    ``channels_last``)."""
    feats, stride, names, dlist, latent, hidden, w_h, b_h, ws, bs = _prepare(features, decoder, dims, main_hw, "feature_decode")
    lib = _lib.load()
    dev = feats.device
    H, W, L = (int(v) for v in feats.shape)
    w_h, b_h = w_h.detach().contiguous(), b_h.detach().contiguous()
    ws, bs = [t.detach().contiguous() for t in ws], [t.detach().contiguous() for t in bs]
    scratch = _scratch(lib, L, hidden, main_hw, dlist, True, dev, "feature_decode")
    outs = [torch.empty((d[1] * d[2], d[0]) if channels_last else d, device=dev, dtype=torch.float32) for d in dlist]
    run("misplat_feature_decode", H, W, L, stride, C.c_void_p(feats.data_ptr()), hidden, ptr(w_h), ptr(b_h), int(main_hw[0]),
        int(main_hw[1]), len(names), _dims_array(dlist), _ptr_array(ws), _ptr_array(bs), _ptr_array(outs), int(channels_last),
        ptr(scratch))
    return dict(zip(names, outs))
