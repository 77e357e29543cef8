"""Evaluation metrics (plumbing around csrc/evalmetrics.hip; no kernels and no arithmetic here).

How good a render is, per view, for the views ``RadegsModel.render_views`` already stacks on the device: PSNR, SSIM, MSE and
L1 of the images, the angular error of the normal maps and the depth errors of Eigen et al. 2014.  The image scores are what
nerfstudio's Splatfacto reports from ``get_metrics_dict`` and ``get_image_metrics_and_images`` (torchmetrics'
``PeakSignalNoiseRatio(data_range=1.0)`` and ``structural_similarity_index_measure``) [UNVERIFIED-UPSTREAM]; the SSIM is the
training loss's valid-region index.  ``mean_angular_error`` is collab_splats/utils/utils.py:63-81.  DESIGN.md section 34.

``color_correct`` / ``color_corrected_metrics`` (csrc/colorcorrect.hip) warp a render onto its ground
truth's colours before it is scored: Splatfacto's ``color_corrected_metrics``, for models trained with the bilateral grid.

Every metric is two launches on the current stream (the colour correction three per round) and returns device tensors; none
reads anything back to the host.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._lib import ptr, require_gpu, run

MAX_VIEWS = 65535
SSIM_WINDOW = 11


def _views(t: Tensor, channels: Optional[int], what: str, name: str) -> Tensor:
    """[B, H, W, channels] from that or [H, W, channels]; channels None: [B, H, W] from that or [B, H, W, 1]."""
    if not isinstance(t, Tensor):
        raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if channels is None:
        if t.dim() == 4 and t.shape[-1] == 1:
            t = t[..., 0]
        if t.dim() != 3:
            raise ValueError(f"{what}: {name} must be [B, H, W] or [B, H, W, 1], got {tuple(t.shape)}")
    else:
        if t.dim() == 3:
            t = t[None]
        if t.dim() != 4 or t.shape[-1] != channels:
            raise ValueError(f"{what}: {name} must be [B, H, W, {channels}] or [H, W, {channels}], got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
    return t


def _sizes(pred: Tensor, gt: Tensor, what: str) -> Tuple[int, int, int]:
    if pred.shape != gt.shape:
        raise ValueError(f"{what}: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape")
    B, H, W = (int(v) for v in pred.shape[:3])
    if not 1 <= B <= MAX_VIEWS:
        raise ValueError(f"{what}: 1..{MAX_VIEWS} views per call, got {B}")
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"{what}: H W must be in 1..2^31 - 1, got {H} x {W}")
    return B, H, W


def _valid(valid: Optional[Tensor], shape, what: str) -> Optional[Tensor]:
    if valid is None:
        return None
    if valid.dim() == 4 and valid.shape[-1] == 1:
        valid = valid[..., 0]
    if valid.dim() == 2 and shape[0] == 1:
        valid = valid[None]
    if tuple(valid.shape) != tuple(shape):
        raise ValueError(f"{what}: valid must be [B, H, W] = {tuple(shape)}, got {tuple(valid.shape)}")
    if valid.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{what}: valid must be bool or uint8, got {valid.dtype}")
    require_gpu(valid)
    valid = valid.contiguous()
    return valid.view(torch.uint8) if valid.dtype == torch.bool else valid


def _scratch(fn, B: int, H: int, W: int, dev, what: str) -> Tensor:
    n = int(fn(B, H, W))
    if n < 0:
        raise ValueError(f"{what}: sizes outside the kernels' limits ({B} views of {H} x {W})")
    return torch.empty(n, device=dev, dtype=torch.float32)


@torch.no_grad()
def image_metrics(pred: Tensor, gt: Tensor, ssim: bool = True) -> Dict[str, Tensor]:
    """Per-view ``{"psnr", "ssim", "mse", "l1"}`` ([B] float32 device tensors; no ``"ssim"`` with ``ssim=False``) of
    ``pred`` against ``gt``, both [B, H, W, 3] or [H, W, 3] float32 on the GPU with values in 0..1:

        mse = mean (pred - gt)^2,  l1 = mean |pred - gt|,  psnr = -10 log10(mse)  (+inf for identical images),
        ssim = the mean over the (H - 10) x (W - 10) valid window positions and the channels of the 11-tap gaussian SSIM

    ``ssim=True`` needs H, W >= 11 (``ValueError`` before any launch)."""
    what = "image_metrics"
    pred, gt = _views(pred, 3, what, "pred"), _views(gt, 3, what, "gt")
    B, H, W = _sizes(pred, gt, what)
    if ssim and (H < SSIM_WINDOW or W < SSIM_WINDOW):
        raise ValueError(f"{what}: SSIM needs H, W >= {SSIM_WINDOW} (one window position), got {H} x {W}; pass ssim=False")
    require_gpu(pred, gt)
    lib = _lib.load()
    pred, gt = pred.detach().contiguous(), gt.detach().contiguous()
    scratch = _scratch(lib.misplat_eval_image_scratch_floats, B, H, W, pred.device, what)
    out = torch.empty(B, 4, device=pred.device, dtype=torch.float32)
    run("misplat_eval_image", B, H, W, ptr(pred), ptr(gt), int(bool(ssim)), ptr(scratch), ptr(out))
    res = {"psnr": out[:, 3], "mse": out[:, 0], "l1": out[:, 1]}
    if ssim:
        res["ssim"] = out[:, 2]
    return res


def psnr(pred: Tensor, gt: Tensor) -> Tensor:
    """[B] PSNR in dB (``image_metrics(pred, gt, ssim=False)["psnr"]``)."""
    return image_metrics(pred, gt, ssim=False)["psnr"]


def ssim(pred: Tensor, gt: Tensor) -> Tensor:
    """[B] SSIM (``image_metrics(pred, gt)["ssim"]``)."""
    return image_metrics(pred, gt, ssim=True)["ssim"]


@torch.no_grad()
def normal_metrics(pred: Tensor, gt: Tensor, valid: Optional[Tensor] = None, encoded: bool = False, normalize: bool = True,
                   return_map: bool = False) -> Dict[str, Tensor]:
    """Per-view angular error of normal maps [B, H, W, 3] (or [H, W, 3]) float32 on the GPU:
    ``{"mean" (radians), "a11.25", "a22.5", "a30" (fractions of the counted pixels below that many degrees), "count"}``, all [B]
    float32, and with ``return_map`` ``"map"`` [B, H, W]: every pixel's angle, NaN where excluded.

    ``encoded``: the maps hold 0..1 colours, decoded with v <- 2 v - 1.  ``normalize``: both vectors are scaled to unit length,
    and a pixel with a squared length <= 1e-12 is excluded.  ``valid`` (or None) [B, H, W] bool: False excludes a pixel.  A view
    without a counted pixel gives NaN and count 0."""
    what = "normal_metrics"
    pred, gt = _views(pred, 3, what, "pred"), _views(gt, 3, what, "gt")
    B, H, W = _sizes(pred, gt, what)
    valid = _valid(valid, (B, H, W), what)
    require_gpu(pred, gt)
    lib = _lib.load()
    pred, gt = pred.detach().contiguous(), gt.detach().contiguous()
    scratch = _scratch(lib.misplat_eval_pixels_scratch_floats, B, H, W, pred.device, what)
    out = torch.empty(B, 5, device=pred.device, dtype=torch.float32)
    amap = torch.empty(B, H, W, device=pred.device, dtype=torch.float32) if return_map else None
    run("misplat_eval_normals", B, H, W, ptr(pred), ptr(gt), ptr(valid), int(bool(encoded)), int(bool(normalize)), ptr(amap),
        ptr(scratch), ptr(out))
    res = {"mean": out[:, 0], "a11.25": out[:, 1], "a22.5": out[:, 2], "a30": out[:, 3], "count": out[:, 4]}
    if return_map:
        res["map"] = amap
    return res


def mean_angular_error(pred: Tensor, gt: Tensor) -> Tensor:
    """collab_splats/utils/utils.py:63-81: [B, C, H, W] predicted and reference normals -> [B, H, W] angles in radians,
    ``acos(clamp(sum_c gt * pred, -1, 1))``; nothing is decoded, normalised or masked."""
    what = "mean_angular_error"
    for name, t in (("pred", pred), ("gt", gt)):
        if not isinstance(t, Tensor) or t.dim() != 4 or t.shape[1] != 3:
            raise ValueError(f"{what}: {name} must be [B, 3, H, W], got {tuple(t.shape) if isinstance(t, Tensor) else type(t).__name__}")
    return normal_metrics(pred.permute(0, 2, 3, 1), gt.permute(0, 2, 3, 1), None, False, False, True)["map"]


@torch.no_grad()
def depth_metrics(pred: Tensor, gt: Tensor, valid: Optional[Tensor] = None, max_depth: Optional[float] = None) -> Dict[str, Tensor]:
    """Per-view depth errors (Eigen et al. 2014) of depth maps [B, H, W] or [B, H, W, 1] float32 on the GPU:
    ``{"abs_rel", "sq_rel", "rmse", "rmse_log", "delta1", "delta2", "delta3", "count"}``, all [B] float32.  A pixel counts where
    ``valid`` (or None) is True, both depths are finite and > 0 and gt <= ``max_depth`` (None or <= 0: no limit):

        abs_rel = mean |p - g| / g,  sq_rel = mean (p - g)^2 / g,  rmse = sqrt(mean (p - g)^2),
        rmse_log = sqrt(mean (ln p - ln g)^2),  delta_k = fraction with max(p / g, g / p) < 1.25^k

    A view without a counted pixel gives NaN and count 0."""
    what = "depth_metrics"
    pred, gt = _views(pred, None, what, "pred"), _views(gt, None, what, "gt")
    B, H, W = _sizes(pred, gt, what)
    valid = _valid(valid, (B, H, W), what)
    require_gpu(pred, gt)
    lib = _lib.load()
    pred, gt = pred.detach().contiguous(), gt.detach().contiguous()
    scratch = _scratch(lib.misplat_eval_pixels_scratch_floats, B, H, W, pred.device, what)
    out = torch.empty(B, 8, device=pred.device, dtype=torch.float32)
    run("misplat_eval_depth", B, H, W, ptr(pred), ptr(gt), ptr(valid), 0.0 if max_depth is None else float(max_depth),
        ptr(scratch), ptr(out))
    names = ("abs_rel", "sq_rel", "rmse", "rmse_log", "delta1", "delta2", "delta3", "count")
    return {k: out[:, i] for i, k in enumerate(names)}


# ------------------------------------------------------------------------------------------- colour-corrected metrics
MAX_COLOR_ITERS = 64


@torch.no_grad()
def color_correct(pred: Tensor, gt: Tensor, num_iters: int = 5, eps: float = 0.5 / 255, return_fit: bool = False):
    """``pred`` warped onto ``gt``'s colours (csrc/colorcorrect.hip): multinerf's ``color_correct`` as
    nerfstudio carries it for Splatfacto's ``color_corrected_metrics``, restated from the published method
    [UNVERIFIED-UPSTREAM].  Both [B, H, W, 3] or [H, W, 3] float32 on the GPU with values in 0..1; the result has ``pred``'s
    shape.  ``num_iters`` times, per view and output channel: a least-squares fit of gt's channel on the 10 monomials (r^2,
    rg, rb, g^2, gb, b^2, r, g, b, 1) of the current image over the pixels where pred's channel, the current image's and
    gt's all lie in [eps, 1 - eps] (fp64 normal equations, eigenvalues <= 2^-46 of the largest dropped, minimum norm), then
    the fit applied to every pixel and clipped to 0..1.  ``num_iters=0`` returns a copy of ``pred``.

    With ``return_fit``: ``(corrected, {"warps": [B, num_iters, 10, 3] float64, "counts": [B, num_iters, 3] int64})``, every
    round's coefficients and the number of pixels that counted.  Three launches per round, no host read."""
    what = "color_correct"
    single = isinstance(pred, Tensor) and pred.dim() == 3
    pred, gt = _views(pred, 3, what, "pred"), _views(gt, 3, what, "gt")
    B, H, W = _sizes(pred, gt, what)
    if isinstance(num_iters, bool) or not isinstance(num_iters, int) or not 0 <= num_iters <= MAX_COLOR_ITERS:
        raise ValueError(f"{what}: num_iters must be an int in 0..{MAX_COLOR_ITERS}, got {num_iters!r}")
    eps = float(eps)
    if not 0.0 <= eps < 0.5:
        raise ValueError(f"{what}: eps must be in [0, 0.5), got {eps}")
    require_gpu(pred, gt)
    lib = _lib.load()
    pred, gt = pred.detach().contiguous(), gt.detach().contiguous()
    scratch = _scratch(lib.misplat_colorcorrect_scratch_floats, B, H, W, pred.device, what)
    out = torch.empty_like(pred)
    warps = torch.empty(B, num_iters, 10, 3, device=pred.device, dtype=torch.float64)
    counts = torch.empty(B, num_iters, 3, device=pred.device, dtype=torch.int64)
    run("misplat_colorcorrect", B, H, W, ptr(pred), ptr(gt), num_iters, eps, ptr(scratch), ptr(out), ptr(warps), ptr(counts))
    if single:
        out = out[0]
    return (out, {"warps": warps, "counts": counts}) if return_fit else out


def color_corrected_metrics(pred: Tensor, gt: Tensor, ssim: bool = True, num_iters: int = 5, eps: float = 0.5 / 255) -> Dict[str, Tensor]:
    """Per-view ``{"cc_psnr", "cc_ssim", "cc_mse", "cc_l1"}`` ([B] float32 device tensors; no ``"cc_ssim"`` with
    ``ssim=False``): ``image_metrics(color_correct(pred, gt, num_iters, eps), gt, ssim)`` under Splatfacto's names."""
    return {"cc_" + k: v for k, v in image_metrics(color_correct(pred, gt, num_iters, eps), gt, ssim).items()}
