"""Restatement of the evaluation metrics (collab_splats_amd/metrics.py, csrc/evalmetrics.hip) in plain torch, written from
their specification and dtype-generic: run in float64 it is the tests' oracle, run in float32 it is
the yardstick whose own error sets the tests' bounds.  TEST INFRASTRUCTURE: nothing under collab_splats_amd imports it.

Images are [B, H, W, 3], normal maps [B, H, W, 3], depth maps [B, H, W]; every result is per view.  The SSIM is written the
way a user would run it in torch -- separable depthwise convolutions of x, y, xx, yy, xy over the batch -- and is also what
scripts/metrics_bench.py times as the baseline.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
THRESHOLDS_DEG = (11.25, 22.5, 30.0)
DELTAS = (1.25, 1.25 ** 2, 1.25 ** 3)
EPS_LENGTH2 = 1e-12


def gauss_window(dtype=torch.float32) -> torch.Tensor:
    """The 11 taps of the project's window (csrc/ssimwin.h, ``make_window``), operation by operation in float32:
    exp(-(c^2) / 4.5) rounded to float32, the taps added ONE AFTER THE OTHER from the left, each tap divided by that sum.
    ``oracle/ssim_oracle.gauss_window`` states the same taps with ``torch.sum``, which adds in another order: its sum is one
    float32 step lower, and every tap one step or none apart.  An SSIM is sensitive to exactly this -- with sum(w) = 1 + d a
    window variance E[xx] - mx^2 of a patch of brightness c moves by c^2 d, against C2 = 8.1e-4 -- so a restatement of the
    kernels has to take the kernels' window (tests/test_metrics_host.py measures what the other one changes)."""
    f32 = np.float32
    taps = [f32(math.exp(float(f32(-(f32(i - 5) * f32(i - 5))) / f32(4.5)))) for i in range(11)]
    total = f32(0.0)
    for t in taps:
        total = f32(total + t)
    return torch.tensor([float(f32(t / total)) for t in taps], dtype=torch.float32).to(dtype)


def _filter(x: torch.Tensor, win: torch.Tensor) -> torch.Tensor:
    """x [B, 3, H, W]: the window along H, then along W, no padding."""
    ch = x.shape[1]
    x = F.conv2d(x, win.view(1, 1, -1, 1).repeat(ch, 1, 1, 1), groups=ch)
    return F.conv2d(x, win.view(1, 1, 1, -1).repeat(ch, 1, 1, 1), groups=ch)


def ssim(pred: torch.Tensor, gt: torch.Tensor, window: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B]: the mean of the index over the (H - 10) x (W - 10) window positions and the channels.  ``window`` (or None: the
    project's, ``gauss_window``): 11 float32 taps."""
    x, y = pred.permute(0, 3, 1, 2), gt.permute(0, 3, 1, 2)
    win = (gauss_window() if window is None else window).to(x.dtype).to(x.device)
    mx, my = _filter(x, win), _filter(y, win)
    sxx = _filter(x * x, win) - mx * mx
    syy = _filter(y * y, win) - my * my
    sxy = _filter(x * y, win) - mx * my
    index = ((2 * mx * my + C1) / (mx * mx + my * my + C1)) * ((2 * sxy + C2) / (sxx + syy + C2))
    return index.flatten(1).mean(-1)


def image_metrics(pred: torch.Tensor, gt: torch.Tensor, dtype=torch.float64, with_ssim: bool = True) -> Dict[str, torch.Tensor]:
    p, g = pred.to(dtype), gt.to(dtype)
    d = p - g
    mse = (d * d).flatten(1).mean(-1)
    out = {"mse": mse, "l1": d.abs().flatten(1).mean(-1), "psnr": -10.0 * torch.log10(mse)}
    if with_ssim:
        out["ssim"] = ssim(p, g)
    return out


def normal_metrics(pred: torch.Tensor, gt: torch.Tensor, valid: Optional[torch.Tensor] = None, encoded: bool = False,
                   normalize: bool = True, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """{"mean", "a11.25", "a22.5", "a30", "count", "map"}: [B] each, map [B, H, W] with NaN where excluded."""
    a, b = pred.to(dtype), gt.to(dtype)
    if encoded:
        a, b = 2 * a - 1, 2 * b - 1
    ok = torch.ones(a.shape[:3], dtype=torch.bool) if valid is None else valid.bool().clone()
    if normalize:
        la, lb = (a * a).sum(-1), (b * b).sum(-1)
        ok &= (la > EPS_LENGTH2) & (lb > EPS_LENGTH2)
        one = torch.ones_like(la)
        a = a / torch.sqrt(torch.where(ok, la, one))[..., None]
        b = b / torch.sqrt(torch.where(ok, lb, one))[..., None]
    theta = torch.acos(torch.clamp((a * b).sum(-1), -1.0, 1.0))
    count = ok.flatten(1).sum(-1)
    n = count.to(dtype)                                                       # 0 / 0 = NaN for a view without a counted pixel
    out = {"mean": torch.where(ok, theta, torch.zeros_like(theta)).flatten(1).sum(-1) / n, "count": n,
           "map": torch.where(ok, theta, torch.full_like(theta, float("nan")))}
    for deg in THRESHOLDS_DEG:
        out[f"a{deg:g}"] = (ok & (theta < math.radians(deg))).flatten(1).sum(-1).to(dtype) / n
    return out


def mean_angular_error(pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """[B, C, H, W] -> [B, H, W]: the angle map without decoding, normalisation or mask."""
    return normal_metrics(pred.permute(0, 2, 3, 1), gt.permute(0, 2, 3, 1), None, False, False, pred.dtype)["map"]


def depth_valid(pred: torch.Tensor, gt: torch.Tensor, valid: Optional[torch.Tensor], max_depth: Optional[float]) -> torch.Tensor:
    ok = torch.isfinite(pred) & torch.isfinite(gt) & (pred > 0) & (gt > 0)
    if valid is not None:
        ok &= valid.bool()
    if max_depth is not None and max_depth > 0:
        ok &= gt <= max_depth
    return ok


def depth_metrics(pred: torch.Tensor, gt: torch.Tensor, valid: Optional[torch.Tensor] = None, max_depth: Optional[float] = None,
                  dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """Eigen et al. 2014: {"abs_rel", "sq_rel", "rmse", "rmse_log", "delta1", "delta2", "delta3", "count"}, [B] each."""
    ok = depth_valid(pred, gt, valid, max_depth)
    one = torch.ones((), dtype=dtype)
    p, g = torch.where(ok, pred.to(dtype), one), torch.where(ok, gt.to(dtype), one)       # excluded pixels add exact zeros
    n = ok.flatten(1).sum(-1).to(dtype)
    mean = lambda t: t.flatten(1).sum(-1) / n                                              # noqa: E731
    d, l = p - g, torch.log(p) - torch.log(g)
    out = {"abs_rel": mean(d.abs() / g), "sq_rel": mean(d * d / g), "rmse": torch.sqrt(mean(d * d)),
           "rmse_log": torch.sqrt(mean(l * l)), "count": n}
    ratio = torch.maximum(p / g, g / p)
    for k, t in enumerate(DELTAS):
        out[f"delta{k + 1}"] = (ok & (ratio < t)).flatten(1).sum(-1).to(dtype) / n
    return out
