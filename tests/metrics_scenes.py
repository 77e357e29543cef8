"""Seeded scenes of the evaluation-metric tests (tests/test_metrics_host.py checks every stated condition on the CPU;
tests/test_metrics_gpu.py runs the kernels on them).  Oracles (the fp64 restatement) and yardsticks (its fp32 run) are computed
once per scene, shared and never written to.

Image scenes: every shape of SHAPES with B = 1 and 3 (different content per view) and four contents:
  random     independent uniform pairs;
  near       a near-identical pair: gt + 1e-3 * gaussian noise, clamped (PSNR ~ 60 dB);
  smooth     a smooth image (low-frequency sinusoids) plus 0.05 * gaussian noise, clamped;
  identical  the same tensor twice (mse exactly 0, psnr +inf).
CONSTANT images are left out of the parity scenes on purpose: for 0.25 against 0.75 the fp32 restatement ITSELF is 1.3e-4
absolute off on SSIM (E[xx] - mx^2 cancels completely and what is left is rounding noise over C2 = 9e-4), so it is no
yardstick there.

Normal scenes: gt is pred rotated by an angle drawn from [1, 179] degrees that keeps 0.5 degrees away from the thresholds
11.25, 22.5 and 30 -- the oracle's angles are then at least 0.05 degrees from every threshold and the three fractions and the
count are exact integers over a count.  Depth scenes: pred = gt * r with r at least 1e-3 (relative) from 1.25^k and 1.25^-k, so
the delta fractions are exact.
"""
from __future__ import annotations

import functools
import math

import torch

import metrics_restatement as R

SHAPES = [(11, 11), (26, 26), (27, 43), (12, 37), (135, 240)]
BATCHES = [1, 3]
CONTENTS = ["random", "near", "smooth", "identical"]
PIXEL_SHAPES = [(5, 7), (17, 33), (64, 64)]
PIXEL_B = 3
ANGLE_GAP_DEG = 0.5
RATIO_GAP = 1e-3


def _seed(shape, B, tag: int) -> int:
    return 1_000_003 * tag + 10_007 * shape[0] + 101 * shape[1] + B


def _smooth(B: int, H: int, W: int, g: torch.Generator) -> torch.Tensor:
    y = torch.arange(H, dtype=torch.float64)[None, :, None, None] / 16.0
    x = torch.arange(W, dtype=torch.float64)[None, None, :, None] / 16.0
    ph = torch.rand(B, 1, 1, 3, 4, generator=g, dtype=torch.float64) * 2 * math.pi
    fr = 0.5 + torch.rand(B, 1, 1, 3, 4, generator=g, dtype=torch.float64)
    img = 0.5 + 0.2 * torch.sin(fr[..., 0] * x + ph[..., 0]) * torch.cos(fr[..., 1] * y + ph[..., 1]) \
        + 0.15 * torch.sin(fr[..., 2] * (x + y) + ph[..., 2]) + 0.1 * torch.cos(fr[..., 3] * (x - y) + ph[..., 3])
    return img.to(torch.float32)


@functools.lru_cache(maxsize=None)
def image_scene(shape, B: int, content: str):
    """(pred, gt): [B, H, W, 3] float32 in 0..1."""
    H, W = shape
    g = torch.Generator().manual_seed(_seed(shape, B, CONTENTS.index(content)))
    if content == "random":
        gt = torch.rand(B, H, W, 3, generator=g)
        pred = torch.rand(B, H, W, 3, generator=g)
    elif content == "near":
        gt = torch.rand(B, H, W, 3, generator=g)
        pred = (gt + 1e-3 * torch.randn(B, H, W, 3, generator=g)).clamp(0.0, 1.0)
    elif content == "smooth":
        gt = _smooth(B, H, W, g)
        pred = (gt + 0.05 * torch.randn(B, H, W, 3, generator=g)).clamp(0.0, 1.0)
    elif content == "identical":
        gt = (_smooth(B, H, W, g) + 0.05 * torch.randn(B, H, W, 3, generator=g)).clamp(0.0, 1.0)
        pred = gt.clone()
    else:
        raise KeyError(content)
    return pred.contiguous(), gt.contiguous()


@functools.lru_cache(maxsize=None)
def image_oracle(shape, B: int, content: str):
    return R.image_metrics(*image_scene(shape, B, content), dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def image_yardstick(shape, B: int, content: str):
    return R.image_metrics(*image_scene(shape, B, content), dtype=torch.float32)


def view_err(got: torch.Tensor, ref: torch.Tensor, relative: bool) -> float:
    """The largest per-view error: |got - ref| / |ref| (relative) or |got - ref|; inf for a NaN."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    e = (got - ref).abs()
    if relative:
        e = e / ref.abs()
    e = float(e.max())
    return e if e == e else float("inf")


# ------------------------------------------------------------------------------------------------------------ normals
def _angles(n: int, hi: torch.Tensor, g: torch.Generator) -> torch.Tensor:
    """n angles in degrees from [1, hi], none within ANGLE_GAP_DEG of a threshold (redrawn until so)."""
    draw = lambda: 1.0 + (hi - 1.0) * torch.rand(n, generator=g, dtype=torch.float64)      # noqa: E731
    a = draw()
    for _ in range(100):
        bad = torch.zeros(n, dtype=torch.bool)
        for t in R.THRESHOLDS_DEG:
            bad |= (a - t).abs() < ANGLE_GAP_DEG
        if not bool(bad.any()):
            return a
        a = torch.where(bad, draw(), a)
    raise RuntimeError("no admissible angles")


def _unit(n: int, g: torch.Generator) -> torch.Tensor:
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return v / v.norm(dim=-1, keepdim=True)


@functools.lru_cache(maxsize=None)
def normal_scene(shape, quantised: bool = False):
    """{"pred", "gt" [B, H, W, 3] float32 unit vectors (to rounding), "valid" [B, H, W] bool with about a third False}.
    The first half of the angles leans to the small end so that every threshold has pixels on both sides.  ``quantised``: both
    maps are snapped to multiples of 2^-11, so that their 0..1 encoding (v + 1) / 2 and its decoding are exact in float32."""
    H, W = shape
    B, n = PIXEL_B, PIXEL_B * H * W
    g = torch.Generator().manual_seed(_seed(shape, B, 50 + int(quantised)))
    p = _unit(n, g)
    r = _unit(n, g)
    u = r - (r * p).sum(-1, keepdim=True) * p
    u = u / u.norm(dim=-1, keepdim=True)
    small = torch.rand(n, generator=g) < 0.5
    ang = _angles(n, torch.where(small, 45.0, 179.0).double(), g)
    rad = torch.deg2rad(ang)[:, None]
    q = torch.cos(rad) * p + torch.sin(rad) * u
    pred, gt = p.to(torch.float32).view(B, H, W, 3), q.to(torch.float32).view(B, H, W, 3)
    if quantised:
        pred, gt = torch.round(pred * 2048.0) / 2048.0, torch.round(gt * 2048.0) / 2048.0
    valid = torch.rand(B, H, W, generator=g) > 1.0 / 3.0
    return {"pred": pred.contiguous(), "gt": gt.contiguous(), "valid": valid, "angles_deg": ang.view(B, H, W)}


def threshold_margin_deg(theta: torch.Tensor) -> float:
    """The smallest distance, in degrees, of a finite angle (radians) to a threshold."""
    deg = torch.rad2deg(theta[torch.isfinite(theta)].double())
    return min(float((deg - t).abs().min()) for t in R.THRESHOLDS_DEG)


@functools.lru_cache(maxsize=None)
def aligned_scene():
    """[1, 8, 16, 3]: the left half identical unit vectors, the right half opposite ones."""
    g = torch.Generator().manual_seed(77)
    p = _unit(8 * 16, g).to(torch.float32).view(1, 8, 16, 3)
    q = p.clone()
    q[:, :, 8:] = -q[:, :, 8:]
    return p.contiguous(), q.contiguous()


# -------------------------------------------------------------------------------------------------------------- depth
@functools.lru_cache(maxsize=None)
def depth_scene(shape):
    """{"pred", "gt" [B, H, W] float32, "valid" [B, H, W] bool}: gt in 0.5..10, pred = gt * 1.25^e, e in -4..4 kept away from the
    integers 1..3 and -1..-3 by more than RATIO_GAP in the ratio."""
    H, W = shape
    B, n = PIXEL_B, PIXEL_B * H * W
    g = torch.Generator().manual_seed(_seed(shape, B, 60))
    gt = 0.5 + 9.5 * torch.rand(n, generator=g, dtype=torch.float64)
    e = -4.0 + 8.0 * torch.rand(n, generator=g, dtype=torch.float64)
    gap = 3.0 * RATIO_GAP / math.log(1.25)
    near = ((e - torch.round(e)).abs() < gap) & (torch.round(e) != 0) & (torch.round(e).abs() <= 3)
    e = torch.where(near, torch.round(e) + 0.5, e)
    pred = gt * torch.pow(torch.tensor(1.25, dtype=torch.float64), e)
    valid = torch.rand(B, H, W, generator=g) > 1.0 / 3.0
    return {"pred": pred.to(torch.float32).view(B, H, W).contiguous(), "gt": gt.to(torch.float32).view(B, H, W).contiguous(),
            "valid": valid}


def ratio_margin(pred: torch.Tensor, gt: torch.Tensor) -> float:
    """The smallest relative distance of max(p / g, g / p) to a delta threshold, over the pixels with positive finite depths."""
    ok = R.depth_valid(pred, gt, None, None)
    p, g = pred[ok].double(), gt[ok].double()
    ratio = torch.maximum(p / g, g / p)
    return min(float((ratio / t - 1.0).abs().min()) for t in R.DELTAS)


@functools.lru_cache(maxsize=None)
def depth_scene_excluded(shape):
    """depth_scene with pixels that must not count written into the first 33 pixels of every view: a zero, a negative, +inf,
    -inf and a NaN in pred, the same five in gt, and one pixel bad in both -- ``n_bad`` = 11 per view; view 2 has no
    admissible gt at all."""
    sc = depth_scene(shape)
    pred, gt = sc["pred"].clone(), sc["gt"].clone()
    H, W = shape
    bad = [0.0, -1.5, float("inf"), float("-inf"), float("nan")]
    flat_p, flat_g = pred.view(PIXEL_B, -1), gt.view(PIXEL_B, -1)
    assert H * W >= 35
    for k, v in enumerate(bad):
        flat_p[:, 3 * k] = v                                          # pixels 0, 3, 6, 9, 12
        flat_g[:, 3 * k + 16] = v                                     # pixels 16, 19, 22, 25, 28
    flat_p[:, 32] = float("nan")
    flat_g[:, 32] = float("inf")                                      # bad in both
    gt[2] = 0.0
    return {"pred": pred.contiguous(), "gt": gt.contiguous(), "valid": sc["valid"], "n_bad": 11}
