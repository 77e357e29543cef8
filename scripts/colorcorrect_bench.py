"""The colour correction on the MI355X: ``color_correct`` (csrc/colorcorrect.hip: 5 rounds of accumulate,
solve and apply, 15 launches) against the torch formulation of the same algorithm on the same device -- fp64 normal equations
through ``A.T @ A`` on the masked design matrix and ``torch.linalg.eigh`` with the same cut (not ``lstsq``: it has no
rank-revealing driver on the device) -- at 1920 x 1080 with B = 1 and 4, on a seeded smooth-plus-noise pair with a colour warp and
a saturated area.  metrics_bench.py's protocol: both routes run in one process in alternating windows of --steps calls between
device events, after a warm-up of every shape; the median of --rounds windows is reported; the whole measurement runs TWICE, the
difference between the two passes' medians is the spread (the largest over the routes), and
``beats_baseline_by_more_than_the_spread`` says whether the fused call's lead over the torch route is larger than it.  A third
route, ``torch_chunked``, is the torch route with its long products split into 1024 batched ones.  The plain torch route takes
seconds per call at this size: ``--torch-steps`` shortens its windows (its 280 calls per batch size would run for over an hour).  Also recorded: the largest difference between the two routes' images, and what the accumulation
needs (fp64 multiply-adds and bytes per view and round) for a share of peak.  No time is a pass condition.

    python scripts/colorcorrect_bench.py [--steps 20] [--rounds 7] [--batches 1 4] [--out build/colorcorrect_bench.json]

Every window prints a line as it ends (the torch route takes seconds per window at this size).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 1080, 1920
NUM_ITERS, EPS, CUT = 5, 0.5 / 255, 2.0 ** -46


def time_window(fn, steps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / steps


def alternate(routes, steps, rounds):
    """steps: calls per window, per route."""
    times = {k: [] for k in routes}
    for i in range(rounds):
        for k, fn in routes.items():
            times[k].append(time_window(fn, steps[k]))
            print(f"  window {i} {k}: {times[k][-1] * 1e6:.1f} us a call", flush=True)
    return {k: float(np.median(v)) for k, v in times.items()}, times


def make_pair(B, dev):
    """gt: low-frequency sinusoids per view and channel plus 0.02 gaussian noise, with an exactly white and an exactly black
    rectangle; pred: a mixing matrix, an offset and a quadratic term of gt plus 0.03 noise, clamped (some of it saturates)."""
    g = torch.Generator().manual_seed(200 + B)
    y = torch.arange(H, dtype=torch.float32)[None, :, None, None] / 64.0
    x = torch.arange(W, dtype=torch.float32)[None, None, :, None] / 64.0
    ph = torch.rand(B, 1, 1, 3, 3, generator=g) * 2 * math.pi
    fr = 0.5 + torch.rand(B, 1, 1, 3, 3, generator=g)
    gt = 0.5 + 0.25 * torch.sin(fr[..., 0] * x + ph[..., 0]) * torch.cos(fr[..., 1] * y + ph[..., 1]) \
        + 0.25 * torch.sin(fr[..., 2] * (x + y) + ph[..., 2])
    gt = (gt + 0.02 * torch.randn(B, H, W, 3, generator=g)).clamp(0.0, 1.0)
    gt[:, 100:300, 200:700] = 1.0
    gt[:, 700:900, 1200:1800] = 0.0
    M = torch.eye(3) + 0.15 * torch.randn(B, 1, 1, 3, 3, generator=g)
    off, quad = 0.05 * torch.randn(B, 1, 1, 3, generator=g), 0.1 * torch.randn(B, 1, 1, 3, generator=g)
    pred = (gt[..., None, :] @ M)[..., 0, :] + off + quad * gt * gt + 0.03 * torch.randn(B, H, W, 3, generator=g)
    return pred.clamp(0.0, 1.0).contiguous().to(dev), gt.contiguous().to(dev)


@torch.no_grad()
def torch_color_correct(pred, gt, num_iters=NUM_ITERS, eps=EPS, chunks=1):
    """The same algorithm in torch on the device, no host read: the masks multiply the design matrix instead of selecting rows.
    chunks > 1: the [10 x P] . [P x 10] product as ``chunks`` batched products that are then summed -- a tuning a user might
    find: one fp64 product with an inner dimension of two million runs for a quarter of a second."""
    lo = torch.tensor(eps, dtype=torch.float32, device=pred.device)
    hi = 1.0 - lo
    out = []
    for b in range(pred.shape[0]):
        p, g = pred[b].reshape(-1, 3), gt[b].reshape(-1, 3)
        m0 = (p >= lo) & (p <= hi) & (g >= lo) & (g <= hi)
        g64 = g.double()
        x = p
        for _ in range(num_iters):
            r, gr, bl = x.double().unbind(-1)
            A = torch.stack([r * r, r * gr, r * bl, gr * gr, gr * bl, bl * bl, r, gr, bl, torch.ones_like(r)], dim=1)
            m = (m0 & (x >= lo) & (x <= hi)).double()
            ws = []
            for c in range(3):
                Am = A * m[:, c:c + 1]
                if chunks > 1 and A.shape[0] % chunks == 0:
                    G = (Am.view(chunks, -1, 10).transpose(1, 2) @ A.view(chunks, -1, 10)).sum(0)
                    rhs = (Am.view(chunks, -1, 10).transpose(1, 2) @ g64[:, c].reshape(chunks, -1, 1)).sum(0)[:, 0]
                else:
                    G, rhs = Am.T @ A, Am.T @ g64[:, c]
                lam, vec = torch.linalg.eigh(G)
                keep = lam > CUT * lam.max().clamp_min(0.0)
                inv = torch.where(keep, 1.0 / torch.where(keep, lam, torch.ones_like(lam)), torch.zeros_like(lam))
                ws.append(vec @ (inv * (vec.T @ rhs)))
            x = (A @ torch.stack(ws, dim=1)).clamp(0.0, 1.0).float()
        out.append(x.reshape(pred.shape[1:]))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--torch-steps", type=int, default=None, help="calls per window of the plain torch route (default: --steps)")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "colorcorrect_bench.json"))      # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("colorcorrect_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    import collab_splats_amd as m
    dev = torch.device("cuda:0")
    rows = []
    for B in args.batches:
        pred, gt = make_pair(B, dev)
        routes = {"fused": lambda: m.color_correct(pred, gt, NUM_ITERS, EPS),
                  "torch": lambda: torch_color_correct(pred, gt),
                  "torch_chunked": lambda: torch_color_correct(pred, gt, chunks=1024)}
        steps = {"fused": args.steps, "torch": args.torch_steps or args.steps, "torch_chunked": args.steps}
        for k, fn in routes.items():                                   # warm-up of every shape, both routes
            for _ in range(3):
                fn()
            print(f"B = {B}: {k} warmed up, one call {time_window(fn, 1) * 1e6:.1f} us", flush=True)
        a, fit = m.color_correct(pred, gt, NUM_ITERS, EPS, return_fit=True)
        b = routes["torch"]()
        before = m.image_metrics(pred, gt)["psnr"].tolist()
        after = m.image_metrics(a, gt)["psnr"].tolist()
        passes = [alternate(routes, steps, args.rounds) for _ in range(2)]                    # the same code twice
        med = {k: [p[0][k] for p in passes] for k in routes}
        spread = max(abs(med[k][0] - med[k][1]) for k in routes)
        lead = min(med["torch"]) - max(med["fused"])
        row = {"B": B, "H": H, "W": W, "num_iters": NUM_ITERS, "steps": steps, "rounds": args.rounds,
               "fused_s": med["fused"], "torch_s": med["torch"], "torch_chunked_s": med["torch_chunked"], "spread_s": spread,
               "lead_s": lead, "lead_over_chunked_s": min(med["torch_chunked"]) - max(med["fused"]),
               "beats_baseline_by_more_than_the_spread": bool(lead > spread),
               "windows_s": [p[1] for p in passes], "fused_minus_torch_max": float((a.double() - b.double()).abs().max()),
               "fused_minus_torch_chunked_max": float((a.double() - routes["torch_chunked"]().double()).abs().max()),
               "masked_fraction_first_round": (1.0 - fit["counts"][:, 0].double() / (H * W)).tolist(),
               "psnr_before": before, "psnr_after": after,
               # what one round's accumulation needs per view: 64 fp64 multiply-adds per counted pixel and channel; the
               # current image, pred and gt read once (the three channels' workgroups share them through the caches)
               "accumulate_fma_per_view_round_at_most": 3 * 64 * H * W, "accumulate_bytes_per_view_round": 3 * 12 * H * W}
        rows.append(row)
        print(json.dumps({"colorcorrect_bench_case": row}), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "cases": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"colorcorrect_bench": res}))


if __name__ == "__main__":
    main()
