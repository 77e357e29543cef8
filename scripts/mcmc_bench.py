"""The MCMC densification on the MI355X: the per-step position noise (``inject_noise_to_position``,
csrc/mcmc.hip: one launch, 56 B per Gaussian) against the same update composed from torch ops on the same inputs -- sigmoid, exp,
the rotation, the [N, 3, 3] covariance, the gate, ``torch.randn_like`` and a batched matrix-vector product, the composition a
torch implementation of the method runs (``torch``), and the same without the batched 3 x 3 products, broadcasts and sums only
(``torch_elementwise``, the baseline the lead is taken against) -- at 1 M and 5 M Gaussians; and one refine step's kernels,
``sample_by_opacity`` plus ``compute_relocation`` for 5 % of N, against ``torch.multinomial`` + ``torch.bincount`` for the draw
alone.  The parent of this feature has no such step: the torch composition is the only baseline there is.  metrics_bench.py's
protocol: the routes run in one process in alternating windows between device events (--steps calls of the torch routes, 25 x
as many of the fused noise step and 5 x as many of the fused refine kernels, so that every window runs for milliseconds), after
a warm-up of every shape; the median of
--rounds windows is reported; the whole measurement runs TWICE, the difference between the two passes' medians is the spread
(the largest over the routes), and ``beats_baseline_by_more_than_the_spread`` says whether the fused call's lead over the torch
route is larger than it.  Also recorded: the share of the HBM roof the 56 B model gives the fused noise step.  No time is a pass
condition.

    python scripts/mcmc_bench.py [--steps 20] [--rounds 7] [--sizes 1000000 5000000] [--out build/mcmc_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOISE_BYTES = 56                    # means read and written (24), opacity (4), scales (12), quats (16)
HBM_ROOF = 8.0e12                   # bytes / s, the MI355X's HBM3E peak
SCALER = 80.0                       # lr 1.6e-4 x noise_lr 5e5


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
    for _ in range(rounds):
        for k, fn in routes.items():
            times[k].append(time_window(fn, steps[k]))
    return {k: float(np.median(v)) for k, v in times.items()}, times


def make_params(n, dev):
    g = torch.Generator().manual_seed(n)
    return {"means": torch.nn.Parameter(torch.randn(n, 3, generator=g).to(dev)),
            "opacities": torch.nn.Parameter((torch.randn(n, 1, generator=g) * 2 - 2).to(dev)),
            "scales": torch.nn.Parameter((torch.rand(n, 3, generator=g) * 3 - 6).to(dev)),
            "quats": torch.nn.Parameter(torch.randn(n, 4, generator=g).to(dev))}


@torch.no_grad()
def torch_noise(params, scaler):
    """The same update from torch ops (the covariance as an [N, 3, 3] tensor, torch's global generator)."""
    from collab_splats_amd.radegs import build_rotation
    o = torch.sigmoid(params["opacities"]).flatten()
    s = torch.exp(params["scales"])
    R = build_rotation(params["quats"])
    cov = (R * (s * s)[:, None, :]) @ R.transpose(1, 2)
    gate = 1.0 / (1.0 + torch.exp(-100.0 * ((1.0 - o) - 0.995)))
    noise = torch.randn_like(params["means"]) * gate[:, None] * scaler
    params["means"].add_(torch.einsum("bij,bj->bi", cov, noise))


@torch.no_grad()
def torch_noise_elementwise(params, scaler):
    """The same again without the two batched 3 x 3 products (a batched GEMM of a million tiny matrices is slow on its own):
    broadcasts and sums only, the kindest torch composition."""
    from collab_splats_amd.radegs import build_rotation
    o = torch.sigmoid(params["opacities"]).flatten()
    s = torch.exp(params["scales"])
    R = build_rotation(params["quats"])
    gate = 1.0 / (1.0 + torch.exp(-100.0 * ((1.0 - o) - 0.995)))
    v = torch.randn_like(params["means"]) * (gate * scaler)[:, None]
    a = (s * s) * (R * v[:, :, None]).sum(1)                              # s^2 * (R^T v)
    params["means"].add_((R * a[:, None, :]).sum(2))                      # R a


def compare(routes, base, steps, rounds):
    """steps: calls per window, per route (a window should run for milliseconds, not microseconds)."""
    for fn in routes.values():
        for _ in range(3):
            fn()
    passes = [alternate(routes, steps, rounds) for _ in range(2)]
    med = {k: [p[0][k] for p in passes] for k in routes}
    spread = max(abs(v[0] - v[1]) for v in med.values())
    lead = min(med[base]) - max(med["fused"])
    return {"median_s": med, "calls_per_window": steps, "baseline": base, "spread_s": spread, "lead_s": lead,
            "beats_baseline_by_more_than_the_spread": bool(lead > spread), "ratio_baseline_over_fused": float(np.mean(med[base]) / np.mean(med["fused"])), "windows_s": [p[1] for p in passes]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 5_000_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "mcmc_bench.json"))             # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mcmc_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    import collab_splats_amd as m
    dev = torch.device("cuda:0")
    rows = []
    for n in args.sizes:
        params = make_params(n, dev)
        step = [0]

        def fused_noise():
            step[0] += 1
            m.inject_noise_to_position(params, {}, {}, SCALER, 0, step[0])

        noise = compare({"fused": fused_noise, "torch": lambda: torch_noise(params, SCALER),
                         "torch_elementwise": lambda: torch_noise_elementwise(params, SCALER)}, "torch_elementwise",
                        {"fused": 25 * args.steps, "torch": max(args.steps // 4, 2), "torch_elementwise": args.steps}, args.rounds)
        noise["fused_share_of_hbm_roof"] = [NOISE_BYTES * n / t / HBM_ROOF for t in noise["median_s"]["fused"]]
        opac = torch.sigmoid(params["opacities"].detach().flatten()).contiguous()
        scales = torch.exp(params["scales"].detach())
        k = n // 20
        binoms = m.mcmc.binomial_table(device=dev)

        def fused_refine():
            idx, counts = m.sample_by_opacity(opac, k, 0, 100, 0.005)
            m.compute_relocation(opac[idx], scales[idx], counts[idx] + 1, binoms)

        def fused_sample():
            m.sample_by_opacity(opac, k, 0, 100, 0.005)

        def torch_sample():
            idx = torch.multinomial(opac, k, replacement=True)
            torch.bincount(idx, minlength=n)

        refine = compare({"fused": fused_sample, "fused_with_relocation": fused_refine, "torch": torch_sample}, "torch",
                         {"fused": 5 * args.steps, "fused_with_relocation": 5 * args.steps, "torch": args.steps}, args.rounds)
        row = {"n": n, "draws": k, "steps": args.steps, "rounds": args.rounds, "noise": noise, "refine": refine}
        rows.append(row)
        print(json.dumps({"mcmc_bench_case": {kk: ({a: b for a, b in v.items() if a != "windows_s"} if isinstance(v, dict) else v)
                                              for kk, v in row.items()}}), flush=True)
        del params
    res = {"device": torch.cuda.get_device_name(0), "cases": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"mcmc_bench": "written", "out": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
