"""The 2-D identity loss on the MI355X: forward + backward of ``ops.identity_loss`` (csrc/identity.hip)
against the route the reference's ``setup_train`` implies, run on the same device -- ``F.conv2d`` onto [K, H, W] logits, then
``F.cross_entropy(ignore_index)`` and autograd -- at 540 x 960 and 1080 x 1920, K = 64 and 256, D = 16 (the [..., 3:19] slice of
a 20-channel render; about 30 % of the pixels unlabelled).  Both routes run in one process, alternating, --rounds windows of
--steps steps each between device events after a warm-up of every shape; the median window is reported, with each route's peak
extra memory (``torch.cuda.max_memory_allocated`` over one step, above what is allocated before it) and the two routes' largest
relative difference at the timed size.  No time is a pass condition.

    python scripts/identity_bench.py [--steps 20] [--rounds 5] [--out build/identity_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_window(fn, steps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / steps


def make_case(dev, H, W, K, D=16):
    g = torch.Generator().manual_seed(0)
    render = torch.randn(H, W, D + 4, generator=g).to(dev)
    weight = (2.0 * torch.randn(K, D, generator=g) / D ** 0.5).to(dev).requires_grad_(True)
    bias = (0.3 * torch.randn(K, generator=g)).to(dev).requires_grad_(True)
    target = torch.randint(1, K + 1, (H, W), generator=g).to(torch.int32)
    target[torch.rand(H, W, generator=g) < 0.3] = 0
    return render, weight, bias, target.to(dev), D


def fused_step(render, weight, bias, target, D):
    from collab_splats_amd import ops
    feats = render[..., 3:3 + D].detach().requires_grad_(True)
    loss = ops.identity_loss(feats, (weight, bias), target, validate=False)
    return loss, torch.autograd.grad(loss, [feats, weight, bias])


def torch_step(render, weight, bias, target64, D):
    feats = render[..., 3:3 + D].detach().requires_grad_(True)
    z = F.conv2d(feats.permute(2, 0, 1).unsqueeze(0), weight[:, :, None, None], bias)
    loss = F.cross_entropy(z, target64, ignore_index=-1)
    return loss, torch.autograd.grad(loss, [feats, weight, bias])


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "identity_bench.json"))          # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("identity_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    import collab_splats_amd as m
    m.load_library()
    dev = torch.device("cuda:0")
    rows = []
    for (H, W) in ((540, 960), (1080, 1920)):
        for K in (64, 256):
            render, weight, bias, target, D = make_case(dev, H, W, K)
            target64 = (target.long() - 1)[None]
            routes = {"fused": lambda: fused_step(render, weight, bias, target, D),
                      "torch": lambda: torch_step(render, weight, bias, target64, D)}
            for fn in routes.values():                                 # warm-up of every shape, both routes
                for _ in range(3):
                    fn()
            (lf, gf), (lt, gtc) = routes["fused"](), routes["torch"]()
            diff = {"loss": abs(float(lf.detach()) - float(lt.detach())) / abs(float(lt.detach()))}
            for k, a, b in zip(("features", "weight", "bias"), gf, gtc):
                diff[k] = float((a - b).abs().max() / b.abs().max())
            del lf, gf, lt, gtc
            times = {k: [] for k in routes}
            for _ in range(args.rounds):                               # alternating windows
                for k, fn in routes.items():
                    times[k].append(time_window(fn, args.steps))
            row = {"H": H, "W": W, "K": K, "D": D, "steps": args.steps, "rounds": args.rounds,
                   "fused_s": float(np.median(times["fused"])), "torch_s": float(np.median(times["torch"])),
                   "fused_windows_s": times["fused"], "torch_windows_s": times["torch"],
                   "fused_peak_extra_bytes": peak_extra(routes["fused"]), "torch_peak_extra_bytes": peak_extra(routes["torch"]),
                   "max_rel_difference": diff}
            rows.append(row)
            print(json.dumps({"identity_bench_case": row}), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "cases": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"identity_bench": res}))


if __name__ == "__main__":
    main()
