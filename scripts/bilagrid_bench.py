"""The bilateral-grid slice and TV loss on the MI355X: forward + backward of ``bilagrid_slice`` at
1080 x 1920 with grid (16, 16, 8), and of ``bilagrid_tv_loss`` over 300 cameras (csrc/bilagrid.hip), against the torch
composition of the same definition on the same device -- a meshgrid, a 5-D ``F.grid_sample`` and a batched 3 x 4 product;
``index_select`` differences for the TV.  Both routes run in one process, alternating, --rounds windows of --steps steps each
between device events after a warm-up of every route; the median window and the spread (min, max) are reported.  The two
routes' values and gradients are compared at the timed size.  No time is a pass condition.

    python scripts/bilagrid_bench.py [--steps 20] [--rounds 7] [--cameras 300] [--out build/bilagrid_bench.json]
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


def torch_slice(rgb, grids, cam):
    H, W = rgb.shape[:2]
    y, x = torch.meshgrid(torch.arange(H, device=rgb.device, dtype=rgb.dtype) / max(H - 1, 1),
                          torch.arange(W, device=rgb.device, dtype=rgb.dtype) / max(W - 1, 1), indexing="ij")
    z = 0.299 * rgb[..., 0] + 0.587 * rgb[..., 1] + 0.114 * rgb[..., 2]
    coords = (torch.stack([x, y, z], dim=-1) - 0.5) * 2
    A = F.grid_sample(grids[cam][None], coords[None, None], mode="bilinear", padding_mode="border", align_corners=True)
    A = A[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
    return torch.matmul(A[..., :3], rgb[..., None]).squeeze(-1) + A[..., 3]


def torch_tv(grids):
    num = grids.shape[0]
    total = 0.0
    for axis in (2, 3, 4):
        n = grids.shape[axis]
        idx = torch.arange(n, device=grids.device)
        d = grids.index_select(axis, idx[1:]) - grids.index_select(axis, idx[:-1])
        total = total + (d * d).sum() / (d.numel() // num)
    return total / num


def summary(times):
    return {"median_s": float(np.median(times)), "min_s": float(np.min(times)), "max_s": float(np.max(times)), "windows_s": times}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cameras", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "bilagrid_bench.json"))          # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bilagrid_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    import collab_splats_amd as m
    m.load_library()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    H, W, cam = 1080, 1920, 7
    rgb = torch.rand(H, W, 3, generator=g).to(dev).requires_grad_(True)
    v_out = torch.randn(H, W, 3, generator=g).to(dev)
    grids = m.BilateralGrid(args.cameras).grids.detach()
    grids = (grids + 0.1 * torch.randn(grids.shape, generator=g)).to(dev).requires_grad_(True)

    def slice_step(fn):
        return torch.autograd.grad(fn(rgb, grids, cam), [rgb, grids], v_out)

    def tv_step(fn):
        return torch.autograd.grad(fn(grids), [grids])

    routes = {"slice_hip": lambda: slice_step(m.bilagrid_slice), "slice_torch": lambda: slice_step(torch_slice),
              "tv_hip": lambda: tv_step(m.bilagrid_tv_loss), "tv_torch": lambda: tv_step(torch_tv)}
    for fn in routes.values():                                          # warm-up of every route
        for _ in range(3):
            fn()
    with torch.no_grad():
        diff = {"slice_out": float((m.bilagrid_slice(rgb, grids, cam) - torch_slice(rgb, grids, cam)).abs().max()),
                "tv": abs(float(m.bilagrid_tv_loss(grids)) - float(torch_tv(grids))) / float(torch_tv(grids))}
    for k, a, b in zip(("slice_v_rgb", "slice_v_grids"), routes["slice_hip"](), routes["slice_torch"]()):
        diff[k] = float((a - b).abs().max() / b.abs().max())
    diff["tv_v_grids"] = float((routes["tv_hip"]()[0] - routes["tv_torch"]()[0]).abs().max() / routes["tv_torch"]()[0].abs().max())
    times = {k: [] for k in routes}
    for _ in range(args.rounds):                                        # alternating windows
        for k, fn in routes.items():
            times[k].append(time_window(fn, args.steps))
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "grid_shape": [16, 16, 8], "cameras": args.cameras,
           "steps": args.steps, "rounds": args.rounds, **{k: summary(v) for k, v in times.items()},
           "slice_torch_over_hip": float(np.median(times["slice_torch"]) / np.median(times["slice_hip"])),
           "tv_torch_over_hip": float(np.median(times["tv_torch"]) / np.median(times["tv_hip"])),
           "max_difference": diff}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"bilagrid_bench": res}))


if __name__ == "__main__":
    main()
