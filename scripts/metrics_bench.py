"""The image metrics on the MI355X: ``image_metrics`` (csrc/evalmetrics.hip: PSNR, SSIM, MSE and L1 of B
stacked views in two launches) against what a user would run otherwise -- the torch formulation of tests/metrics_restatement.py
in float32 on the same device -- at 1920 x 1080 with B = 1 and 4, on a seeded smooth-plus-noise pair.  Both routes run in one
process in alternating windows of --steps calls between device events, after a warm-up of every shape; the median of --rounds
windows is reported.  The whole measurement runs TWICE: the difference between the two passes' medians is the spread, and
``beats_baseline_by_more_than_the_spread`` says whether the fused call's lead is larger than it.  Also recorded, on one view:
the entry point alone next to ``misplat_ssim_fwd`` (which also writes the backward's derivative maps), a device copy of the same
two images as the memory roof, and the fused call's difference from the torch route.  No time is a pass condition.

    python scripts/metrics_bench.py [--steps 20] [--rounds 7] [--out build/metrics_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 1080, 1920


def time_window(fn, steps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / steps


def make_pair(B, dev):
    """gt: low-frequency sinusoids per view and channel; pred: gt + 0.05 gaussian noise, clamped."""
    g = torch.Generator().manual_seed(100 + B)
    y = torch.arange(H, dtype=torch.float32)[None, :, None, None] / 64.0
    x = torch.arange(W, dtype=torch.float32)[None, None, :, None] / 64.0
    ph = torch.rand(B, 1, 1, 3, 3, generator=g) * 2 * math.pi
    fr = 0.5 + torch.rand(B, 1, 1, 3, 3, generator=g)
    gt = 0.5 + 0.2 * torch.sin(fr[..., 0] * x + ph[..., 0]) * torch.cos(fr[..., 1] * y + ph[..., 1]) \
        + 0.2 * torch.sin(fr[..., 2] * (x + y) + ph[..., 2])
    pred = (gt + 0.05 * torch.randn(B, H, W, 3, generator=g)).clamp(0.0, 1.0)
    return pred.contiguous().to(dev), gt.contiguous().to(dev)


def alternate(routes, steps, rounds):
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            times[k].append(time_window(fn, steps))
    return {k: float(np.median(v)) for k, v in times.items()}, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "metrics_bench.json"))           # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    import collab_splats_amd as m
    from collab_splats_amd import _lib
    import metrics_restatement as R
    lib = m.load_library()
    dev = torch.device("cuda:0")
    rows = []
    for B in (1, 4):
        pred, gt = make_pair(B, dev)
        routes = {"fused": lambda: m.image_metrics(pred, gt),
                  "torch": lambda: R.image_metrics(pred, gt, dtype=torch.float32)}
        for fn in routes.values():                                     # warm-up of every shape, both routes
            for _ in range(3):
                fn()
        a, b = routes["fused"](), routes["torch"]()
        diff = {k: float((a[k].double() - b[k].double()).abs().max()) for k in ("mse", "l1", "ssim", "psnr")}
        passes = [alternate(routes, args.steps, args.rounds) for _ in range(2)]                    # the same code twice
        med = {k: [p[0][k] for p in passes] for k in routes}
        spread = max(abs(med[k][0] - med[k][1]) for k in routes)
        lead = min(med["torch"]) - max(med["fused"])
        row = {"B": B, "H": H, "W": W, "steps": args.steps, "rounds": args.rounds,
               "fused_s": med["fused"], "torch_s": med["torch"], "spread_s": spread, "lead_s": lead,
               "beats_baseline_by_more_than_the_spread": bool(lead > spread),
               "windows_s": [p[1] for p in passes], "fused_minus_torch": diff}
        rows.append(row)
        print(json.dumps({"metrics_bench_case": row}), flush=True)
        if B != 1:
            continue
        # ---- one view: the entry point alone, misplat_ssim_fwd on the same image, and a copy of the two images
        i32 = C.c_int32
        n_eval = int(lib.misplat_eval_image_scratch_floats(i32(1), i32(H), i32(W)))
        n_ssim = int(lib.misplat_ssim_scratch_floats(i32(H), i32(W)))
        s_eval, s_ssim = torch.empty(n_eval, device=dev), torch.empty(n_ssim, device=dev)
        out4, out1, out2 = torch.empty(4, device=dev), torch.empty(1, device=dev), torch.empty(1, device=dev)
        p, q = pred[0].contiguous(), gt[0].contiguous()
        copy_dst = torch.empty(2, H, W, 3, device=dev)
        copy_src = torch.stack((p, q))
        ptr, sp = _lib.ptr, _lib.stream_ptr
        kernels = {
            "eval_image": lambda: lib.misplat_eval_image(i32(1), i32(H), i32(W), ptr(p), ptr(q), i32(1), ptr(s_eval), ptr(out4), sp()),
            "eval_image_no_ssim": lambda: lib.misplat_eval_image(i32(1), i32(H), i32(W), ptr(p), ptr(q), i32(0), ptr(s_eval), ptr(out4), sp()),
            "ssim_fwd": lambda: lib.misplat_ssim_fwd(i32(H), i32(W), ptr(p), ptr(q), ptr(s_ssim), C.c_void_p(0), C.c_float(0.2),
                                                     ptr(out1), ptr(out2), sp()),
            "copy_two_images": lambda: copy_dst.copy_(copy_src)}
        for fn in kernels.values():
            for _ in range(3):
                fn()
        kp = [alternate(kernels, args.steps, args.rounds)[0] for _ in range(2)]
        bytes_in = 2 * H * W * 3 * 4
        krow = {k: [x[k] for x in kp] for k in kernels}
        krow["bytes_read_per_view"] = bytes_in
        krow["eval_image_GBps"] = bytes_in / min(krow["eval_image"]) / 1e9
        krow["eval_image_no_ssim_GBps"] = bytes_in / min(krow["eval_image_no_ssim"]) / 1e9
        krow["copy_GBps_read_plus_write"] = 2 * bytes_in / min(krow["copy_two_images"]) / 1e9
        rows.append({"one_view_entry_points_s": krow})
        print(json.dumps({"metrics_bench_entry_points": krow}), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "cases": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"metrics_bench": res}))


if __name__ == "__main__":
    main()
