"""The features model's decoder + cosine feature loss on the MI355X: forward + backward of
``ops.feature_loss`` (csrc/featloss.hip) against the reference's own route -- the same PyTorch-ROCm op chain on the device
(``F.interpolate``, two ``conv2d``, ``F.cosine_similarity``, autograd) -- at the production shape: render 1080 x 1920 x 13 (the
[..., 3:16] slice of a 17-channel render), main branch 768 x 64 x 114, second branch 384 channels at 64 x 114 and at a differing
resolution (--second, default 37 x 37).  Both routes run in one process, alternating, --rounds windows of --steps steps each
between device events after a warm-up of every shape; the median window is reported.  The two routes' losses and gradients are
compared at the timed size.  Launch counts come from torch's profiler in a pass of their own (or "not measured").  No time is a
pass condition.

    python scripts/featureloss_bench.py [--steps 50] [--rounds 5] [--second 37 37] [--out build/featureloss_bench.json]
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


def make_case(dev, second_hw):
    g = torch.Generator().manual_seed(0)
    H, W, L, Hd = 1080, 1920, 13, 64
    dims = {"clip": (768, 64, 114), "dino": (384,) + tuple(second_hw)}
    render = torch.rand(H, W, 17, generator=g).to(dev)
    params = {"w_hidden": torch.randn(Hd, L, generator=g) / L ** 0.5, "b_hidden": 0.1 * torch.randn(Hd, generator=g)}
    for n, d in dims.items():
        params["w_out." + n] = torch.randn(d[0], Hd, generator=g) / Hd ** 0.5
        params["b_out." + n] = 0.1 * torch.randn(d[0], generator=g)
    params = {k: v.to(dev).requires_grad_(True) for k, v in params.items()}
    gt = {n: torch.randn(*d, generator=g).to(dev) for n, d in dims.items()}
    for t in gt.values():
        t[:, 0, 0] = 0.0
    return render, params, gt, dims


def fused_step(render, params, gt):
    from collab_splats_amd import ops
    feats = render[..., 3:16].detach().requires_grad_(True)
    dec = (params["w_hidden"], params["b_hidden"], {n: (params["w_out." + n], params["b_out." + n]) for n in gt})
    loss = ops.feature_loss(feats, dec, gt, "clip", 0.1, 1e-3)
    grads = torch.autograd.grad(loss, [feats] + list(params.values()))
    return loss, grads


def torch_step(render, params, gt):
    """The reference's route (rade_features_model.py:149-189, :545-584) on the same tensors."""
    feats = render[..., 3:16].detach().requires_grad_(True)
    x = F.interpolate(feats.permute(2, 0, 1).unsqueeze(0), size=gt["clip"].shape[1:], mode="bilinear", align_corners=False)
    h = F.relu(F.conv2d(x, params["w_hidden"][:, :, None, None], params["b_hidden"]))
    loss = torch.tensor(0.0, device=render.device)
    for n, g in gt.items():
        p = F.conv2d(h, params["w_out." + n][:, :, None, None], params["b_out." + n])
        if n != "clip":
            p = F.interpolate(p, size=g.shape[1:], mode="bilinear", align_corners=False)
        loss = loss + (1 - F.cosine_similarity(p.squeeze(0), g, dim=0)).mean() * (1.0 if n == "clip" else 0.1)
    loss = loss * 1e-3
    grads = torch.autograd.grad(loss, [feats] + list(params.values()))
    return loss, grads


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        from torch.autograd import DeviceType
        n = sum(e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA)   # kernels, copies, memsets
        return n if n > 0 else "not measured"
    except Exception as exc:                                            # the profiler is optional: say so, do not guess
        return f"not measured ({type(exc).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--second", type=int, nargs=2, action="append", default=None, help="H W of the second branch")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "featureloss_bench.json"))       # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("featureloss_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    import collab_splats_amd as m
    m.load_library()
    dev = torch.device("cuda:0")
    rows = []
    for second in (args.second or [[64, 114], [37, 37]]):
        render, params, gt, dims = make_case(dev, second)
        routes = {"fused": lambda: fused_step(render, params, gt), "torch": lambda: torch_step(render, params, gt)}
        for fn in routes.values():                                     # warm-up of every shape, both routes
            for _ in range(3):
                fn()
        (lf, gf), (lt, gtc) = routes["fused"](), routes["torch"]()
        names = ["features"] + list(params)
        diff = {"loss": abs(float(lf.detach()) - float(lt.detach())) / abs(float(lt.detach()))}
        for k, a, b in zip(names, gf, gtc):
            diff[k] = float((a - b).abs().max() / b.abs().max())
        times = {k: [] for k in routes}
        for _ in range(args.rounds):                                   # alternating windows
            for k, fn in routes.items():
                times[k].append(time_window(fn, args.steps))
        row = {"dims": {n: list(d) for n, d in dims.items()}, "steps": args.steps, "rounds": args.rounds,
               "fused_s": float(np.median(times["fused"])), "torch_s": float(np.median(times["torch"])),
               "fused_windows_s": times["fused"], "torch_windows_s": times["torch"],
               "fused_launches": count_launches(routes["fused"]), "torch_launches": count_launches(routes["torch"]),
               "max_rel_difference": diff}
        rows.append(row)
        print(json.dumps({"featureloss_bench_case": row}), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "cases": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"featureloss_bench": res}))


if __name__ == "__main__":
    main()
