"""Gaussian grouping on the MI355X: times, with device events (median of --reps after a warm-up), one
view's selection (``front_gaussians`` on --gaussians projected Gaussians, a --width x --height image of --masks masks, 32 x 32
patches, the default fraction 0.5) and one ``MemoryBank.associate`` step against a bank of --labels labels built from
--bank-views earlier views.  The projected means, radii and depths are synthetic (uniform over the image and a margin around it,
a fifth of the Gaussians invalid): the selection's cost does not depend on where they come from.

The host baseline is the reference's loop structure (the numpy restatement's per-mask, per-patch form: one gather of an [H W]
boolean through all N pixel indices per non-empty patch) at a REDUCED size, --cpu-gaussians Gaussians and --cpu-masks masks on a
quarter-size image, on one thread; it is labelled as such in the output and is not extrapolated.

    python scripts/grouping_bench.py [--gaussians 1000000] [--width 1920] [--height 1080] [--masks 64] [--labels 300]
                                     [--reps 5] [--no-cpu] [--out build/grouping_bench.json]

Per-kernel times: run it under `rocprofv3 --kernel-trace --stats` (with --no-cpu --reps 1).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def time_gpu(fn, reps):
    fn()                                                               # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
    return float(np.median(ts))


def view(seed, N, W, H):
    rng = np.random.default_rng(seed)
    means = np.stack([rng.uniform(-0.05 * W, 1.05 * W, N), rng.uniform(-0.05 * H, 1.05 * H, N)], axis=1).astype(np.float32)
    radii = np.where(rng.random((N, 1)) < 0.2, 1, rng.integers(2, 30, (N, 2))).astype(np.int32)
    depths = rng.uniform(0.5, 20.0, N).astype(np.float32)
    return radii, means, depths


def mask_image(seed, W, H, n_masks):
    """n_masks rectangular blocks on a grid (a tenth of the blocks background), ids with gaps"""
    rng = np.random.default_rng(seed)
    gw = int(np.ceil(np.sqrt(n_masks * W / H)))
    gh = -(-n_masks // gw)
    ids = (np.arange(gw * gh) % n_masks) * 3 + 1
    grid = rng.permutation(ids).reshape(gh, gw)
    grid[rng.random((gh, gw)) < 0.1] = 0
    bw, bh = -(-W // gw), -(-H // gh)
    return np.kron(grid, np.ones((bh, bw), np.int64))[:H, :W].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--masks", type=int, default=64)
    ap.add_argument("--labels", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-gaussians", type=int, default=50_000)
    ap.add_argument("--cpu-masks", type=int, default=8)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "grouping_bench.json"))        # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grouping_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    torch.set_num_threads(1)
    import collab_splats_amd as m
    import grouping_restatement as R
    m.load_library()
    dev = torch.device("cuda:0")
    N, W, H, M = args.gaussians, args.width, args.height, args.masks
    res = {"device": torch.cuda.get_device_name(0), "gaussians": N, "width": W, "height": H, "masks": M, "num_patches": 32,
           "front_percentage": 0.5}

    def meta_of(seed):
        radii, means, depths = view(seed, N, W, H)
        return {"radii": torch.from_numpy(radii).to(dev)[None], "means2d": torch.from_numpy(means).to(dev)[None],
                "depths": torch.from_numpy(depths).to(dev)[None], "width": W, "height": H}

    # ---- one view's selection
    meta = meta_of(0)
    mask = torch.from_numpy(mask_image(0, W, H, M)).to(dev)
    front = m.front_gaussians(meta, mask)
    res["selection"] = {"masks_found": front.num_masks, "selected": int(front.counts.sum()),
                        "project_gaussians_s": time_gpu(lambda: m.project_gaussians(meta), args.reps),
                        "front_gaussians_s": time_gpu(lambda: m.front_gaussians(meta, mask), args.reps)}
    print(f"selection {res['selection']}", flush=True)

    # ---- one associate step against a bank of a few hundred labels: earlier views with shifted masks under a high threshold
    views = -(-args.labels // max(front.num_masks, 1))
    fronts = [m.front_gaussians(meta_of(1 + v), torch.from_numpy(mask_image(1 + v, W, H, M)).to(dev)) for v in range(views)]

    def bank_of():
        bank = m.MemoryBank(N, 2.0)                                  # every mask opens a label: views x masks labels
        for f in fronts:
            bank.associate(f)
        bank.iou_threshold = 0.1
        return bank

    bank = bank_of()
    labels_before, pairs = bank.total_masks, bank._pairs
    assign_s = time_gpu(lambda: bank.assign(front), args.reps)
    banks = [bank_of() for _ in range(args.reps + 1)]                # associate changes the bank: a fresh one per repetition
    it = iter(banks)
    associate_s = time_gpu(lambda: next(it).associate(front), args.reps)
    labels = banks[0].assign(front)
    res["associate"] = {"bank_views": views, "labels_before": labels_before, "pairs_before": pairs,
                        "labels_after": banks[0].total_masks, "matched_old": int((labels < labels_before).sum()),
                        "assign_s": assign_s, "associate_s": associate_s,
                        "convert_matched_mask_s": time_gpu(lambda: m.convert_matched_mask(labels, mask), args.reps)}
    print(f"associate {res['associate']}", flush=True)

    # ---- the host loop, at a reduced size
    if not args.no_cpu:
        n, w, h, k = args.cpu_gaussians, W // 4, H // 4, args.cpu_masks
        radii, means, depths = view(0, n, w, h)
        comp = mask_image(0, w, h, k)
        flat, valid = R.project(radii, means, w, h)
        t0 = time.perf_counter()
        R.front_sets_brute(flat, valid, depths, comp, 0.5, 32)
        res["cpu_reduced"] = {"gaussians": n, "width": w, "height": h, "masks": int(len(R.mask_ids(comp))),
                              "front_sets_s": time.perf_counter() - t0,
                              "note": "REDUCED size: the reference's per-mask, per-patch loop restated in numpy, one thread"}
        print(f"cpu_reduced {res['cpu_reduced']}", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"grouping_bench": res}))


if __name__ == "__main__":
    main()
