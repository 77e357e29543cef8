"""Quadric-error simplification on the MI355X: the marching-cubes mesh of an analytic density (three
overlapping Gaussians, level 0.5) at two voxel sizes, simplified to one fifth of its triangles.  Prints the rounds, the time
of the call (device events plus the host reads, wall clock, median of --reps after a warm-up), the time per round, and the share
of the radix sorts and their scans in the kernel time (from torch's profiler; "unmeasured" where it records no kernel).

    python scripts/decimate_bench.py [--voxel-size 0.01 0.006] [--fraction 0.2] [--reps 3] [--out build/decimate_bench.json]

Per-kernel times: run it under `rocprofv3 --kernel-trace --stats` (with --reps 1).
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


def blob_mesh(h, dev):
    import collab_splats_amd as m
    means = torch.tensor([[0.0, 0.0, 0.0], [0.45, 0.1, 0.0], [-0.2, 0.4, 0.15]], device=dev)
    quats = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * 3, device=dev)
    scales = torch.tensor([[0.4, 0.4, 0.4], [0.3, 0.25, 0.3], [0.25, 0.3, 0.2]], device=dev)
    colours = torch.tensor([[1.0, 0.2, 0.2], [0.2, 1.0, 0.2], [0.2, 0.2, 1.0]], device=dev)
    field = m.DensityField(means, quats, scales, torch.ones(3, device=dev), h)
    return field.extract_mesh(0.5, values=colours)


def sort_share(fn):
    """The share of the radix-sort and scan kernels in the kernel time of fn(), or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        total = sorts = 0.0
        for ev in prof.key_averages():
            t = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0))
            total += t
            if any(s in ev.key for s in ("radix_", "scan_")):
                sorts += t
        return sorts / total if total > 0 else None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel-size", type=float, nargs="*", default=[0.01, 0.006])
    ap.add_argument("--fraction", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "decimate_bench.json"))       # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decimate_bench.py measures the MI355X: no GPU here (figures are 'unmeasured')")
    import collab_splats_amd as m
    m.load_library()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "meshes": []}
    for h in args.voxel_size:
        v, t, c = blob_mesh(h, dev)
        target = int(t.shape[0] * args.fraction)
        run = lambda: m.simplify_quadric_decimation(v, t, target, attributes=(c,))       # noqa: E731
        out = run()                                                     # warm-up
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        total = float(np.median(ts))
        share = sort_share(run)
        stats = m.mesh_edge_stats(out[0], out[1])
        row = {"voxel_size": h, "vertices": int(v.shape[0]), "triangles": int(t.shape[0]), "target": target,
               "triangles_out": int(out[1].shape[0]), "vertices_out": int(out[0].shape[0]), "rounds": out[4], "total_s": total,
               "per_round_ms": 1e3 * total / max(out[4], 1), "sort_share": share if share is not None else "unmeasured",
               "boundary_in": m.mesh_edge_stats(v, t)["n_boundary"], "boundary_out": stats["n_boundary"],
               "nonmanifold_out": stats["n_nonmanifold"]}
        res["meshes"].append(row)
        print(f"decimate {row}", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"decimate_bench": res}))


if __name__ == "__main__":
    main()
