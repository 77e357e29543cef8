"""Screened Poisson reconstruction on the MI355X: times, with device events (median of --reps after a
warm-up), each stage of ``poisson_reconstruct`` (splat, system, solve, iso value, extraction with the vertex attributes) and the
whole call, at every depth of --depths, on --points seeded points of the tsdf_scenes sphere (or, with --model, on
``RadegsModel.depth_normal_points``' cloud of that sphere).  It reports the solver's iterations, the time per iteration and the
bytes per iteration by the count of section 20.3 (56 B a cell) against a streaming copy of the same size measured in the same
process.  No time is a pass condition.  Every depth runs in a child process of its own under a time limit.

    python scripts/poisson_bench.py [--points 2000000] [--depths 8 9] [--reps 3] [--model] [--limit 300]
                                    [--out build/poisson_bench.json]

Per-kernel times: run one depth under `rocprofv3 --kernel-trace --stats` (-- python scripts/poisson_bench.py --child 8 --reps 1).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BYTES_PER_CELL = 56                  # stencil 12 (p, D, Ap), update 32 (x, r, p, Ap, D read; x, r, z written), direction 12 (z, p; p)


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


def cloud(args, dev):
    import tsdf_scenes as S
    if args.model:
        model = S.sphere_gaussians(200_000).to(dev)
        model.eval()
        W, H = 640, 480
        _, vms, _, _ = S.sphere_views(32, 8, 8)
        K = S.intrinsics(W, H, 60.0)
        out = model.depth_normal_points([S.pinhole_camera(M, K, W, H) for M in vms], total_points=args.points, min_accumulation=0.5)
        return out["points"], out["normals"], out["colors"]
    g = torch.Generator().manual_seed(0)
    d = torch.randn(args.points, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    p = torch.tensor([0.1, -0.05, 0.2]) + 0.3 * d
    return p.to(dev), d.to(dev), torch.from_numpy(S.texture(p.double().numpy())).float().to(dev)


def child(args):
    import collab_splats_amd as m
    from collab_splats_amd import poisson as P
    from collab_splats_amd._lib import load, ptr, stream_ptr
    m.load_library()
    dev = torch.device("cuda:0")
    depth = args.child
    p, n, c = cloud(args, dev)
    o, h = P._grid("poisson_bench", p, depth, 1.1)
    ws = P._workspace(depth, p.shape[0], dev)
    W, V, Cq = P._splat(p, n, c, depth, o, h)
    Wf, b, D = P._system(W, V, depth, 1.0, ws)
    chi, info = P._solve(b, D, depth, 1e-5, 8 << depth, ws)
    iso = P._iso(chi, depth, o, h, p, ws)
    v, t, col, dens = P._extract(chi, iso, depth, o, h, Wf, Cq)
    cells = 1 << (3 * depth)
    row = {"depth": depth, "points": int(p.shape[0]), "cells": cells, "vertices": int(v.shape[0]), "triangles": int(t.shape[0]),
           "iterations": info["iterations"], "residual": info["residual"], "converged": info["converged"],
           "splat_s": time_gpu(lambda: P._splat(p, n, c, depth, o, h), args.reps),
           "system_s": time_gpu(lambda: P._system(W, V, depth, 1.0, ws), args.reps),
           "solve_s": time_gpu(lambda: P._solve(b, D, depth, 1e-5, 8 << depth, ws), args.reps),
           "iso_s": time_gpu(lambda: P._iso(chi, depth, o, h, p, ws), args.reps),
           "extract_s": time_gpu(lambda: P._extract(chi, iso, depth, o, h, Wf, Cq), args.reps)}
    del W, V, b, D, v, t, col, dens
    row["reconstruct_s"] = time_gpu(lambda: m.poisson_reconstruct(p, n, c, depth=depth), args.reps)
    # a streaming copy of one iteration's bytes (half read, half written), the library's own copy kernel
    n16 = BYTES_PER_CELL * cells // 2 // 16
    src = torch.empty(n16 * 4, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    row["copy_s"] = time_gpu(lambda: load().misplat_stream_copy(ptr(src), ptr(dst), C.c_int64(n16), 0, stream_ptr()), max(3, args.reps))
    row["bytes_per_iteration"] = BYTES_PER_CELL * cells
    row["iteration_s"] = row["solve_s"] / max(1, info["iterations"])
    row["iteration_TBps"] = row["bytes_per_iteration"] / row["iteration_s"] / 1e12
    row["copy_TBps"] = 2 * 16 * n16 / row["copy_s"] / 1e12
    print(json.dumps({"poisson_bench_depth": row}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--depths", type=int, nargs="+", default=[8, 9])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--limit", type=int, default=300, help="seconds per depth")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "poisson_bench.json"))        # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("poisson_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    if args.child is not None:
        return child(args)
    rows = []
    for depth in args.depths:                                          # one process per depth, each under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(depth), "--points", str(args.points), "--reps", str(args.reps)]
        cmd += ["--model"] if args.model else []
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"poisson_bench.py: depth {depth} ran past {args.limit} s; nothing more is started")
        if out.returncode != 0:
            sys.stderr.write(out.stderr[-4000:])
            raise SystemExit(f"poisson_bench.py: depth {depth} ended with status {out.returncode}; nothing more is started")
        line = [ln for ln in out.stdout.splitlines() if ln.startswith('{"poisson_bench_depth"')][-1]
        rows.append(json.loads(line)["poisson_bench_depth"])
        print(f"depth {depth}: {rows[-1]}", flush=True)
    res = {"device": torch.cuda.get_device_name(0), "source": "model" if args.model else "sphere", "depths": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"poisson_bench": res}))


if __name__ == "__main__":
    main()
