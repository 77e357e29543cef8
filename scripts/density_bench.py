"""The Gaussian density field on the MI355X: for synthetic scenes (``synthetic.random_scene``) of --gaussians
Gaussians at --voxel-size, the allocated units and (unit, Gaussian) pairs, the seconds of every build stage (each synchronised;
the host reads are inside ``bounds``, ``count`` and ``emit_alloc``), the accumulate kernel alone with and without sub-brick
skipping (device events, median of --reps after a warm-up) and its voxel-terms per second (4096 n_pairs / time: every voxel of a
unit against every record of the unit's list, skipped or not), a query at --points random points, and one level set.  No time
is a pass condition.  Every scene runs in a child process of its own under a time limit.

    python scripts/density_bench.py [--gaussians 100000 1000000] [--voxel-size 0.01] [--reps 3] [--points 1000000] [--limit 300]
                                    [--out build/density_bench.json]

Per-kernel times: run one scene under `rocprofv3 --kernel-trace --stats` (-- python scripts/density_bench.py --child 100000 --reps 1).
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


def child(args):
    import collab_splats_amd as m
    from collab_splats_amd._lib import check, load, ptr, stream_ptr
    from collab_splats_amd.synthetic import random_scene
    lib = m.load_library()
    dev = torch.device("cuda:0")
    n = args.child
    sc = random_scene(n, 1920, 1080, seed=42, device="cuda:0")
    gauss = (sc["means"], sc["quats"], torch.exp(sc["log_scales"]), torch.sigmoid(sc["opacity_logits"]))
    m.DensityField(*gauss, args.voxel_size)                            # warm-up (allocator, code objects)
    stages = {}
    f = m.DensityField(*gauss, args.voxel_size, _timings=stages)
    row = {"gaussians": n, "voxel_size": args.voxel_size, "map_units": int(np.prod(f.dims)), "units": f.n_units, "pairs": f.n_pairs,
           "pool_GB": f.n_units * 5 * 4096 * 4 / 1e9, "stages_s": stages, "build_s": float(sum(stages.values()))}
    grid = f._grid()

    def accumulate(flags):
        check(lib.misplat_density_accumulate(C.byref(grid), ptr(f._touched), f.n_units, ptr(f._records), ptr(f._ids), ptr(f._ranges),
                                             C.c_float(f.cutoff), flags, ptr(f._pool), stream_ptr()), "misplat_density_accumulate")

    # (measured twice, in both orders: the second figure of each is the one reported; the first shows what the order costs)
    row["accumulate_noskip_first_s"] = time_gpu(lambda: accumulate(1), args.reps)
    row["accumulate_skip_first_s"] = time_gpu(lambda: accumulate(0), args.reps)
    row["accumulate_noskip_s"] = time_gpu(lambda: accumulate(1), args.reps)
    row["accumulate_skip_s"] = time_gpu(lambda: accumulate(0), args.reps)
    row["voxel_terms"] = 4096 * f.n_pairs
    row["voxel_terms_per_s"] = row["voxel_terms"] / row["accumulate_skip_s"]
    row["voxel_terms_per_s_noskip"] = row["voxel_terms"] / row["accumulate_noskip_s"]
    g = torch.Generator(device="cuda").manual_seed(1)
    idx = torch.randint(0, n, (args.points,), generator=g, device=dev)
    pts = sc["means"][idx] + 0.01 * torch.randn(args.points, 3, generator=g, device=dev)
    vals = torch.rand(n, 3, generator=g, device=dev)
    row["query_points"] = args.points
    row["query_s"] = time_gpu(lambda: f.query(pts, vals), args.reps)
    v, t, _ = f.extract_mesh(0.5, values=vals)
    row["vertices"], row["triangles"] = int(v.shape[0]), int(t.shape[0])
    del v, t
    row["extract_s"] = time_gpu(lambda: f.extract_mesh(0.5, values=vals), args.reps)
    print(json.dumps({"density_bench_scene": row}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--limit", type=int, default=300, help="seconds per scene")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "density_bench.json"))        # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("density_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    if args.child is not None:
        return child(args)
    rows = []
    for n in args.gaussians:                                           # one process per scene, each under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--voxel-size", str(args.voxel_size), "--reps",
               str(args.reps), "--points", str(args.points)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"density_bench.py: {n} Gaussians ran past {args.limit} s; nothing more is started")
        if out.returncode != 0:
            sys.stderr.write(out.stderr[-4000:])
            raise SystemExit(f"density_bench.py: {n} Gaussians ended with status {out.returncode}; nothing more is started")
        line = [ln for ln in out.stdout.splitlines() if ln.startswith('{"density_bench_scene"')][-1]
        rows.append(json.loads(line)["density_bench_scene"])
        print(f"{n} Gaussians: {rows[-1]}", flush=True)
    res = {"device": torch.cuda.get_device_name(0), "scenes": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"density_bench": res}))


if __name__ == "__main__":
    main()
