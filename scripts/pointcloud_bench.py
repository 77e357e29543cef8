"""Point-cloud cleaning on the MI355X: times remove_statistical_outlier (k = 20), radius_count
(r = 0.03), voxel_down_sample (0.01) and clean_pcd with device events around each public call, host reads included (median
of --reps after a warm-up), on the sphere shell of tests/pointcloud_scenes.py at --shell sizes and on a uniform cloud of
--uniform points, each with and without the 1 % far outliers.  Beside each row: the same algorithm on one CPU thread of the
same host (scipy cKDTree / numpy, fp64).  --tuning also times knn_mean_distance at 1 and 8 lanes per query and at several
occupancy targets.

    python scripts/pointcloud_bench.py [--shell 200000 1000000] [--uniform 1000000] [--reps 3] [--no-cpu] [--tuning]
                                       [--only SCENE N OUTLIERS] [--cpu-only] [--cpu-radius-max N] [--out build/pointcloud_bench.json]

Per-kernel times: run it under `rocprofv3 --kernel-trace --stats` (e.g. with --no-cpu --only shell 1000000 1 --reps 1).
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

K, STD_RATIO, RADIUS, VOXEL = 20, 2.0, 0.03, 0.01


def make_scene(kind, n, outliers, seed=0):
    import pointcloud_scenes as S
    if kind == "shell":
        return S.shell(n, seed, outliers=0.01 if outliers else 0.0)
    P = S.uniform(n, seed)
    if outliers:
        rng = np.random.default_rng(seed + 1)
        m = n // 100
        P[rng.choice(n, m, replace=False)] = rng.uniform(-1.5, 1.5, (m, 3)).astype(np.float32)
    return P


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
    return float(np.median(ts)), [min(ts), max(ts)]


# ------------------------------------------------------------------------------------------- one CPU thread, fp64
def cpu_outlier(P64, k=K, ratio=STD_RATIO):
    from scipy.spatial import cKDTree
    dist, _ = cKDTree(P64).query(P64, k=min(k, len(P64)))
    avg = dist.reshape(len(P64), -1).mean(1)
    valid = avg > 0
    mu = avg[valid].mean()
    thr = mu + ratio * np.sqrt(((avg[valid] - mu) ** 2).sum() / (valid.sum() - 1))
    return np.nonzero(valid & (avg < thr))[0]


def cpu_radius_count(P64, r=RADIUS, queries=None):
    from scipy.spatial import cKDTree
    return cKDTree(P64).query_ball_point(P64 if queries is None else queries, r, return_length=True)


def cpu_voxel(P64, voxel=VOXEL):
    cell = np.floor((P64 - (P64.min(0) - voxel / 2)) / voxel).astype(np.int64)
    _, first, inverse, counts = np.unique(cell, axis=0, return_index=True, return_inverse=True, return_counts=True)
    acc = np.zeros((len(first), 3))
    np.add.at(acc, inverse.reshape(-1), P64)
    return acc / counts[:, None], first


def cpu_clean(P64, voxel=0.015, radius=0.05, max_distance=1.0):
    vs = voxel
    if len(P64) > 10000:
        vs = voxel * max(0.5, min(2.0, 50.0 / max(1e-6, float(cpu_radius_count(P64, 2 * radius, P64[:1000]).mean()))))
    pts, first = cpu_voxel(P64, vs)
    ind = cpu_outlier(pts)
    pts, first = pts[ind], first[ind]
    near = np.linalg.norm(pts - pts.mean(0), axis=1) <= max_distance
    return pts[near], first[near]


def time_cpu(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shell", type=int, nargs="*", default=[200_000, 1_000_000])
    ap.add_argument("--uniform", type=int, nargs="*", default=[1_000_000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-only", action="store_true", help="the CPU baselines alone (no GPU needed)")
    ap.add_argument("--tuning", action="store_true", help="also time the kNN at 1 / 8 lanes per query and other occupancy targets")
    ap.add_argument("--cpu-radius-max", type=int, default=200_000,
                    help="the CPU radius count (minutes at 10^6 points) is measured up to this many points only")
    ap.add_argument("--only", nargs=3, metavar=("SCENE", "N", "OUTLIERS"), help="one scene: shell|uniform, points, 0|1")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "pointcloud_bench.json"))      # build/: git-ignored
    args = ap.parse_args()
    if not args.cpu_only and not torch.cuda.is_available():
        raise SystemExit("pointcloud_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    scenes = [("shell", n, o) for n in args.shell for o in (0, 1)] + [("uniform", n, o) for n in args.uniform for o in (0, 1)]
    if args.only:
        scenes = [(args.only[0], int(args.only[1]), int(args.only[2]))]
    res = {"device": None if args.cpu_only else torch.cuda.get_device_name(0), "rows": []}
    if not args.cpu_only:
        import collab_splats_amd as m
        import collab_splats_amd.pointcloud as pc
        m.load_library()
        dev = torch.device("cuda:0")
    for kind, n, outl in scenes:
        P = make_scene(kind, n, outl)
        row = {"scene": kind, "points": n, "outliers": bool(outl)}
        if not args.cpu_only:
            p = torch.from_numpy(P).to(dev)
            calls = {"remove_statistical_outlier": lambda: m.remove_statistical_outlier(p, K, STD_RATIO),
                     "radius_count": lambda: m.radius_count(p, RADIUS),
                     "voxel_down_sample": lambda: m.voxel_down_sample(p, VOXEL),
                     "clean_pcd": lambda: m.clean_pcd(p)}
            for name, fn in calls.items():
                t, spread = time_gpu(fn, args.reps)
                row[name + "_s"], row[name + "_spread_s"] = t, spread
            row["kept"] = int(m.remove_statistical_outlier(p, K, STD_RATIO)[1].shape[0])
            row["voxels"] = int(m.voxel_down_sample(p, VOXEL)[0].shape[0])
            row["cleaned"] = int(m.clean_pcd(p)[1].shape[0])
            if args.tuning:
                row["tuning"] = {}
                try:
                    for lanes in (1, 8):
                        for occ in (0.25, 0.5, 1.0, 2.0, 4.0):
                            pc.LANES_PER_QUERY, pc.OCCUPANCY_PER_K = lanes, occ
                            row["tuning"][f"knn_lanes{lanes}_occ{occ}_s"] = time_gpu(lambda: m.knn_mean_distance(p, K), args.reps)[0]
                finally:
                    pc.LANES_PER_QUERY, pc.OCCUPANCY_PER_K = 8, 1.0
        if not args.no_cpu:
            P64 = P.astype(np.float64)
            row["cpu"] = {"remove_statistical_outlier_s": time_cpu(lambda: cpu_outlier(P64)),
                          "radius_count_s": time_cpu(lambda: cpu_radius_count(P64)) if n <= args.cpu_radius_max else None,
                          "voxel_down_sample_s": time_cpu(lambda: cpu_voxel(P64)),
                          "clean_pcd_s": time_cpu(lambda: cpu_clean(P64)),
                          "note": "scipy cKDTree / numpy, fp64, one thread"}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"pointcloud_bench": {f"{r['scene']}_{r['points']}_{int(r['outliers'])}_outlier_ms":
                                           r.get("remove_statistical_outlier_s", float("nan")) * 1e3 for r in res["rows"]}}))


if __name__ == "__main__":
    main()
