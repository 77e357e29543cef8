"""Mesh finishing on the MI355X: times, with device events (median of --reps after a warm-up),
mesh_edge_stats, mesh_components, filter_mesh_components, mesh_holes and fill_holes on the TSDF mesh of the tsdf_scenes sphere
at voxel_size 0.004, plane_inlier_counts for each tile size and segment_plane on clouds of 1 M and 5 M points x 1000
hypotheses (60 % on a planted plane).  The CPU baseline is the one-thread numpy restatement (tests/meshclean_restatement.py) on
the same inputs; an inlier count of more than --cpu-max-pairs (point, plane) pairs is timed on the first hypotheses only and
reported as such.

    python scripts/meshclean_bench.py [--voxel-size 0.004] [--points 1000000 5000000] [--hypotheses 1000] [--reps 3]
                                      [--no-cpu] [--out build/meshclean_bench.json]

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


def sphere_mesh(vs, dev, n_views=100, W=320, H=240):
    """TSDF mesh of the sphere of tsdf_scenes, on the device (as scripts/meshquery_bench.py builds it)."""
    import tsdf_scenes as S
    from collab_splats_amd import TSDFVolume
    d, vm, K, rgb = S.sphere_views(n_views, W, H)
    vol = TSDFVolume(vs, 3 * vs if vs > 0.005 else 0.02, 3.0, device=dev)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    for b in range(0, n_views, 32):
        vol.integrate(t(d[b:b + 32]), t(vm[b:b + 32]), t(K[b:b + 32]), t(rgb[b:b + 32]))
    return vol.extract_mesh()


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


def time_cpu(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel-size", type=float, default=0.004)
    ap.add_argument("--points", type=int, nargs="*", default=[1_000_000, 5_000_000])
    ap.add_argument("--hypotheses", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-mesh", action="store_true")
    ap.add_argument("--cpu-max-pairs", type=float, default=2e8)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "meshclean_bench.json"))      # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshclean_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    torch.set_num_threads(1)
    import collab_splats_amd as m
    import meshclean_restatement as R
    import meshclean_scenes as Q
    from collab_splats_amd import meshclean
    m.load_library()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "mesh": {}, "plane": []}
    if not args.no_mesh:
        v, f, c = sphere_mesh(args.voxel_size, dev)
        row = {"voxel_size": args.voxel_size, "vertices": int(v.shape[0]), "triangles": int(f.shape[0])}
        calls = {"mesh_edge_stats": lambda: m.mesh_edge_stats(v, f), "mesh_components": lambda: m.mesh_components(v, f),
                 "filter_mesh_components": lambda: m.filter_mesh_components(v, f, attributes=(c,)),
                 "mesh_holes": lambda: m.mesh_holes(v, f), "fill_holes": lambda: m.fill_holes(v, f, 3.0, (c,))}
        for name, fn in calls.items():
            row[name + "_s"] = time_gpu(fn, args.reps)
        row["stats"] = m.mesh_edge_stats(v, f)
        row["components"] = int(m.mesh_components(v, f)[1].shape[0])
        if not args.no_cpu:
            vh, fh = v.cpu().numpy(), f.cpu().numpy()
            row["cpu"] = {"mesh_edge_stats_s": time_cpu(lambda: R.mesh_edge_stats(vh, fh)),
                          "mesh_components_s": time_cpu(lambda: R.mesh_components(vh, fh)),
                          "mesh_holes_s": time_cpu(lambda: R.mesh_holes(vh, fh)), "note": "numpy restatement, one thread"}
        res["mesh"] = row
        print(f"mesh {row}", flush=True)
    for n in args.points:
        P, _ = Q.planted_plane(n, seed=1)
        p = torch.from_numpy(P).to(dev)
        _, planes = m.ransac_planes(p, args.hypotheses, 0)
        row = {"points": n, "hypotheses": args.hypotheses}
        tile = meshclean.PLANE_TILE
        for other in (8, 16, 32):
            meshclean.PLANE_TILE = other
            row[f"plane_inlier_counts_tile{other}_s"] = time_gpu(lambda: m.plane_inlier_counts(p, planes, 0.02), args.reps)
        meshclean.PLANE_TILE = tile
        row["segment_plane_s"] = time_gpu(lambda: m.segment_plane(p, 0.02, 3, args.hypotheses, 0), args.reps)
        plane, inl = m.segment_plane(p, 0.02, 3, args.hypotheses, 0)
        row["inliers"] = int(inl.shape[0])
        if not args.no_cpu:
            h = max(1, min(args.hypotheses, int(args.cpu_max_pairs // n)))
            ph = planes[:h].cpu().numpy()
            row["cpu"] = {"plane_inlier_counts_s": time_cpu(lambda: R.plane_inlier_counts(P, ph, 0.02)), "hypotheses": h,
                          "note": "numpy restatement, one thread" + ("" if h == args.hypotheses else f", the first {h} hypotheses only")}
        res["plane"].append(row)
        print(f"plane {row}", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"meshclean_bench": res}))


if __name__ == "__main__":
    main()
