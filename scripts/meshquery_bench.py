"""Radius-graph clustering of mesh vertices on the MI355X: times meshquery.cluster_labels with device
events (median of --reps after a warm-up) on the TSDF meshes of the tsdf_scenes sphere at voxel_size 0.01 and 0.004 and on a
synthetic cloud of --cloud points on the same sphere, for masks of about 5 % and 30 % of the vertices (the vertices of
highest blob similarity) and r = 0.01 and 0.03.  The CPU baseline is the reference's algorithm in its feasible sparse form
(scipy cKDTree.query_pairs + connected_components, fp64, one thread; the reference's dense n_valid x n_valid adjacency cannot
be allocated beyond a few 10^4 selected vertices), run where its pair list stays below --cpu-max-pairs.

    python scripts/meshquery_bench.py [--cloud 1000000] [--reps 3] [--no-cpu] [--only MESH FRACTION RADIUS]
                                      [--out build/meshquery_bench.json]

Per-kernel times: run it under `rocprofv3 --kernel-trace --stats` (e.g. with --no-cpu --only 0.004 0.3 0.03 --reps 1).
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

CENTRE, RADIUS = np.array([0.1, -0.05, 0.2]), 0.3


def sphere_mesh(vs, dev, n_views=100, W=320, H=240):
    """TSDF mesh of the sphere of tsdf_scenes, on the device (as scripts/meshmap_bench.py builds it)."""
    import tsdf_scenes as S
    from collab_splats_amd import TSDFVolume
    d, vm, K, rgb = S.sphere_views(n_views, W, H)
    vol = TSDFVolume(vs, 3 * vs if vs > 0.005 else 0.02, 3.0, device=dev)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    for b in range(0, n_views, 32):
        vol.integrate(t(d[b:b + 32]), t(vm[b:b + 32]), t(K[b:b + 32]), t(rgb[b:b + 32]))
    return vol.extract_mesh()[0]


def sphere_cloud(n, dev, seed=0):
    d = np.random.default_rng(seed).standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return torch.from_numpy((CENTRE + RADIUS * d).astype(np.float32)).to(dev)


def blob_similarity(V, seed=1, n_blobs=12, width=0.15, noise=0.05):
    """A similarity field of Gaussian blobs on the sphere plus noise, [M] fp32 on V's device."""
    g = torch.Generator().manual_seed(seed)
    c = torch.nn.functional.normalize(torch.randn(n_blobs, 3, generator=g), dim=1).to(V.device)
    d = torch.nn.functional.normalize(V - torch.as_tensor(CENTRE, dtype=torch.float32, device=V.device), dim=1)
    s = torch.exp(-(2 - 2 * d @ c.T) / (2 * width ** 2)).max(1).values                  # |d - c|^2 = 2 - 2 d.c
    return s + noise * torch.randn(len(V), generator=g).to(V.device)


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


def bench_cpu(V, mask, r, max_pairs):
    """mask -> cKDTree radius pairs -> sparse adjacency -> connected_components -> the > 10 filter (counted only)."""
    try:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import connected_components
        from scipy.spatial import cKDTree
    except ImportError:
        return {"note": "scipy not importable: not measured"}
    Vh = V.double().cpu().numpy()
    mh = mask.cpu().numpy()
    valid = np.where(mh)[0]
    tree = cKDTree(Vh[valid])
    est = (int(tree.count_neighbors(tree, r)) - len(valid)) // 2
    if est > max_pairs:
        return {"note": f"about {est} pairs: above --cpu-max-pairs, not measured"}
    t0 = time.perf_counter()
    valid = np.where(mh)[0]
    tree = cKDTree(Vh[valid])
    pairs = tree.query_pairs(r, output_type="ndarray")
    n = len(valid)
    adj = csr_matrix((np.ones(len(pairs), bool), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    n_comp, lab = connected_components(adj, directed=False)
    kept = int((np.bincount(lab, minlength=n_comp) > 10).sum())
    return {"cpu_s": time.perf_counter() - t0, "pairs": int(len(pairs)), "clusters": kept,
            "note": "scipy cKDTree.query_pairs + connected_components, fp64, one thread"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel-sizes", type=float, nargs="*", default=[0.01, 0.004])
    ap.add_argument("--cloud", type=int, default=1_000_000)
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.05, 0.3])
    ap.add_argument("--radii", type=float, nargs="+", default=[0.01, 0.03])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-max-pairs", type=int, default=60_000_000)
    ap.add_argument("--only", nargs=3, metavar=("MESH", "FRACTION", "RADIUS"),
                    help="one workload: MESH is a voxel size or 'cloud'")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "meshquery_bench.json"))      # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshquery_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    import collab_splats_amd
    from collab_splats_amd.meshquery import cluster_labels
    collab_splats_amd.load_library()
    dev = torch.device("cuda:0")
    if args.only:
        args.fractions, args.radii = [float(args.only[1])], [float(args.only[2])]
        args.voxel_sizes, args.cloud = ([], args.cloud) if args.only[0] == "cloud" else ([float(args.only[0])], 0)
    meshes = {f"voxel {vs}": sphere_mesh(vs, dev) for vs in args.voxel_sizes}
    if args.cloud > 0:
        meshes[f"cloud {args.cloud}"] = sphere_cloud(args.cloud, dev)
    res = {"device": torch.cuda.get_device_name(0), "rows": []}
    for name, V in meshes.items():
        sim = blob_similarity(V)
        for frac in args.fractions:
            mask = sim > torch.quantile(sim[:: max(1, len(sim) // 1_000_000)], 1.0 - frac)
            for r in args.radii:
                t, spread = time_gpu(lambda: cluster_labels(V, mask, r), args.reps)
                labels, sizes = cluster_labels(V, mask, r)
                row = {"mesh": name, "vertices": int(V.shape[0]), "selected": int(mask.sum()), "radius": r,
                       "cluster_labels_s": t, "spread_s": spread, "clusters": int(sizes.shape[0]),
                       "largest": int(sizes.max()) if len(sizes) else 0}
                if not args.no_cpu:
                    row["cpu"] = bench_cpu(V, mask, r, args.cpu_max_pairs)
                    if "clusters" in row["cpu"]:
                        row["cpu"]["same_cluster_count"] = row["cpu"]["clusters"] == row["clusters"]
                res["rows"].append(row)
                print(f"{name}: {row['vertices']} vertices, {row['selected']} selected ({100 * frac:.0f} %), r = {r}: "
                      f"{t * 1e3:.3f} ms, {row['clusters']} clusters (largest {row['largest']})"
                      + (f"; CPU {row['cpu']}" if "cpu" in row else ""), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"meshquery_bench": {f"{r['mesh']}_{r['selected']}_{r['radius']}_ms": r["cluster_labels_s"] * 1e3
                                          for r in res["rows"]}}))


if __name__ == "__main__":
    main()
