"""Hole filling with subdivision and fairing on the MI355X: times, with device events (median of --reps
after a warm-up), fill_holes (the fan alone) and fill_holes_nicely on the marching-cubes mesh of the tsdf_scenes sphere with
three caps cut out of it (angular radii --caps: holes of perimeter 2 pi 0.3 sin(theta)), at each of --voxel-sizes; then, on
the subdivided fans of the same mesh, fair_vertices with the LDS path (one workgroup per patch, all iterations) and with one
launch per iteration.  Synthetic scenes only.

    python scripts/meshfill_bench.py [--voxel-sizes 0.01 0.005] [--caps 0.15 0.3 0.5] [--reps 3] [--out build/meshfill_bench.json]

Per-kernel times: run it under `rocprofv3 --kernel-trace --stats` (with --reps 1).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

CENTRE, AXES = (0.1, -0.05, 0.2), ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, -1.0))


def cut_caps(v, f, caps):
    """The faces of the sphere mesh without those whose centroid lies within caps[k] radians of AXES[k]."""
    c = v[f.long()].mean(1) - torch.tensor(CENTRE, device=v.device)
    c = c / c.norm(dim=1, keepdim=True)
    keep = torch.ones(f.shape[0], dtype=torch.bool, device=v.device)
    for theta, axis in zip(caps, AXES):
        keep &= (c * torch.tensor(axis, device=v.device)).sum(1) < float(np.cos(theta))
    return f[keep].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel-sizes", type=float, nargs="*", default=[0.01, 0.005])
    ap.add_argument("--caps", type=float, nargs="*", default=[0.15, 0.3, 0.5])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "meshfill_bench.json"))      # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshfill_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    import collab_splats_amd as m
    from collab_splats_amd import meshfill
    from meshclean_bench import sphere_mesh, time_gpu
    m.load_library()
    dev = torch.device("cuda:0")
    default = meshfill.ENABLE_LDS_FAIR
    res = {"device": torch.cuda.get_device_name(0), "lds_max_vertices": meshfill.LDS_MAX_VERTICES, "rows": []}
    for vs in args.voxel_sizes:
        v, f, c = sphere_mesh(vs, dev)
        f = cut_caps(v, f, args.caps)
        st = m.mesh_edge_stats(v, f)
        row = {"voxel_size": vs, "vertices": int(v.shape[0]), "triangles": int(f.shape[0]), "n_boundary": st["n_boundary"],
               "mean_edge_length": st["mean_edge_length"]}
        row["fill_holes_s"] = time_gpu(lambda: m.fill_holes(v, f, 3.0, (c,)), args.reps)
        for lds in (True, False):
            meshfill.ENABLE_LDS_FAIR = lds
            row["fill_holes_nicely_s" + ("" if lds else "_no_lds")] = time_gpu(lambda: m.fill_holes_nicely(v, f, 3.0, attributes=(c,)), args.reps)
        meshfill.ENABLE_LDS_FAIR = default
        v4, f4, _, n_filled, info = m.fill_holes_nicely(v, f, 3.0, attributes=(c,))
        row.update(n_filled=n_filled, n_splits=info["n_splits"], rounds=info["rounds"], iterations=info["iterations"].tolist(),
                   n_new_vertices=info["n_new_vertices"], n_boundary_after=m.mesh_edge_stats(v4, f4)["n_boundary"])
        # the two halves apart, and fairing on both paths: the fans, their subdivision, then fair_vertices alone
        v2, f2, _, _ = m.fill_holes(v, f, 3.0)
        max_len = st["mean_edge_length"]
        region = torch.arange(f2.shape[0], device=dev) >= f.shape[0]
        row["subdivide_mesh_s"] = time_gpu(lambda: m.subdivide_mesh(v2, f2, max_len, 10000 * n_filled, region), args.reps)
        v3, f3, _, _, _, _ = m.subdivide_mesh(v2, f2, max_len, 10000 * n_filled, region)
        free = torch.arange(v3.shape[0], device=dev) >= v.shape[0]
        for lds in (True, False):
            meshfill.ENABLE_LDS_FAIR = lds
            row["fair_vertices_s" + ("_lds" if lds else "_launches")] = time_gpu(lambda: m.fair_vertices(v3, f3, free, 1e-3 * max_len), args.reps)
        meshfill.ENABLE_LDS_FAIR = default
        res["rows"].append(row)
        print(f"meshfill {row}", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"meshfill_bench": res}))


if __name__ == "__main__":
    main()
