"""Angle-and-area hole triangulation and curvature fairing on the MI355X: times, with device events
(median of --reps after a warm-up), triangulate_holes under both metrics, fair_vertices_curvature alone over the subdivided
patches (with the iterations of every patch), and fill_holes_nicely with min_area + flips against the same with angle_area and
curvature fairing, on the meshes of scripts/meshtri_bench.py (the marching-cubes mesh of the tsdf_scenes sphere with three caps
cut out, at each of --voxel-sizes, and a sheet with --small-holes holes of one quad each); then triangulate_holes under both
metrics on single rims of --loops edges (a dome: the rim is not flat against its faces).  Synthetic scenes only.

    python scripts/meshsmooth_bench.py [--voxel-sizes 0.01 0.005] [--small-holes 4096] [--loops 64 163 164 512 1024] [--reps 3]
                                       [--out build/meshsmooth_bench.json]

Per-kernel times: run it under `rocprofv3 --kernel-trace --stats` (with --reps 1).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SMOOTH = dict(triangulation="min_area", metric="angle_area", flip=True, fairing="curvature")


def measure(m, time_gpu, v, f, c, size, reps):
    """The row of one mesh: the triangulation under both metrics, the curvature solve alone, the two fills."""
    dev = v.device
    st = m.mesh_edge_stats(v, f)
    row = {"vertices": int(v.shape[0]), "triangles": int(f.shape[0]), "n_boundary": st["n_boundary"], "mean_edge_length": st["mean_edge_length"]}
    for metric in ("area", "angle_area"):
        row[f"triangulate_holes_{metric}_s"] = time_gpu(lambda: m.triangulate_holes(v, f, size, (c,), metric=metric), reps)
    tinfo = m.triangulate_holes(v, f, size, metric="angle_area")[4]
    row.update(n_triangulated=tinfo["n_triangulated"], n_fans=tinfo["n_fans"], badness_max=int(tinfo["badness"].max()) if tinfo["n_triangulated"] else 0)
    plain = dict(triangulation="min_area", metric="angle_area", flip=True)
    v4, f4, _, _, info = m.fill_holes_nicely(v, f, size, attributes=(c,), **plain)       # the membrane's result: the solve's start
    free = torch.arange(v4.shape[0], device=dev) >= v.shape[0]
    row["fair_vertices_curvature_s"] = time_gpu(lambda: m.fair_vertices_curvature(v4, f4, free), reps)
    cinfo = m.fair_vertices_curvature(v4, f4, free)[1]
    row.update(n_free=int(free.sum()), membrane_iterations=info["iterations"].tolist()[:8], curvature_iterations=cinfo["iterations"].tolist()[:8],
               curvature_iterations_max=int(cinfo["iterations"].max()) if cinfo["iterations"].numel() else 0,
               curvature_converged=int(cinfo["converged"].sum()), curvature_patches=int(cinfo["code"].numel()),
               curvature_codes=torch.bincount(cinfo["code"].long(), minlength=4).tolist(),
               curvature_residual_max=float(cinfo["residual"].max()) if cinfo["residual"].numel() else 0.0)
    row["fill_holes_nicely_min_area_flips_s"] = time_gpu(
        lambda: m.fill_holes_nicely(v, f, size, attributes=(c,), triangulation="min_area", flip=True), reps)
    row["fill_holes_nicely_angle_area_flips_s"] = time_gpu(lambda: m.fill_holes_nicely(v, f, size, attributes=(c,), **plain), reps)
    row["fill_holes_nicely_smooth_s"] = time_gpu(lambda: m.fill_holes_nicely(v, f, size, attributes=(c,), **SMOOTH), reps)
    v5, f5 = m.fill_holes_nicely(v, f, size, attributes=(c,), **SMOOTH)[:2]
    row["n_boundary_after"] = m.mesh_edge_stats(v5, f5)["n_boundary"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel-sizes", type=float, nargs="*", default=[0.01, 0.005])
    ap.add_argument("--caps", type=float, nargs="*", default=[0.15, 0.3, 0.5])
    ap.add_argument("--small-holes", type=int, default=4096)
    ap.add_argument("--loops", type=int, nargs="*", default=[64, 163, 164, 512, 1024])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "meshsmooth_bench.json"))    # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshsmooth_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    import collab_splats_amd as m
    from collab_splats_amd import meshfill
    from meshclean_bench import sphere_mesh, time_gpu
    from meshfill_bench import cut_caps
    from meshtri_bench import holed_sheet
    import meshsmooth_scenes as S
    m.load_library()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "angle_lds_loop": meshfill.ANGLE_LDS_LOOP, "lds_loop": meshfill.LDS_LOOP,
           "cg_vertices": meshfill.CG_VERTICES, "rows": [], "loops": []}
    for vs in args.voxel_sizes:
        v, f, c = sphere_mesh(vs, dev)
        f = cut_caps(v, f, args.caps)
        row = {"mesh": f"sphere, voxel {vs}"}
        row.update(measure(m, time_gpu, v, f, c, 3.0, args.reps))
        res["rows"].append(row)
        print(f"meshsmooth {row}", flush=True)
    if args.small_holes > 0:
        (V, T), size = holed_sheet(args.small_holes)
        v, f = torch.from_numpy(V).to(dev), torch.from_numpy(T).to(dev)
        row = {"mesh": f"sheet, {args.small_holes} one-quad holes"}
        row.update(measure(m, time_gpu, v, f, torch.from_numpy(S.colour_ramp(V)).to(dev), size, args.reps))
        res["rows"].append(row)
        print(f"meshsmooth {row}", flush=True)
    for n in args.loops:                                            # one rim of n edges: the table's path by its length
        V, T = S.dome(n, 0.1, 0.05, n, lift=0.1 * 0.2 * math.pi / n)    # (lifted by a tenth of an edge: the perimeter stays 0.63)
        v, f = torch.from_numpy(V).to(dev), torch.from_numpy(T).to(dev)
        row = {"edges": n, "path_area": "lds" if n <= meshfill.LDS_LOOP else "workspace",
               "path_angle_area": "lds" if n <= meshfill.ANGLE_LDS_LOOP else "workspace",
               "n_triangulated": m.triangulate_holes(v, f, 1.0, metric="angle_area")[4]["n_triangulated"]}
        for metric in ("area", "angle_area"):
            row[f"triangulate_holes_{metric}_s"] = time_gpu(lambda: m.triangulate_holes(v, f, 1.0, metric=metric), args.reps)
        res["loops"].append(row)
        print(f"meshsmooth loop {row}", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"meshsmooth_bench": res}))


if __name__ == "__main__":
    main()
