"""Minimum-area hole triangulation and edge flips on the MI355X: times, with device events (median of
--reps after a warm-up), triangulate_holes, flip_edges over the triangulated and subdivided patches, and fill_holes_nicely with
the fan against min_area + flips, on the two meshes of scripts/meshfill_bench.py (the marching-cubes mesh of the tsdf_scenes
sphere with three caps cut out, at each of --voxel-sizes) and on a sheet with --small-holes holes of one quad each; then
triangulate_holes alone on single rims of --loops edges, which reports the LDS path (up to LDS_LOOP edges) and the workspace
path apart.  Synthetic scenes only.

    python scripts/meshtri_bench.py [--voxel-sizes 0.01 0.005] [--small-holes 4096] [--loops 64 176 177 512 1024] [--reps 3]
                                    [--out build/meshtri_bench.json]

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


def holed_sheet(n_holes):
    """A sheet with every fourth quad of every fourth row missing, n_holes of them in all: rims of four edges."""
    import meshclean_scenes as MS
    side = int(np.ceil(np.sqrt(n_holes)))
    n = 1 << int(np.ceil(np.log2(4 * side + 1)))
    holes = [(4 * (k % side) + 1, 4 * (k % side) + 2, 4 * (k // side) + 1, 4 * (k // side) + 2) for k in range(n_holes)]
    return MS.sheet(n, holes), 8.0 / n


def measure(m, time_gpu, v, f, c, size, reps):
    """The row of one mesh: the three calls, and the patch's counts."""
    dev = v.device
    st = m.mesh_edge_stats(v, f)
    row = {"vertices": int(v.shape[0]), "triangles": int(f.shape[0]), "n_boundary": st["n_boundary"], "mean_edge_length": st["mean_edge_length"]}
    row["fill_holes_s"] = time_gpu(lambda: m.fill_holes(v, f, size, (c,)), reps)
    row["triangulate_holes_s"] = time_gpu(lambda: m.triangulate_holes(v, f, size, (c,)), reps)
    v2, f2, _, n_filled, tinfo = m.triangulate_holes(v, f, size)
    row.update(n_filled=n_filled, n_triangulated=tinfo["n_triangulated"], n_fans=tinfo["n_fans"])
    region = torch.arange(f2.shape[0], device=dev) >= f.shape[0]
    v3, f3, _, origin, _, _ = m.subdivide_mesh(v2, f2, st["mean_edge_length"], 10000 * max(n_filled, 1), region)
    region = region[origin]
    row["flip_edges_s"] = time_gpu(lambda: m.flip_edges(v3, f3, region), reps)
    _, n_flips, rounds = m.flip_edges(v3, f3, region)
    row.update(flip_faces=int(f3.shape[0]), flip_region_faces=int(region.sum()), n_flips=n_flips, flip_rounds=rounds)
    row["fill_holes_nicely_fan_s"] = time_gpu(lambda: m.fill_holes_nicely(v, f, size, attributes=(c,)), reps)
    row["fill_holes_nicely_min_area_flips_s"] = time_gpu(
        lambda: m.fill_holes_nicely(v, f, size, attributes=(c,), triangulation="min_area", flip=True), reps)
    v4, f4, _, _, info = m.fill_holes_nicely(v, f, size, attributes=(c,), triangulation="min_area", flip=True)
    row["min_area_flips"] = {k: (x.tolist()[:8] if isinstance(x, torch.Tensor) else x) for k, x in info.items()}      # (eight patches' iterations)
    row["n_boundary_after"] = m.mesh_edge_stats(v4, f4)["n_boundary"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel-sizes", type=float, nargs="*", default=[0.01, 0.005])
    ap.add_argument("--caps", type=float, nargs="*", default=[0.15, 0.3, 0.5])
    ap.add_argument("--small-holes", type=int, default=4096)
    ap.add_argument("--loops", type=int, nargs="*", default=[64, 176, 177, 512, 1024])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "meshtri_bench.json"))       # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshtri_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    import collab_splats_amd as m
    from collab_splats_amd import meshfill
    from meshclean_bench import sphere_mesh, time_gpu
    from meshfill_bench import cut_caps
    import meshtri_scenes as S
    m.load_library()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "lds_loop": meshfill.LDS_LOOP, "max_loop": meshfill.MAX_LOOP, "rows": [], "loops": []}
    for vs in args.voxel_sizes:
        v, f, c = sphere_mesh(vs, dev)
        f = cut_caps(v, f, args.caps)
        row = {"mesh": f"sphere, voxel {vs}"}
        row.update(measure(m, time_gpu, v, f, c, 3.0, args.reps))
        res["rows"].append(row)
        print(f"meshtri {row}", flush=True)
    if args.small_holes > 0:
        (V, T), size = holed_sheet(args.small_holes)
        v, f = torch.from_numpy(V).to(dev), torch.from_numpy(T).to(dev)
        row = {"mesh": f"sheet, {args.small_holes} one-quad holes"}
        row.update(measure(m, time_gpu, v, f, torch.from_numpy(S.colour_ramp(V)).to(dev), size, args.reps))
        res["rows"].append(row)
        print(f"meshtri {row}", flush=True)
    for n in args.loops:                                            # one rim of n edges: the table's path by its length
        V, T = S.annulus(S.circle(n, 0.1, 0.1 * 0.2 * np.pi / n, n))       # (lifted by a tenth of an edge: the perimeter stays 0.63)
        v, f = torch.from_numpy(V).to(dev), torch.from_numpy(T).to(dev)
        row = {"edges": n, "path": "lds" if n <= meshfill.LDS_LOOP else "workspace",
               "n_triangulated": m.triangulate_holes(v, f, 1.0)[4]["n_triangulated"],
               "triangulate_holes_s": time_gpu(lambda: m.triangulate_holes(v, f, 1.0), args.reps),
               "mesh_holes_s": time_gpu(lambda: m.mesh_holes(v, f), args.reps)}
        res["loops"].append(row)
        print(f"meshtri loop {row}", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"meshtri_bench": res}))


if __name__ == "__main__":
    main()
