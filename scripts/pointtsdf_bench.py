"""Point-cloud TSDF fusion with space carving on the MI355X: a synthetic room with a sphere in it, seen
at 1080p from inside, every pixel integrated from its camera's centre (PointTSDFVolume.integrate_depth), carving on and off.

    python scripts/pointtsdf_bench.py [--views 4] [--width 1920 --height 1080] [--voxel 0.01] [--trunc 0.03]
                                      [--out build/pointtsdf_bench.json]

Per mode: ms per view and stage (each stage synchronised: count, emit + allocation, sort + ranges, accumulate; the whole call
with device events, lift included), units allocated, (unit, ray) pairs, voxel updates (the sum of the count plane) and the
accumulate kernel's updates per second -- the figure to set beside the 23 G/s of poisson_splat_kernel's scattered 64-bit
global atomics.
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


def scene(args, dev):
    from tsdf_bench import render_room, room_views
    centre, radius, room = (0.0, 0.0, 1.0), 0.3, ((-2.5, -2.5, 0.0), (2.5, 2.5, 2.6))
    vms, Ks = room_views(args.views, args.width, args.height, centre, radius)
    maps = [render_room(vms[j], Ks[j], args.width, args.height, centre, radius, room, dev) for j in range(args.views)]
    c2w = np.stack([(np.linalg.inv(M.astype(np.float64)) @ np.diag([1.0, -1.0, -1.0, 1.0]))[:3, :4] for M in vms]).astype(np.float32)
    intr = np.stack([Ks[:, 0, 0], Ks[:, 1, 1], Ks[:, 0, 2], Ks[:, 1, 2]], 1).astype(np.float32)
    return (torch.stack([m[0] for m in maps]), torch.stack([m[1] for m in maps]), torch.from_numpy(c2w).to(dev),
            torch.from_numpy(intr).to(dev))


def bench(args, carve, depths, rgbs, c2w, intr, dev):
    from collab_splats_amd import PointTSDFVolume
    V = depths.shape[0]

    def run(timings=None):
        vol = PointTSDFVolume(args.voxel, args.trunc, carve, device=dev)
        for j in range(V):                                               # a view per call, as the model's batches arrive
            vol.integrate_depth(depths[j:j + 1], c2w[j:j + 1], intr[j:j + 1], rgbs=rgbs[j:j + 1], _timings=timings)
        return vol

    run()                                                                # warm-up
    stages: dict = {}
    vol = run(stages)
    updates = int(vol._count[:vol.n_units].sum())
    res = {"space_carving": carve, "views": V, "rays": vol.n_rays, "units_allocated": vol.n_units, "pairs": vol.n_pairs,
           "voxel_updates": updates, "unit_bytes": vol.n_units * 112 * 1024,
           "stage_ms_per_view": {k: 1e3 * v / V for k, v in stages.items()},
           "accumulate_updates_per_s": updates / stages["accumulate"]}
    del vol
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        vol = run()
        e1.record()
        mesh = vol.extract_mesh(args.min_weight)
        e2.record()
        torch.cuda.synchronize()
        times.append((e0.elapsed_time(e1), e1.elapsed_time(e2)))
        res["triangles"] = int(mesh[1].shape[0])
        del vol, mesh
    res["integrate_ms_per_view"] = float(np.median([t[0] for t in times])) / V
    res["extract_ms"] = float(np.median([t[1] for t in times]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--trunc", type=float, default=0.03)
    ap.add_argument("--min-weight", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "pointtsdf_bench.json"))   # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointtsdf_bench.py measures the MI355X: no GPU here")
    import collab_splats_amd
    collab_splats_amd.load_library()
    dev = torch.device("cuda:0")
    depths, rgbs, c2w, intr = scene(args, dev)
    res = {"device": torch.cuda.get_device_name(0), "width": args.width, "height": args.height, "voxel_size": args.voxel,
           "sdf_trunc": args.trunc, "modes": [bench(args, carve, depths, rgbs, c2w, intr, dev) for carve in (True, False)]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    for r in res["modes"]:
        st = ", ".join(f"{k} {v:.2f}" for k, v in r["stage_ms_per_view"].items())
        print(f"carving {'on' if r['space_carving'] else 'off'}: {r['views']} views {args.width}x{args.height}, {r['rays']} rays: "
              f"{r['integrate_ms_per_view']:.1f} ms/view (stages, synchronised: {st}), extract {r['extract_ms']:.1f} ms, "
              f"{r['units_allocated']} units ({r['unit_bytes'] / 2 ** 20:.0f} MiB), {r['pairs']} pairs, {r['voxel_updates']} voxel updates, "
              f"accumulate {r['accumulate_updates_per_s'] / 1e9:.2f} G updates/s, {r['triangles']} triangles")
    print(json.dumps({"pointtsdf_bench": res["modes"]}))


if __name__ == "__main__":
    main()
