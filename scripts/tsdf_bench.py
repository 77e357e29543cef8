"""TSDF fusion + marching cubes on the MI355X: times TSDFVolume.integrate / extract_mesh with device
events and RadegsModel.extract_mesh end to end; the fp32 numpy restatement at a small size is the CPU baseline.

    python scripts/tsdf_bench.py [--views 256] [--width 1920 --height 1080] [--gaussians 1000000] [--mesh-views 100]
                                 [--out build/tsdf_bench.json]

Rates: voxel-view pairs/s (a pair = one voxel of a unit the view touches, whether or not it projects into the image --
what the integrate kernel processes).  Share of peak = the least time the hardware could take over the measured time of
the whole integrate() call (an end-to-end figure, not one kernel's), the larger of (VALU lane-instructions / peak issue
rate) and (bytes / HBM peak); the bound named is the larger one.  Per-kernel times: run it under
`rocprofv3 --kernel-trace --stats`.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# MI355X: 256 CUs x 4 SIMDs x 32 lanes/cycle at 2.4 GHz for plain VALU instructions; 8 TB/s HBM3E (spec)
PEAK_VALU_LANE_OPS = 256 * 4 * 32 * 2.4e9
PEAK_HBM = 8.0e12
# VALU instructions per voxel-view pair in tsdf_integrate_kernel: 828 VALU instructions in the kernel body for its 4 voxels
# per lane (hipcc -O3 -ffp-contract=off -S for gfx950; a correctly rounded fp32 division is ~8 of them and a pair has 9) --
# about 200 per pair, loads / stores and the per-view prologue included
VALU_PER_PAIR = 200


def look_at(eye, target):
    from tsdf_scenes import look_at as la
    return la(eye, target, up=(0, 0, 1))


def room_views(n, W, H, centre, radius, seed=0):
    """n cameras inside a room, 0.6 - 0.9 m from the sphere, looking at points near it."""
    from tsdf_scenes import intrinsics
    rng = np.random.default_rng(seed)
    K = intrinsics(W, H, 70.0)
    vms = []
    for k in range(n):
        ang = 2 * math.pi * k / n
        r = 0.6 + 0.3 * rng.random()
        eye = np.asarray(centre) + np.array([r * math.cos(ang), r * math.sin(ang), 0.3 * rng.standard_normal()])
        tgt = np.asarray(centre) + 0.15 * rng.standard_normal(3)
        vms.append(look_at(eye, tgt))
    return np.stack(vms).astype(np.float32), np.repeat(K[None], n, 0).astype(np.float32)


@torch.no_grad()
def render_room(vm, K, W, H, centre, radius, room, dev):
    """z-depth and texture colour of a sphere inside an axis-aligned room (ray casts on the device, fp64)."""
    M = torch.as_tensor(vm, dtype=torch.float64, device=dev)
    Kt = torch.as_tensor(K, dtype=torch.float64, device=dev)
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                          indexing="ij")
    dc = torch.stack([(u - Kt[0, 2]) / Kt[0, 0], (v - Kt[1, 2]) / Kt[1, 1], torch.ones_like(u)], -1)
    R, t = M[:3, :3], M[:3, 3]
    o = -R.T @ t
    d = dc @ R
    c = torch.as_tensor(centre, dtype=torch.float64, device=dev)
    oc = o - c
    a = (d * d).sum(-1)
    b = 2 * (d * oc).sum(-1)
    disc = b * b - 4 * a * (oc @ oc - radius * radius)
    ts = torch.where(disc >= 0, (-b - torch.sqrt(disc.clamp_min(0))) / (2 * a), torch.full_like(a, math.inf))
    ts = torch.where(ts > 0, ts, torch.full_like(ts, math.inf))
    lo, hi = (torch.as_tensor(x, dtype=torch.float64, device=dev) for x in room)
    t1, t2 = (lo - o) / d, (hi - o) / d
    ts = torch.minimum(ts, torch.maximum(t1, t2).amin(-1))
    p = o + d * ts[..., None]
    col = (0.5 + 0.45 * torch.stack([torch.sin(7 * p[..., 0]), torch.sin(5 * p[..., 1] + 1), torch.cos(6 * p[..., 2])], -1))
    return ts.float()[..., None], col.clamp(0, 1).float()


def popcount_sum(words: torch.Tensor) -> int:
    n = torch.zeros((), dtype=torch.int64, device=words.device)
    for k in range(64):
        n += ((words >> k) & 1).sum()
    return int(n)


def bench_fusion(args, vs, dev):
    from collab_splats_amd import TSDFVolume
    centre, radius, room = (0.0, 0.0, 1.0), 0.3, ((-2.5, -2.5, 0.0), (2.5, 2.5, 2.6))
    vms, Ks = room_views(args.views, args.width, args.height, centre, radius)
    maps = [render_room(vms[j], Ks[j], args.width, args.height, centre, radius, room, dev) for j in range(args.views)]
    depths = torch.stack([m[0] for m in maps])
    rgbs = torch.stack([m[1] for m in maps])
    del maps
    vm_t, K_t = torch.from_numpy(vms).to(dev), torch.from_numpy(Ks).to(dev)
    tr, dt = 0.03, 1.0

    # counting pass: one kernel batch per call, the batch's view words are still in place after it
    vol = TSDFVolume(vs, tr, dt, device=dev)
    pairs = touched_unit_batches = 0
    for b in range(0, args.views, 64):
        vol.integrate(depths[b:b + 64], vm_t[b:b + 64], K_t[b:b + 64], rgbs[b:b + 64])
        pairs += popcount_sum(vol._words) * 4096
        touched_unit_batches += int((vol._words != 0).sum())
    n_units = vol.n_units
    v, f, c = vol.extract_mesh()
    n_v, n_f = int(v.shape[0]), int(f.shape[0])
    del vol, v, f, c

    t_int, t_ext = [], []
    for rep in range(args.reps + 1):                                   # rep 0: warm-up
        torch.cuda.synchronize()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        vol = TSDFVolume(vs, tr, dt, device=dev)
        e0.record()
        vol.integrate(depths, vm_t, K_t, rgbs)
        e1.record()
        vol.extract_mesh()
        e2.record()
        torch.cuda.synchronize()
        if rep:
            t_int.append(e0.elapsed_time(e1) / 1e3)
            t_ext.append(e1.elapsed_time(e2) / 1e3)
        del vol
    ti, te = float(np.median(t_int)), float(np.median(t_ext))
    valu_s = pairs * VALU_PER_PAIR / PEAK_VALU_LANE_OPS
    # bytes (a lower bound): every touched unit's 5 planes read and written once per batch + the depth rows the allocation
    # samples (every 4th row; the pixels voxels project to are scene-dependent and not counted)
    bytes_ = touched_unit_batches * 2 * 5 * 4096 * 4 + depths.numel() * 4 // 4
    hbm_s = bytes_ / PEAK_HBM
    return {
        "voxel_size": vs, "sdf_trunc": tr, "depth_trunc": dt, "views": args.views, "width": args.width, "height": args.height,
        "units_allocated": n_units, "unit_batches": touched_unit_batches, "voxel_view_pairs": pairs, "vertices": n_v, "triangles": n_f,
        "integrate_s": ti, "extract_s": te, "integrate_spread_s": [min(t_int), max(t_int)],
        "pairs_per_s": pairs / ti, "views_per_s": args.views / ti,
        "share_of_peak": max(valu_s, hbm_s) / ti, "bound": "VALU issue" if valu_s >= hbm_s else "HBM bandwidth",
        "valu_bound_s": valu_s, "hbm_bound_s": hbm_s,
    }


def bench_model(args, dev):
    import tsdf_scenes as S
    model = S.sphere_gaussians(args.gaussians).to(dev)
    model.eval()
    _, vms, _, _ = S.sphere_views(args.mesh_views, 8, 8)
    K = S.intrinsics(args.width, args.height, 60.0)
    cams = [S.pinhole_camera(M, K, args.width, args.height) for M in vms]
    out = None
    times = []
    for rep in range(2):                                               # rep 0: warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.extract_mesh(cams, voxel_size=0.01, sdf_trunc=0.03, depth_trunc=1.0, batch_size=4)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return {"gaussians": args.gaussians, "views": args.mesh_views, "width": args.width, "height": args.height,
            "extract_mesh_s": times[1], "vertices": int(out[0].shape[0]), "triangles": int(out[1].shape[0])}


def bench_cpu_restatement():
    import tsdf_scenes as S
    from tsdf_restatement import RestatedTSDF
    d, vm, K, rgb = S.sphere_views(24, 128, 96)
    r = RestatedTSDF(0.01, 0.03, 1.0)
    t0 = time.perf_counter()
    pairs = 0
    for j in range(24):
        pairs += len(r.touched_units(d[j, ..., 0], vm[j], K[j])) * 4096
        r.integrate_view(d[j, ..., 0], vm[j], K[j], rgb[j])
    t1 = time.perf_counter()
    v, f, c = r.extract_mesh()
    t2 = time.perf_counter()
    return {"views": 24, "width": 128, "height": 96, "voxel_size": 0.01, "voxel_view_pairs": pairs,
            "integrate_s": t1 - t0, "extract_s": t2 - t1, "pairs_per_s": pairs / (t1 - t0), "triangles": int(len(f)),
            "note": "numpy fp32 restatement, one CPU thread (touched-unit enumeration included in integrate_s)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--mesh-views", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "tsdf_bench.json"))      # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_bench.py measures the MI355X: no GPU here (CPU figures are 'not measured')")
    import collab_splats_amd
    collab_splats_amd.load_library()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "fusion": [bench_fusion(args, vs, dev) for vs in (0.01, 0.004)]}
    torch.cuda.empty_cache()
    res["radegs_extract_mesh"] = bench_model(args, dev)
    res["cpu_restatement"] = bench_cpu_restatement()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    for r in res["fusion"]:
        print(f"fusion vs={r['voxel_size']}: {r['views']} views {r['width']}x{r['height']}: integrate {r['integrate_s'] * 1e3:.1f} ms "
              f"({r['pairs_per_s'] / 1e9:.2f} G voxel-view pairs/s, {r['views_per_s']:.0f} views/s, "
              f"{100 * r['share_of_peak']:.1f} % of peak, {r['bound']}-bound), extract {r['extract_s'] * 1e3:.1f} ms, "
              f"{r['units_allocated']} units, {r['triangles']} triangles")
    m = res["radegs_extract_mesh"]
    print(f"RadegsModel.extract_mesh: {m['gaussians']} Gaussians, {m['views']} views {m['width']}x{m['height']}: "
          f"{m['extract_mesh_s']:.3f} s, {m['triangles']} triangles")
    c = res["cpu_restatement"]
    print(f"CPU restatement: {c['views']} views {c['width']}x{c['height']}: integrate {c['integrate_s']:.2f} s "
          f"({c['pairs_per_s'] / 1e6:.2f} M pairs/s), extract {c['extract_s']:.2f} s")
    print(json.dumps({"tsdf_bench": {"integrate_ms_vs0.01": res["fusion"][0]["integrate_s"] * 1e3,
                                     "integrate_ms_vs0.004": res["fusion"][1]["integrate_s"] * 1e3,
                                     "extract_mesh_1M_s": m["extract_mesh_s"]}}))


if __name__ == "__main__":
    main()
