"""The level-set search along rays on the MI355X: for synthetic scenes (``synthetic.random_scene``) of
--gaussians Gaussians at --voxel-size, ``DensityField.raycast`` at --rays rays through the rendered depths of the scene's own
camera (a seeded sample of the pixels with alpha > 0; the ray from the camera centre through the depth point, searched over
+- 8 voxels around it), three levels, against the same search composed from ``DensityField.query`` calls alone (what the field
could do before the kernel: [64 M, 3] points and [64 M] densities per pass, one list walk per sample).  Device events, median of
--reps after a warm-up; the hits per level and the longest and mean list length go with the times.  No time is a pass
condition.  Every scene runs in a child process of its own under a time limit.

    python scripts/levelset_bench.py [--gaussians 100000 1000000] [--rays 10000 100000] [--voxel-size 0.01] [--reps 11]
                                     [--limit 300] [--out build/levelset_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = (0.1, 0.3, 0.5)


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


def composed(field, o, v, t0, t1, levels):
    """The search of DESIGN.md section 26.1 from query calls (tests/test_levelset_gpu.py holds the bit-exact form)."""
    M = o.shape[0]
    j = torch.arange(64, dtype=torch.float32, device=o.device)
    valid = torch.isfinite(o).all(1) & torch.isfinite(v).all(1) & torch.isfinite(t0) & torch.isfinite(t1) & (t1 > t0)
    tk = t0[:, None] + j[None, :] * ((t1 - t0) / 63.0)[:, None]
    D = field.query((o[:, None, :] + tk[:, :, None] * v[:, None, :]).reshape(-1, 3))["density"].reshape(M, 64)
    t_out = torch.zeros((len(levels), M), dtype=torch.float32, device=o.device)
    hit_out = torch.zeros((len(levels), M), dtype=torch.bool, device=o.device)
    for li, lev in enumerate(levels):
        cross = (D[:, :-1] < lev) & (lev <= D[:, 1:]) & valid[:, None]
        rows = torch.nonzero(cross.any(1))[:, 0]
        if rows.numel() == 0:
            continue
        k = cross[rows].to(torch.int32).argmax(1)
        a, b = tk[rows, k], tk[rows, k + 1]
        u = a[:, None] + j[None, :] * ((b - a) / 63.0)[:, None]
        u[:, 0], u[:, 63] = a, b
        F = field.query((o[rows, None, :] + u[:, :, None] * v[rows, None, :]).reshape(-1, 3))["density"].reshape(-1, 64)
        F[:, 0], F[:, 63] = D[rows, k], D[rows, k + 1]
        js = ((F[:, :-1] < lev) & (lev <= F[:, 1:])).to(torch.int32).argmax(1)
        r = torch.arange(rows.numel(), device=o.device)
        uj, un, Fj, Fn = u[r, js], u[r, js + 1], F[r, js], F[r, js + 1]
        t_out[li, rows] = uj + (un - uj) * ((lev - Fj) / (Fn - Fj))
        hit_out[li, rows] = True
    return t_out, hit_out


def child(args):
    import collab_splats_amd as m
    from collab_splats_amd.synthetic import random_scene
    dev = torch.device("cuda:0")
    n, W, H = args.child, 1920, 1080
    sc = random_scene(n, W, H, seed=42, device="cuda:0")
    gauss = (sc["means"], sc["quats"], torch.exp(sc["log_scales"]), torch.sigmoid(sc["opacity_logits"]))
    with torch.no_grad():
        out = m.rasterization(*gauss, sc["sh"], sc["viewmats"], sc["Ks"], W, H, sh_degree=3, render_mode="RGB+ED",
                              return_depth_normal=True)
    depth, alpha = out[2][0].reshape(-1).contiguous(), out[1][0].reshape(-1).contiguous()
    cand = torch.nonzero((alpha > 0) & torch.isfinite(depth) & (depth > 0))[:, 0]
    del out
    f = m.DensityField(*gauss, args.voxel_size)
    lengths = (f._ranges[:, 1] - f._ranges[:, 0]).float()
    row = {"gaussians": n, "voxel_size": args.voxel_size, "units": f.n_units, "pairs": f.n_pairs,
           "list_mean": float(lengths.mean()), "list_max": int(lengths.max()), "rays": []}
    K = sc["Ks"][0]
    g = torch.Generator(device="cuda").manual_seed(1)
    for n_rays in args.rays:
        pix = cand[torch.randperm(cand.numel(), generator=g, device=dev)[:n_rays]]
        d = depth[pix]
        x = ((pix % W).float() + 0.5 - K[0, 2]) * d / K[0, 0]
        y = ((pix // W).float() + 0.5 - K[1, 2]) * d / K[1, 1]
        P = torch.stack([x, y, d], 1)                                  # (the scene's camera is the world frame)
        t_c = torch.linalg.norm(P, dim=1)
        v = (P / t_c[:, None]).contiguous()
        o = torch.zeros_like(v)
        radius = 8.0 * args.voxel_size
        t0, t1 = torch.clamp(t_c - radius, min=0.0), t_c + radius
        got = f.raycast(o, v, t0, t1, LEVELS)
        ref = composed(f, o, v, t0, t1, LEVELS)
        entry = {"rays": int(pix.numel()), "hits": got["hit"].sum(1).tolist(), "hits_composed": ref[1].sum(1).tolist(),
                 "raycast_s": time_gpu(lambda: f.raycast(o, v, t0, t1, LEVELS), args.reps),
                 "composed_s": time_gpu(lambda: composed(f, o, v, t0, t1, LEVELS), args.reps)}
        entry["composed_over_raycast"] = entry["composed_s"] / entry["raycast_s"]
        row["rays"].append(entry)
    print(json.dumps({"levelset_bench_scene": row}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--rays", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--limit", type=int, default=300, help="seconds per scene")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "levelset_bench.json"))       # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("levelset_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    if args.child is not None:
        return child(args)
    rows = []
    for n in args.gaussians:                                           # one process per scene, each under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--voxel-size", str(args.voxel_size), "--reps",
               str(args.reps), "--rays"] + [str(r) for r in args.rays]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"levelset_bench.py: {n} Gaussians ran past {args.limit} s; nothing more is started")
        if out.returncode != 0:
            sys.stderr.write(out.stderr[-4000:])
            raise SystemExit(f"levelset_bench.py: {n} Gaussians ended with status {out.returncode}; nothing more is started")
        line = [ln for ln in out.stdout.splitlines() if ln.startswith('{"levelset_bench_scene"')][-1]
        rows.append(json.loads(line)["levelset_bench_scene"])
        print(f"{n} Gaussians: {rows[-1]}", flush=True)
    res = {"device": torch.cuda.get_device_name(0), "levels": LEVELS, "scenes": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"levelset_bench": res}))


if __name__ == "__main__":
    main()
