"""Depth-map point clouds on the MI355X: times, with device events (median of --reps after a warm-up),
each stage of ``depth_normal_cloud`` (depth_edges, the candidate mask + sample_pixels, backproject) and the whole call on
--views maps of --width x --height in batches of --batch, ``RadegsModel.depth_normal_points`` end to end (rendering included)
on the tsdf_scenes sphere, and ``gaussian_mask_filter`` at --gaussians x --filter-views.  total_points = 2 M / 300 x views, edge
filter at the reference's 0.004 / 10.  The CPU baseline is the reference's path in torch on one thread, frame by frame
(conv2d, 10 dilations, nonzero, randperm standing in for the hash, the back-projection) on --cpu-frames frames, and the numpy
restatement of the mask filter on --cpu-filter-views views; both are reported per frame / per view.

    python scripts/depthcloud_bench.py [--views 32] [--width 1920] [--height 1080] [--batch 4] [--reps 5] [--no-cpu] [--no-model]
                                       [--out build/depthcloud_bench.json]

Per-kernel times: run it under `rocprofv3 --kernel-trace --stats` (with --no-cpu --no-model --reps 1).
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


def cpu_frame(depth, rgb, normals, c2w, intr, samples, thr, dil):
    """One frame of mesh.py:904-954 in torch on the host: the edge filter, nonzero, randperm, the back-projection."""
    import torch.nn.functional as F
    H, W = depth.shape
    lap_k = torch.tensor([[0.0, 1.0, 0.0], [1.0, -4.0, 1.0], [0.0, 1.0, 0.0]])[None, None]
    lap = F.conv2d((1.0 / (depth + 1e-6))[None, None], lap_k, padding=1)
    e = (lap > thr).float()
    for _ in range(dil):
        e = F.conv2d(e, torch.ones(1, 1, 3, 3), padding=1)
    valid = (~(e[0, 0] > 0)) & (depth > 0)
    idx = torch.nonzero(valid.ravel())[:, 0]
    if samples < len(idx):
        idx = idx[torch.randperm(len(idx))[:samples]]
    R = c2w[:, :3] * torch.tensor([1.0, -1.0, -1.0])
    d = depth.ravel()[idx]
    x = ((idx % W).float() + 0.5 - intr[2]) * d / intr[0]
    y = ((idx // W).float() + 0.5 - intr[3]) * d / intr[1]
    pts = torch.stack([x, y, d], 1) @ R.T + c2w[:, 3]
    n = 2 * normals.reshape(-1, 3)[idx] - 1
    n = torch.nn.functional.normalize(n * torch.tensor([1.0, -1.0, -1.0]), dim=1) @ R.T
    return pts, n, rgb.reshape(-1, 3)[idx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--filter-views", type=int, default=300)
    ap.add_argument("--model-gaussians", type=int, default=200_000)
    ap.add_argument("--cpu-frames", type=int, default=2)
    ap.add_argument("--cpu-filter-views", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "depthcloud_bench.json"))     # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depthcloud_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    torch.set_num_threads(1)
    import collab_splats_amd as m
    import depthcloud_restatement as R
    import depthcloud_scenes as Q
    import tsdf_scenes as S
    m.load_library()
    dev = torch.device("cuda:0")
    V, W, H, B = args.views, args.width, args.height, args.batch
    total = 2_000_000 * V // 300
    spf = (total + V) // V
    thr, dil = 0.004, 10
    res = {"device": torch.cuda.get_device_name(0), "views": V, "width": W, "height": H, "batch": B, "samples_per_frame": spf,
           "edge_threshold": thr, "edge_dilation": dil}

    # ---- the stages, on B maps at a time (what depth_normal_points hands over), and all V at once
    base = torch.from_numpy(Q.edge_scene(H, W, seed=1)).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    for n_maps in sorted({B, V}):
        depth = (base[None] + 0.01 * torch.arange(n_maps, device=dev)[:, None, None]) * (base[None] > 0)
        rgb = torch.rand((n_maps, H, W, 3), device=dev, generator=g)
        nrm = torch.rand((n_maps, H, W, 3), device=dev, generator=g)
        c2w_h, intr_h = Q.cameras(n_maps)
        intr_h = intr_h.copy()
        intr_h[:, :2], intr_h[:, 2], intr_h[:, 3] = 0.9 * W, W / 2.0, H / 2.0
        c2w, intr = torch.from_numpy(c2w_h).to(dev), torch.from_numpy(intr_h).to(dev)
        edges = m.depth_edges(depth, thr, dil)
        cand = (depth > 0) & ~edges
        f, p, counts = m.sample_pixels(cand, spf, seed=0)
        row = {"maps": n_maps, "edge_fraction": float(edges.float().mean()), "candidates_per_frame": int(cand[0].sum()),
               "points": int(f.shape[0]),
               "depth_edges_s": time_gpu(lambda: m.depth_edges(depth, thr, dil), args.reps),
               "sample_pixels_s": time_gpu(lambda: m.sample_pixels(cand, spf, seed=0), args.reps),
               "backproject_s": time_gpu(lambda: m.backproject(depth, rgb, nrm, c2w, intr, f, p), args.reps),
               "depth_normal_cloud_s": time_gpu(lambda: m.depth_normal_cloud(depth, rgb, nrm, c2w, intr, spf, filter_edges=True,
                                                                             edge_threshold=thr, edge_dilation=dil), args.reps),
               "depth_normal_cloud_no_edges_s": time_gpu(lambda: m.depth_normal_cloud(depth, rgb, nrm, c2w, intr, spf), args.reps)}
        # the least HBM traffic of the edge pass: 4 B read per pixel, 1 B written (the bool image)
        row["depth_edges_bytes"] = 5 * n_maps * H * W
        res.setdefault("stages", []).append(row)
        print(f"stages {row}", flush=True)
        if not args.no_cpu and n_maps == B:
            k = min(args.cpu_frames, n_maps)
            host = [x.cpu() for x in (depth[:k], rgb[:k], nrm[:k], c2w[:k], intr[:k])]
            t0 = time.perf_counter()
            for v in range(k):
                cpu_frame(host[0][v], host[1][v], host[2][v], host[3][v], host[4][v], spf, thr, dil)
            res["cpu_frame_s"] = (time.perf_counter() - t0) / k
            res["cpu_note"] = f"torch on one thread, per frame, mean of {k} frames"
            print(f"cpu per frame {res['cpu_frame_s']:.3f} s", flush=True)
        del depth, rgb, nrm, edges, cand

    # ---- the model call, rendering included
    if not args.no_model:
        model = S.sphere_gaussians(args.model_gaussians).to(dev)
        model.eval()
        _, vms, _, _ = S.sphere_views(V, 8, 8)
        K = S.intrinsics(W, H, 60.0)
        cams = [S.pinhole_camera(M, K, W, H) for M in vms]
        kw = dict(total_points=total, filter_edges=True, edge_threshold=thr, edge_dilation=dil, batch_size=B)
        out = model.depth_normal_points(cams, **kw)
        res["model"] = {"gaussians": args.model_gaussians, "points": int(out["points"].shape[0]),
                        "depth_normal_points_s": time_gpu(lambda: model.depth_normal_points(cams, **kw), max(1, args.reps // 2)),
                        "render_views_only_s": time_gpu(lambda: [model.render_views(cams[b:b + B], batch_size=B) for b in range(0, V, B)],
                                                        max(1, args.reps // 2))}
        print(f"model {res['model']}", flush=True)
        del model, out

    # ---- the Gaussian mask filter
    N, FV = args.gaussians, args.filter_views
    c2w_h, intr_h = Q.cameras(FV)
    intr_h = intr_h.copy()
    intr_h[:, :2], intr_h[:, 2], intr_h[:, 3] = 0.9 * W, W / 2.0, H / 2.0
    rng = np.random.default_rng(0)
    P = (rng.uniform(-4, 4, (N, 3))).astype(np.float32)
    masks = (torch.rand((FV, H, W), device=dev, generator=g) < 0.98)
    p_d, c2w, intr = torch.from_numpy(P).to(dev), torch.from_numpy(c2w_h).to(dev), torch.from_numpy(intr_h).to(dev)
    keep = m.gaussian_mask_filter(p_d, c2w, intr, masks)
    row = {"gaussians": N, "views": FV, "kept": int(keep.sum()),
           "gaussian_mask_filter_s": time_gpu(lambda: m.gaussian_mask_filter(p_d, c2w, intr, masks), args.reps)}
    if not args.no_cpu:
        k = min(args.cpu_filter_views, FV)
        mh = masks[:k].cpu().numpy()
        t0 = time.perf_counter()
        R.gaussian_mask_filter(P, c2w_h[:k], intr_h[:k], mh)
        row["cpu_per_view_s"] = (time.perf_counter() - t0) / k
        row["cpu_note"] = f"numpy restatement (vectorised over the Gaussians), one thread, per view, mean of {k} views"
    res["gaussian_filter"] = row
    print(f"gaussian_filter {row}", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"depthcloud_bench": res}))


if __name__ == "__main__":
    main()
