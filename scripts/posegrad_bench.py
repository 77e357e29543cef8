"""The camera pose gradient on the MI355X, on ``synthetic.random_scene`` at 1 M Gaussians and 1080p:

* ``misplat_project_bwd_pose`` (the view-matrix gradient: two launches) next to ``misplat_project_bwd`` (the gradients of means,
  quats and scales) on the same inputs -- they read the same bytes; the ratio of the two times is recorded;
* a forward + backward step of ``rasterization`` (SH degree 3, RGB, antialiased) with ``viewmats.requires_grad`` -- the generic
  staged path -- next to the same step without it -- the fused node.

All routes run in one process, alternating, --rounds windows of --steps steps each between device events after a warm-up of
every route; the median window and the spread (min, max) are reported.  No time is a pass condition.

    python scripts/posegrad_bench.py [--gaussians 1000000] [--steps 20] [--rounds 7] [--out build/posegrad_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_window(fn, steps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / steps


def summary(times):
    return {"median_s": float(np.median(times)), "min_s": float(np.min(times)), "max_s": float(np.max(times)), "windows_s": times}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "posegrad_bench.json"))          # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("posegrad_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    import collab_splats_amd as m
    from collab_splats_amd import _lib, ops
    from collab_splats_amd._lib import ptr, stream_ptr
    from collab_splats_amd.synthetic import random_scene
    lib = m.load_library()
    dev = torch.device("cuda:0")
    N, W, H = args.gaussians, 1920, 1080
    sc = random_scene(N, W, H, seed=42)
    means, quats = sc["means"].to(dev), sc["quats"].to(dev)
    scales, opac = torch.exp(sc["log_scales"]).to(dev), torch.sigmoid(sc["opacity_logits"]).to(dev)
    sh, V, K = sc["sh"].to(dev), sc["viewmats"].to(dev), sc["Ks"].to(dev)

    # ---- the two projection backward entries on the same inputs
    P = _lib.make_params(N, 1, W, H, antialiased=True)
    with torch.no_grad():
        radii = ops.project(means, quats, scales, opac, V, K, P)[0]
    g = torch.Generator().manual_seed(1)
    ups = [(torch.rand(s, generator=g) - 0.5).to(dev) for s in [(1, N, 2), (1, N), (1, N, 3), (1, N), (1, N), (1, N, 2), (1, N, 3)]]
    v_means, v_quats, v_scales = torch.empty_like(means), torch.empty_like(quats), torch.empty_like(scales)
    v_V = torch.empty_like(V)
    work = torch.empty(int(lib.misplat_project_bwd_pose_workspace(C.c_int32(N), C.c_int32(1))), device=dev, dtype=torch.uint8)
    common = [C.byref(P), ptr(means), ptr(quats), ptr(scales), ptr(V), ptr(K), ptr(radii)] + [ptr(t) for t in ups]

    def project_bwd():
        _lib.check(lib.misplat_project_bwd(*common, ptr(v_means), ptr(v_quats), ptr(v_scales), stream_ptr()), "misplat_project_bwd")

    def project_bwd_pose():
        _lib.check(lib.misplat_project_bwd_pose(*common, ptr(work), ptr(v_V), stream_ptr()), "misplat_project_bwd_pose")

    # ---- the whole step, with and without a pose gradient
    leaves = [t.clone().requires_grad_(True) for t in (means, quats, scales, opac, sh)]
    v_render = torch.rand(1, H, W, 3, generator=g).to(dev)

    def step(pose):
        Vl = V.clone().requires_grad_(pose)
        out = m.rasterization(*leaves, Vl, K, W, H, sh_degree=3, render_mode="RGB", rasterize_mode="antialiased")
        grads = torch.autograd.grad([out[0]], leaves + ([Vl] if pose else []), [v_render])
        return grads

    routes = {"project_bwd": project_bwd, "project_bwd_pose": project_bwd_pose,
              "step_fused": lambda: step(False), "step_pose_staged": lambda: step(True)}
    for fn in routes.values():                                          # warm-up of every route
        for _ in range(3):
            fn()
    # the two steps compute the same parameter gradients (different kernels: compared, not bitwise)
    a, b = step(False), step(True)
    diff = {n: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
            for n, x, y in zip(("v_means", "v_quats", "v_scales", "v_opacities", "v_sh"), b, a)}
    tie = V[0, :3, :3] @ b[0].double().sum(0).float()
    diff["translation_identity"] = float((b[5][0, :3, 3] - tie).abs().max() / tie.abs().max())
    times = {k: [] for k in routes}
    for _ in range(args.rounds):                                        # alternating windows
        for k, fn in routes.items():
            times[k].append(time_window(fn, args.steps))
    visible = int(((radii[..., 0] > 0) | (radii[..., 1] > 0)).sum())
    res = {"device": torch.cuda.get_device_name(0), "gaussians": N, "image": [H, W], "visible": visible,
           "steps": args.steps, "rounds": args.rounds, **{k: summary(v) for k, v in times.items()},
           "pose_over_project_bwd": float(np.median(times["project_bwd_pose"]) / np.median(times["project_bwd"])),
           "staged_over_fused_step": float(np.median(times["step_pose_staged"]) / np.median(times["step_fused"])),
           "max_difference": diff}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"posegrad_bench": res}))


if __name__ == "__main__":
    main()
