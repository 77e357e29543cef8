"""kNN mapping of Gaussian normals and features onto mesh vertices on the MI355X: times
RadegsModel.mesh_attributes (one kNN, [normals | distill_features] mapped in one call) with device events, for
tsdf_scenes.sphere_gaussians at 1 M and 5 M Gaussians onto TSDF meshes of the same sphere at voxel_size 0.01 and 0.004;
the CPU baseline is the reference's algorithm (scipy cKDTree query + np.add.at, fp64, one thread), restated, if scipy
imports.

    python scripts/meshmap_bench.py [--gaussians 1000000 5000000] [--reps 3] [--out build/meshmap_bench.json]

Per-kernel times: run it under `rocprofv3 --kernel-trace --stats` (e.g. with --gaussians 1000000 --no-cpu).
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

LATENT = 13


def sphere_mesh(vs, dev, n_views=100, W=320, H=240):
    """TSDF mesh of the sphere of tsdf_scenes (same centre and radius as sphere_gaussians), on the device."""
    import tsdf_scenes as S
    from collab_splats_amd import TSDFVolume
    d, vm, K, rgb = S.sphere_views(n_views, W, H)
    vol = TSDFVolume(vs, 3 * vs if vs > 0.005 else 0.02, 3.0, device=dev)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    for b in range(0, n_views, 32):
        vol.integrate(t(d[b:b + 32]), t(vm[b:b + 32]), t(K[b:b + 32]), t(rgb[b:b + 32]))
    return vol.extract_mesh()[0]


def features_model(n, dev):
    import tsdf_scenes as S
    from collab_splats_amd import radegs
    base = S.sphere_gaussians(n)
    g = torch.Generator().manual_seed(1)
    p = base.gauss_params
    m = radegs.RadegsFeaturesModel(radegs.RadegsFeaturesModelConfig(features_latent_dim=LATENT), p["means"].data,
                                   p["scales"].data, p["quats"].data, p["opacities"].data, p["features_dc"].data,
                                   p["features_rest"].data, torch.randn(n, LATENT, generator=g))
    return m.to(dev)


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


def bench_gpu(model, V, reps):
    from collab_splats_amd.meshmap import _knn
    n = model.means.shape[0]
    t_all, spread = time_gpu(lambda: model.mesh_attributes(V), reps)
    means = model.means.detach()
    t_knn, _ = time_gpu(lambda: _knn(V, means, 5, 0.03), reps)
    _, d, valid = _knn(V, means, 5, 0.03)
    return {"gaussians": n, "vertices": int(V.shape[0]), "channels": 3 + LATENT, "mesh_attributes_s": t_all,
            "mesh_attributes_spread_s": spread, "knn_s": t_knn, "valid_fraction": float(valid.float().mean()),
            "mean_kth_distance": float(d[valid][:, -1].mean())}


def bench_cpu(model, V):
    """The reference's two host maps (features2vertex then normals2vertex), each with its own cKDTree and query."""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return {"note": "scipy not importable: not measured"}
    P = model.means.detach().double().cpu().numpy()
    Vh = V.double().cpu().numpy()
    maps = {"features": model.distill_features.detach().double().cpu().numpy(),
            "normals": model.normals.detach().double().cpu().numpy()}
    out = {}
    for name, F in maps.items():
        t0 = time.perf_counter()
        d, idx = cKDTree(Vh).query(P, k=5)
        keep = d[:, 0] <= 0.03
        d, idx, Fk = d[keep], idx[keep], F[keep]
        sigma = d.mean()
        w = np.exp(-d ** 2 / (2 * sigma ** 2))
        w /= w.sum(1, keepdims=True)
        num = np.zeros((len(Vh), F.shape[1]))
        den = np.zeros(len(Vh))
        for j in range(5):
            np.add.at(num, idx[:, j], w[:, j:j + 1] * Fk)
            np.add.at(den, idx[:, j], w[:, j])
        res = np.where(den[:, None] > 0, num / np.maximum(den, 1e-300)[:, None], 0)
        if name == "normals":
            res = res / (np.linalg.norm(res, axis=1, keepdims=True) + 1e-8)
        out[name + "_s"] = time.perf_counter() - t0
    out["total_s"] = out["features_s"] + out["normals_s"]
    out["note"] = "scipy cKDTree + np.add.at, fp64, one thread, per map its own tree (the reference's algorithm)"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, nargs="+", default=[1_000_000, 5_000_000])
    ap.add_argument("--voxel-sizes", type=float, nargs="+", default=[0.01, 0.004])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "meshmap_bench.json"))       # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshmap_bench.py measures the MI355X: no GPU here (CPU figures are 'not measured')")
    import collab_splats_amd
    collab_splats_amd.load_library()
    dev = torch.device("cuda:0")
    meshes = {vs: sphere_mesh(vs, dev) for vs in args.voxel_sizes}
    res = {"device": torch.cuda.get_device_name(0), "gpu": [], "cpu": []}
    for n in args.gaussians:
        model = features_model(n, dev)
        for vs, V in meshes.items():
            r = bench_gpu(model, V, args.reps)
            r["voxel_size"] = vs
            res["gpu"].append(r)
            print(f"mesh_attributes: {n} Gaussians onto {r['vertices']} vertices (voxel {vs}), D = 3 + {LATENT}: "
                  f"{r['mesh_attributes_s'] * 1e3:.2f} ms (kNN alone {r['knn_s'] * 1e3:.2f} ms, "
                  f"{100 * r['valid_fraction']:.1f} % valid)", flush=True)
            if not args.no_cpu and n <= 1_000_000 and vs == min(args.voxel_sizes):
                c = bench_cpu(model, V)
                c.update(gaussians=n, vertices=r["vertices"], voxel_size=vs)
                res["cpu"].append(c)
                print(f"CPU baseline: {c}", flush=True)
        del model
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"meshmap_bench": {f"mesh_attributes_ms_{r['gaussians']}_{r['vertices']}": r["mesh_attributes_s"] * 1e3
                                        for r in res["gpu"]}}))


if __name__ == "__main__":
    main()
