"""The text-query similarity map on the MI355X: the similarity step of ``get_outputs_for_camera`` --
``ops.similarity_map`` (csrc/textquery.hip: folded queries, no decoded tensor) -- against the route the repository offered
before, ``feature_decode`` at ``resize_factor=8.0`` + ``query_similarity`` + the bilinear resize of the heat map, at the
production shape: render 1080 x 1920 x 13 (the [..., 3:16] slice of a 17-channel render), main branch 768 x 64 x 114 (working
map 512 x 912), second branch 384 channels, Q = 5 embeddings (2 positive), both methods.  And ``ops.gaussian_similarity`` at
--rows rows against ``TwoLayerMLP.per_gaussian_forward`` + ``query_similarity``.  Both routes run in one process, alternating,
--rounds windows of --steps calls each between device events after a warm-up of every shape; the median window is reported,
with the peak allocated memory of each route (``torch.cuda.max_memory_allocated`` above what was allocated before the call) and
the largest difference between the two routes' results.  No time is a pass condition.

    python scripts/textquery_bench.py [--steps 20] [--rounds 5] [--rows 1000000] [--out build/textquery_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, L, HD = 1080, 1920, 13, 64
DIMS = {"clip": (768, 64, 114), "dino": (384, 64, 114)}
RESIZE = 8.0
Q, N_POS = 5, 2


def time_window(fn, steps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / steps


def peak_bytes(fn):
    """The most the route holds above what was allocated before it (its result included)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def compare(routes, steps, rounds):
    for fn in routes.values():                                         # warm-up of every shape, both routes
        for _ in range(3):
            fn()
    a, b = routes["fused"](), routes["decoded"]()
    diff = float((a - b).abs().max())
    del a, b
    times = {k: [] for k in routes}
    for _ in range(rounds):                                            # alternating windows
        for k, fn in routes.items():
            times[k].append(time_window(fn, steps))
    return {"fused_s": float(np.median(times["fused"])), "decoded_s": float(np.median(times["decoded"])),
            "fused_windows_s": times["fused"], "decoded_windows_s": times["decoded"],
            "fused_peak_bytes": peak_bytes(routes["fused"]), "decoded_peak_bytes": peak_bytes(routes["decoded"]),
            "max_abs_difference": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "textquery_bench.json"))         # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("textquery_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    import collab_splats_amd as m
    m.load_library()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    render = torch.rand(H, W, 17, generator=g).to(dev)
    feats = render[..., 3:16]
    torch.manual_seed(0)
    mlp = m.TwoLayerMLP(L, HD, DIMS).to(dev)
    with torch.no_grad():                                               # unit scale, as the tests' scenes
        for n, d in DIMS.items():
            mlp.feature_branch_dict[n].weight.copy_(torch.randn(d[0], HD, 1, 1, generator=g) / HD ** 0.5)
            mlp.feature_branch_dict[n].bias.copy_(0.1 * torch.randn(d[0], generator=g))
        mlp.hidden_conv.weight.copy_(torch.randn(HD, L, 1, 1, generator=g) / L ** 0.5)
        mlp.hidden_conv.bias.copy_(0.1 * torch.randn(HD, generator=g))
    emb = F.normalize(torch.randn(Q, DIMS["clip"][0], generator=g), dim=1).to(dev)
    work = (int(DIMS["clip"][1] * RESIZE), int(DIMS["clip"][2] * RESIZE))
    query = m.fold_text_queries(mlp, "clip", emb, N_POS)
    dims8 = {"clip": (DIMS["clip"][0],) + work, "dino": DIMS["dino"]}   # what decode_features(resize_factor=8.0) asks for
    rows = torch.rand(args.rows, L, generator=g).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "rounds": args.rounds,
           "render": [H, W, L], "work": list(work), "queries": Q, "n_positive": N_POS, "rows": args.rows, "cases": {}}
    for method in ("pairwise", "standard"):
        def fused_map():
            return m.similarity_map(feats, query, work, (H, W), method=method)

        def decoded_map():
            main = m.feature_decode(feats, mlp, dims8, work)["clip"]                                 # [768, 512, 912]
            sim = m.query_similarity(main.reshape(main.shape[0], -1).t(), emb, N_POS, method=method)
            return F.interpolate(sim.reshape(1, 1, *work), size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)

        def fused_rows():
            return m.gaussian_similarity(rows, query, method=method)

        def decoded_rows():
            return m.query_similarity(mlp.per_gaussian_forward(rows)["clip"], emb, N_POS, method=method)

        for what, routes in (("map", {"fused": fused_map, "decoded": decoded_map}),
                             ("rows", {"fused": fused_rows, "decoded": decoded_rows})):
            row = compare(routes, args.steps, args.rounds)
            res["cases"][f"{what}.{method}"] = row
            print(json.dumps({"textquery_bench_case": {"what": what, "method": method, **row}}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"textquery_bench": res}))


if __name__ == "__main__":
    main()
