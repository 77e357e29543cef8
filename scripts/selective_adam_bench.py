"""The row-selective Adam on the MI355X: ``selective_adam_step_all`` (csrc/optim.hip
``misplat_adam_step_rows`` behind the four launches that list the flagged rows) against ``FusedAdam.step_all`` on the SAME
tensors -- the six Gaussian groups of widths 3, 3, 45, 1, 3 and 4 (59 floats a row) at 1 M and 5 M rows -- at mask densities of
100 %, 50 %, 11 % and 2 % (the last two: the touched fractions csrc/optim.hip documents for the 1 M and the 5 M scene), each
with randomly scattered rows and with one contiguous block of rows.

Protocol (metrics_bench.py's): the routes run in one process in alternating windows of --steps calls between device events,
after a warm-up of every route; the median of --rounds windows is reported.  Per point: ms of the selective step (the list
build included), of the list build alone and of the dense step in the same windows, and the effective rate 28 B x elements
stepped / time (dense: all N x 59 elements).  Per size and layout: the density at which the selective step stops being faster
than the dense one, interpolated linearly between the two measured densities around the crossing.  Before the timing, once per
size: the rows an 11 % scattered mask selects equal the dense result bit for bit and the other rows are untouched (the 64-bit
row offsets at workload scale).  No time is a pass condition.

    python scripts/selective_adam_bench.py [--steps 10] [--rounds 7] [--sizes 1000000 5000000] [--out build/selective_adam_bench.json]
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

NAMES = ("means", "features_dc", "features_rest", "opacities", "scales", "quats")
ROW_SHAPES = ((3,), (3,), (15, 3), (1,), (3,), (4,))
LRS = (1.6e-4, 0.0025, 0.0025 / 20, 0.05, 0.005, 0.001)
W = 59
BYTES_PER_ELEMENT = 28              # 16 B read (p, g, m, v) + 12 B written
DENSITIES = (1.0, 0.5, 0.11, 0.02)


def time_window(fn, steps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / steps


def alternate(routes, steps, rounds):
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            times[k].append(time_window(fn, steps))
    return {k: float(np.median(v)) for k, v in times.items()}


def make_optimizers(n, dev, cls, like=None):
    """{name: optimizer over one group} with the state of step 999 injected; ``like``: copy another set's tensors (and share its
    gradients)."""
    g = torch.Generator(device=dev).manual_seed(n)
    out = {}
    for name, shape, lr in zip(NAMES, ROW_SHAPES, LRS):
        if like is None:
            p = torch.nn.Parameter(torch.randn((n,) + shape, device=dev, generator=g) * (16 * lr))
            p.grad = torch.randn((n,) + shape, device=dev, generator=g) * 1e-3
            s = torch.rand((n,) + shape, device=dev, generator=g) * 1e-3
            m, v = s * (2 * torch.rand((n,) + shape, device=dev, generator=g) - 1), s * s
        else:
            q = like[name].param_groups[0]["params"][0]
            p = torch.nn.Parameter(q.detach().clone())
            p.grad = q.grad
            m, v = like[name].state[q]["exp_avg"].clone(), like[name].state[q]["exp_avg_sq"].clone()
        out[name] = cls([p], lr=lr, eps=1e-15)
        out[name].state[p] = {"step": torch.tensor(999.0), "exp_avg": m, "exp_avg_sq": v}
    return out


def tensors_of(opts):
    for name in NAMES:
        p = opts[name].param_groups[0]["params"][0]
        yield name + ".p", p.detach()
        yield name + ".exp_avg", opts[name].state[p]["exp_avg"]
        yield name + ".exp_avg_sq", opts[name].state[p]["exp_avg_sq"]


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def make_mask(n, density, layout, dev):
    if layout == "block":
        k = int(round(density * n))
        start = (n - k) // 2
        mask = torch.zeros(n, dtype=torch.bool, device=dev)
        mask[start:start + k] = True
        return mask
    if density >= 1.0:
        return torch.ones(n, dtype=torch.bool, device=dev)
    return torch.rand(n, device=dev, generator=torch.Generator(device=dev).manual_seed(int(1000 * density) + n)) < density


def check_bits(n, dev, m):
    """Selected rows = the dense result, the others untouched, bit for bit, at this size (an 11 % scattered mask)."""
    sel = make_optimizers(n, dev, m.SelectiveAdam)
    before = {k: t.clone() for k, t in tensors_of(sel)}
    den = make_optimizers(n, dev, m.FusedAdam, like=sel)
    mask = make_mask(n, 0.11, "scattered", dev)
    m.fused_adam_step_all(den)
    m.selective_adam_step_all(sel, mask)
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(tensors_of(sel), tensors_of(den)):
        assert same_bits(a[mask], b[mask]), f"n = {n}: selected rows of {k} differ from FusedAdam's"
        assert same_bits(a[~mask], before[k][~mask]), f"n = {n}: unselected rows of {k} moved"
        assert not same_bits(a[mask], before[k][mask]), f"n = {n}: {k} was not stepped"
    return int(mask.sum())


def break_even(points):
    """The density at which selective - dense changes sign, between the two measured densities around it (None: selective
    is faster at every measured density, 0.0: at none)."""
    pts = sorted((p["density"], p["selective_s"] - p["dense_s"]) for p in points)
    if pts[0][1] >= 0:
        return 0.0
    for (d0, y0), (d1, y1) in zip(pts, pts[1:]):
        if y0 < 0 <= y1:
            return float(d0 + (d1 - d0) * (-y0) / (y1 - y0))
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 5_000_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "selective_adam_bench.json"))     # build/: git-ignored
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("selective_adam_bench.py measures the MI355X: no GPU here (figures are 'not measured')")
    import collab_splats_amd as m
    from collab_splats_amd import optim
    dev = torch.device("cuda:0")
    cases = []
    for n in args.sizes:
        checked_rows = check_bits(n, dev, m)
        torch.cuda.empty_cache()
        opts = make_optimizers(n, dev, m.SelectiveAdam)
        points = []
        for layout in ("scattered", "block"):
            for density in DENSITIES:
                mask = make_mask(n, density, layout, dev)
                rows = int(mask.sum())
                routes = {"selective": lambda: m.selective_adam_step_all(opts, mask), "list": lambda: optim._row_list(mask),
                          "dense": lambda: m.fused_adam_step_all(opts)}
                for fn in routes.values():
                    for _ in range(3):
                        fn()
                t = alternate(routes, args.steps, args.rounds)
                point = {"n": n, "layout": layout, "density": density, "rows": rows, "selective_s": t["selective"],
                         "list_s": t["list"], "dense_s": t["dense"],
                         "selective_GBps": BYTES_PER_ELEMENT * rows * W / t["selective"] / 1e9,
                         "dense_GBps": BYTES_PER_ELEMENT * n * W / t["dense"] / 1e9,
                         "dense_over_selective": t["dense"] / t["selective"]}
                points.append(point)
                print(json.dumps({"selective_adam_bench_point": point}), flush=True)
        case = {"n": n, "bits_checked_rows": checked_rows, "steps": args.steps, "rounds": args.rounds, "points": points,
                "break_even_density": {layout: break_even([p for p in points if p["layout"] == layout])
                                       for layout in ("scattered", "block")}}
        cases.append(case)
        print(json.dumps({"selective_adam_bench_case": {k: v for k, v in case.items() if k != "points"}}), flush=True)
        del opts
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "cases": cases}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"selective_adam_bench": "written", "out": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
