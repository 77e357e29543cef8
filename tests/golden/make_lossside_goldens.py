"""Generates tests/golden/lossside_goldens.npz by RUNNING THE REFERENCE's own depth -> normal code
(/root/reference/collab_splats/utils/camera_utils.py, loaded as make_camera_goldens.py loads it) in fp64 on depth maps
WITH HOLES -- exact zeros where a render has alpha == 0 -- at sizes around the backward's 32 x 8 tile.

Container-only tooling: the reference cannot travel, only the vectors are committed.

    python tests/golden/make_lossside_goldens.py

Per case ``c{i}`` (W, H, fx, fy in CASES):
  inputs     d1, d2 [H,W], nrm [H,W,3] (fp32), rays [H,W,2] (the reference's fp32 ray table, read off a run on unit depth)
  upstreams  v_n2 [2,H,W,3], v_err [2,H,W] (fp32); at every interior centre whose fp64 normal is exactly zero both are
             multiplied by 1e-12, so that the 1e12 of F.normalize's eps leaves gradients of O(1) there
  fp64       normals2, err, g_d1, g_d2, g_nrm: the reference on the same fp32 values upcast (its ray table stays fp32)
  e32        [5] for (normals2, err, g_d1, g_d2, g_nrm): max-abs error of the reference's own fp32 run / fp64 tensor max
Per fused-node case ``f{j}`` (the get_outputs node: the stencil composed with oracle/camera_oracle.outputs_post in ONE
fp64 autograd graph): inputs render [H,W,4], alpha [H,W] (0 exactly where a depth is 0), bg [3]; upstreams u_rgb, u_depth,
u_median, u_normals, u_err, u_depth_im; fp64 outputs o_* and gradients g_render, g_alpha, g_d1, g_d2, g_nrm; e32o [6], e32g [5].
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_camera_goldens import DuckCamera, load_reference  # noqa: E402
from oracle import camera_oracle as co  # noqa: E402

OUT = os.path.join(HERE, "lossside_goldens.npz")
CASES = [(32, 8, 40.0, 37.0), (33, 9, 40.0, 37.0), (65, 17, 100.0, 80.0), (9, 7, 300.5, 310.25),
         (3, 3, 5.0, 5.0), (2, 5, 5.0, 5.0), (5, 2, 5.0, 5.0), (1, 1, 5.0, 5.0)]
FUSED = [1, 2]                                       # 33 x 9 and 65 x 17
BG = [0.2, 0.5, 0.9]


def punch(d1, d2, W, H):
    """Exact zeros: a 3 x 3 block (its middle is a centre inside a hole), the whole row next to the bottom border, a
    corner, an isolated pixel; in d1 the two row neighbours of (W-4, 2), in d2 the two column neighbours of (W-2, 3) --
    the other pair of neighbours stays filled.  Larger images get a second block across the tile edges x = 32, y = 8."""
    for d in (d1, d2):
        d[1:4, 1:4] = 0.0
        d[H - 2, :] = 0.0
        d[0, 0] = 0.0
        d[1, W - 2] = 0.0
        if W >= 40 and H >= 12:
            d[6:11, 30:35] = 0.0
    d1[1, W - 4] = d1[3, W - 4] = 0.0
    d2[3, W - 3] = d2[3, W - 1] = 0.0


def make_inputs(W, H, g):
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    base = 3.0 + 0.02 * xx - 0.013 * yy                                   # tilted plane (make_camera_goldens.py)
    d1 = base + 0.05 * torch.rand(H, W, generator=g)
    d2 = base + 0.3 * torch.sin(xx / 5.0) * torch.cos(yy / 7.0)
    if W >= 9 and H >= 7:
        punch(d1, d2, W, H)
    nrm = torch.nn.functional.normalize(torch.randn(1, H, W, 3, generator=g), dim=-1) * torch.rand(1, H, W, 1, generator=g)
    return d1.reshape(1, H, W, 1), d2.reshape(1, H, W, 1), nrm


def stencil(ref, cam, d1, d2, nrm):
    n2 = ref.depth_double_to_normal(cam, d1, d2)                           # [2,H,W,3]
    err = 1 - (nrm.unsqueeze(0) * n2).sum(dim=-1).squeeze(0)               # rade_gs_model.py:212-214
    return n2, err


def rel(a32, a64):
    s = float(a64.abs().max()) if a64.numel() else 0.0
    return 0.0 if s == 0.0 else float((a32.double() - a64).abs().max()) / s


def main():
    ref = load_reference()
    g = torch.Generator().manual_seed(20)
    out = {"cases": np.array(CASES), "fused": np.array(FUSED), "bg": np.array(BG)}
    for i, (W, H, fx, fy) in enumerate(CASES):
        c2w = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1)
        K = torch.tensor([[fx, 0, W / 2], [0, fy, H / 2], [0, 0, 1]])
        cam = DuckCamera(c2w, K, W, H)
        cc = ref.convert_to_colmap_camera(cam)
        out[f"c{i}_fxfy"] = np.array([W / (2 * np.tan(cc.fovx / 2)), H / (2 * np.tan(cc.fovy / 2))])
        ones = torch.ones(1, H, W, 1, dtype=torch.float64)
        p1, _ = ref._depths_double_to_points(cam, ones, ones)              # unit depth: the points ARE the fp32 ray table
        assert bool((p1[2] == 1).all())
        out[f"c{i}_rays"] = p1[:2].permute(1, 2, 0).float().numpy()
        assert np.array_equal(out[f"c{i}_rays"].astype(np.float64), p1[:2].permute(1, 2, 0).numpy())
        d1, d2, nrm = make_inputs(W, H, g)
        v_n2 = torch.randn(2, H, W, 3, generator=g)
        v_err = torch.randn(2, H, W, generator=g)
        with torch.no_grad():
            n2_plain, _ = stencil(ref, cam, d1.double(), d2.double(), nrm.double())
        dead = torch.zeros(2, H, W, dtype=torch.bool)
        dead[:, 1:-1, 1:-1] = (n2_plain == 0).all(-1)[:, 1:-1, 1:-1]
        v_n2[dead] *= 1e-12
        v_err[dead] *= 1e-12
        res = {}
        for dt in (torch.float64, torch.float32):
            leaves = [t.clone().to(dt).requires_grad_(True) for t in (d1, d2, nrm)]
            n2, err = stencil(ref, cam, *leaves)
            torch.autograd.backward([n2, err], [v_n2.to(dt), v_err.to(dt)])
            res[dt] = [n2.detach(), err.detach(), leaves[0].grad[0, ..., 0], leaves[1].grad[0, ..., 0], leaves[2].grad[0]]
        names = ("normals2", "err", "g_d1", "g_d2", "g_nrm")
        for name, t in zip(names, res[torch.float64]):
            assert bool(torch.isfinite(t).all()), (i, name)
            out[f"c{i}_{name}"] = t.numpy()
        out[f"c{i}_e32"] = np.array([rel(a, b) for a, b in zip(res[torch.float32], res[torch.float64])])
        out[f"c{i}_d1"], out[f"c{i}_d2"] = d1.numpy()[0, ..., 0], d2.numpy()[0, ..., 0]
        out[f"c{i}_nrm"], out[f"c{i}_v_n2"], out[f"c{i}_v_err"] = nrm.numpy()[0], v_n2.numpy(), v_err.numpy()
        print(f"case {i} {W}x{H}: {int(dead.sum())} zero-normal centres, e32 =", out[f"c{i}_e32"])

        if i not in FUSED:
            continue
        j = FUSED.index(i)
        hole = (d1 == 0) | (d2 == 0)
        alpha = torch.where(hole, torch.zeros(()), 0.3 + 0.7 * torch.rand(1, H, W, 1, generator=g))
        render = torch.rand(1, H, W, 4, generator=g) * 1.4 - 0.2
        shapes = [(1, H, W, 3), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3), (2, H, W), (1, H, W, 1)]
        ups = [torch.randn(s, generator=g) for s in shapes]
        ups[4][dead] *= 1e-12
        res = {}
        for dt in (torch.float64, torch.float32):
            leaves = [t.clone().to(dt).requires_grad_(True) for t in (render, alpha, d1, d2, nrm)]
            _, err = stencil(ref, cam, leaves[2], leaves[3], leaves[4])
            rgb, depth, median, normals, depth_im = co.outputs_post(*leaves, torch.tensor(BG, dtype=dt))
            outs = [rgb, depth, median, normals, err, depth_im]
            torch.autograd.backward(outs, [u.to(dt) for u in ups])
            res[dt] = ([o.detach() for o in outs], [t.grad for t in leaves])
        onames = ("rgb", "depth", "median", "normals", "err", "depth_im")
        gnames = ("render", "alpha", "d1", "d2", "nrm")
        for name, t, u in zip(onames, res[torch.float64][0], ups):
            out[f"f{j}_o_{name}"] = t.numpy()[0] if name != "err" else t.numpy()
            out[f"f{j}_u_{name}"] = u.numpy()[0] if name != "err" else u.numpy()
        for name, t in zip(gnames, res[torch.float64][1]):
            assert bool(torch.isfinite(t).all()), (j, name)
            out[f"f{j}_g_{name}"] = t.numpy()[0]
        out[f"f{j}_render"], out[f"f{j}_alpha"] = render.numpy()[0], alpha.numpy()[0, ..., 0]
        out[f"f{j}_e32o"] = np.array([rel(a, b) for a, b in zip(res[torch.float32][0], res[torch.float64][0])])
        out[f"f{j}_e32g"] = np.array([rel(a, b) for a, b in zip(res[torch.float32][1], res[torch.float64][1])])
        print(f"fused {j}: e32o =", out[f"f{j}_e32o"], "e32g =", out[f"f{j}_e32g"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(out), "arrays", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
