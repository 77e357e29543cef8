"""Inputs of the depth-cloud tests (numpy only; tests/golden/make_depthcloud_goldens.py builds its scenes from these too)."""
from __future__ import annotations

import math

import numpy as np

F = np.float32

# (rotation angles, translation, fx, fy, W, H): the three poses of tests/golden/make_camera_goldens.py
POSES = [((0.0, 0.0, 0.0), (0.1, -0.2, 0.3), 40.0, 40.0, 16, 12),
         ((0.3, -0.5, 0.2), (1.0, 2.0, -0.5), 100.0, 80.0, 121, 67),
         ((-1.1, 0.7, 2.0), (-3.0, 0.25, 4.0), 300.5, 310.25, 64, 48)]


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(F)


def pose(i):
    """(c2w [3,4] fp32, intrinsics (fx, fy, cx, cy) fp32 with an off-centre principal point, W, H) of pose i."""
    ang, t, fx, fy, W, H = POSES[i]
    c2w = np.concatenate([rot(*ang), np.asarray(t, F)[:, None]], 1).astype(F)
    return c2w, np.array([fx, fy, W / 2 + 1.5, H / 2 - 0.75], F), W, H


def edge_scene(H, W, seed):
    """fp32 [H,W] depth: a tilted plane with a low sinusoid, a box 0.6 nearer, uniform noise of 5e-4 and a disc of zero depth."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = 3.0 + 0.9 * xx / W - 0.6 * yy / H + 0.05 * np.sin(xx / 9.0) * np.cos(yy / 7.0)
    d[H // 5:H // 5 + max(2, H // 3), W // 6:W // 6 + max(2, W // 3)] -= 0.6
    d += rng.uniform(-5e-4, 5e-4, (H, W))
    d[(yy - 0.7 * H) ** 2 + (xx - 0.7 * W) ** 2 < (0.15 * min(H, W)) ** 2] = 0.0
    return d.astype(F)


def spikes(V, H, W, where, base=2.0, far=8.0):
    """fp32 [V,H,W]: a flat depth with single farther pixels at ``where`` = [(v, y, x)].  Exactly those pixels are edges for a
    threshold in (0, 0.5): inv is 0.5 on the flat and 0.125 at a spike, so the Laplacian is >= 1 - 0.5 at a spike (a corner has
    two neighbours inside the image) and negative or zero everywhere else, the border included."""
    d = np.full((V, H, W), base, F)
    for v, y, x in where:
        d[v, y, x] = far
    return d


def maps(V, H, W, seed):
    """Random maps of one batch: depth in [1.5, 4.5] with a few zeros, rgb and normals in [0, 1] (one normal exactly 0.5: a zero
    vector)."""
    rng = np.random.default_rng(seed)
    depth = rng.uniform(1.5, 4.5, (V, H, W)).astype(F)
    depth[rng.random((V, H, W)) < 0.05] = 0.0
    rgb = rng.random((V, H, W, 3)).astype(F)
    normals = rng.random((V, H, W, 3)).astype(F)
    normals[:, 0, 0] = 0.5
    return depth, rgb, normals


def cameras(V):
    """c2w [V,3,4] and intrinsics [V,4] cycling through the three poses (the image size is the caller's)."""
    ps = [pose(i % 3) for i in range(V)]
    return np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])
