"""Scenes for the point-cloud TSDF tests (tests/test_pointtsdf_host.py, tests/test_pointtsdf_gpu.py): analytic scans as
(points, origin, colours) per view, ray bundles that meet the walk's edge cases, and an fp64 segment-against-cube test that
shares nothing with the restatement."""
from __future__ import annotations

import numpy as np

import tsdf_scenes as S

F = np.float32


def opengl_c2w(M):
    """nerfstudio's [3,4] OpenGL camera-to-world of an OpenCV world -> camera matrix."""
    return (np.linalg.inv(np.asarray(M, np.float64)) @ np.diag([1.0, -1.0, -1.0, 1.0]))[:3, :4].astype(np.float32)


def sphere_scan(n=8, W=48, H=36, centre=(0.1, -0.05, 0.2), radius=0.5, dist=1.6, shift=(0.0, 0.0, 0.0)):
    """n views of a sphere: dict(depths [n,H,W,1], c2w [n,3,4], intr [n,4], rgbs [n,H,W,3], views: [(points, origin, colours)])
    with the points lifted analytically (origin + ray * depth in float64, then float32).  ``shift``: the views' points and
    origins and ``centre`` translated by it, in float64 before the cast (the maps and the poses stay where they are)."""
    d, vms, Ks, rgb = S.sphere_views(n, W, H, centre=centre, radius=radius, dist=dist)
    shift = np.asarray(shift, np.float64)
    views = []
    for k in range(n):
        o, dirs = S._rays(vms[k].astype(np.float64), Ks[k].astype(np.float64), W, H)
        o = o + shift
        dep = d[k, ..., 0].astype(np.float64)
        hit = dep > 0
        views.append(((o + dirs[hit] * dep[hit][:, None]).astype(np.float32), o.astype(np.float32), rgb[k][hit]))
    intr = np.stack([Ks[:, 0, 0], Ks[:, 1, 1], Ks[:, 0, 2], Ks[:, 1, 2]], 1).astype(np.float32)
    return dict(depths=d, c2w=np.stack([opengl_c2w(M) for M in vms]), intr=intr, rgbs=rgb, views=views,
                centre=np.asarray(centre) + shift, radius=radius, vms=vms, Ks=Ks)


def clump(scan, view=0, at=0.2, n=20, side=0.05, seed=3):
    """A floater: n points in a small square patch across view ``view``'s line of sight to the sphere's centre, ``at`` of the
    way along it, scanned from an origin off to the side.  The views of ``scan`` see through it onto the sphere."""
    rng = np.random.default_rng(seed)
    eye = scan["views"][view][1].astype(np.float64)
    c = eye + at * (scan["centre"] - eye)
    z = (scan["centre"] - eye) / np.linalg.norm(scan["centre"] - eye)
    x = np.cross(z, (0.3, 0.5, 0.8)); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    uv = rng.uniform(-side / 2, side / 2, (n, 2))
    pts = c + uv[:, :1] * x + uv[:, 1:] * y
    origin = c - 0.5 * z + 0.1 * x
    return pts.astype(np.float32), origin.astype(np.float32), np.tile(F([1.0, 0.0, 0.0]), (n, 1)), c


def column_rays(vs, repeat, nx=6, ny=6, length=12, at=(3, -2, 5)):
    """Parallel rays down -z through the centres of an nx x ny patch of voxel columns, each ``repeat`` times: every voxel they
    pass takes exactly ``repeat`` updates.  (points, origins per point)."""
    gx, gy = np.meshgrid(np.arange(nx) + at[0], np.arange(ny) + at[1])
    xy = (np.stack([gx.ravel(), gy.ravel()], 1) + 0.5) * vs
    p = np.concatenate([xy, np.full((len(xy), 1), (at[2] + 0.5) * vs)], 1)
    o = p + np.array([0.0, 0.0, length * vs])
    return np.repeat(p, repeat, 0).astype(np.float32), np.repeat(o, repeat, 0).astype(np.float32)


def fan(vs, n, seed=7):
    """n rays from one origin (voxel (2, 4, 7) of unit (0, 0, 0)) into one small patch 30 voxels away, with colours: every ray
    passes the origin's voxel, so that voxel counts exactly n and its unit's list holds n rays.  (points, origin [3], colours)."""
    rng = np.random.default_rng(seed)
    o = (np.array([2.3, 4.6, 7.2]) * vs).astype(np.float32)
    p = (o + np.array([30.0, 22.0, 17.0]) * vs + rng.uniform(-2, 2, (n, 3)) * vs).astype(np.float32)
    return p, o, rng.random((n, 3)).astype(np.float32)


def edge_rays(vs, n=320, reach=24.0, offset=0.0, seed=0):
    """(points, origins) [n,3] float32: random rays and the walk's edge cases, in eighths -- along each axis (both senses), an
    origin on a voxel face, on a voxel corner, on a unit corner, a point on a voxel corner, exact diagonals (ties between
    axes) -- all shifted by ``offset`` voxels."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-20, 20, (n, 3))
    p = o + rng.uniform(-reach, reach, (n, 3))
    k = n // 8
    ax = rng.integers(0, 3, k)
    for j in range(k):                                                          # axis-parallel
        keep = p[j, ax[j]]
        p[j] = o[j]
        p[j, ax[j]] = keep
    o[k:2 * k, 0] = np.round(o[k:2 * k, 0])                                     # on a voxel face
    o[2 * k:3 * k] = np.round(o[2 * k:3 * k])                                   # on a voxel corner
    o[3 * k:4 * k] = np.round(o[3 * k:4 * k] / 16) * 16                         # on a unit corner
    p[4 * k:5 * k] = np.round(p[4 * k:5 * k])                                   # the point on a corner
    sgn = np.sign(rng.uniform(-1, 1, (k, 3)))
    o[5 * k:6 * k] = np.round(o[5 * k:6 * k])
    p[5 * k:6 * k] = o[5 * k:6 * k] + sgn * 13                                  # exact diagonals from a corner
    o, p = (o + offset) * vs, (p + offset) * vs
    return p.astype(np.float32), o.astype(np.float32)


def segment_meets_cubes(a, b, lo, hi):
    """fp64 slab test: does the segment a -> b ([3]) meet each box lo[i] .. hi[i] ([m,3])?  bool [m]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = b - a
    t0, t1 = np.zeros(len(lo)), np.ones(len(lo))
    ok = np.ones(len(lo), bool)
    for k in range(3):
        if d[k] == 0.0:
            ok &= (a[k] >= lo[:, k]) & (a[k] <= hi[:, k])
            continue
        u, v = (lo[:, k] - a[k]) / d[k], (hi[:, k] - a[k]) / d[k]
        t0, t1 = np.maximum(t0, np.minimum(u, v)), np.minimum(t1, np.maximum(u, v))
    return ok & (t0 <= t1)
