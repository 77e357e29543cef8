"""Analytic depth / colour maps for the TSDF tests and scripts/tsdf_bench.py: ray casts of a sphere, a box and a plane
seen by pinhole cameras (OpenCV axes, world -> camera viewmats, z-depth as Open3D takes it)."""
from __future__ import annotations

import math

import numpy as np


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """world -> camera [4,4] (OpenCV: x right, y down, z forward)."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    if np.linalg.norm(x) < 1e-6:
        x = np.cross(z, (1.0, 0.0, 0.0))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, -R @ eye
    return M


def fibonacci_dirs(n, seed_offset=0.5):
    k = np.arange(n) + seed_offset
    zs = 1 - 2 * k / n
    phi = k * np.pi * (3 - np.sqrt(5))
    r = np.sqrt(1 - zs * zs)
    return np.stack([r * np.cos(phi), r * np.sin(phi), zs], 1)


def intrinsics(W, H, fov_deg=60.0):
    f = 0.5 * W / np.tan(np.radians(fov_deg) / 2)
    return np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]])


def _rays(M, K, W, H):
    """World ray origins and directions (per pixel, direction with camera z-component 1)."""
    u, v = np.meshgrid(np.arange(W) + 0.0, np.arange(H) + 0.0)
    dc = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)
    R, t = M[:3, :3], M[:3, 3]
    return -R.T @ t, dc @ R                                                      # origin [3], dirs [H,W,3] (world)


def texture(p):
    return np.clip(0.5 + 0.45 * np.stack([np.sin(7 * p[..., 0]), np.sin(5 * p[..., 1] + 1), np.cos(6 * p[..., 2])], -1), 0, 1)


def render_sphere(M, K, W, H, centre, radius, room=None):
    """Depth (z) and colour of a sphere, optionally inside an axis-aligned room box [[min], [max]] seen from inside."""
    o, d = _rays(M, K, W, H)
    oc = o - np.asarray(centre, np.float64)
    a = (d * d).sum(-1)
    b = 2 * (d * oc).sum(-1)
    c = oc @ oc - radius * radius
    disc = b * b - 4 * a * c
    t = np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
    t = np.where(t > 0, t, np.inf)
    if room is not None:
        lo, hi = (np.asarray(x, np.float64) for x in room)
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (lo - o) / d, (hi - o) / d
        tr = np.maximum(t1, t2).min(-1)                                          # exit of the room from inside
        t = np.minimum(t, tr)
    depth = np.where(np.isfinite(t), t, 0.0)                                     # direction has camera z = 1: t is z-depth
    p = o + d * depth[..., None]
    return depth.astype(np.float32), texture(p).astype(np.float32)


def render_box(M, K, W, H, lo, hi):
    o, d = _rays(M, K, W, H)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
    tn, tf = np.minimum(t1, t2).max(-1), np.maximum(t1, t2).min(-1)
    hit = (tn <= tf) & (tn > 0)
    depth = np.where(hit, tn, 0.0)
    return depth.astype(np.float32), texture(o + d * depth[..., None]).astype(np.float32)


def render_plane(M, K, W, H, z0=0.0):
    o, d = _rays(M, K, W, H)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (z0 - o[2]) / d[..., 2]
    depth = np.where(t > 0, t, 0.0)
    return depth.astype(np.float32), texture(o + d * depth[..., None]).astype(np.float32)


def sphere_views(n, W, H, centre=(0.1, -0.05, 0.2), radius=0.3, dist=0.9, fov=60.0):
    """n views of a sphere from directions spread over the whole sphere (every part of the surface is seen)."""
    K = intrinsics(W, H, fov)
    vms, deps, rgbs = [], [], []
    for dvec in fibonacci_dirs(n):
        eye = np.asarray(centre) + dist * dvec
        M = look_at(eye, centre, up=(0, 0, 1) if abs(dvec[2]) < 0.9 else (0, 1, 0))
        dep, rgb = render_sphere(M, K, W, H, centre, radius)
        vms.append(M); deps.append(dep); rgbs.append(rgb)
    return (np.stack(deps)[..., None], np.stack(vms).astype(np.float32), np.repeat(K[None], n, 0).astype(np.float32),
            np.stack(rgbs))


def box_views(n, W, H, lo=(-0.2, -0.15, -0.1), hi=(0.25, 0.2, 0.15), dist=0.8):
    K = intrinsics(W, H, 60.0)
    c = 0.5 * (np.asarray(lo) + np.asarray(hi))
    vms, deps, rgbs = [], [], []
    for dvec in fibonacci_dirs(n, 0.3):
        M = look_at(c + dist * dvec, c, up=(0, 0, 1) if abs(dvec[2]) < 0.9 else (0, 1, 0))
        dep, rgb = render_box(M, K, W, H, lo, hi)
        vms.append(M); deps.append(dep); rgbs.append(rgb)
    return (np.stack(deps)[..., None], np.stack(vms).astype(np.float32), np.repeat(K[None], n, 0).astype(np.float32),
            np.stack(rgbs))


def plane_views(n, W, H, height=0.6, seed=0):
    """A plane z = 0 seen obliquely from above; masks cut a disc out of every view (mask False: no data)."""
    rng = np.random.default_rng(seed)
    K = intrinsics(W, H, 70.0)
    vms, deps, rgbs, masks = [], [], [], []
    for k in range(n):
        ang = 2 * np.pi * k / n
        eye = np.array([0.4 * np.cos(ang), 0.4 * np.sin(ang), height + 0.1 * rng.random()])
        M = look_at(eye, (0.05 * rng.standard_normal(), 0.05 * rng.standard_normal(), 0.0))
        dep, rgb = render_plane(M, K, W, H)
        yy, xx = np.mgrid[:H, :W]
        cx, cy = rng.uniform(0.2, 0.8) * W, rng.uniform(0.2, 0.8) * H
        masks.append(((xx - cx) ** 2 + (yy - cy) ** 2) > (0.15 * W) ** 2)
        vms.append(M); deps.append(dep); rgbs.append(rgb)
    return (np.stack(deps)[..., None], np.stack(vms).astype(np.float32), np.repeat(K[None], n, 0).astype(np.float32),
            np.stack(rgbs), np.stack(masks))


ROOM = ((-0.5, -0.4, -0.3), (0.6, 0.5, 0.45))


def room_views(n, W, H, K, room=ROOM, radius=0.08, offset=(0.0, 0.0, 0.0), eye_radius=0.25, seed=0):
    """n views from INSIDE an axis-aligned room with a small sphere in it, all shifted by the world ``offset``.  K = (fx, fy,
    cx, cy) is the caller's (off-centre, fx != fy allowed).  Eyes are drawn within eye_radius of the room's centre (clear of
    the sphere); each looks at a point drawn anywhere in the room, so walls cross every image border, parts of the volume lie
    behind every camera and parts project off all four image sides."""
    rng = np.random.default_rng(seed)
    off = np.asarray(offset, np.float64)
    lo, hi = np.asarray(room[0], np.float64) + off, np.asarray(room[1], np.float64) + off
    mid = 0.5 * (lo + hi)
    centre = mid + np.array([0.22, -0.17, -0.12])
    fx, fy, cx, cy = (float(x) for x in K)
    Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    vms, deps, rgbs = [], [], []
    while len(vms) < n:
        e = rng.standard_normal(3)
        eye = mid + eye_radius * rng.random() ** (1 / 3) * e / np.linalg.norm(e)
        target = lo + (hi - lo) * rng.random(3)
        if np.linalg.norm(eye - centre) < radius + 0.05 or np.linalg.norm(target - eye) < 0.1:
            continue
        z = (target - eye) / np.linalg.norm(target - eye)
        M = look_at(eye, target, up=(0, 0, 1) if abs(z[2]) < 0.9 else (0, 1, 0))
        dep, rgb = render_sphere(M, Km, W, H, centre, radius, room=(lo, hi))
        vms.append(M); deps.append(dep); rgbs.append(rgb)
    return (np.stack(deps)[..., None], np.stack(vms).astype(np.float32), np.repeat(Km[None], n, 0).astype(np.float32),
            np.stack(rgbs))


def projection_reach(r, depths, vms, Ks, views):
    """What the integration of ``views`` meets, recomputed from the restatement's formulas over the voxels of the units each
    view touches (``r``: a RestatedTSDF with the volume's parameters): voxels behind the camera, voxels in front of it that
    project off each image side, and voxels landing in the first half pixel (0.0001 <= u_f < 0.5)."""
    from tsdf_restatement import LOCAL
    F = np.float32
    H, W = depths.shape[1:3]
    out = dict(behind=0, left=0, right=0, top=0, bottom=0, first_half_pixel=0, inside=0)
    for j in views:
        M, K = np.asarray(vms[j], np.float32), np.asarray(Ks[j], np.float32)
        U = r.touched_units(np.asarray(depths[j], np.float32).reshape(H, W), M, K)
        if len(U) == 0:
            continue
        g = (U[:, None, :] * 16 + LOCAL[None]).astype(np.float32)
        x, y, z = [((g[..., a] + F(0.5)) * r.vs) for a in range(3)]
        with np.errstate(all="ignore"):
            zc = ((M[2, 0] * x + M[2, 1] * y) + M[2, 2] * z) + M[2, 3]
            xc = ((M[0, 0] * x + M[0, 1] * y) + M[0, 2] * z) + M[0, 3]
            yc = ((M[1, 0] * x + M[1, 1] * y) + M[1, 2] * z) + M[1, 3]
            uf = ((xc * K[0, 0]) / zc + K[0, 2]) + F(0.5)
            vf = ((yc * K[1, 1]) / zc + K[1, 2]) + F(0.5)
        front = zc > 0
        out["behind"] += int((~front).sum())
        out["left"] += int((front & (uf < F(0.0001))).sum())
        out["right"] += int((front & (uf >= F(W))).sum())
        out["top"] += int((front & (vf < F(0.0001))).sum())
        out["bottom"] += int((front & (vf >= F(H))).sum())
        out["first_half_pixel"] += int((front & (uf >= F(0.0001)) & (uf < F(0.5))).sum())
        out["inside"] += int((front & (uf >= F(0.0001)) & (uf < F(W)) & (vf >= F(0.0001)) & (vf < F(H))).sum())
    return out


def pinhole_camera(M, K, W, H):
    """A ``radegs.PinholeCamera`` (nerfstudio conventions: OpenGL c2w) for the OpenCV world -> camera matrix M."""
    import torch
    from collab_splats_amd.radegs import PinholeCamera
    c2w = np.linalg.inv(np.asarray(M, np.float64)) @ np.diag([1.0, -1.0, -1.0, 1.0])
    return PinholeCamera.make(torch.tensor(c2w[:3, :4], dtype=torch.float32), float(K[0, 0]), float(K[1, 1]), W, H,
                              cx=float(K[0, 2]), cy=float(K[1, 2]))


def sphere_gaussians(n, centre=(0.1, -0.05, 0.2), radius=0.3, seed=0):
    """A RaDe-GS model of n flat, opaque Gaussians tiling a textured sphere (CPU tensors)."""
    import torch
    from collab_splats_amd import radegs
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    means = torch.tensor(centre, dtype=torch.float32) + radius * d
    spacing = radius * math.sqrt(4 * math.pi / n)
    scales = torch.log(torch.tensor([spacing, spacing, spacing * 0.05])).expand(n, 3).clone()
    z = torch.tensor([0.0, 0.0, 1.0]).expand(n, 3)
    axis = torch.cross(z, d, dim=1)                                   # rotate local z onto the normal d
    s = axis.norm(dim=1, keepdim=True).clamp_min(1e-8)
    ang = torch.atan2(s, d[:, 2:3])
    quats = torch.cat([torch.cos(ang / 2), torch.sin(ang / 2) * axis / s], 1)
    opac = torch.full((n, 1), 4.0)
    col = torch.from_numpy(texture(means.double().numpy())).float()
    dc = (col - 0.5) / 0.28209479177387814                            # SH degree 0: colour = 0.5 + C0 dc
    rest = torch.zeros(n, 15, 3)
    cfg = radegs.RadegsModelConfig()
    m = radegs.RadegsModel(cfg, means, scales, quats, opac, dc, rest)
    m.step = 10 ** 6
    return m
