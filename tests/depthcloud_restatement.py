"""numpy restatement of csrc/depthcloud.hip: the oracle of the depth-cloud tests.

Every fp32 expression is evaluated in the order written here, one numpy float32 operation at a time (numpy never contracts
a multiply and an add); the kernels are compiled with -ffp-contract=off and write the same orders, so integers must be equal
and floats bit for bit.  The hash runs in uint32 (Python integers masked to 32 bits, or uint64 arrays masked after each step).
"""
from __future__ import annotations

import numpy as np

F = np.float32
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------- hash
def mix32(seed, i, draw):
    """Two rounds of a 32-bit finaliser over (seed, i, draw): csrc/hashmix.h.  ``draw`` may be an array."""
    draw = np.asarray(draw, np.uint64)
    x = (np.uint64(seed * 0x9E3779B1 & M32) + np.uint64(i * 0x85EBCA77 & M32) + ((draw * np.uint64(0xC2B2AE3D)) & np.uint64(M32))
         + np.uint64(0x27D4EB2F)) & np.uint64(M32)

    def mul(x, c):
        return (x * np.uint64(c)) & np.uint64(M32)

    x ^= x >> np.uint64(16); x = mul(x, 0x85EBCA6B); x ^= x >> np.uint64(13); x = mul(x, 0xC2B2AE35); x ^= x >> np.uint64(16)
    x = (x + np.uint64(i & M32)) & np.uint64(M32)
    x ^= x >> np.uint64(15); x = mul(x, 0x2C1B3C6D); x ^= x >> np.uint64(12); x = mul(x, 0x297A2D39); x ^= x >> np.uint64(15)
    return x.astype(np.uint32)


# ------------------------------------------------------------------------------------------------------------ edges
def laplacian(depth):
    """fp32 [V,H,W]: lap = ((up + left) + (right + down)) - 4 inv of inv = 1 / (d + 1e-6), zeros outside the image."""
    d = np.asarray(depth, F)
    inv = (F(1.0) / (d + F(1e-6))).astype(F)
    pad = np.zeros((d.shape[0], d.shape[1] + 2, d.shape[2] + 2), F)
    pad[:, 1:-1, 1:-1] = inv
    up, down = pad[:, :-2, 1:-1], pad[:, 2:, 1:-1]
    left, right = pad[:, 1:-1, :-2], pad[:, 1:-1, 2:]
    return ((up + left) + (right + down)) - F(4.0) * inv


def dilate(edges, r):
    """A square of Chebyshev radius r, clipped at the border (r rounds of a 3 x 3 box)."""
    e = np.asarray(edges, bool)
    V, H, W = e.shape
    out = np.zeros_like(e)
    for dy in range(-r, r + 1):
        ys, yd = slice(max(0, -dy), min(H, H - dy)), slice(max(0, dy), min(H, H + dy))
        if ys.start >= ys.stop:
            continue
        for dx in range(-r, r + 1):
            xs, xd = slice(max(0, -dx), min(W, W - dx)), slice(max(0, dx), min(W, W + dx))
            if xs.start >= xs.stop:
                continue
            out[:, yd, xd] |= e[:, ys, xs]
    return out


def depth_edges(depth, threshold=0.01, dilation_itr=3):
    return dilate(laplacian(depth) > F(threshold), dilation_itr)


def candidates(depth, masks=None, valid=None, edges=None):
    c = np.asarray(depth, F) > 0
    for m in (masks, valid):
        if m is not None:
            c &= np.asarray(m, bool).reshape(c.shape)
    if edges is not None:
        c &= ~np.asarray(edges, bool)
    return c


# --------------------------------------------------------------------------------------------------------- sampling
def pixel_keys(shape, seed=0, frame_offset=0):
    """uint32 [V,H,W]: the key of pixel p = y W + x of frame v is mix32(seed, frame_offset + v, p)."""
    V, H, W = shape
    pix = np.arange(H * W, dtype=np.uint64)
    return np.stack([mix32(seed, frame_offset + v, pix) for v in range(V)]).reshape(V, H, W)


def sample_pixels(cand, samples_per_frame, seed=0, frame_offset=0, keys=None):
    """(frame_ids int32 [P], pixel_ids int32 [P], counts int32 [V]): per frame the min(S, n) candidates first in the order
    (key, pixel), reported by frame, then pixel."""
    cand = np.asarray(cand, bool)
    V = cand.shape[0]
    k = pixel_keys(cand.shape, seed, frame_offset) if keys is None else np.asarray(keys).view(np.uint32)
    frames, pixels, counts = [], [], []
    for v in range(V):
        pix = np.nonzero(cand[v].ravel())[0]
        order = np.lexsort((pix, k[v].ravel()[pix]))                # by key, ties by pixel
        chosen = np.sort(pix[order[:samples_per_frame]])
        frames.append(np.full(len(chosen), v, np.int32))
        pixels.append(chosen.astype(np.int32))
        counts.append(len(chosen))
    return np.concatenate(frames), np.concatenate(pixels), np.asarray(counts, np.int32)


# --------------------------------------------------------------------------------------------------- back-projection
def _pose(c2w):
    """R = c2w[:3,:3] diag(1,-1,-1) and t, fp32."""
    c2w = np.asarray(c2w, F)
    return (c2w[:, :3] * np.array([1.0, -1.0, -1.0], F)).astype(F), c2w[:, 3]


def camera_abs(depth, intrinsics, frame_ids, pixel_ids):
    """fp64 [P]: |x| + |y| + |z| of each sample's camera-space point (the scale of the back-projection's rounding bound)."""
    depth = np.asarray(depth, np.float64)
    V, H, W = depth.shape[:3]
    f, p = np.asarray(frame_ids, np.int64), np.asarray(pixel_ids, np.int64)
    intr = np.asarray(intrinsics, np.float64)[f]
    d = depth.reshape(V, H * W)[f, p]
    x = ((p % W) + 0.5 - intr[:, 2]) * d / intr[:, 0]
    y = ((p // W) + 0.5 - intr[:, 3]) * d / intr[:, 1]
    return np.abs(x) + np.abs(y) + np.abs(d)


def backproject(depth, rgb, normals, c2w, intrinsics, frame_ids, pixel_ids):
    """(points, normals or None, colors) fp32 [P,3] in the kernel's operation order."""
    depth = np.asarray(depth, F)
    V, H, W = depth.shape[:3]
    depth = depth.reshape(V, H * W)
    rgb = np.asarray(rgb, F).reshape(V, H * W, 3)
    f, p = np.asarray(frame_ids, np.int64), np.asarray(pixel_ids, np.int64)
    n = len(f)
    points, colors = np.zeros((n, 3), F), rgb[f, p]
    out_n = None if normals is None else np.zeros((n, 3), F)
    nrm = None if normals is None else np.asarray(normals, F).reshape(V, H * W, 3)
    intr = np.asarray(intrinsics, F)
    for v in range(V):
        sel = np.nonzero(f == v)[0]
        if not len(sel):
            continue
        R, t = _pose(c2w[v])
        fx, fy, cx, cy = intr[v]
        pix = p[sel]
        d = depth[v, pix]
        x = (((pix % W).astype(F) + F(0.5)) - cx) * d / fx
        y = (((pix // W).astype(F) + F(0.5)) - cy) * d / fy
        for a in range(3):
            points[sel, a] = ((R[a, 0] * x + R[a, 1] * y) + R[a, 2] * d) + t[a]
        if nrm is not None:
            m = nrm[v, pix]
            nx, ny, nz = F(2.0) * m[:, 0] - F(1.0), -(F(2.0) * m[:, 1] - F(1.0)), -(F(2.0) * m[:, 2] - F(1.0))
            ln = np.maximum(np.sqrt((nx * nx + ny * ny) + nz * nz), F(1e-12))
            nx, ny, nz = nx / ln, ny / ln, nz / ln
            for a in range(3):
                out_n[sel, a] = (R[a, 0] * nx + R[a, 1] * ny) + R[a, 2] * nz
    return points, out_n, colors


# ---------------------------------------------------------------------------------------------- Gaussian mask filter
def project(means, c2w, intrinsics):
    """(u, v, z) fp32 [N] of one view: c = (p - t) @ R, each component (d0 R0j + d1 R1j) + d2 R2j; u = x fx / z + cx."""
    P = np.asarray(means, F)
    R, t = _pose(c2w)
    fx, fy, cx, cy = np.asarray(intrinsics, F)
    d0, d1, d2 = P[:, 0] - t[0], P[:, 1] - t[1], P[:, 2] - t[2]
    c = [(d0 * R[0, j] + d1 * R[1, j]) + d2 * R[2, j] for j in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        return c[0] * fx / c[2] + cx, c[1] * fy / c[2] + cy, c[2]


def gaussian_mask_filter(means, c2w, intrinsics, masks):
    masks = np.asarray(masks, bool)
    V, H, W = masks.shape[:3]
    masks = masks.reshape(V, H, W)
    keep = np.ones(len(means), bool)
    for v in range(V):
        u, w, z = project(means, c2w[v], intrinsics[v])
        with np.errstate(invalid="ignore"):
            iu, iv = np.floor(u - F(0.5)), np.floor(w - F(0.5))
            inside = (z > 0) & (iu > 0) & (iu < W) & (iv > 0) & (iv < H)
        ii = np.nonzero(inside)[0]
        keep[ii[~masks[v, iv[ii].astype(np.int64), iu[ii].astype(np.int64)]]] = False
    return keep
