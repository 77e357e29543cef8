"""Oriented point clouds from depth and normal maps on the MI355X (csrc/depthcloud.hip).

The reference's Poisson exporters turn a trained model into an oriented, coloured point cloud (collab_splats/utils/mesh.py
``DepthAndNormalMapsPoisson.main``, :864-1002, with ``find_depth_edges``, ``pick_indices_at_random`` and camera_utils.py's
``get_colored_points_from_depth``; ``GaussiansToPoisson.main``, :676-791, with its per-Gaussian Python loop over the masks).
Here the same stages run on the stacked maps ``RadegsModel.render_views`` leaves on the device: the depth-edge filter, the
candidate mask, a seeded uniform sample per frame, the back-projection with normals and colours, and the mask filter of the
Gaussian centres are HIP kernels.  There is no CPU fallback.

Two things differ from the reference on purpose.  The sample is not ``torch.randperm``: every candidate pixel gets a 32-bit key
from a counter-based hash of (seed, global frame index, pixel) and a frame keeps the candidates with the smallest keys, a uniform
subset without replacement that does not depend on how frames are batched; the output is ordered by frame, then pixel (the
reference's order is a permutation of it; a cloud has no order).  And a pixel must have depth > 0 (and a true mask) to be a
candidate: the reference picks its indices before it zeroes masked depths, and with the edge filter ignores the depth
altogether, so masked pixels and holes become points at the camera centre there.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from ._lib import MisplatError, load, ptr, require_gpu, run
from .meshmap import _prep
from .pointcloud import _cloud

MAX_DILATION = 63
_EDGES, _SAMPLE = range(2)


# ---------------------------------------------------------------------------------------------------------- helpers
def _depth(name: str, depth: Tensor) -> Tuple[int, int, int]:
    if not isinstance(depth, Tensor) or not (depth.dim() == 3 or (depth.dim() == 4 and depth.shape[3] == 1)):
        raise ValueError(f"{name}: depth must be [V,H,W] or [V,H,W,1], got "
                         f"{tuple(depth.shape) if isinstance(depth, Tensor) else type(depth).__name__}")
    v, h, w = (int(x) for x in depth.shape[:3])
    if v < 1 or h < 1 or w < 1:
        raise ValueError(f"{name}: depth must hold at least one view and one pixel, got {tuple(depth.shape)}")
    return v, h, w


def _flag(name: str, what: str, x: Optional[Tensor], shape: Tuple[int, int, int]) -> Optional[Tensor]:
    """A [V,H,W(,1)] boolean map as contiguous uint8 (non-zero: true), or None."""
    if x is None:
        return None
    if not isinstance(x, Tensor) or x.numel() != shape[0] * shape[1] * shape[2] or tuple(x.shape[:3]) != shape:
        raise ValueError(f"{name}: {what} must be [V,H,W] = {shape} (or with a last axis of 1), got "
                         f"{tuple(x.shape) if isinstance(x, Tensor) else type(x).__name__}")
    x = x.detach().reshape(shape)
    return (x if x.dtype == torch.bool else x != 0).contiguous().view(torch.uint8)


def _map3(name: str, what: str, x: Tensor, shape: Tuple[int, int, int]) -> Tensor:
    if not isinstance(x, Tensor) or tuple(x.shape) != shape + (3,):
        raise ValueError(f"{name}: {what} must be [V,H,W,3] = {shape + (3,)}, got "
                         f"{tuple(x.shape) if isinstance(x, Tensor) else type(x).__name__}")
    return _prep(x)


def _cameras(name: str, c2w: Tensor, intrinsics: Tensor, v: int) -> Tuple[Tensor, Tensor]:
    if not isinstance(c2w, Tensor) or tuple(c2w.shape) != (v, 3, 4):
        raise ValueError(f"{name}: c2w must be [V,3,4] with V = {v}, got {tuple(c2w.shape) if isinstance(c2w, Tensor) else type(c2w).__name__}")
    if not isinstance(intrinsics, Tensor) or tuple(intrinsics.shape) != (v, 4):
        raise ValueError(f"{name}: intrinsics must be [V,4] = (fx, fy, cx, cy) with V = {v}, got "
                         f"{tuple(intrinsics.shape) if isinstance(intrinsics, Tensor) else type(intrinsics).__name__}")
    return _prep(c2w), _prep(intrinsics)


def _u32(name: str, what: str, v) -> int:
    if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v < 1 << 32:
        raise ValueError(f"{name}: {what} must be an integer in 0..2^32-1, got {v!r}")
    return v


def _workspace(shape: Tuple[int, int, int], kind: int, device) -> Tensor:
    b = int(load().misplat_depthcloud_workspace(shape[0], shape[1], shape[2], kind))
    if b < 0:
        raise ValueError(f"depthcloud: maps of shape {shape} are beyond the library's limits (V <= 65535, H W < 2^31)")
    return torch.empty(b, dtype=torch.uint8, device=device)


def _check_edges(name: str, threshold, dilation_itr) -> float:
    if not isinstance(dilation_itr, int) or isinstance(dilation_itr, bool) or not 0 <= dilation_itr <= MAX_DILATION:
        raise ValueError(f"{name}: dilation_itr must be an integer in 0..{MAX_DILATION}, got {dilation_itr!r}")
    try:
        t = float(threshold)
    except (TypeError, ValueError):
        t = float("nan")
    if t != t:
        raise ValueError(f"{name}: threshold must be a number, got {threshold!r}")
    return t


# ------------------------------------------------------------------------------------------------------------ edges
def _edges(d: Tensor, shape, threshold: float, dilation: int) -> Tensor:
    out = torch.empty(shape, dtype=torch.uint8, device=d.device)
    ws = _workspace(shape, _EDGES, d.device)
    run("misplat_depthcloud_edges", ptr(d), shape[0], shape[1], shape[2], threshold, dilation, ptr(ws), ws.numel(), ptr(out))
    return out


def depth_edges(depth: Tensor, threshold: float = 0.01, dilation_itr: int = 3) -> Tensor:
    """bool [V,H,W]: the reference's ``find_depth_edges`` per view.  inv = 1 / (d + 1e-6) in fp32; lap = ((up + left) + (right
    + down)) - 4 inv with zeros outside the image (the reference pads with zeros); a pixel is an edge when lap > threshold
    (fp32); the edges are dilated by ``dilation_itr`` rounds of a 3 x 3 box, i.e. by a square of Chebyshev radius
    ``dilation_itr`` clipped at the border.  0 <= dilation_itr <= 63."""
    name = "depth_edges"
    shape = _depth(name, depth)
    t = _check_edges(name, threshold, dilation_itr)
    require_gpu(depth)
    return _edges(_prep(depth).reshape(shape), shape, t, dilation_itr).view(torch.bool)


# --------------------------------------------------------------------------------------------------------- sampling
def _sample(cand: Tensor, keys: Optional[Tensor], shape, s: int, seed: int, frame_offset: int):
    v, p = shape[0], shape[1] * shape[2]
    cap = v * min(s, p)
    if cap >= 1 << 31:
        raise ValueError(f"sample_pixels: {v} frames of up to {min(s, p)} samples are beyond the library's limits (< 2^31 in all)")
    dev = cand.device
    frame_ids = torch.empty(cap, dtype=torch.int32, device=dev)
    pixel_ids = torch.empty(cap, dtype=torch.int32, device=dev)
    counts = torch.empty(v, dtype=torch.int32, device=dev)
    base = torch.empty(v + 1, dtype=torch.int32, device=dev)
    ws = _workspace(shape, _SAMPLE, dev)
    run("misplat_depthcloud_sample", ptr(cand), ptr(keys), shape[0], shape[1], shape[2], s, seed, frame_offset, ptr(ws),
        ws.numel(), ptr(frame_ids), ptr(pixel_ids), ptr(counts), ptr(base))
    total = int(base[v].item())                                     # the call's host read
    return frame_ids[:total], pixel_ids[:total], counts


def _check_sample(name: str, samples_per_frame, seed, frame_offset, v: int) -> None:
    if not isinstance(samples_per_frame, int) or isinstance(samples_per_frame, bool) or not 1 <= samples_per_frame < 1 << 31:
        raise ValueError(f"{name}: samples_per_frame must be an integer in 1..2^31-1, got {samples_per_frame!r}")
    _u32(name, "seed", seed)
    _u32(name, "frame_offset", frame_offset)
    if frame_offset + v > 1 << 32:
        raise ValueError(f"{name}: frame_offset + V must not exceed 2^32")


def sample_pixels(candidates: Tensor, samples_per_frame: int, seed: int = 0, frame_offset: int = 0, keys: Optional[Tensor] = None
                  ) -> Tuple[Tensor, Tensor, Tensor]:
    """(frame_ids int32 [P], pixel_ids int32 [P], counts int32 [V]) from candidates bool [V,H,W]: frame v keeps the
    min(samples_per_frame, n_v) candidates with the smallest key, ties to the lowest pixel index; the key of pixel p = y W + x
    is the 32-bit hash of (seed, frame_offset + v, p) (two rounds of a 32-bit finaliser, csrc/hashmix.h), so the result does
    not depend on how frames are batched.  ``keys`` (int32 [V,H,W] holding uint32 bits) replaces the hash.  The output is
    ordered by frame, then pixel; frame_ids index this call's frames.  This stands for the reference's
    ``randperm(n)[:S]`` (``pick_indices_at_random``): a uniform subset without replacement, whose order there is a
    permutation of this one."""
    name = "sample_pixels"
    shape = _depth(name, candidates)
    _check_sample(name, samples_per_frame, seed, frame_offset, shape[0])
    cand = _flag(name, "candidates", candidates, shape)
    if keys is not None:
        if not isinstance(keys, Tensor) or tuple(keys.shape) != shape or keys.dtype != torch.int32:
            raise ValueError(f"{name}: keys must be int32 [V,H,W] = {shape}")
        keys = keys.detach().contiguous()
    require_gpu(candidates, keys)
    return _sample(cand, keys, shape, samples_per_frame, seed, frame_offset)


# --------------------------------------------------------------------------------------------------- back-projection
def _ids(name: str, frame_ids: Tensor, pixel_ids: Tensor) -> Tuple[Tensor, Tensor]:
    for what, x in (("frame_ids", frame_ids), ("pixel_ids", pixel_ids)):
        if not isinstance(x, Tensor) or x.dim() != 1 or x.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{name}: {what} must be an integer [P] tensor")
    if frame_ids.shape != pixel_ids.shape:
        raise ValueError(f"{name}: frame_ids and pixel_ids must have one entry per sample, got {tuple(frame_ids.shape)} and "
                         f"{tuple(pixel_ids.shape)}")
    return frame_ids.detach().to(torch.int32).contiguous(), pixel_ids.detach().to(torch.int32).contiguous()


def _backproject(d, rgb, nrm, c2w, intr, shape, f, p):
    n = f.shape[0]
    dev = d.device
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((n, 3), dtype=torch.float32, device=dev)
    normals = None if nrm is None else torch.empty((n, 3), dtype=torch.float32, device=dev)
    run("misplat_depthcloud_backproject", ptr(d), ptr(rgb), ptr(nrm), ptr(c2w), ptr(intr), shape[0], shape[1], shape[2], ptr(f),
        ptr(p), n, ptr(points), ptr(normals), ptr(colors))
    return points, normals, colors


def backproject(depth: Tensor, rgb: Tensor, normals: Optional[Tensor], c2w: Tensor, intrinsics: Tensor, frame_ids: Tensor,
                pixel_ids: Tensor) -> Tuple[Tensor, Optional[Tensor], Tensor]:
    """(points [P,3], normals [P,3] or None, colors [P,3]) of the sampled pixels.  ``c2w`` [V,3,4] is nerfstudio's OpenGL pose,
    ``intrinsics`` [V,4] = (fx, fy, cx, cy).  Per sample at pixel (u, v) of depth d, in fp32 in this order: R = c2w[:3,:3]
    diag(1,-1,-1); x = ((u + 0.5) - cx) d / fx, y = ((v + 0.5) - cy) d / fy; p = ((R0 x + R1 y) + R2 d) + t with R0..R2 the
    columns of R (``get_means3d_backproj``; the reference multiplies by inv(R) from the right, which for an orthonormal R
    equals R p).  Normals (mesh.py:937-954): n = 2 m - 1, y and z flipped, divided by max(sqrt((nx nx + ny ny) + nz nz), 1e-12),
    rotated by R.  Colours are gathered."""
    name = "backproject"
    shape = _depth(name, depth)
    d = _prep(depth).reshape(shape)
    rgb_ = _map3(name, "rgb", rgb, shape)
    nrm = None if normals is None else _map3(name, "normals", normals, shape)
    pose, intr = _cameras(name, c2w, intrinsics, shape[0])
    f, p = _ids(name, frame_ids, pixel_ids)
    if f.numel():
        lo_f, hi_f = (int(x) for x in torch.aminmax(f))
        lo_p, hi_p = (int(x) for x in torch.aminmax(p))
        if lo_f < 0 or hi_f >= shape[0] or lo_p < 0 or hi_p >= shape[1] * shape[2]:
            raise ValueError(f"{name}: frame_ids must lie in 0..{shape[0] - 1} and pixel_ids in 0..{shape[1] * shape[2] - 1}")
    require_gpu(depth, rgb, normals, c2w, intrinsics, frame_ids, pixel_ids)
    return _backproject(d, rgb_, nrm, pose, intr, shape, f, p)


# ------------------------------------------------------------------------------------------------------ composition
def depth_normal_cloud(depth: Tensor, rgb: Tensor, normals: Optional[Tensor], c2w: Tensor, intrinsics: Tensor,
                       samples_per_frame: int, seed: int = 0, frame_offset: int = 0, masks: Optional[Tensor] = None,
                       valid: Optional[Tensor] = None, filter_edges: bool = False, edge_threshold: float = 0.004,
                       edge_dilation: int = 10) -> Dict[str, Optional[Tensor]]:
    """The per-frame body of the reference's ``DepthAndNormalMapsPoisson.main`` for a batch of views: ``{"points", "normals",
    "colors", "frame_ids", "pixel_ids", "counts"}``.  A pixel is a candidate when depth > 0, ``masks`` is true there (when
    given), ``valid`` is true there (when given) and, with ``filter_edges``, it is not a dilated depth edge
    (``depth_edges(depth, edge_threshold, edge_dilation)``); ``sample_pixels`` takes ``samples_per_frame`` of them per frame
    and ``backproject`` lifts them.  Without masks and edge filter the candidates are the reference's ``nonzero(ravel(depth))``
    whenever depths are finite and non-negative; a masked pixel or a hole never becomes a point (the reference puts those at
    the camera centre)."""
    name = "depth_normal_cloud"
    shape = _depth(name, depth)
    _check_sample(name, samples_per_frame, seed, frame_offset, shape[0])
    t = _check_edges(name, edge_threshold, edge_dilation) if filter_edges else 0.0
    d = _prep(depth).reshape(shape)
    rgb_ = _map3(name, "rgb", rgb, shape)
    nrm = None if normals is None else _map3(name, "normals", normals, shape)
    pose, intr = _cameras(name, c2w, intrinsics, shape[0])
    m = _flag(name, "masks", masks, shape)
    ok = _flag(name, "valid", valid, shape)
    require_gpu(depth, rgb, normals, c2w, intrinsics, masks, valid)
    edges = _edges(d, shape, t, edge_dilation) if filter_edges else None
    cand = torch.empty(shape, dtype=torch.uint8, device=d.device)
    run("misplat_depthcloud_candidates", ptr(d), ptr(m), ptr(ok), ptr(edges), cand.numel(), ptr(cand))
    f, p, counts = _sample(cand, None, shape, samples_per_frame, seed, frame_offset)
    points, out_normals, colors = _backproject(d, rgb_, nrm, pose, intr, shape, f, p)
    return {"points": points, "normals": out_normals, "colors": colors, "frame_ids": f, "pixel_ids": p, "counts": counts}


# ---------------------------------------------------------------------------------------------- Gaussian mask filter
def gaussian_mask_filter(means: Tensor, c2w: Tensor, intrinsics: Tensor, masks: Tensor) -> Tensor:
    """bool [N]: the Gaussians the reference's mask loop keeps (mesh.py:692-740), in one kernel over N x V.  Per view, in fp32:
    p_cam = (p - t) @ R, R = c2w[:3,:3] diag(1,-1,-1), each component (d0 R0j + d1 R1j) + d2 R2j; u = x fx / z + cx, v likewise
    (``project_pix``); (iu, iv) = floor((u, v) - 0.5); the Gaussian is dropped when 0 < iu < W, 0 < iv < H (the reference's strict
    > 0 is kept) and the mask is false there.  A Gaussian survives if no view drops it (the reference filters view by view: the
    same set).  One deviation: a Gaussian with z <= 0 in a view is not tested by that view (the reference tests its mirrored
    projection)."""
    name = "gaussian_mask_filter"
    _cloud(name, "means", means)
    shape = _depth(name, masks)
    m = _flag(name, "masks", masks, shape)
    pose, intr = _cameras(name, c2w, intrinsics, shape[0])
    require_gpu(means, c2w, intrinsics, masks)
    p = _prep(means)
    keep = torch.empty(p.shape[0], dtype=torch.uint8, device=p.device)
    run("misplat_depthcloud_gaussian_filter", ptr(p), p.shape[0], ptr(pose), ptr(intr), ptr(m), shape[0], shape[1], shape[2],
        ptr(keep))
    return keep.view(torch.bool)


__all__ = ["depth_edges", "sample_pixels", "backproject", "depth_normal_cloud", "gaussian_mask_filter", "MisplatError"]
