"""Bilateral-grid colour correction of a training view and the grids' total-variation loss (plumbing around
csrc/bilagrid.hip; no kernels here).

Reference call sites: collab_splats/models/rade_gs_model.py:231-234 (``_apply_bilateral_grid`` after the
background composite, training only, ``camera.metadata["cam_idx"]``), :284-289 (``tv_loss``) and
configs/rade_gs_method.py:78-83 (the ``bilateral_grid`` optimizer group).  The grid module, the slice and the TV loss
themselves are nerfstudio's Splatfacto [UNVERIFIED-UPSTREAM: absent from the reference tree; restated from the published
method, Wang et al., *Bilateral Guided Radiance Field Processing*, as gsplat / nerfstudio use it].  ``bilagrid_slice`` is one
autograd node over ``misplat_bilagrid_slice_fwd`` / ``_bwd``, ``bilagrid_tv_loss`` one over ``misplat_bilagrid_tv_fwd`` /
``_bwd``.  DESIGN.md section 24.
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import torch
from torch import Tensor, nn

from . import _lib
from ._lib import MisplatError, ptr, require_gpu, run

MAX_GRID_XY = 256
MAX_GRID_L = 16
MAX_SIDE = 32768
TV_BLOCKS = 1024                                # MISPLAT_BILAGRID_TV_BLOCKS
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _check_grid_sizes(grid_x: int, grid_y: int, grid_w: int, what: str) -> None:
    if not (1 <= int(grid_x) <= MAX_GRID_XY and 1 <= int(grid_y) <= MAX_GRID_XY):
        raise ValueError(f"{what}: the grid's width and height must be 1..{MAX_GRID_XY}, got (GW, GH) = ({grid_x}, {grid_y})")
    if not 1 <= int(grid_w) <= MAX_GRID_L:
        raise ValueError(f"{what}: the grid's guidance depth must be 1..{MAX_GRID_L}, got L = {grid_w}")


class BilateralGrid(nn.Module):
    """One bilateral grid per training camera: ``grids`` [num, 12, L, GH, GW] float32, channel 4 c + j = entry (c, j) of a
    3 x 4 affine colour transform, every cell initialised to the identity.  Name, layout and initialisation are nerfstudio's
    ``BilateralGrid`` [UNVERIFIED-UPSTREAM], so the ``bil_grids.grids`` entry of its checkpoints loads with
    ``load_state_dict``.  ``grid_X`` = GW, ``grid_Y`` = GH, ``grid_W`` = L (the guidance axis)."""

    def __init__(self, num: int, grid_X: int = 16, grid_Y: int = 16, grid_W: int = 8):
        super().__init__()
        if int(num) < 1:
            raise ValueError(f"BilateralGrid: one grid per training camera, got num = {num}")
        _check_grid_sizes(grid_X, grid_Y, grid_W, "BilateralGrid")
        eye = torch.tensor(IDENTITY, dtype=torch.float32).view(1, 12, 1, 1, 1)
        self.grids = nn.Parameter(eye.repeat(int(num), 1, int(grid_W), int(grid_Y), int(grid_X)))

    def forward(self, rgb: Tensor, cam_idx: int) -> Tensor:
        return bilagrid_slice(rgb, self.grids, cam_idx)

    def tv_loss(self) -> Tensor:
        return bilagrid_tv_loss(self.grids)


def _check_grids(grids: Tensor, what: str) -> Tuple[int, int, int, int]:
    if not isinstance(grids, Tensor) or grids.dim() != 5:
        raise ValueError(f"{what}: grids must be [num, 12, L, GH, GW], got {tuple(getattr(grids, 'shape', ()))}")
    num, ch, L, GH, GW = (int(v) for v in grids.shape)
    if ch != 12:
        raise ValueError(f"{what}: grids must carry 12 channels (a 3 x 4 affine), got {tuple(grids.shape)}")
    if num < 1:
        raise ValueError(f"{what}: grids of no camera {tuple(grids.shape)}")
    _check_grid_sizes(GW, GH, L, what)
    return num, L, GH, GW


def _check_plain(what: str, **tensors: Tensor) -> None:
    """fp32, on the GPU, contiguous -- every tensor's dtype first, then the devices, then the layouts; anything else is
    refused (there is no CPU fallback and no silent copy)."""
    for name, t in tensors.items():
        if t.dtype != torch.float32:
            raise MisplatError(f"{what}: {name} must be float32, got {t.dtype}")
    for name, t in tensors.items():
        if not t.is_cuda:
            raise MisplatError(f"{what}: {name} {tuple(t.shape)} is on {t.device}: the bilateral grid runs on the MI355X only "
                               "(there is no CPU fallback; the restatement under tests/ is test infrastructure)")
    for name, t in tensors.items():
        if not t.is_contiguous():
            raise MisplatError(f"{what}: {name} must be contiguous, got shape {tuple(t.shape)} with strides {tuple(t.stride())}")


class _Slice(torch.autograd.Function):
    """The slice as ONE autograd node: one launch forward, three backward; only ``rgb`` and ``grids`` are saved -- no
    [H, W, 12] affine field exists, and the gradient of the grids is a gather (no atomics: two runs are equal bit for bit)."""

    @staticmethod
    def forward(ctx, rgb, grids, cam, geo):
        H, W, num, L, GH, GW = geo
        out = torch.empty_like(rgb)
        per_cam = 12 * L * GH * GW
        grid = C.c_void_p(grids.data_ptr() + 4 * per_cam * cam)
        run("misplat_bilagrid_slice_fwd", H, W, ptr(rgb), grid, GW, GH, L, ptr(out))
        ctx.save_for_backward(rgb, grids)
        ctx.cam, ctx.geo = cam, geo
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, v_out):
        if v_out is None:
            return None, None, None, None
        lib = _lib.load()
        rgb, grids = ctx.saved_tensors
        H, W, num, L, GH, GW = ctx.geo
        v_out = v_out.to(torch.float32).contiguous()
        n = int(lib.misplat_bilagrid_scratch_floats(H, W, GW, GH, L))
        if n < 0:
            raise MisplatError(f"bilagrid_slice: sizes outside the kernels' limits (image {(H, W)}, grid {(GW, GH, L)})")
        scratch = torch.empty(n, device=rgb.device, dtype=torch.float32)
        v_rgb, v_grids = torch.empty_like(rgb), torch.empty_like(grids)
        run("misplat_bilagrid_slice_bwd", H, W, ptr(rgb), ptr(grids), num, ctx.cam, GW, GH, L, ptr(v_out), ptr(v_rgb),
            ptr(v_grids), ptr(scratch))
        return v_rgb, v_grids, None, None


def bilagrid_slice(rgb: Tensor, grids: Tensor, cam_idx: int) -> Tensor:
    """The colour transform of camera ``cam_idx`` applied to a rendered image [UNVERIFIED-UPSTREAM]:

        out[y, x] = A(y, x) (r, g, b, 1),   A = trilinear(grids[cam_idx] at (x / (W - 1), y / (H - 1), 0.299 r + 0.587 g + 0.114 b))

    ``rgb`` [H, W, 3] or [1, H, W, 3], float32 in 0..1, contiguous, on the GPU; ``grids`` [num, 12, L, GH, GW]; ``cam_idx`` a
    host int in [0, num).  The grid is sampled with border clamping and ``align_corners=True`` (what
    ``F.grid_sample(grids[cam_idx][None], ((x, y, z) - 0.5) * 2, padding_mode="border", align_corners=True)`` returns); the
    result is not clamped.  Gradients go to ``rgb`` (the path through the luma included) and to ``grids`` (the slices of the
    other cameras are exact zeros).  The identity grid returns ``rgb`` bit for bit."""
    what = "bilagrid_slice"
    if not isinstance(rgb, Tensor) or rgb.dim() not in (3, 4) or rgb.shape[-1] != 3 or (rgb.dim() == 4 and rgb.shape[0] != 1):
        raise ValueError(f"{what}: rgb must be [H, W, 3] or [1, H, W, 3], got {tuple(getattr(rgb, 'shape', ()))}")
    num, L, GH, GW = _check_grids(grids, what)
    if isinstance(cam_idx, Tensor):
        raise ValueError(f"{what}: cam_idx must be a host int, got a tensor (the camera is chosen before any GPU call)")
    cam = int(cam_idx)
    if not 0 <= cam < num:
        raise ValueError(f"{what}: cam_idx {cam} outside [0, {num}) of grids {tuple(grids.shape)}")
    H, W = int(rgb.shape[-3]), int(rgb.shape[-2])
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"{what}: an image of 1..{MAX_SIDE} rows and columns, got rgb {tuple(rgb.shape)}")
    _check_plain(what, rgb=rgb, grids=grids)
    require_gpu(rgb, grids)
    out = _Slice.apply(rgb.view(H, W, 3), grids, cam, (H, W, num, L, GH, GW))
    return out.view(rgb.shape)


class _TvLoss(torch.autograd.Function):
    """The TV loss as ONE autograd node: two launches forward (fp64 partial sums met in index order), one backward."""

    @staticmethod
    def forward(ctx, grids, geo):
        num, L, GH, GW = geo
        partials = torch.empty(3 * TV_BLOCKS, device=grids.device, dtype=torch.float64)
        loss = torch.empty((), device=grids.device, dtype=torch.float32)
        run("misplat_bilagrid_tv_fwd", ptr(grids), num, GW, GH, L, ptr(partials), ptr(loss))
        ctx.save_for_backward(grids)
        ctx.geo = geo
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        (grids,) = ctx.saved_tensors
        num, L, GH, GW = ctx.geo
        g = g.to(torch.float32).contiguous()
        v_grids = torch.empty_like(grids)
        run("misplat_bilagrid_tv_bwd", ptr(grids), num, GW, GH, L, ptr(g), ptr(v_grids))
        return v_grids, None


def bilagrid_tv_loss(grids: Tensor) -> Tensor:
    """The total variation of ALL cameras' grids as a device scalar with a gradient [UNVERIFIED-UPSTREAM]:

        tv = (1 / num) * sum over the axes L, GH, GW of sum (G[i + 1] - G[i])^2 / count_axis

    with ``count_axis`` = 12 (n_axis - 1) (the other two sizes), the number of differences of one camera along that axis; an
    axis of size 1 adds 0.  The model's ``tv_loss`` is 10 times this."""
    geo = _check_grids(grids, "bilagrid_tv_loss")
    _check_plain("bilagrid_tv_loss", grids=grids)
    require_gpu(grids)
    return _TvLoss.apply(grids, geo)
