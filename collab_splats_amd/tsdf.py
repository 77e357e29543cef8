"""TSDF fusion of depth maps and marching-cubes mesh extraction on the MI355X (csrc/tsdf.hip).

``TSDFVolume`` restates Open3D's legacy ``ScalableTSDFVolume`` (what the reference's ``Open3DTSDFFusion`` integrates into,
collab_splats/utils/mesh.py:1473-1630) in fp32: units of 16^3 voxels allocated per view from the depth samples, each view
updating only the units it touches, and ``extract_triangle_mesh`` as a deterministic marching cubes.  Everything stays on
the device; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from ._lib import MisplatError, check, load, ptr, require_gpu, run, stream_ptr  # noqa: F401
from .unitvolume import (MAX_UNITS, UNIT, UNIT_VOXELS, Grid, GrowingVolume, _unit_range, empty_mesh, make_grid,  # noqa: F401
                         map_span, marching_cubes, unit_coords)

MAX_VIEWS = 64                       # views per kernel batch (bits of a unit's view word)


class TSDFVolume(GrowingVolume):
    """Scalable TSDF volume on the GPU.

    ``voxel_size`` / ``sdf_trunc`` / ``depth_trunc`` as Open3D's ``ScalableTSDFVolume(voxel_length, sdf_trunc)`` and
    ``create_from_color_and_depth(depth_trunc, depth_scale=1)``.  ``bounds`` (optional, ``[[xmin, ymin, zmin], [xmax, ymax,
    zmax]]``): units that do not overlap the box are never allocated.  The dense unit map otherwise covers the views' frusta
    cut at ``depth_trunc`` (padded by ``sdf_trunc``) and grows with them; more than ``max_units`` units raise ``MisplatError``.
    """

    _name, _what = "TSDFVolume", "the views' frusta"
    _advice = "pass bounds=, a smaller depth_trunc or a larger voxel_size"

    def __init__(self, voxel_size: float, sdf_trunc: float, depth_trunc: float = 3.0, bounds=None,
                 device=None, max_units: int = MAX_UNITS):
        if not (voxel_size > 0 and sdf_trunc > 0 and depth_trunc > 0):
            raise ValueError("TSDFVolume: voxel_size, sdf_trunc and depth_trunc must be positive")
        super().__init__(voxel_size, device, max_units)
        self.sdf_trunc, self.depth_trunc = float(sdf_trunc), float(depth_trunc)
        if bounds is not None:
            b = np.asarray(bounds, np.float64).reshape(2, 3)
            if not np.all(b[1] >= b[0]):
                raise ValueError("TSDFVolume: bounds must be [[min xyz], [max xyz]]")
            self.clip = _unit_range(b[0], b[1], self.ulen)
        self.n_views = 0
        self._pool = None

    # ------------------------------------------------------------------------------------------------------------ plumbing
    def _grid(self) -> Grid:
        return make_grid(self.voxel_size, self.sdf_trunc, self.depth_trunc, self.lo, self.dims)

    def _frusta_units(self, viewmats: Tensor, Ks: Tensor, H: int, W: int) -> Tuple[np.ndarray, np.ndarray]:
        """Units overlapping the AABB of the views' frusta cut at depth_trunc, padded by sdf_trunc (one host read)."""
        vm, K = viewmats.double(), Ks.double()
        R, t = vm[:, :3, :3], vm[:, :3, 3]
        D = self.depth_trunc
        uv = torch.tensor([[0.0, 0.0], [W, 0.0], [0.0, H], [W, H]], dtype=torch.float64, device=vm.device)
        x = (uv[None, :, 0] - K[:, None, 0, 2]) * D / K[:, None, 0, 0]
        y = (uv[None, :, 1] - K[:, None, 1, 2]) * D / K[:, None, 1, 1]
        pc = torch.stack([x, y, torch.full_like(x, D)], -1)                        # [V,4,3] camera space
        pc = torch.cat([pc, torch.zeros_like(pc[:, :1])], 1)                        # + the camera centre
        pw = torch.einsum("vji,vkj->vki", R, pc - t[:, None, :])                    # R^T (p - t)
        box = torch.stack([pw.amin((0, 1)), pw.amax((0, 1))]).cpu().numpy()
        if not np.all(np.isfinite(box)):
            raise ValueError("TSDFVolume.integrate: non-finite camera parameters")
        lo, hi = _unit_range(box[0] - self.sdf_trunc, box[1] + self.sdf_trunc, self.ulen)
        return lo - 1, hi + 1

    def _grow_pool(self, n: int) -> None:
        cap = 0 if self._pool is None else self._pool.shape[0]
        if n <= cap:
            return
        new = torch.zeros((max(n, cap + cap // 2, 64), 5, UNIT_VOXELS), dtype=torch.float32, device=self.device)
        if self.n_units:
            new[:self.n_units] = self._pool[:self.n_units]
        self._pool = new

    # ------------------------------------------------------------------------------------------------------------ public
    def integrate(self, depths: Tensor, viewmats: Tensor, Ks: Tensor, rgbs: Optional[Tensor] = None,
                  masks: Optional[Tensor] = None) -> None:
        """Integrate V views in order (after every view integrated before).  depths [V,H,W,1] (or [V,H,W]) fp32, metres along
        the optical axis; viewmats [V,4,4] world->camera (OpenCV axes, the rasterizer's); Ks [V,3,3]; rgbs [V,H,W,3] in
        [0,1] (colour uint8(rgb * 255)) or None (black); masks [V,H,W(,1)] bool or None (False: no data)."""
        if depths.dim() == 4 and depths.shape[-1] == 1:
            depths = depths.squeeze(-1)
        if depths.dim() != 3 or depths.shape[0] < 1 or depths.shape[1] < 1 or depths.shape[2] < 1:
            raise ValueError(f"TSDFVolume.integrate: depths must be [V,H,W,1], got {tuple(depths.shape)}")
        V, H, W = depths.shape
        if tuple(viewmats.shape) != (V, 4, 4) or tuple(Ks.shape) != (V, 3, 3):
            raise ValueError(f"TSDFVolume.integrate: viewmats [V,4,4] and Ks [V,3,3] expected for V={V}, got "
                             f"{tuple(viewmats.shape)} and {tuple(Ks.shape)}")
        if rgbs is not None and tuple(rgbs.shape) != (V, H, W, 3):
            raise ValueError(f"TSDFVolume.integrate: rgbs must be [{V},{H},{W},3], got {tuple(rgbs.shape)}")
        if masks is not None:
            if masks.dim() == 4 and masks.shape[-1] == 1:
                masks = masks.squeeze(-1)
            if tuple(masks.shape) != (V, H, W):
                raise ValueError(f"TSDFVolume.integrate: masks must be [{V},{H},{W}(,1)], got {tuple(masks.shape)}")
        require_gpu(depths, viewmats, Ks, rgbs, masks)
        self._adopt_device(depths)
        depths = depths.to(torch.float32).contiguous()
        viewmats = viewmats.to(torch.float32).contiguous()
        Ks = Ks.to(torch.float32).contiguous()
        rgbs = rgbs.to(torch.float32).contiguous() if rgbs is not None else None
        masks = masks.to(torch.uint8).contiguous() if masks is not None else None
        if not self._cover(*self._frusta_units(viewmats, Ks, H, W)):
            self.n_views += V                      # every view lies outside the bounds: nothing to update
            return
        grid = self._grid()
        for b in range(0, V, MAX_VIEWS):
            n = min(MAX_VIEWS, V - b)
            d, vm, k = depths[b:b + n], viewmats[b:b + n], Ks[b:b + n]
            c = rgbs[b:b + n] if rgbs is not None else None
            mk = masks[b:b + n] if masks is not None else None
            self._begin_batch()
            run("misplat_tsdf_mark", C.byref(grid), ptr(d), ptr(mk), n, H, W, ptr(vm), ptr(k), ptr(self._words))
            n_units, n_touched = self._alloc(grid)                               # the batch's one host read
            if n_touched == 0:
                continue
            self._grow_pool(n_units)
            self.n_units = n_units
            run("misplat_tsdf_integrate", C.byref(grid), ptr(self._touched), n_touched, ptr(self._words), ptr(d), ptr(mk),
                ptr(c), n, H, W, ptr(vm), ptr(k), ptr(self._pool))
        self.n_views += V

    def extract_mesh(self) -> Tuple[Tensor, Tensor, Tensor]:
        """Marching cubes over the allocated voxels: (vertices [M,3] fp32, triangles [T,3] int32, colors [M,3] fp32 in [0,1]),
        on the device, in the deterministic order of DESIGN.md section 14 (two host reads: nothing else)."""
        mesh = marching_cubes(self._grid(), self._slot_map, self.n_units, self._pool) if self.n_units else None
        return mesh or empty_mesh(self.device)

    def units(self):
        """The allocated units in map order, on the host (for tests and inspection): (coords [n,3] int64, tsdf [n,4096],
        weight [n,4096], rgb [n,4096,3]); voxel i = lx + 16 ly + 256 lz."""
        if self.n_units == 0:
            z = np.zeros((0, UNIT_VOXELS), np.float32)
            return np.zeros((0, 3), np.int64), z, z, np.zeros((0, UNIT_VOXELS, 3), np.float32)
        m = self._map_order()
        slots = self._slot_map[m].long()
        data = self._pool[slots].cpu().numpy()
        coords = unit_coords(m.cpu().numpy(), self.lo, self.dims)
        return coords, data[:, 0], data[:, 1], np.ascontiguousarray(data[:, 2:5].transpose(0, 2, 1))


def write_ply(path: str, vertices, triangles, colors=None, normals=None) -> None:
    """Binary little-endian PLY: float x y z, float nx ny nz (only if ``normals`` are given), uchar red green blue
    (round(255 colour)), int32 faces.  No Open3D needed."""
    def host(x):
        return np.asarray(x.detach().cpu() if isinstance(x, Tensor) else x, np.float32)

    v = host(vertices).reshape(-1, 3)
    f = np.asarray(triangles.detach().cpu() if isinstance(triangles, Tensor) else triangles, np.int32).reshape(-1, 3)
    if colors is None:
        c = np.zeros_like(v)
    else:
        c = host(colors).reshape(-1, 3)
    if c.shape != v.shape:
        raise ValueError("write_ply: colors must match vertices")
    n = None if normals is None else host(normals).reshape(-1, 3)
    if n is not None and n.shape != v.shape:
        raise ValueError("write_ply: normals must match vertices")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if n is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    vrec = np.empty(len(v), dtype=fields + [("r", "u1"), ("g", "u1"), ("b", "u1")])
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if n is not None:
        vrec["nx"], vrec["ny"], vrec["nz"] = n[:, 0], n[:, 1], n[:, 2]
    cu = np.round(np.clip(c, 0.0, 1.0) * 255.0).astype(np.uint8)
    vrec["r"], vrec["g"], vrec["b"] = cu[:, 0], cu[:, 1], cu[:, 2]
    frec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    frec["n"] = 3
    frec["i"] = f
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              + ("property float nx\nproperty float ny\nproperty float nz\n" if n is not None else "")
              + "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def obb_bounds(obb, pad: float = 0.0):
    """World AABB ``[[min], [max]]`` of an oriented box with nerfstudio ``OrientedBox`` fields ``R`` [3,3], ``T`` [3] and
    ``S`` [3] (full side lengths), padded by ``pad``; None if the object has no such fields."""
    if obb is None or not all(hasattr(obb, k) for k in ("R", "T", "S")):
        return None
    R = np.asarray(torch.as_tensor(obb.R).detach().double().cpu()).reshape(3, 3)
    T = np.asarray(torch.as_tensor(obb.T).detach().double().cpu()).reshape(3)
    S = np.asarray(torch.as_tensor(obb.S).detach().double().cpu()).reshape(3)
    half = np.abs(R) @ (S / 2.0)
    return np.stack([T - half - pad, T + half + pad])


def camera_frame(camera) -> Tuple[Tensor, Tensor]:
    """fp32 (viewmat [4,4], K [3,3]) the reference hands to Open3D for one view (mesh.py:1591-1604):
    ``inv(c2w @ diag(1,-1,-1,1))`` in float64, and the camera's own intrinsics (fx, fy, cx, cy)."""
    c2w = torch.eye(4, dtype=torch.float64)
    c2w[:3, :4] = camera.camera_to_worlds.reshape(-1, 3, 4)[0].detach().double().cpu()
    c2w = c2w @ torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=torch.float64))
    K = camera.get_intrinsics_matrices().reshape(-1, 3, 3)[0].detach().double().cpu()
    return torch.linalg.inv(c2w).float(), K.float()


__all__ = ["TSDFVolume", "write_ply", "obb_bounds", "camera_frame", "Grid", "MAX_VIEWS", "MAX_UNITS"]
