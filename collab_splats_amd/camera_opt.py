"""``CameraOptimizer`` -- a learned per-training-camera pose refinement (the ``camera_opt`` optimizer group of the reference's
method configs: configs/rade_gs_method.py:72-77, rade_features_method.py:83).

[UNVERIFIED-UPSTREAM] nerfstudio is not vendored with the reference and is absent here: this restates its published
``CameraOptimizer`` (``nerfstudio/cameras/camera_optimizers.py``) -- modes ``off`` / ``SO3xR3`` / ``SE3``, the parameter
``pose_adjustment [num_cameras, 6]`` (translation, then rotation vector), ``apply_to_camera`` as a right multiplication of the
OpenGL camera-to-world matrix, the L2 regulariser and the two metrics -- from its public description.  Parity with
nerfstudio's code is unpinned; what IS pinned (tests/test_camera_opt_host.py) is the mathematics: the exponential maps and
their Jacobians against closed forms / ``torch.linalg.matrix_exp``, and the composition against ``torch.linalg.inv``.

Pure torch (a handful of 4x4 operations per step: plumbing, not a hot path); runs on CPU and GPU.  The gradient that reaches
``pose_adjustment`` comes from the rasterizer's ``viewmats`` gradient (csrc/project.hip: project_bwd_pose_kernel).
"""
from __future__ import annotations

from typing import Dict, List, Union

import torch
from torch import Tensor, nn

MODES = ("off", "SO3xR3", "SE3")

# Below theta^2 = _SERIES_T the coefficients come from their Taylor series in t = theta^2 -- a polynomial in the components of
# omega, so value and every derivative are finite and exact at omega = 0 (where training starts); 10 terms leave a
# truncation below 1e-20 there.  Above it the closed forms are well conditioned.
_SERIES_T = 0.25
_N_TERMS = 10


def _series(t: Tensor, first: int) -> Tensor:
    """sum_k (-t)^k / (2k + first)!  -- first = 1: sin(th)/th, 2: (1 - cos th)/th^2, 3: (th - sin th)/th^3, t = th^2."""
    import math
    out = torch.zeros_like(t)
    for k in reversed(range(_N_TERMS)):
        out = out * (-t) + 1.0 / math.factorial(2 * k + first)
    return out


def _coefficients(omega: Tensor):
    """A = sin(th)/th, B = (1 - cos th)/th^2, C = (th - sin th)/th^3 for th = |omega|; [n] each."""
    t = (omega * omega).sum(-1)
    small = t < _SERIES_T
    ts = torch.where(small, t, torch.zeros_like(t))            # the series sees t where it is used, 0 elsewhere
    tl = torch.where(small, torch.ones_like(t), t)             # the closed forms never see a theta near 0
    th = torch.sqrt(tl)
    half = torch.sin(0.5 * th) / (0.5 * th)
    A = torch.where(small, _series(ts, 1), torch.sin(th) / th)
    B = torch.where(small, _series(ts, 2), 0.5 * half * half)  # (1 - cos) = 2 sin^2(th / 2): no cancellation
    C = torch.where(small, _series(ts, 3), (th - torch.sin(th)) / (tl * th))
    return A, B, C


def _hat(omega: Tensor) -> Tensor:
    x, y, z = omega.unbind(-1)
    o = torch.zeros_like(x)
    return torch.stack([o, -z, y, z, o, -x, -y, x, o], dim=-1).reshape(omega.shape[:-1] + (3, 3))


def exp_map_SO3xR3(tangent: Tensor) -> Tensor:
    """[n,6] (tau, omega) -> [n,3,4] = [exp(omega^) | tau]."""
    tau, omega = tangent[..., :3], tangent[..., 3:]
    A, B, _ = _coefficients(omega)
    K = _hat(omega)
    eye = torch.eye(3, dtype=tangent.dtype, device=tangent.device)
    R = eye + A[..., None, None] * K + B[..., None, None] * (K @ K)
    return torch.cat((R, tau[..., :, None]), dim=-1)


def exp_map_SE3(tangent: Tensor) -> Tensor:
    """[n,6] twist (tau, omega) -> [n,3,4] = the top rows of exp([[omega^, tau], [0, 0]]) = [R | V tau]."""
    tau, omega = tangent[..., :3], tangent[..., 3:]
    A, B, Cc = _coefficients(omega)
    K = _hat(omega)
    K2 = K @ K
    eye = torch.eye(3, dtype=tangent.dtype, device=tangent.device)
    R = eye + A[..., None, None] * K + B[..., None, None] * K2
    V = eye + B[..., None, None] * K + Cc[..., None, None] * K2
    return torch.cat((R, V @ tau[..., :, None]), dim=-1)


class CameraOptimizer(nn.Module):
    """``pose_adjustment [num_cameras, 6]`` (zeros at the start; absent in mode ``off``) and what Splatfacto does with it."""

    def __init__(self, num_cameras: int, mode: str = "off", trans_l2_penalty: float = 1e-2, rot_l2_penalty: float = 1e-3):
        super().__init__()
        if mode not in MODES:
            raise ValueError(f"CameraOptimizer: mode must be one of {MODES}, got {mode!r}")
        if mode != "off" and int(num_cameras) < 1:
            raise ValueError(f"CameraOptimizer: mode {mode!r} needs num_cameras >= 1, got {num_cameras}")
        self.num_cameras, self.mode = int(num_cameras), mode
        self.trans_l2_penalty, self.rot_l2_penalty = float(trans_l2_penalty), float(rot_l2_penalty)
        if mode != "off":
            # (the name is nerfstudio's: a checkpoint's ``camera_optimizer.pose_adjustment`` loads unchanged)
            self.pose_adjustment = nn.Parameter(torch.zeros(self.num_cameras, 6))

    def forward(self, indices: Union[Tensor, int, List[int]]) -> Tensor:
        """The adjustment matrices [n,3,4] of the cameras ``indices``."""
        if self.mode == "off":
            n = len(indices) if hasattr(indices, "__len__") else (indices.numel() if isinstance(indices, Tensor) else 1)
            return torch.eye(4)[None, :3, :4].repeat(n, 1, 1)
        idx = torch.as_tensor(indices, dtype=torch.long, device=self.pose_adjustment.device).reshape(-1)
        tangent = self.pose_adjustment[idx]
        return exp_map_SO3xR3(tangent) if self.mode == "SO3xR3" else exp_map_SE3(tangent)

    def apply_to_c2w(self, c2w: Tensor, cam_idx) -> Tensor:
        """``c2w [n,3,4]`` (OpenGL camera-to-world) -> ``c2w . adj``: the refinement acts in the camera's own frame."""
        if self.mode == "off":
            return c2w
        adj = self(cam_idx).to(c2w.dtype)
        R, t = c2w[..., :3, :3], c2w[..., :3, 3:]
        return torch.cat((R @ adj[..., :3, :3], R @ adj[..., :3, 3:] + t), dim=-1)

    def apply_to_viewmat(self, viewmats: Tensor, cam_idx) -> Tensor:
        """The same refinement on the OpenCV world-to-camera matrix ``viewmats [n,4,4]`` that ``camera_parameters()``
        produces: V = F inv(c2w), so V' = F inv(c2w . adj) = F adj^-1 F V with F = diag(1,-1,-1,1) and
        adj^-1 = [R^T | -R^T tau]."""
        if self.mode == "off":
            return viewmats
        adj = self(cam_idx).to(viewmats.dtype)
        Rt = adj[..., :3, :3].transpose(-1, -2)
        f = torch.tensor([1.0, -1.0, -1.0], dtype=viewmats.dtype, device=viewmats.device)
        Ra = f[:, None] * Rt * f[None, :]                                   # F3 R^T F3
        ta = -(f[:, None] * (Rt @ adj[..., :3, 3:]))                        # -F3 R^T tau
        top = torch.cat((Ra @ viewmats[..., :3, :3], Ra @ viewmats[..., :3, 3:] + ta), dim=-1)
        return torch.cat((top, viewmats[..., 3:, :]), dim=-2)

    def get_loss_dict(self, loss_dict: Dict[str, Tensor]) -> None:
        if self.mode != "off":
            loss_dict["camera_opt_regularizer"] = (
                self.pose_adjustment[:, :3].norm(dim=-1).mean() * self.trans_l2_penalty
                + self.pose_adjustment[:, 3:].norm(dim=-1).mean() * self.rot_l2_penalty)

    def get_metrics_dict(self, metrics_dict: Dict[str, Tensor]) -> None:
        if self.mode != "off":
            metrics_dict["camera_opt_translation"] = self.pose_adjustment[:, :3].detach().norm()
            metrics_dict["camera_opt_rotation"] = self.pose_adjustment[:, 3:].detach().norm()

    def get_param_groups(self, param_groups: Dict[str, List[nn.Parameter]]) -> None:
        if self.mode != "off":
            param_groups["camera_opt"] = list(self.parameters())
