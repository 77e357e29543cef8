"""Host-side mirror of the reference's RaDe-GS model path around the rasterizer.

Reproduces, with the reference's names, argument meaning and error behaviour:
  a1  ``RadegsModel._get_camera_parameters`` + ``convert_to_colmap_camera``
      (/root/reference/collab_splats/models/rade_gs_model.py:311-346, utils/camera_utils.py:74-135)
  a3  ``RadegsModel.get_outputs`` post-processing (rade_gs_model.py:200-272)
  a4  ``depth_double_to_normal`` (camera_utils.py:176-279) -- one fused HIP stencil kernel
  a5  ``RadegsModel.get_loss_dict`` depth-normal term (rade_gs_model.py:289-307)
  a6  ``RadegsModel.normals`` / ``build_rotation`` (rade_gs_model.py:65-78, camera_utils.py:138-168)
  a7  ``RadegsModel._prefilter_voxel`` (rade_gs_model.py:348-399)
The reference's Python does not travel to the GPU box and depends on nerfstudio (absent), so this
module is the build's own counterpart; nerfstudio's ``Cameras`` is duck-typed (only
``camera_to_worlds``, ``width``, ``height``, ``get_intrinsics_matrices()``, ``shape`` are touched by
the reference: camera_utils.py:76-88, rade_gs_model.py:94-95, 135).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import ops
from ._lib import MisplatError, make_params
from .rendering import rasterization
from .strategy import DefaultStrategy


# ----------------------------------------------------------------------------- cameras (a1)

@dataclass
class PinholeCamera:
    """Duck-type of the nerfstudio ``Cameras`` attributes the reference touches."""
    camera_to_worlds: Tensor          # [1, 3, 4], OpenGL axes (nerfstudio convention)
    fx: float
    fy: float
    cx: float
    cy: float
    width: Tensor                     # [[W]]
    height: Tensor                    # [[H]]
    metadata: Optional[dict] = None

    @classmethod
    def make(cls, camera_to_worlds: Tensor, fx: float, fy: float, width: int, height: int,
             cx: Optional[float] = None, cy: Optional[float] = None) -> "PinholeCamera":
        c2w = camera_to_worlds.reshape(1, 3, 4)
        return cls(c2w, float(fx), float(fy), width / 2.0 if cx is None else float(cx),
                   height / 2.0 if cy is None else float(cy), torch.tensor([[int(width)]]),
                   torch.tensor([[int(height)]]))

    @property
    def shape(self):
        return (self.camera_to_worlds.shape[0],)

    def get_intrinsics_matrices(self) -> Tensor:
        K = torch.tensor([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]])
        return K[None].to(self.camera_to_worlds.device)

    def rescale_output_resolution(self, scale: float) -> None:
        if scale == 1 or scale == 1.0:
            return
        self.fx *= scale; self.fy *= scale; self.cx *= scale; self.cy *= scale
        self.width = (self.width * scale).to(torch.int64)
        self.height = (self.height * scale).to(torch.int64)


def focal2fov(focal: float, pixels: float) -> float:
    """camera_utils.py:134-135."""
    return 2 * math.atan(pixels / (2 * focal))


# Small host->device transfers without a hidden synchronisation: ``torch.tensor(..., device=cuda)`` and ``.to(cuda)`` of
# pageable memory block the host until the copy has run, i.e. until everything queued before it on the stream -- the
# whole previous step -- has finished, and the GPU then idles through this step's host work (measured: 0.36 ms per 1 M
# model step).  Camera data therefore travels as ONE asynchronous copy from a ring of pinned buffers, and constants
# are cached per device.
_PIN_RING: Dict[torch.device, list] = {}
_DEV_CONST: Dict[tuple, Tensor] = {}


def _upload(values: Tensor, device: torch.device) -> Tensor:
    """float32 CPU tensor (flat) -> device, asynchronously, through a ring of pinned staging buffers."""
    if device.type != "cuda":
        return values.to(device)
    ring = _PIN_RING.get(device)
    if ring is None:                                      # (not setdefault: its default would be built -- 32 pinned allocations -- on every call)
        ring = _PIN_RING[device] = [0, [torch.empty(64, dtype=torch.float32).pin_memory() for _ in range(32)], [None] * 32]
    ring[0] = (ring[0] + 1) % len(ring[1])
    ev = ring[2][ring[0]]
    if ev is not None:
        ev.synchronize()                                  # the copy that last used this slot (32 uploads ago) has long run
    buf = ring[1][ring[0]][:values.numel()]
    buf.copy_(values)
    out = buf.to(device, non_blocking=True)
    if not torch.cuda.is_current_stream_capturing():
        ev = ring[2][ring[0]] or torch.cuda.Event()
        ev.record()
        ring[2][ring[0]] = ev
    return out


def _device_const(key: tuple, device: torch.device, make) -> Tensor:
    k = (key, device)
    t = _DEV_CONST.get(k)
    if t is None:
        t = _DEV_CONST[k] = make().to(device)
    return t


def camera_parameters(camera, device: Optional[torch.device] = None) -> Dict[str, Union[Tensor, int, float]]:
    """``_get_camera_parameters`` (rade_gs_model.py:311-346) without the reference's host syncs.

    nerfstudio c2w (OpenGL) -> OpenCV world->camera: flip the y/z camera axes (camera_utils.py:79),
    invert (for the rigid c2w the inverse is [R^T | -R^T t], which is what ``torch.linalg.inv``
    returns up to rounding; :82-84, 94-105), rebuild ``Ks`` from the field of view with the
    principal point FORCED to the image centre (rade_gs_model.py:322-334).
    """
    c2w = camera.camera_to_worlds[0].to(torch.float32)                  # [3,4]
    device = torch.device(device) if device is not None else c2w.device
    W, H = int(camera.width.item()), int(camera.height.item())
    if isinstance(getattr(camera, "fx", None), float) and isinstance(getattr(camera, "fy", None), float):
        fx_in, fy_in = camera.fx, camera.fy                               # host floats: no intrinsics matrix round trip
    else:
        K = camera.get_intrinsics_matrices()
        fx_in, fy_in = float(K[0, 0, 0]), float(K[0, 1, 1])
    fovx = focal2fov(fx_in, W)
    fovy = focal2fov(fy_in, H)
    fx = W / (2 * math.tan(fovx * 0.5))
    fy = H / (2 * math.tan(fovy * 0.5))
    if c2w.device.type == "cpu":
        # 4x4 arithmetic on the host, one asynchronous upload of viewmat (16) + Ks (9) + camera centre (3)
        Rw = (c2w[:3, :3] * torch.tensor([1.0, -1.0, -1.0])).transpose(0, 1)
        t = -(Rw @ c2w[:3, 3])
        pack = torch.zeros(28, dtype=torch.float32)
        vm = pack[:16].view(4, 4)
        vm[:3, :3] = Rw
        vm[:3, 3] = t
        vm[3, 3] = 1.0
        pack[16], pack[18], pack[20], pack[21], pack[24] = fx, W / 2.0, fy, H / 2.0, 1.0
        pack[25:28] = c2w[:3, 3]
        d = _upload(pack, device)
        return {"Ks": d[16:25].view(1, 3, 3), "viewmats": d[:16].view(1, 4, 4), "image_width": W, "image_height": H,
                "camera_center": d[25:28], "fx": fx, "fy": fy}
    flip = _device_const(("flip",), c2w.device, lambda: torch.tensor([1.0, -1.0, -1.0], dtype=torch.float32))
    Rc = c2w[:3, :3] * flip[None, :]                                      # c2w[:3, 1:3] *= -1
    Rw = Rc.transpose(0, 1)
    t = -(Rw @ c2w[:3, 3])
    viewmat = _device_const(("eye4",), c2w.device, lambda: torch.eye(4, dtype=torch.float32)).clone()
    viewmat[:3, :3] = Rw
    viewmat[:3, 3] = t
    Ks = _device_const(("Ks", fx, fy, W, H), device,
                       lambda: torch.tensor([[[fx, 0.0, W / 2.0], [0.0, fy, H / 2.0], [0.0, 0.0, 1.0]]], dtype=torch.float32))
    return {"Ks": Ks, "viewmats": viewmat[None].to(device), "image_width": W,
            "image_height": H, "camera_center": c2w[:3, 3].to(device), "fx": fx, "fy": fy}


def tsdf_frame(camera):
    """Extrinsic / intrinsic pair the reference hands to Open3D's TSDF integration for one view
    (mesh.py:1591-1604, 1626-1630): ``extrinsic = inv(c2w @ diag(1,-1,-1,1))`` (OpenGL -> OpenCV, world -> camera,
    float64 numpy) and ``dict(width, height, fx, fy, cx, cy)`` for ``o3d.camera.PinholeCameraIntrinsic``."""
    import numpy as np
    c2w = torch.eye(4, dtype=torch.float64)
    c2w[:3, :4] = camera.camera_to_worlds.reshape(-1, 3, 4)[0].detach().double().cpu()
    c2w = c2w @ torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=torch.float64))
    K = camera.get_intrinsics_matrices().reshape(-1, 3, 3)[0].detach().double().cpu()
    intr = dict(width=int(camera.width.item()), height=int(camera.height.item()), fx=float(K[0, 0]), fy=float(K[1, 1]),
                cx=float(K[0, 2]), cy=float(K[1, 2]))
    return np.linalg.inv(c2w.numpy()), intr


def build_rotation(quats: Tensor) -> Tensor:
    """wxyz -> [N,3,3]; normalised inside (camera_utils.py:138-168)."""
    q = quats / torch.sqrt((quats * quats).sum(dim=-1, keepdim=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=-1)
    return R.reshape(-1, 3, 3)


def depth_double_to_normal(camera_or_params, depth1: Tensor, depth2: Tensor) -> Tensor:
    """camera_utils.py:176-188: two z-depth maps [1,H,W,1] -> normals [2,H,W,3] (HIP stencil)."""
    cp = camera_or_params if isinstance(camera_or_params, dict) else camera_parameters(camera_or_params)
    H, W = cp["image_height"], cp["image_width"]
    zeros = torch.zeros(H, W, 3, device=depth1.device, dtype=torch.float32)
    normals2, _ = ops.depth_normal(depth1.reshape(H, W), depth2.reshape(H, W), zeros, cp["fx"], cp["fy"])
    return normals2


# ----------------------------------------------------------------------------- model

@dataclass
class RadegsModelConfig:
    """The hot-path fields of the reference's config (rade_gs_model.py:29-55 + the Splatfacto
    fields ``get_outputs`` reads)."""
    regularization_from_iter: int = 15000
    use_depth_normal_loss: bool = True
    depth_normal_lambda: float = 0.05
    depth_ratio: float = 0.6
    render_mode: str = "RGB"
    prefilter_voxel: bool = False
    sh_degree: int = 3
    sh_degree_interval: int = 1000
    rasterize_mode: str = "classic"
    output_depth_during_training: bool = False
    background_color: str = "black"
    absgrad: bool = False
    # Splatfacto's image loss [UNVERIFIED-UPSTREAM]: main_loss = (1 - ssim_lambda) L1 + ssim_lambda (1 - SSIM); scale
    # regularisation (PhysGaussian) off by default, applied every 10th step when on
    ssim_lambda: float = 0.2
    use_scale_regularization: bool = False
    max_gauss_ratio: float = 10.0
    # Splatfacto's training-time resolution schedule [UNVERIFIED-UPSTREAM]: the camera is rendered at 1 / 2^k of its
    # resolution, k = max(num_downscales - step // resolution_schedule, 0) (rade_gs_model.py:132-133 rescales the camera by
    # the factor ``_get_downscale_factor()`` returns and back, :223)
    num_downscales: int = 0
    resolution_schedule: int = 3000
    # Splatfacto's per-camera bilateral grid [UNVERIFIED-UPSTREAM]: a learned affine colour transform per training camera,
    # applied to the training render (rade_gs_model.py:231-234), with its TV loss (:284-289); grid_shape = (GW, GH, L)
    use_bilateral_grid: bool = False
    grid_shape: Tuple[int, int, int] = (16, 16, 8)
    # Splatfacto's camera optimizer [UNVERIFIED-UPSTREAM] (the ``camera_opt`` group of configs/rade_gs_method.py:72-77): a
    # learned pose refinement per training camera, "off" | "SO3xR3" | "SE3" (camera_opt.py), applied to the training
    # camera's view matrix; the rasterizer's viewmats gradient trains it
    camera_optimizer_mode: str = "off"
    camera_opt_trans_l2_penalty: float = 1e-2
    camera_opt_rot_l2_penalty: float = 1e-3
    # Splatfacto's ``color_corrected_metrics`` [UNVERIFIED-UPSTREAM]: evaluation also reports cc_psnr / cc_ssim, the scores of
    # the render after ``metrics.color_correct`` has warped it onto the ground truth's colours (what a model trained with
    # ``use_bilateral_grid`` is judged by: no grid applies to a held-out view)
    color_corrected_metrics: bool = False
    # Splatfacto's ``strategy`` field and its MCMC settings [UNVERIFIED-UPSTREAM]: "default" (adaptive density control,
    # strategy.DefaultStrategy) | "mcmc" (fixed budget ``cap_max``, mcmc.RelocationStrategy), with the two
    # regularisers the MCMC method trains under: mcmc_opacity_reg * mean(opacity) and mcmc_scale_reg * mean(scale)
    strategy: str = "default"
    cap_max: int = 1_000_000
    noise_lr: float = 5e5
    mcmc_opacity_reg: float = 0.01
    mcmc_scale_reg: float = 0.01

    def __post_init__(self):
        if self.strategy not in ("default", "mcmc"):
            raise ValueError(f"RadegsModelConfig: strategy must be 'default' or 'mcmc', got {self.strategy!r}")


class RadegsModel(nn.Module):
    """Gaussian parameters + the reference's ``get_outputs`` / ``get_loss_dict`` for the hot path.

    Parameter names match the reference's ``gauss_params`` (rade_gs_model.py:110-122) so a
    ``state_dict`` of those six tensors loads unchanged.
    """

    def __init__(self, config: RadegsModelConfig, means: Tensor, scales: Tensor, quats: Tensor,
                 opacities: Tensor, features_dc: Tensor, features_rest: Tensor, num_train_data: int = 0):
        super().__init__()
        self.config = config
        if config.use_bilateral_grid:
            # Splatfacto's ``bil_grids`` [UNVERIFIED-UPSTREAM]: one grid per training image (``num_train_data``)
            from .bilagrid import BilateralGrid
            if int(num_train_data) < 1:
                raise ValueError(f"RadegsModel: use_bilateral_grid needs num_train_data >= 1 (one grid per training camera), "
                                 f"got {num_train_data}")
            if len(config.grid_shape) != 3:
                raise ValueError(f"RadegsModel: grid_shape must be (GW, GH, L), got {tuple(config.grid_shape)}")
            self.bil_grids = BilateralGrid(int(num_train_data), *(int(v) for v in config.grid_shape))
        if config.camera_optimizer_mode != "off":
            # Splatfacto's ``camera_optimizer`` [UNVERIFIED-UPSTREAM]: one pose adjustment per training image
            from .camera_opt import CameraOptimizer
            if int(num_train_data) < 1:
                raise ValueError(f"RadegsModel: camera_optimizer_mode {config.camera_optimizer_mode!r} needs num_train_data >= 1 "
                                 f"(one pose adjustment per training camera), got {num_train_data}")
            self.camera_optimizer = CameraOptimizer(int(num_train_data), config.camera_optimizer_mode,
                                                    config.camera_opt_trans_l2_penalty, config.camera_opt_rot_l2_penalty)
        self.gauss_params = nn.ParameterDict({
            "means": nn.Parameter(means), "scales": nn.Parameter(scales), "quats": nn.Parameter(quats),
            "opacities": nn.Parameter(opacities.reshape(-1, 1)), "features_dc": nn.Parameter(features_dc),
            "features_rest": nn.Parameter(features_rest)})
        self.step = 0
        if config.strategy == "default":
            self.strategy = DefaultStrategy(absgrad=config.absgrad)
        elif config.strategy == "mcmc":
            from .mcmc import RelocationStrategy
            self.strategy = RelocationStrategy(cap_max=int(config.cap_max), noise_lr=float(config.noise_lr))
        else:
            raise ValueError(f"RadegsModel: strategy must be 'default' or 'mcmc', got {config.strategy!r}")
        self.strategy_state = self.strategy.initialize_state()
        self.optimizers: Dict = {}
        self.info: Dict = {}
        self.crop_box = None

    means = property(lambda self: self.gauss_params["means"])
    scales = property(lambda self: self.gauss_params["scales"])
    quats = property(lambda self: self.gauss_params["quats"])
    opacities = property(lambda self: self.gauss_params["opacities"])
    features_dc = property(lambda self: self.gauss_params["features_dc"])
    features_rest = property(lambda self: self.gauss_params["features_rest"])

    @property
    def device(self):
        return self.means.device

    @property
    def normals(self) -> Tensor:
        """rade_gs_model.py:65-78: world normal = rotation column of the smallest scale axis."""
        scales = torch.exp(self.scales)
        axis = F.one_hot(torch.argmin(scales, dim=-1), num_classes=3).float()
        rots = build_rotation(self.quats)
        return F.normalize(torch.bmm(rots, axis[:, :, None]).squeeze(-1), dim=1)

    def _background_list(self) -> List[float]:
        c = {"black": [0.0, 0.0, 0.0], "white": [1.0, 1.0, 1.0]}.get(self.config.background_color)
        if c is None:
            raise ValueError(f"Unknown background_color: {self.config.background_color}")
        return c

    def _get_background_color(self) -> Tensor:
        c = self._background_list()
        return _device_const(("background", tuple(c)), torch.device(self.device), lambda: torch.tensor(c, dtype=torch.float32))

    def _get_camera_parameters(self, camera) -> Dict:
        return camera_parameters(camera, self.device)

    def _get_downscale_factor(self) -> int:
        """Splatfacto's resolution schedule [UNVERIFIED-UPSTREAM]: 2^max(num_downscales - step // resolution_schedule, 0)
        while training, 1 in evaluation -- the factor rade_gs_model.py:132 asks for."""
        if self.training:
            return 2 ** max(self.config.num_downscales - self.step // max(self.config.resolution_schedule, 1), 0)
        return 1

    def _downscale_if_required(self, image: Tensor) -> Tensor:
        """Splatfacto's ``_downscale_if_required`` [UNVERIFIED-UPSTREAM]: while the resolution schedule renders at 1 / d, the
        ground truth is box-filtered by the same d (a d x d mean with stride d, nerfstudio's ``resize_image``), so that the
        image loss compares like with like -- a data manager hands out full-resolution images whatever the schedule says."""
        d = self._get_downscale_factor()
        if d <= 1:
            return image
        x = image.to(torch.float32).permute(2, 0, 1)[:, None]
        weight = torch.full((1, 1, d, d), 1.0 / (d * d), device=x.device, dtype=torch.float32)
        return torch.nn.functional.conv2d(x, weight, stride=d).squeeze(1).permute(1, 2, 0)

    def get_gt_img(self, image: Tensor) -> Tensor:
        """Splatfacto's ``get_gt_img`` [UNVERIFIED-UPSTREAM]: uint8 -> 0..1 floats, then the schedule's downscale."""
        if image.dtype == torch.uint8:
            image = image.to(torch.float32) / 255.0
        return self._downscale_if_required(image)

    def _prefilter_voxel(self, camera_params: Dict) -> Tensor:
        """rade_gs_model.py:348-399: visibility mask from projection radii."""
        from .wrapper import fully_fused_projection
        means, scales, quats = self.means, torch.exp(self.scales), self.quats
        N, Cn = means.shape[0], camera_params["viewmats"].shape[0]
        assert means.shape == (N, 3), means.shape
        assert quats.shape == (N, 4), quats.shape
        assert scales.shape == (N, 3), scales.shape
        assert camera_params["viewmats"].shape == (Cn, 4, 4), camera_params["viewmats"].shape
        assert camera_params["Ks"].shape == (Cn, 3, 3), camera_params["Ks"].shape
        radii = fully_fused_projection(means, None, quats, scales, camera_params["viewmats"],
                                       camera_params["Ks"], int(camera_params["image_width"]),
                                       int(camera_params["image_height"]), eps2d=0.3, packed=False,
                                       near_plane=0.01, far_plane=1e10, radius_clip=0.0,
                                       sparse_grad=False, calc_compensations=False)[0]
        return torch.sum(radii, dim=-1).squeeze() > 0

    def _features_for_render(self, pick):
        """[N,F] feature channels composited behind the colours, or None (the features model overrides this)."""
        return None

    def _render(self, means, quats, scales, opacities, colors, render_mode, sh_degree_to_use,
                camera_params, visible_mask=None, features=None):
        """rade_gs_model.py:401-467 (``features``: rade_features_model.py:390-478 -- SH colours and feature channels go to the
        rasterizer side by side, ``rasterization(..., features=...)``, instead of through spherical_harmonics / clamp / cat)."""
        if visible_mask is not None:
            means, quats, scales = means[visible_mask], quats[visible_mask], scales[visible_mask]
            opacities = opacities[visible_mask]
            colors = tuple(c[visible_mask] for c in colors) if isinstance(colors, tuple) else colors[visible_mask]
            features = features[visible_mask] if features is not None else None
        # (the activations of rade_gs_model.py:443-444 run inside the projection kernels: see rendering.rasterization)
        return rasterization(
            means=means, quats=quats, scales=scales, scales_are_log=True,
            opacities=opacities.squeeze(-1), opacities_are_logit=True, colors=colors,
            viewmats=camera_params["viewmats"], Ks=camera_params["Ks"],
            width=int(camera_params["image_width"]), height=int(camera_params["image_height"]),
            packed=False, near_plane=0.01, far_plane=1e10, render_mode=render_mode,
            sh_degree=sh_degree_to_use, sparse_grad=False,
            absgrad=self.strategy.absgrad if isinstance(self.strategy, DefaultStrategy) else False,
            rasterize_mode=self.config.rasterize_mode, return_depth_normal=True,
            **({"features": features} if features is not None and sh_degree_to_use is not None else {}))

    def get_outputs(self, camera) -> Dict[str, Union[Tensor, List, None]]:
        """rade_gs_model.py:80-272."""
        if not hasattr(camera, "camera_to_worlds"):
            print("Called get_outputs with not a camera")
            return {}
        if self.training:
            assert camera.shape[0] == 1, "Only one camera at a time"
        # cropping (rade_gs_model.py:96-119): evaluation only; an empty crop short-circuits to get_empty_outputs
        crop_ids = None
        if self.crop_box is not None and not self.training:
            crop_ids = self.crop_box.within(self.means).squeeze()
            if crop_ids.sum() == 0:
                return self.get_empty_outputs(int(camera.width.item()), int(camera.height.item()),
                                              self._get_background_color())
        pick = (lambda t: t[crop_ids]) if crop_ids is not None else (lambda t: t)
        # the reference concatenates the two colour parameters every step (rade_gs_model.py:128-130:
        # a 192 B/Gaussian copy + its backward split); the colour kernels read them in place instead
        colors_crop = (pick(self.features_dc), pick(self.features_rest))
        # rade_gs_model.py:132-136: the camera is rescaled by 1 / the schedule's factor for this call -- and back (:223).  The
        # reference undoes it in straight-line code, so an exception in between leaves the caller's camera shrunk (SURVEY
        # A.5); here the camera's intrinsics and size are restored exactly, whatever happens
        camera_scale_fac = self._get_downscale_factor()
        saved = None
        if camera_scale_fac != 1 and hasattr(camera, "rescale_output_resolution"):
            saved = {k: (v.clone() if isinstance(v, Tensor) else v) for k, v in
                     ((k, getattr(camera, k)) for k in ("fx", "fy", "cx", "cy", "width", "height") if hasattr(camera, k))}
            camera.rescale_output_resolution(1 / camera_scale_fac)
        try:
            W, H = int(camera.width.item()), int(camera.height.item())
            self.last_size = (H, W)
            camera_params = self._get_camera_parameters(camera)
            cam_meta = getattr(camera, "metadata", None)
            if (self.config.camera_optimizer_mode != "off" and self.training and cam_meta is not None
                    and "cam_idx" in cam_meta):
                # Splatfacto's ``camera_optimizer.apply_to_camera`` (the call the reference's get_outputs override dropped),
                # on the OpenCV view matrix: the training render sees the refined pose, evaluation the stored one
                vm = self.camera_optimizer.apply_to_viewmat(camera_params["viewmats"], int(cam_meta["cam_idx"]))
                camera_params = dict(camera_params, viewmats=vm,
                                     camera_center=-(vm[0, :3, :3].transpose(0, 1) @ vm[0, :3, 3]))
        finally:
            if saved is not None:
                for k, v in saved.items():
                    setattr(camera, k, v)
        voxel_visible_mask = self._prefilter_voxel(camera_params) if (self.config.prefilter_voxel and crop_ids is None) else None
        if self.config.rasterize_mode not in ["antialiased", "classic"]:
            raise ValueError("Unknown rasterize_mode: %s", self.config.rasterize_mode)
        render_mode = "RGB+ED" if (self.config.output_depth_during_training or not self.training) else "RGB"
        if self.config.sh_degree > 0:
            sh_degree_to_use = min(self.step // self.config.sh_degree_interval, self.config.sh_degree)
        else:
            colors_crop = torch.sigmoid(pick(self.features_dc))         # [N, 1, 3] -> [N, 3]  (:163)
            sh_degree_to_use = None

        feats = self._features_for_render(pick)
        if feats is not None and sh_degree_to_use is None:
            colors_crop, feats = torch.cat((colors_crop, feats), dim=-1), None      # (degree-0 model: sigmoid colours, pass-through)
        render, alpha, expected_depths, median_depths, expected_normals, self.info = self._render(
            means=pick(self.means), quats=pick(self.quats), scales=pick(self.scales), opacities=pick(self.opacities),
            colors=colors_crop, render_mode=render_mode, sh_degree_to_use=sh_degree_to_use,
            visible_mask=voxel_visible_mask, camera_params=camera_params, features=feats)
        feature_image = None
        n_feat = int(getattr(self.config, "features_latent_dim", 0))
        if n_feat > 0 and render.shape[-1] >= 3 + n_feat:
            # rade_features_model.py:360: features = render[..., 3 : 3 + latent_dim]; the colour (+ ED) channels go on to the
            # post-processing below.  (The reference takes depth_im from render[..., 3:4] there (:347) -- a feature channel; the
            # ED channel is the LAST one, which is what this mirror hands on.)
            feature_image = render[..., 3:3 + n_feat]
            render = (torch.cat((render[..., :3], render[..., 3 + n_feat:]), dim=-1) if render.shape[-1] > 3 + n_feat
                      else render[..., :3].contiguous())

        if self.training:
            self.strategy.step_pre_backward(self.gauss_params, self.optimizers, self.strategy_state,
                                            self.step, self.info)

        # a3 + a4: clamp / background / (n+1)/2 / where(alpha > 0, x, x.detach().max()) (rade_gs_model.py:221-254) and,
        # when the depth-normal loss is active, depth_double_to_normal + "1 - <n, n_depth>" (:206-214) -- one
        # autograd node, three kernels forward, two backward
        bg_list = self._background_list()
        background = self._get_background_color()
        want_depth_im = render_mode == "RGB+ED"
        if self.config.use_depth_normal_loss and self.step >= self.config.regularization_from_iter:
            ep = ops.get_outputs_epilogue(render, alpha, expected_depths, median_depths, expected_normals, bg_list,
                                          want_depth_im, camera_params["fx"], camera_params["fy"])
            rgb, expected_depths, median_depths, normals, normal_error_map = ep[0], ep[1], ep[2], ep[3], ep[4]
            depth_im = ep[5].squeeze(0) if want_depth_im else None
        else:
            # the reference builds zeros(2, 1, H) here (rade_gs_model.py:217-219); the
            # entries are unused under the same condition -- emit the intended [2, H, W]
            normal_error_map = torch.zeros(2, H, W, device=expected_normals.device)
            ep = ops.outputs_epilogue(render, alpha, expected_depths, median_depths, expected_normals, bg_list, want_depth_im)
            rgb, expected_depths, median_depths, normals = ep[0], ep[1], ep[2], ep[3]
            depth_im = ep[4].squeeze(0) if want_depth_im else None
        if self.config.use_bilateral_grid and self.training and cam_meta is not None and "cam_idx" in cam_meta:
            # rade_gs_model.py:231-234: the camera's colour transform, on the composited and clamped training render only
            rgb = ops.bilagrid_slice(rgb.contiguous(), self.bil_grids.grids, int(cam_meta["cam_idx"]))
        if background.shape[0] == 3 and not self.training:
            background = background.expand(H, W, 3)
        out = {
            "rgb": rgb.squeeze(0), "depth": expected_depths.squeeze(0), "median_depth": median_depths.squeeze(0),
            "depth_im": depth_im, "accumulation": alpha.squeeze(0), "normals": normals.squeeze(0),
            "depth_normal_error_map": normal_error_map[0, ...].unsqueeze(-1),
            "middepth_normal_error_map": normal_error_map[1, ...].unsqueeze(-1),
            "background": background,
        }
        if feature_image is not None:
            out["features"] = feature_image.squeeze(0)                   # rade_features_model.py:387
        return out

    @staticmethod
    def get_empty_outputs(width: int, height: int, background: Tensor) -> Dict[str, Union[Tensor, List]]:
        """Splatfacto's outputs for a view that contains no Gaussian (what rade_gs_model.py:100-105 returns for an
        empty crop): the background colour everywhere, depth 10, zero accumulation [UNVERIFIED-UPSTREAM: nerfstudio
        is absent; restated from its public Splatfacto]."""
        rgb = background.repeat(height, width, 1)
        depth = background.new_ones(*rgb.shape[:2], 1) * 10
        accumulation = background.new_zeros(*rgb.shape[:2], 1)
        return {"rgb": rgb, "depth": depth, "accumulation": accumulation, "background": background}

    def set_crop(self, crop_box) -> None:
        """Splatfacto's ``set_crop``: the box (anything with ``within(points[N,3]) -> bool[N(,1)]``, nerfstudio's
        ``OrientedBox``) that ``get_outputs`` applies in evaluation (rade_gs_model.py:96-105), or None."""
        self.crop_box = crop_box

    @torch.no_grad()
    def get_outputs_for_camera(self, camera, obb_box=None) -> Dict[str, Union[Tensor, List, None]]:
        """Splatfacto's no-grad entry used by the meshing loop, which passes ``obb_box=crop_box`` (mesh.py:1581-1584):
        the box becomes the model's crop box (``set_crop``) and ``get_outputs`` renders the Gaussians inside it -- in
        evaluation mode, as the reference's cropping is (rade_gs_model.py:96-119)."""
        self.set_crop(obb_box)
        return self.get_outputs(camera.to(self.device) if hasattr(camera, "to") else camera)

    @torch.no_grad()
    def render_views(self, cameras: Sequence, batch_size: int = 4, crop_box=None) -> Dict[str, Tensor]:
        """Eval-time batch rendering for the TSDF hand-off (the reference renders
        every training view one by one through ``get_outputs_for_camera`` and copies each map to the host,
        mesh.py:1572-1630).  ``batch_size`` views go through ONE rasterization call (the camera batch dimension of
        the kernels), the a3 epilogue runs per view (its ``max`` reductions are per image), and the stacked maps
        ``rgb[V,H,W,3] depth[V,H,W,1] median_depth[V,H,W,1] accumulation[V,H,W,1] normals[V,H,W,3]`` stay on
        the device.  Values are identical to ``get_outputs`` in eval mode, view by view.  ``crop_box`` (or None): only the
        Gaussians inside it are rendered, as ``get_outputs`` does with the model's crop box in evaluation; it must keep at
        least one Gaussian (``get_outputs`` returns ``get_empty_outputs`` instead, which has no depth maps)."""
        if self.config.rasterize_mode not in ["antialiased", "classic"]:
            raise ValueError("Unknown rasterize_mode: %s", self.config.rasterize_mode)
        pick = lambda t: t                                                                   # noqa: E731
        if crop_box is not None:
            crop_ids = crop_box.within(self.means).squeeze()
            if crop_ids.sum() == 0:
                raise ValueError("render_views: the crop box holds no Gaussian")
            pick = lambda t: t[crop_ids]                                                     # noqa: E731
        if self.config.sh_degree > 0:
            colors = (pick(self.features_dc), pick(self.features_rest))
            sh_degree_to_use = min(self.step // self.config.sh_degree_interval, self.config.sh_degree)
        else:
            colors, sh_degree_to_use = torch.sigmoid(pick(self.features_dc)), None
        bg_list = self._background_list()
        out: Dict[str, List[Tensor]] = {k: [] for k in ("rgb", "depth", "median_depth", "accumulation", "normals")}
        cameras = list(cameras)
        for b in range(0, len(cameras), max(1, int(batch_size))):
            params = [self._get_camera_parameters(c) for c in cameras[b:b + max(1, int(batch_size))]]
            W, H = int(params[0]["image_width"]), int(params[0]["image_height"])
            if any((int(p["image_width"]), int(p["image_height"])) != (W, H) for p in params):
                raise ValueError("render_views: the views of one batch must share a resolution")
            cp = dict(params[0])
            cp["viewmats"] = torch.cat([p["viewmats"] for p in params], dim=0)
            cp["Ks"] = torch.cat([p["Ks"] for p in params], dim=0)
            render, alpha, exp_d, med_d, exp_n, _ = self._render(
                means=pick(self.means), quats=pick(self.quats), scales=pick(self.scales), opacities=pick(self.opacities),
                colors=colors,
                render_mode="RGB+ED", sh_degree_to_use=sh_degree_to_use, camera_params=cp)
            for c in range(len(params)):
                sl = slice(c, c + 1)
                ep = ops.outputs_epilogue(render[sl], alpha[sl], exp_d[sl], med_d[sl], exp_n[sl], bg_list, False)
                out["rgb"].append(ep[0]); out["depth"].append(ep[1]); out["median_depth"].append(ep[2])
                out["normals"].append(ep[3]); out["accumulation"].append(alpha[sl])
        return {k: torch.cat(v, dim=0) for k, v in out.items()}

    @torch.no_grad()
    def extract_mesh(self, cameras: Sequence, voxel_size: float = 0.01, sdf_trunc: float = 0.03, depth_trunc: float = 1.0,
                     depth_name: str = "median_depth", masks=None, obb_box=None, batch_size: int = 4):
        """The TSDF part of the reference's ``Open3DTSDFFusion.main`` (mesh.py:1557-1632) on the device: crop (``set_crop``),
        render ``batch_size`` views at a time (``render_views``), integrate each batch into a ``TSDFVolume`` and extract
        the mesh.  Per view: depth ``outputs[depth_name]``, colour ``outputs["rgb"]``, extrinsic ``inv(c2w @ diag(1,-1,-1,1))``
        and the camera's own intrinsics (``tsdf.camera_frame``); ``masks`` ([V,H,W(,1)] bool, or None) zero the depth where
        False.  With ``obb_box`` the volume's bounds are the box's AABB padded by ``sdf_trunc`` (``tsdf.obb_bounds``), and a
        box with no Gaussian inside gives an empty mesh.  Rendered maps are freed batch by batch and never reach the host.
        Returns ``(vertices [M,3], triangles [T,3] int32, colors [M,3])`` on the device."""
        from .tsdf import TSDFVolume, camera_frame, obb_bounds
        self.set_crop(obb_box)
        cameras = list(cameras)
        vol = TSDFVolume(voxel_size, sdf_trunc, depth_trunc, bounds=obb_bounds(obb_box, sdf_trunc), device=self.device)
        if obb_box is not None and obb_box.within(self.means).squeeze().sum() == 0:
            return vol.extract_mesh()
        if masks is not None:
            masks = torch.as_tensor(masks).to(self.device)
            if masks.shape[0] != len(cameras):
                raise ValueError("extract_mesh: one mask per camera")
        bs = max(1, int(batch_size))
        for b in range(0, len(cameras), bs):
            chunk = cameras[b:b + bs]
            maps = self.render_views(chunk, batch_size=bs, crop_box=obb_box)
            if depth_name not in maps:
                raise KeyError(f"extract_mesh: depth_name {depth_name!r} is not among the rendered maps {sorted(maps)}")
            frames = [camera_frame(c) for c in chunk]
            vm = torch.stack([f[0] for f in frames]).to(self.device)
            Ks = torch.stack([f[1] for f in frames]).to(self.device)
            vol.integrate(maps[depth_name], vm, Ks, rgbs=maps["rgb"], masks=None if masks is None else masks[b:b + bs])
            del maps
        return vol.extract_mesh()

    @torch.no_grad()
    def mesh_attributes(self, vertices: Tensor, k: int = 5, sdf_trunc: float = 0.03) -> Dict[str, Tensor]:
        """What the reference's ``Open3DTSDFFusion.main`` maps onto the extracted mesh (mesh.py:1661-1702), on the device:
        ``{"normals": [M,3]}`` (``normals2vertex`` of ``self.normals``) and, for a model with ``distill_features``, also
        ``"distill_features": [M, latent]`` (``features2vertex``).  The points are all the means, uncropped.  One kNN serves
        both maps: ``[normals | features]`` is mapped in one call, its first 3 channels then normalised; every channel
        equals the separate call bit for bit."""
        from .meshmap import map_to_vertices
        # self.normals picks the rotation column with a one-hot bmm (a 13 ms batched GEMM at 1 M Gaussians); a gather of the
        # same column gives the same bits (the products by 0 and 1 and the sums with 0 are exact)
        rots = build_rotation(self.quats)
        col = torch.argmin(torch.exp(self.scales), dim=-1)
        normals = F.normalize(rots.gather(2, col[:, None, None].expand(-1, 3, 1)).squeeze(-1), dim=1)
        feats = getattr(self, "distill_features", None)
        vals = normals if feats is None else torch.cat([normals, feats.detach().float()], 1)
        out = map_to_vertices(vertices, self.means.detach(), vals, k=k, sdf_trunc=sdf_trunc, n_unit=3)
        res = {"normals": out[:, :3].contiguous()}
        if feats is not None:
            res["distill_features"] = out[:, 3:].contiguous()
        return res

    @torch.no_grad()
    def finish_mesh(self, vertices: Tensor, triangles: Tensor, colors: Tensor, clean_repair: bool = True, use_largest: bool = False,
                    max_hole_size: float = 3.0, align: bool = True, k: int = 5, sdf_trunc: float = 0.03, fill: str = "fan"
                    ) -> Dict[str, Tensor]:
        """What the reference's ``Open3DTSDFFusion.main`` does to the extracted mesh (mesh.py:1634-1718), on the device:
        ``clean_repair``: ``filter_mesh_components`` then ``fill_holes`` (the colours are carried exactly; a fan's new vertex
        takes the mean of its loop's), or with ``fill="nicely"`` ``fill_holes_nicely`` (the reference's default,
        ``use_advanced_fill``: the fans subdivided to the mesh's edge length and faired, the colours with them; ``fill_info`` is
        then its ``info``), or with ``fill="min_area"`` the same from the loops' minimum-area triangulations, with edge flips
        between the subdivisions (``triangulation="min_area", flip=True``), or with ``fill="smooth"`` the same under the
        angle-and-area weight and with curvature fairing on top (``metric="angle_area", fairing="curvature"``: the patch continues
        the rim's tangent planes); ``mesh_attributes`` on the result; ``align``: ``align_floor`` of the mesh, the same
        rotation applied to the mapped normals (Open3D's ``rotate`` turns them too) and the rigid motion to the means
        (mesh.py:1709).  Returns ``vertices``, ``triangles``, ``colors``, the attributes, ``vertex_index`` ([M'] int64: the
        row of the input each vertex was, -1 for a vertex the fill created), ``means`` (moved, [N,3]), ``n_removed``, ``n_filled`` and
        ``mesh_transform`` ([4,4] fp64 on the host, [[R, t], [0, 0, 0, 1]] as mesh.py:1712-1718; the identity without
        ``align``).  The model itself is not changed."""
        from .meshclean import align_floor, apply_rigid, fill_holes, filter_mesh_components
        if fill not in ("fan", "nicely", "min_area", "smooth"):
            raise ValueError(f"finish_mesh: fill must be 'fan' or 'nicely' or 'min_area' or 'smooth', got {fill!r}")
        index = torch.arange(vertices.shape[0], dtype=torch.int64, device=vertices.device)
        n_removed = n_filled = 0
        info = None
        if clean_repair:
            vertices, triangles, index, (colors,), n_removed = filter_mesh_components(vertices, triangles, use_largest, (colors,))
            if fill != "fan":
                from .meshfill import fill_holes_nicely
                how = dict(triangulation="min_area", flip=True) if fill in ("min_area", "smooth") else {}
                if fill == "smooth":
                    how.update(metric="angle_area", fairing="curvature")
                vertices, triangles, (colors,), n_filled, info = fill_holes_nicely(vertices, triangles, max_hole_size,
                                                                                   attributes=(colors,), **how)
            else:
                vertices, triangles, (colors,), n_filled = fill_holes(vertices, triangles, max_hole_size, (colors,))
            index = torch.cat([index, index.new_full((vertices.shape[0] - index.shape[0],), -1)])
        out = {"triangles": triangles, "colors": colors, "vertex_index": index, "n_removed": n_removed, "n_filled": n_filled}
        if info is not None:
            out["fill_info"] = info
        out.update(self.mesh_attributes(vertices, k=k, sdf_trunc=sdf_trunc))
        means = self.means.detach()
        transform = torch.eye(4, dtype=torch.float64)
        if align:
            vertices, R, translation = align_floor((vertices, triangles))
            means = apply_rigid(means, R, translation)[1]
            out["normals"] = apply_rigid(out["normals"], R)[0]
            transform[:3, :3] = R
            transform[:3, 3] = translation
        out.update(vertices=vertices, means=means, mesh_transform=transform)
        return out

    @torch.no_grad()
    def clean_gaussians(self, **kwargs) -> Tensor:
        """``pointcloud.clean_pcd`` (the reference's ``clean_pcd``: voxel reduction, statistical outliers, far points) on the
        Gaussian means, with its keyword arguments: the int64 indices of the Gaussians that survive, on the device."""
        from .pointcloud import clean_pcd
        return clean_pcd(self.means.detach(), **kwargs)[1]

    @staticmethod
    def _camera_poses(cameras: Sequence, device) -> tuple:
        """(c2w [V,3,4], intrinsics [V,4] = (fx, fy, cx, cy)) of the cameras' own poses and intrinsics (what the reference's
        exporters hand to ``get_colored_points_from_depth`` and ``project_pix``), built on the host, one upload each."""
        c2w = torch.stack([c.camera_to_worlds.reshape(-1, 3, 4)[0].detach().float().cpu() for c in cameras])
        rows = []
        for c in cameras:
            if all(isinstance(getattr(c, k, None), float) for k in ("fx", "fy", "cx", "cy")):
                rows.append([c.fx, c.fy, c.cx, c.cy])
            else:
                K = c.get_intrinsics_matrices().reshape(-1, 3, 3)[0].detach().double().cpu()
                rows.append([float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])])
        return c2w.to(device), torch.tensor(rows, dtype=torch.float32).to(device)

    @staticmethod
    def _finish_cloud(out: Dict, down_sample_voxel, outlier_removal: bool, std_ratio: float) -> Dict:
        """mesh.py:798-805: ``voxel_down_sample`` (normals and colours averaged with the points), then
        ``remove_statistical_outlier(nb_neighbors=20, std_ratio)``.  Either drops the per-sample ids: a voxel's mean has none."""
        from .pointcloud import remove_statistical_outlier, voxel_down_sample
        if down_sample_voxel is not None and out["points"].shape[0] > 0:
            names = [k for k in ("normals", "colors") if out.get(k) is not None]
            pts, att, _, _ = voxel_down_sample(out["points"], down_sample_voxel, tuple(out[k] for k in names))
            out.update(points=pts, frame_ids=None, pixel_ids=None, **dict(zip(names, att)))
        if outlier_removal and out["points"].shape[0] > 0:
            pts, ind = remove_statistical_outlier(out["points"], 20, std_ratio)
            out["points"] = pts
            for k in ("normals", "colors", "frame_ids", "pixel_ids"):
                if out.get(k) is not None:
                    out[k] = out[k][ind]
        return out

    @torch.no_grad()
    def depth_normal_points(self, cameras: Sequence, total_points: int = 2_000_000, depth_name: str = "depth", masks=None,
                            obb_box=None, filter_edges: bool = False, edge_threshold: float = 0.004, edge_dilation: int = 10,
                            min_accumulation: Optional[float] = None, down_sample_voxel: Optional[float] = None,
                            outlier_removal: bool = False, std_ratio: float = 2.0, seed: int = 0, batch_size: int = 4
                            ) -> Dict[str, Optional[Tensor]]:
        """The cloud of the reference's ``DepthAndNormalMapsPoisson.main`` (mesh.py:864-1002, ``normal_maps``) on the device:
        ``samples_per_frame = (total_points + V) // V`` (:879); ``render_views`` batch by batch, nothing goes to the host;
        ``depthcloud.depth_normal_cloud`` on ``maps[depth_name]``, ``rgb`` and ``normals`` with the cameras' own poses and
        intrinsics and ``frame_offset`` = the batch's first frame, so ``batch_size`` changes no result; the crop
        ``obb_box.within(points)`` (:988-994); the batches concatenated; then optionally ``voxel_down_sample`` and
        ``remove_statistical_outlier(20, std_ratio)``.  ``masks`` ([V,H,W(,1)] bool) and the edge filter narrow the candidates
        as ``depth_normal_cloud`` says.  ``min_accumulation`` None keeps the reference's behaviour: the depth maps carry the
        image's maximum depth where alpha is 0, so those pixels are back-projected; a number makes ``accumulation >
        min_accumulation`` part of the candidate rule.  Returns the dict of ``depth_normal_cloud`` with global ``frame_ids``
        (``frame_ids`` and ``pixel_ids`` are None after a voxel reduction)."""
        from .depthcloud import depth_normal_cloud
        cameras = list(cameras)
        n_views = len(cameras)
        if n_views == 0:
            raise ValueError("depth_normal_points: no cameras")
        if not isinstance(total_points, int) or isinstance(total_points, bool) or total_points < 0:
            raise ValueError(f"depth_normal_points: total_points must be a non-negative integer, got {total_points!r}")
        samples_per_frame = (total_points + n_views) // n_views
        if masks is not None:
            masks = torch.as_tensor(masks).to(self.device)
            if masks.shape[0] != n_views:
                raise ValueError("depth_normal_points: one mask per camera")
        c2w, intr = self._camera_poses(cameras, self.device)
        bs = max(1, int(batch_size))
        parts: Dict[str, List[Tensor]] = {k: [] for k in ("points", "normals", "colors", "frame_ids", "pixel_ids", "counts")}
        for b in range(0, n_views, bs):
            maps = self.render_views(cameras[b:b + bs], batch_size=bs)
            if depth_name not in maps:
                raise KeyError(f"depth_normal_points: depth_name {depth_name!r} is not among the rendered maps {sorted(maps)}")
            valid = None if min_accumulation is None else maps["accumulation"] > float(min_accumulation)
            out = depth_normal_cloud(maps[depth_name], maps["rgb"], maps["normals"], c2w[b:b + bs], intr[b:b + bs], samples_per_frame,
                                     seed=seed, frame_offset=b, masks=None if masks is None else masks[b:b + bs], valid=valid,
                                     filter_edges=filter_edges, edge_threshold=edge_threshold, edge_dilation=edge_dilation)
            del maps
            out["frame_ids"] = out["frame_ids"] + b
            if obb_box is not None:
                inside = obb_box.within(out["points"]).reshape(-1)
                out["counts"] = torch.bincount(out["frame_ids"][inside] - b, minlength=out["counts"].shape[0]).to(torch.int32)
                for k in ("points", "normals", "colors", "frame_ids", "pixel_ids"):
                    out[k] = out[k][inside]
            for k in parts:
                parts[k].append(out[k])
        cloud = {k: torch.cat(v, dim=0) for k, v in parts.items()}
        return self._finish_cloud(cloud, down_sample_voxel, outlier_removal, std_ratio)

    @torch.no_grad()
    def gaussian_points(self, cameras: Optional[Sequence] = None, masks=None, min_opacity: Optional[float] = None,
                        mask_color: Optional[Sequence[float]] = None, obb_box=None, down_sample_voxel: Optional[float] = None,
                        outlier_removal: bool = False, std_ratio: float = 2.0) -> Dict[str, Optional[Tensor]]:
        """The cloud of the reference's ``GaussiansToPoisson.main`` (mesh.py:676-805) on the device: the Gaussians themselves,
        ``{"points", "normals", "colors", "indices"}`` (``indices`` int64: the Gaussian each point is, None after a voxel
        reduction).  In order: ``depthcloud.gaussian_mask_filter`` against ``masks`` ([V,H,W(,1)] bool, with ``cameras``);
        ``sigmoid(opacities) > min_opacity``; the ``mask_color`` test (a Gaussian is dropped unless all three clamped colour
        channels differ from it, mesh.py:753-760); ``self.normals`` and the colours clamped to [0, 1]; the crop
        ``obb_box.within``; ``voxel_down_sample`` and ``remove_statistical_outlier(20, std_ratio)``.  The colours are
        Splatfacto's ``colors`` [UNVERIFIED-UPSTREAM]: 0.28209479177387814 features_dc + 0.5.  ``sh_degree == 0`` raises
        ValueError where the reference asserts (:680)."""
        from .depthcloud import gaussian_mask_filter
        if not self.config.sh_degree > 0:
            raise ValueError("gaussian_points: the model must have sh_degree > 0")
        if (cameras is None) != (masks is None):
            raise ValueError("gaussian_points: masks and cameras go together")
        means = self.means.detach()
        colors = torch.clamp(self.features_dc.detach().reshape(-1, 3) * 0.28209479177387814 + 0.5, 0.0, 1.0).float()
        keep = torch.ones(means.shape[0], dtype=torch.bool, device=means.device)
        if masks is not None:
            cameras = list(cameras)
            masks = torch.as_tensor(masks).to(self.device)
            if masks.shape[0] != len(cameras):
                raise ValueError("gaussian_points: one mask per camera")
            c2w, intr = self._camera_poses(cameras, self.device)
            keep &= gaussian_mask_filter(means, c2w, intr, masks)
        if min_opacity is not None:
            keep &= torch.sigmoid(self.opacities.detach()).reshape(-1) > float(min_opacity)
        if mask_color is not None:
            keep &= torch.all(colors != torch.tensor([list(mask_color)], dtype=colors.dtype, device=colors.device), dim=-1)
        if obb_box is not None:
            keep &= obb_box.within(means).reshape(-1)
        ind = torch.nonzero(keep)[:, 0]
        out = {"points": means[ind].float(), "normals": self.normals.detach()[ind], "colors": colors[ind], "frame_ids": ind,
               "pixel_ids": None}
        out = self._finish_cloud(out, down_sample_voxel, outlier_removal, std_ratio)
        out["indices"] = out.pop("frame_ids")
        del out["pixel_ids"]
        return out

    @torch.no_grad()
    def poisson_mesh(self, cameras: Optional[Sequence], source: str = "depth_normal", depth: int = 8,
                     trim_quantile: float = 0.01, min_density: Optional[float] = None, **cloud_kwargs
                     ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        """What the reference's ``DepthAndNormalMapsPoisson.main`` and ``GaussiansToPoisson.main`` end in (mesh.py:809-818,
        1023-1032) on the device: the oriented cloud of ``depth_normal_points(cameras, **cloud_kwargs)`` (``source``
        "depth_normal") or ``gaussian_points(cameras, **cloud_kwargs)`` ("gaussians"), ``poisson.poisson_reconstruct`` at
        ``depth`` and ``poisson.poisson_trim(quantile=trim_quantile, min_density=min_density)`` with the colours carried
        along.  Returns ``(vertices [M,3], triangles [T,3] int32, colors [M,3], density [M])``: what ``extract_mesh`` returns,
        plus the sampling density.  The solve is this project's dense-grid restatement, not Open3D's octree solver (DESIGN.md
        section 20)."""
        from .poisson import poisson_reconstruct, poisson_trim
        if source == "depth_normal":
            cloud = self.depth_normal_points(cameras, **cloud_kwargs)
        elif source == "gaussians":
            cloud = self.gaussian_points(cameras, **cloud_kwargs)
        else:
            raise ValueError(f"poisson_mesh: source must be 'depth_normal' or 'gaussians', got {source!r}")
        v, t, c, d, _ = poisson_reconstruct(cloud["points"], cloud["normals"], cloud["colors"], depth=depth)
        v, t, d, (c,), _ = poisson_trim(v, t, d, quantile=trim_quantile, min_density=min_density, attributes=(c,))
        return v, t, c, d

    # ------------------------------------------------------------------ the mixture's own density
    @property
    def colors(self) -> Tensor:
        """Splatfacto's ``colors`` [UNVERIFIED-UPSTREAM]: ``clamp(0.28209479177387814 features_dc + 0.5, 0, 1)``, or
        ``sigmoid(features_dc)`` at ``sh_degree == 0``; [N,3]."""
        dc = self.features_dc.reshape(-1, 3)
        if self.config.sh_degree > 0:
            return torch.clamp(dc * 0.28209479177387814 + 0.5, 0.0, 1.0)
        return torch.sigmoid(dc)

    def _activated(self, keep: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        pick = (lambda t: t[keep]) if keep is not None else (lambda t: t)
        return (pick(self.means.detach()).float(), pick(self.quats.detach()).float(),
                torch.exp(pick(self.scales.detach()).float()), torch.sigmoid(pick(self.opacities.detach()).float()).reshape(-1))

    @torch.no_grad()
    def density_field(self, voxel_size: float, cutoff: float = 3.0, min_opacity: float = 1.0 / 255.0, bounds=None, obb_box=None):
        """``density.DensityField`` of the model's Gaussians (activated scales and opacities).  With ``obb_box`` the Gaussians
        outside it are dropped, as ``set_crop`` drops them from a render, and ``bounds`` default to the box's AABB
        (``tsdf.obb_bounds``).  The field's Gaussian ids index the kept Gaussians: ``field.kept`` holds their indices in the
        model (None without a box)."""
        from .density import DensityField
        from .tsdf import obb_bounds
        keep = None
        if obb_box is not None:
            keep = torch.nonzero(obb_box.within(self.means.detach()).reshape(-1))[:, 0]
            if bounds is None:
                bounds = obb_bounds(obb_box)
        field = DensityField(*self._activated(keep), voxel_size, cutoff, min_opacity, bounds=bounds)
        field.kept = keep
        return field

    @torch.no_grad()
    def get_density(self, points: Tensor, voxel_size: Optional[float] = None, cutoff: float = 3.0,
                    min_opacity: float = 1.0 / 255.0) -> Tensor:
        """The mixture's density [P] at ``points [P,3]`` (what the reference's exporters call, mesh.py:1300):
        ``density.gaussian_density`` on the activated parameters."""
        from .density import gaussian_density
        return gaussian_density(points, *self._activated(), voxel_size, cutoff, min_opacity)

    @torch.no_grad()
    def get_density_grad(self, points: Tensor, voxel_size: Optional[float] = None, cutoff: float = 3.0,
                         min_opacity: float = 1.0 / 255.0) -> Tensor:
        """The density's gradient [P,3] (mesh.py:968): ``density.gaussian_density_grad`` on the activated parameters."""
        from .density import gaussian_density_grad
        return gaussian_density_grad(points, *self._activated(), voxel_size, cutoff, min_opacity)

    @torch.no_grad()
    def marching_cubes_mesh(self, cameras: Optional[Sequence] = None, camera_radius_multiplier: float = 2.0, resolution: int = 512,
                            isosurface_threshold: float = 0.5, voxel_size: Optional[float] = None, obb_box=None,
                            cutoff: float = 3.0, min_opacity: float = 1.0 / 255.0,
                            target_triangles: Optional[int] = None) -> Tuple[Tensor, Tensor, Tensor]:
        """The reference's ``MarchingCubesMesh.main`` (mesh.py:1234-1359) on the device, with no dense grid: the level set
        ``isosurface_threshold`` of the mixture's density.  With ``cameras``: the reference's cube, centred on the world origin,
        half side ``camera_radius_multiplier`` x the largest distance of a camera centre from their mean (:1266-1275), sampled
        at ``h = 2 radius / (resolution - 1)``.  With ``voxel_size`` instead: that ``h`` over the Gaussians' own bounds (the
        box's AABB with ``obb_box``).  Gaussians outside ``obb_box`` are dropped.  Returns ``(vertices [M,3], triangles [T,3]
        int32, colors [M,3])``, the colours ``self.colors`` blended by the Gaussians' terms at the vertex (the reference takes the
        closest Gaussian's): ready for ``finish_mesh`` and ``tsdf.write_ply``.  With ``target_triangles`` the mesh is then
        simplified to at most that many triangles (``decimate.simplify_quadric_decimation``, the colours averaged along), the
        reference's last step (mesh.py:1350-1352); its default there is 1 000 000, here ``None``: the raw mesh."""
        name = "marching_cubes_mesh"
        if target_triangles is not None and (not isinstance(target_triangles, int) or isinstance(target_triangles, bool)
                                             or target_triangles < 0):
            raise ValueError(f"{name}: target_triangles must be None or a non-negative integer, got {target_triangles!r}")
        bounds = None
        if voxel_size is None:
            if cameras is None:
                raise ValueError(f"{name}: pass cameras (the reference's cube) or voxel_size")
            cameras = list(cameras)
            if not cameras:
                raise ValueError(f"{name}: no cameras")
            if not isinstance(resolution, int) or isinstance(resolution, bool) or resolution < 2:
                raise ValueError(f"{name}: resolution must be an integer >= 2, got {resolution!r}")
            centres = torch.stack([c.camera_to_worlds.reshape(-1, 3, 4)[0, :, 3].detach().double().cpu() for c in cameras])
            radius = float(camera_radius_multiplier) * float(torch.linalg.norm(centres - centres.mean(0, keepdim=True), dim=-1).max())
            if not (radius > 0 and math.isfinite(radius)):
                raise ValueError(f"{name}: the cameras span no volume (radius {radius!r}): pass voxel_size")
            voxel_size = 2.0 * radius / (resolution - 1)
            bounds = [[-radius] * 3, [radius] * 3]
        field = self.density_field(voxel_size, cutoff, min_opacity, bounds=bounds, obb_box=obb_box)
        colors = self.colors.detach().float()
        if field.kept is not None:
            colors = colors[field.kept]
        vertices, triangles, vcol = field.extract_mesh(isosurface_threshold, values=colors.contiguous())
        if target_triangles is not None:
            from .decimate import simplify_quadric_decimation
            vertices, triangles, (vcol,), _, _ = simplify_quadric_decimation(vertices, triangles, target_triangles, attributes=(vcol,))
        return vertices, triangles, vcol

    # ------------------------------------------------------------------ point-cloud TSDF with carving
    @torch.no_grad()
    def tsdf_points_mesh(self, cameras: Sequence, voxel_size: float = 0.01, sdf_trunc: float = 0.03, depth_name: str = "depth",
                         rgb_name: str = "rgb", min_weight: int = 5, space_carving: bool = True, masks=None,
                         target_triangles: Optional[int] = None, batch_size: int = 4, crop_box=None
                         ) -> Tuple[Tensor, Tensor, Tensor]:
        """The reference's ``TSDFFusion.main`` (mesh.py:1363-1469) on the device: ``render_views`` ``batch_size`` views at a
        time, every pixel of ``maps[depth_name]`` back-projected and integrated from its camera's centre into a
        ``pointtsdf.PointTSDFVolume(voxel_size, sdf_trunc, space_carving)`` (``integrate_depth``, colours ``maps[rgb_name]``),
        ``extract_mesh(min_weight)`` and, with ``target_triangles``, ``decimate.simplify_quadric_decimation`` (the colours
        averaged along).  ``masks`` ([V,H,W(,1)] bool, or None): a pixel where False is no ray.  With ``crop_box`` only the
        Gaussians inside it are rendered and the volume's bounds are the box's AABB padded by ``sdf_trunc``.  Returns
        ``(vertices [M,3], triangles [T,3] int32, colors [M,3])``: what ``extract_mesh`` returns."""
        from .pointtsdf import PointTSDFVolume
        from .tsdf import obb_bounds
        name = "tsdf_points_mesh"
        if target_triangles is not None and (not isinstance(target_triangles, int) or isinstance(target_triangles, bool)
                                             or target_triangles < 0):
            raise ValueError(f"{name}: target_triangles must be None or a non-negative integer, got {target_triangles!r}")
        cameras = list(cameras)
        if masks is not None:
            masks = torch.as_tensor(masks).to(self.device)
            if masks.shape[0] != len(cameras):
                raise ValueError(f"{name}: one mask per camera")
        vol = PointTSDFVolume(voxel_size, sdf_trunc, space_carving, bounds=obb_bounds(crop_box, sdf_trunc), device=self.device)
        bs = max(1, int(batch_size))
        for b in range(0, len(cameras), bs):
            chunk = cameras[b:b + bs]
            maps = self.render_views(chunk, batch_size=bs, crop_box=crop_box)
            for key in (depth_name, rgb_name):
                if key not in maps:
                    raise KeyError(f"{name}: {key!r} is not among the rendered maps {sorted(maps)}")
            c2w, intr = self._camera_poses(chunk, self.device)
            vol.integrate_depth(maps[depth_name], c2w, intr, rgbs=maps[rgb_name], masks=None if masks is None else masks[b:b + bs])
            del maps
        vertices, triangles, colors = vol.extract_mesh(min_weight)
        if target_triangles is not None and triangles.shape[0] > 0:
            from .decimate import simplify_quadric_decimation
            vertices, triangles, (colors,), _, _ = simplify_quadric_decimation(vertices, triangles, target_triangles,
                                                                              attributes=(colors,))
        return vertices, triangles, colors

    # ------------------------------------------------------------------ level-set surface points
    _NORMAL_MODES = ("analytical", "closest_gaussian", "average")

    @staticmethod
    def _level_set_args(name: str, cameras, total_points, surface_levels, return_normal, search_radius, voxel_size) -> tuple:
        from .density import _levels, _scalars
        cameras = list(cameras)
        if not cameras:
            raise ValueError(f"{name}: no cameras")
        if return_normal not in RadegsModel._NORMAL_MODES:
            raise ValueError(f"{name}: return_normal must be one of {RadegsModel._NORMAL_MODES}, got {return_normal!r}")
        if not isinstance(total_points, int) or isinstance(total_points, bool) or total_points < 0:
            raise ValueError(f"{name}: total_points must be a non-negative integer, got {total_points!r}")
        levels = _levels(name, surface_levels)
        h = _scalars(name, voxel_size, 3.0, 0.0)[0]
        radius = 8.0 * h if search_radius is None else search_radius
        try:
            radius = float(radius)
        except (TypeError, ValueError):
            radius = math.nan
        if not (radius > 0 and math.isfinite(radius)):
            raise ValueError(f"{name}: search_radius must be a finite number > 0, got {search_radius!r}")
        return cameras, levels, radius

    @torch.no_grad()
    def level_set_points(self, cameras: Sequence, voxel_size: float, total_points: int = 2_000_000,
                         surface_levels: Sequence[float] = (0.1, 0.3, 0.5), return_normal: str = "closest_gaussian",
                         depth_name: str = "depth", search_radius: Optional[float] = None, masks=None, obb_box=None,
                         outlier_removal: bool = True, nb_neighbors: int = 20, std_ratio: float = 20.0, seed: int = 0,
                         batch_size: int = 4, cutoff: float = 3.0, min_opacity: float = 1.0 / 255.0) -> Dict[float, Dict[str, Tensor]]:
        """The cloud of the reference's ``LevelSetExtractor.main`` (mesh.py:1077-1144, cleaned as :1171) on the device:
        ``{level: {"points", "normals", "colors", "frame_ids", "pixel_ids"}}``.  One ``density_field(voxel_size, ...,
        obb_box=obb_box)``; ``samples_per_frame = (total_points + V) // V``; per batch ``render_views``, the candidates
        ``accumulation > 0`` with a finite positive ``depth_name`` (and a true mask), ``depthcloud.sample_pixels`` with
        ``frame_offset`` = the batch's first frame (so ``batch_size`` changes no result) and ``backproject`` to the depth point
        ``P``.  The ray of a sample starts at the camera centre ``o``, ``v = (P - o) / |P - o|``, and is searched over
        ``[max(t_c - search_radius, 0), t_c + search_radius]`` around ``t_c = |P - o|`` (``search_radius`` None: 8 voxels,
        half a unit) by ``density.level_surface_points`` with the kept Gaussians' ``colors`` and normals as values.
        ``return_normal``: ``"analytical"`` = ``-grad / |grad|``; ``"closest_gaussian"`` = the dominant Gaussian's normal, flipped
        where ``n . v > 0``; ``"average"`` = the Gaussians' normals, each first flipped to face the view's camera centre, blended
        by the terms and normalised (one query per frame), flipped where the blend still has ``n . v > 0``.  A normal of zero
        length drops its point.  Then the crop ``obb_box.within``, the batches concatenated and, per level,
        ``remove_statistical_outlier(nb_neighbors, std_ratio)``."""
        from .density import level_surface_points
        from .depthcloud import backproject, sample_pixels
        from .pointcloud import remove_statistical_outlier
        name = "level_set_points"
        cameras, levels, radius = self._level_set_args(name, cameras, total_points, surface_levels, return_normal, search_radius,
                                                       voxel_size)
        n_views = len(cameras)
        samples_per_frame = (total_points + n_views) // n_views
        field = self.density_field(voxel_size, cutoff, min_opacity, obb_box=obb_box)
        pick = (lambda x: x[field.kept]) if field.kept is not None else (lambda x: x)
        colors = pick(self.colors.detach().float())
        normals = pick(self.normals.detach().float())
        means = pick(self.means.detach().float())
        if masks is not None:
            masks = torch.as_tensor(masks).to(self.device)
            if masks.shape[0] != n_views:
                raise ValueError(f"{name}: one mask per camera")
        c2w, intr = self._camera_poses(cameras, self.device)
        bs = max(1, int(batch_size))
        keys = ("points", "normals", "colors", "frame_ids", "pixel_ids")
        parts: Dict[float, Dict[str, List[Tensor]]] = {lv: {k: [] for k in keys} for lv in levels}
        for b in range(0, n_views, bs):
            maps = self.render_views(cameras[b:b + bs], batch_size=bs, crop_box=obb_box)
            if depth_name not in maps:
                raise KeyError(f"{name}: depth_name {depth_name!r} is not among the rendered maps {sorted(maps)}")
            depth = maps[depth_name]
            cand = (maps["accumulation"] > 0) & torch.isfinite(depth) & (depth > 0)
            if masks is not None:
                cand &= masks[b:b + bs].reshape(cand.shape).bool()
            f, p, _ = sample_pixels(cand.squeeze(-1), samples_per_frame, seed=seed, frame_offset=b)
            P = backproject(depth, maps["rgb"], None, c2w[b:b + bs], intr[b:b + bs], f, p)[0]
            del maps, depth, cand
            fl = f.long()
            o = c2w[b:b + bs][:, :, 3].contiguous()[fl]
            diff = P - o
            t_c = torch.linalg.norm(diff, dim=1)
            v = diff / t_c[:, None]
            t0, t1 = torch.clamp(t_c - radius, min=0.0), t_c + radius
            # ("average" blends per-view normals: one search per frame; the rays of a frame are contiguous)
            groups = [torch.nonzero(fl == i)[:, 0] for i in range(min(bs, n_views - b))] if return_normal == "average" else [None]
            for i, sel in enumerate(groups):
                take = (lambda x: x) if sel is None else (lambda x, sel=sel: x[sel])
                nrm = normals
                if sel is not None:
                    away = ((means - c2w[b + i, :, 3]) * normals).sum(1) > 0
                    nrm = torch.where(away[:, None], -normals, normals)
                found = level_surface_points(field, take(o), take(v), take(t0), take(t1), levels,
                                             values=torch.cat([colors, nrm], 1).contiguous())
                for lv in levels:
                    r = found[lv]
                    rays = r["ray_ids"]
                    vv = take(v)[rays]
                    if return_normal == "analytical":
                        n = -r["grad"]
                    elif return_normal == "closest_gaussian":
                        n = normals[r["dominant"].long().clamp(min=0)]
                    else:
                        n = r["values"][:, 3:6]
                    length = torch.linalg.norm(n, dim=1)
                    n = n / length[:, None]
                    if return_normal != "analytical":
                        n = torch.where(((n * vv).sum(1) > 0)[:, None], -n, n)
                    keep = (length > 0) & torch.isfinite(n).all(1) & (r["dominant"] >= 0)
                    if obb_box is not None:
                        keep &= obb_box.within(r["points"]).reshape(-1)
                    out = {"points": r["points"], "normals": n, "colors": r["values"][:, 0:3].contiguous(),
                           "frame_ids": take(fl)[rays] + b, "pixel_ids": take(p)[rays]}
                    for k in keys:
                        parts[lv][k].append(out[k][keep])
        cloud: Dict[float, Dict[str, Tensor]] = {}
        for lv in levels:
            c = {k: torch.cat(parts[lv][k], dim=0) for k in keys}
            if outlier_removal and c["points"].shape[0] > 0:
                pts, ind = remove_statistical_outlier(c["points"], nb_neighbors, std_ratio)
                c = {k: (pts if k == "points" else c[k][ind]) for k in keys}
            cloud[lv] = c
        return cloud

    @torch.no_grad()
    def level_set_mesh(self, cameras: Sequence, voxel_size: float, surface_level: float = 0.3, poisson_depth: int = 9,
                       trim_quantile: float = 0.01, smooth_iterations: int = 2, **points_kwargs
                       ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        """What the reference's ``LevelSetExtractor.main`` ends in (mesh.py:1194-1223) on the device: the cloud of
        ``level_set_points(cameras, voxel_size, surface_levels=(surface_level,), **points_kwargs)``,
        ``poisson.poisson_reconstruct`` at ``poisson_depth``, ``poisson.poisson_trim(quantile=trim_quantile)`` and
        ``meshclean.smooth_laplacian(iterations=smooth_iterations)`` with the colours carried along (the reference calls
        ``filter_smooth_laplacian`` twice with one iteration each).  Returns ``(vertices [M,3], triangles [T,3] int32, colors
        [M,3], density [M])``.  The solve is this project's dense-grid restatement, not Open3D's octree solver (DESIGN.md section
        20)."""
        from .meshclean import smooth_laplacian
        from .poisson import poisson_reconstruct, poisson_trim
        name = "level_set_mesh"
        if "surface_levels" in points_kwargs:
            raise ValueError(f"{name}: pass surface_level, not surface_levels")
        try:
            level = float(surface_level)
        except (TypeError, ValueError):
            raise ValueError(f"{name}: surface_level must be a number, got {surface_level!r}") from None
        if not isinstance(smooth_iterations, int) or isinstance(smooth_iterations, bool) or smooth_iterations < 0:
            raise ValueError(f"{name}: smooth_iterations must be a non-negative integer, got {smooth_iterations!r}")
        cloud = self.level_set_points(cameras, voxel_size, surface_levels=(level,), **points_kwargs)[level]
        v, t, c, d, _ = poisson_reconstruct(cloud["points"], cloud["normals"], cloud["colors"], depth=poisson_depth)
        v, t, d, (c,), _ = poisson_trim(v, t, d, quantile=trim_quantile, min_density=None, attributes=(c,))
        v, (c,) = smooth_laplacian(v, t, smooth_iterations, attributes=(c,))
        return v, t, c, d

    @torch.no_grad()
    def associate_masks(self, cameras: Sequence, composite_masks: Sequence, front_percentage: float = 0.5, num_patches: int = 32,
                        iou_threshold: float = 0.1, bank=None):
        """The reference's ``GroupingClassifier.associate`` loop (grouping.py:226-282) on the device, for views whose segmentation
        is given: every camera is rendered in evaluation mode, the front Gaussians of every mask of its ``composite_masks[i]``
        ([H,W] integer ids, 0 the background) are selected from ``self.info`` (``grouping.front_gaussians``), labelled against the
        bank and merged into it.  Views are processed in order, ALL of them (the reference's loop ends with a stray ``break`` after
        the first frame).  ``bank`` (or None: a new ``grouping.MemoryBank`` with ``iou_threshold``) carries labels over from
        earlier calls.  Returns ``(bank, labels, matched)``: per view the int64 labels [M] of its masks and the int32 image of
        ``grouping.convert_matched_mask``.  The crop box must be unset: the bank indexes all the model's Gaussians."""
        from .grouping import MemoryBank, convert_matched_mask, front_gaussians
        cameras, composite_masks = list(cameras), list(composite_masks)
        if len(cameras) != len(composite_masks):
            raise ValueError(f"associate_masks: {len(cameras)} cameras but {len(composite_masks)} composite masks")
        if self.crop_box is not None:
            raise ValueError("associate_masks: unset the crop box first (set_crop(None)): the bank indexes all Gaussians")
        n = int(self.means.shape[0])
        if bank is None:
            bank = MemoryBank(n, iou_threshold)
        elif not isinstance(bank, MemoryBank) or bank.num_gaussians != n:
            raise ValueError(f"associate_masks: bank must be a MemoryBank over the model's {n} Gaussians")
        labels: List[Tensor] = []
        matched: List[Tensor] = []
        was_training = self.training
        self.eval()
        try:
            for camera, mask in zip(cameras, composite_masks):
                self.get_outputs(camera.to(self.device) if hasattr(camera, "to") else camera)
                front = front_gaussians(self.info, mask, front_percentage, num_patches)
                labels.append(bank.associate(front))
                matched.append(convert_matched_mask(labels[-1], mask))
        finally:
            self.train(was_training)
        return bank, labels, matched

    def render_identities(self, camera, field) -> Tensor:
        """[H, W, D]: ``field.identities`` composited as pass-through colours (``sh_degree=None``, ``render_mode="RGB"``) over
        the model's own Gaussians, which are detached -- the result is attached to ``field.identities`` only.  The camera is
        handled as ``get_outputs`` does in evaluation (the stored pose, no resolution schedule).  The crop box must be unset, as
        in ``associate_masks``: the field indexes all Gaussians.  DESIGN.md section 33."""
        if self.crop_box is not None:
            raise ValueError("render_identities: unset the crop box first (set_crop(None)): the field indexes all Gaussians")
        if field.identities.shape[0] != self.means.shape[0]:
            raise ValueError(f"render_identities: the field holds {field.identities.shape[0]} identities, the model "
                             f"{self.means.shape[0]} Gaussians")
        camera = camera.to(self.device) if hasattr(camera, "to") else camera
        cp = self._get_camera_parameters(camera)
        render = rasterization(
            means=self.means.detach(), quats=self.quats.detach(), scales=self.scales.detach(), scales_are_log=True,
            opacities=self.opacities.detach().squeeze(-1), opacities_are_logit=True, colors=field.identities,
            viewmats=cp["viewmats"].detach(), Ks=cp["Ks"], width=int(cp["image_width"]), height=int(cp["image_height"]),
            packed=False, near_plane=0.01, far_plane=1e10, render_mode="RGB", sh_degree=None, sparse_grad=False,
            absgrad=False, rasterize_mode=self.config.rasterize_mode)[0]
        return render[0]

    def identity_neighbours(self, num_samples: int = 1000, k: int = 5, radius: float = 1.0, seed: int = 0):
        """The pairs of the 3-D identity loss over the model's means (``identity.identity_neighbours``).  ``num_samples`` = 1000
        and ``k`` = 5 are the Gaussian Grouping paper's; ``radius`` (scene units, the kNN's cut-off) is this project's."""
        from .identity import identity_neighbours
        return identity_neighbours(self.means.detach(), num_samples, k, radius, seed)

    def fit_identities(self, cameras: Sequence, matched: Sequence, num_classes: int, steps: int, lr: float = 5e-4,
                       lambda_3d: float = 2.0, every_3d: int = 5, field=None, identity_dim: int = 16, radius: float = 1.0):
        """Identity training after ``associate_masks``: a plain loop over the views in order -- ``render_identities``, the 2-D
        cross-entropy against ``matched[i]``, on every ``every_3d``-th step ``lambda_3d`` times the 3-D consistency loss, one
        ``FusedAdam`` step over the field's parameters -- and the trained ``identity.IdentityField`` comes back.
        ``identity_dim`` = 16, ``lambda_3d`` = 2.0 and the 3-D loss's 1000 samples of 5 neighbours are the Gaussian Grouping
        paper's; ``lr`` = 5e-4 is its released configuration's classifier rate; ``every_3d`` and ``radius`` are this project's
        (the paper does not state them).  The reference has no such loop (grouping.py:110-136 stops at ``setup_train``)."""
        from .identity import IdentityField
        from .optim import FusedAdam
        cameras, matched = list(cameras), list(matched)
        if not cameras or len(cameras) != len(matched):
            raise ValueError(f"fit_identities: {len(cameras)} cameras but {len(matched)} matched images")
        if int(steps) < 0 or int(every_3d) < 1:
            raise ValueError(f"fit_identities: steps >= 0 and every_3d >= 1, got {steps} and {every_3d}")
        if field is None:
            field = IdentityField(int(self.means.shape[0]), int(num_classes), identity_dim).to(self.device)
        elif field.num_classes != int(num_classes):
            raise ValueError(f"fit_identities: the field classifies onto {field.num_classes} classes, not {num_classes}")
        optimizer = FusedAdam(list(field.parameters()), lr=lr)
        neighbours = self.identity_neighbours(radius=radius) if lambda_3d > 0 else None
        matched = [m.to(self.device) for m in matched]
        for step in range(int(steps)):
            i = step % len(cameras)
            optimizer.zero_grad(set_to_none=True)
            loss = field.loss_2d(self.render_identities(cameras[i], field), matched[i])
            if neighbours is not None and step % int(every_3d) == 0:
                loss = loss + lambda_3d * field.loss_3d(neighbours)
            loss.backward()
            optimizer.step()
        return field

    def _scale_reg(self, dev) -> Tensor:
        """Splatfacto's scale regularisation: 0.1 * mean(max(max(s) / min(s), max_gauss_ratio) - max_gauss_ratio) of the
        activated scales, every 10th step; 0 otherwise [UNVERIFIED-UPSTREAM]."""
        if self.config.use_scale_regularization and self.step % 10 == 0:
            scale_exp = torch.exp(self.scales)
            ratio = scale_exp.amax(dim=-1) / scale_exp.amin(dim=-1)
            cap = torch.tensor(self.config.max_gauss_ratio, device=ratio.device, dtype=ratio.dtype)
            return 0.1 * (torch.maximum(ratio, cap) - self.config.max_gauss_ratio).mean()
        zero = self.__dict__.get("_zero_scalar")                       # (one device scalar, not a host-to-device copy per step)
        if zero is None or zero.device != torch.device(dev):
            zero = self.__dict__["_zero_scalar"] = torch.zeros((), device=dev)
        return zero

    def get_loss_dict(self, outputs, batch, metrics_dict=None) -> Dict[str, Tensor]:
        """rade_gs_model.py:274-309.  ``super().get_loss_dict`` (:289) is nerfstudio's Splatfacto (third-party, absent from
        the reference tree) [UNVERIFIED-UPSTREAM]: ``main_loss`` = (1 - ssim_lambda) * mean |gt - rgb| + ssim_lambda *
        (1 - SSIM(gt, rgb)) and ``scale_reg``; the depth-normal term (:291-307) is added to it.  On the GPU the means, the
        SSIM and their backward are one autograd node (``ops.mean_losses``: a handful of launches instead of ~60)."""
        loss_dict: Dict[str, Tensor] = {}
        rgb = outputs["rgb"]
        # (Splatfacto takes whatever the data manager hands it -- a full-resolution, sliced, permuted, uint8 or float64 batch
        # image: get_gt_img brings it to the render's resolution and to 0..1 floats first)
        gt = self.get_gt_img(batch["image"].to(rgb.device)) if batch is not None and "image" in batch else None
        if gt is not None and rgb.is_cuda:
            gt = gt.to(rgb.dtype).contiguous()
            rgb = rgb.contiguous()
        with_dn = self.config.use_depth_normal_loss and self.step >= self.config.regularization_from_iter
        e1 = outputs["depth_normal_error_map"] if with_dn else None
        e2 = outputs["middepth_normal_error_map"] if with_dn else None

        def plain(t):
            return t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous())

        if rgb.is_cuda and plain(rgb) and plain(gt) and plain(e1) and plain(e2) and (gt is None or gt.shape == rgb.shape) \
                and (gt is not None or with_dn) and (e1 is None or e1.shape == e2.shape):
            # (the two maps are the halves of the epilogue's [2,H,W] tensor: its gradient then arrives as one tensor too)
            base = e1._base if with_dn and e1._base is not None and e1._base is e2._base else None
            packed = (base is not None and base.dim() == 3 and base.shape[0] == 2 and base.is_contiguous()
                      and e1.data_ptr() == base.data_ptr() and e2.data_ptr() == base[1].data_ptr())
            main_loss, dn_loss = ops.mean_losses(rgb if gt is not None else None, gt, base if packed else None,
                                                 None if packed else e1, None if packed else e2,
                                                 self.config.depth_ratio, self.config.depth_normal_lambda,
                                                 ssim_lambda=self.config.ssim_lambda if gt is not None else 0.0)
            if gt is not None:
                loss_dict["main_loss"] = main_loss
                loss_dict["scale_reg"] = self._scale_reg(rgb.device)
            if with_dn:
                loss_dict["depth_normal_loss"] = dn_loss
            return self._add_mcmc_reg(self._add_camera_opt_loss(self._add_tv_loss(loss_dict)))
        if gt is not None:
            if self.config.ssim_lambda > 0:
                raise MisplatError(f"get_loss_dict: main_loss (L1 + SSIM) takes float32 images of equal shape on the GPU; got "
                                   f"rgb {tuple(rgb.shape)} {rgb.dtype} on {rgb.device} and gt {tuple(gt.shape)} {gt.dtype} on "
                                   f"{gt.device} (there is no CPU fallback in the product: oracle/ is test infrastructure)")
            loss_dict["main_loss"] = torch.abs(gt - rgb).mean()
            loss_dict["scale_reg"] = self._scale_reg(rgb.device)
        if with_dn:
            depth_normal_loss = ((1 - self.config.depth_ratio) * e1.mean() + self.config.depth_ratio * e2.mean())
            loss_dict["depth_normal_loss"] = self.config.depth_normal_lambda * depth_normal_loss
        return self._add_mcmc_reg(self._add_camera_opt_loss(self._add_tv_loss(loss_dict)))

    def _add_mcmc_reg(self, loss_dict: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """Splatfacto's MCMC regularisers [UNVERIFIED-UPSTREAM] (Kheradmand et al. 2024, section 4.3), while training with
        ``strategy="mcmc"``: ``opacity_reg`` = mcmc_opacity_reg * mean(sigmoid(opacities)) and mcmc_scale_reg *
        mean(exp(scales)) added to ``scale_reg``; otherwise the dict as it is.  Two plain reductions a step."""
        if self.config.strategy == "mcmc" and self.training:
            loss_dict["opacity_reg"] = self.config.mcmc_opacity_reg * torch.sigmoid(self.opacities).mean()
            scale_reg = self.config.mcmc_scale_reg * torch.exp(self.scales).mean()
            loss_dict["scale_reg"] = loss_dict["scale_reg"] + scale_reg if "scale_reg" in loss_dict else scale_reg
        return loss_dict

    def _add_camera_opt_loss(self, loss_dict: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """Splatfacto's ``camera_optimizer.get_loss_dict`` [UNVERIFIED-UPSTREAM]: the L2 regulariser of the pose adjustments,
        while training with a camera optimizer; otherwise the dict as it is."""
        if self.config.camera_optimizer_mode != "off" and self.training:
            self.camera_optimizer.get_loss_dict(loss_dict)
        return loss_dict

    def _add_tv_loss(self, loss_dict: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """Splatfacto's "total variation loss (cameras)" (rade_gs_model.py:284-289) [UNVERIFIED-UPSTREAM]: 10 x the TV of every
        camera's grid, while training with ``use_bilateral_grid``; otherwise the dict as it is."""
        if self.config.use_bilateral_grid and self.training:
            loss_dict["tv_loss"] = 10 * ops.bilagrid_tv_loss(self.bil_grids.grids)
        return loss_dict

    # ------------------------------------------------------------------------------------------------------- evaluation
    @property
    def num_points(self) -> int:
        return int(self.means.shape[0])

    def composite_with_background(self, image: Tensor, background: Tensor) -> Tensor:
        """Splatfacto's ``composite_with_background`` [UNVERIFIED-UPSTREAM]: an RGBA ground truth goes over the background
        the render was composited on (alpha * rgb + (1 - alpha) * background); an RGB one is returned as it is."""
        if image.shape[-1] == 4:
            alpha = image[..., 3:4]
            return alpha * image[..., :3] + (1 - alpha) * background.to(image.device)
        return image

    def _eval_pair(self, outputs, batch) -> Tuple[Tensor, Tensor]:
        """(rgb, gt): the render and the ground truth it is scored against, float32 [H, W, 3] on the render's device."""
        rgb = outputs["rgb"]
        gt = self.composite_with_background(self.get_gt_img(batch["image"].to(rgb.device)), outputs["background"])
        return rgb.detach().to(torch.float32).contiguous(), gt.detach().to(torch.float32).contiguous()

    @torch.no_grad()
    def get_metrics_dict(self, outputs, batch) -> Dict[str, Union[Tensor, int]]:
        """Splatfacto's ``get_metrics_dict`` [UNVERIFIED-UPSTREAM], which it calls on every training step: ``psnr`` (a device
        scalar: ``metrics.image_metrics(..., ssim=False)``, two launches, no host read) of the render against the ground
        truth over the render's background, ``gaussian_count``, and the camera optimizer's entries when there is one."""
        from .metrics import image_metrics
        rgb, gt = self._eval_pair(outputs, batch)
        metrics_dict: Dict[str, Union[Tensor, int]] = {"psnr": image_metrics(rgb, gt, ssim=False)["psnr"][0],
                                                       "gaussian_count": self.num_points}
        if self.config.camera_optimizer_mode != "off":
            self.camera_optimizer.get_metrics_dict(metrics_dict)
        return metrics_dict

    @torch.no_grad()
    def get_image_metrics_and_images(self, outputs, batch) -> Tuple[Dict[str, float], Dict[str, Tensor]]:
        """Splatfacto's ``get_image_metrics_and_images`` [UNVERIFIED-UPSTREAM], what an evaluation run calls for each view:
        ``({"psnr", "ssim"} as floats, {"img": the ground truth and the render side by side, [H, 2 W, 3]})``.  One fused
        metric call and one host read.  With the config's ``color_corrected_metrics`` also ``"cc_psnr"`` and ``"cc_ssim"``
        (``metrics.color_corrected_metrics``), in the same host read.  There is no ``"lpips"`` key: LPIPS is a trained
        network whose weights are not part of this package, and nothing is downloaded."""
        from .metrics import color_corrected_metrics, image_metrics
        rgb, gt = self._eval_pair(outputs, batch)
        m = image_metrics(rgb, gt, ssim=True)
        names, values = ["psnr", "ssim"], [m["psnr"][0], m["ssim"][0]]
        if self.config.color_corrected_metrics:
            cc = color_corrected_metrics(rgb, gt, ssim=True)
            names += ["cc_psnr", "cc_ssim"]
            values += [cc["cc_psnr"][0], cc["cc_ssim"][0]]
        scores = torch.stack(values).tolist()                                          # the one host read
        return {k: float(v) for k, v in zip(names, scores)}, {"img": torch.cat([gt, rgb], dim=1)}

    @torch.no_grad()
    def evaluate_views(self, cameras: Sequence, images: Sequence, normals: Optional[Sequence] = None,
                       depths: Optional[Sequence] = None, valid: Optional[Sequence] = None, batch_size: int = 4,
                       color_correct: Optional[bool] = None) -> Dict[str, Dict]:
        """Scores the model on ``cameras`` against their ground truth: ``batch_size`` views at a time are rendered by
        ``render_views`` and scored on the device (``metrics.image_metrics`` / ``normal_metrics`` / ``depth_metrics``); the
        one host read is at the end.  ``images`` [V] of [H, W, 3 or 4] (uint8 or float; RGBA goes over the model's background);
        ``normals`` (or None) [V] of [H, W, 3] maps in the 0..1 encoding of the model's ``normals`` output; ``depths`` (or
        None) [V] of [H, W] or [H, W, 1], compared with the rendered ``depth``; ``valid`` (or None) [V] of [H, W] bool masks for
        the normal and depth scores.  Returns ``{"per_view": {name: [V] device tensor}, "mean": {name: float}}`` with the
        names ``psnr ssim mse l1``, ``normal_mean normal_a11.25 normal_a22.5 normal_a30 normal_count`` and ``depth_abs_rel
        depth_sq_rel depth_rmse depth_rmse_log depth_delta1 depth_delta2 depth_delta3 depth_count``, and with ``color_correct``
        (None: the config's ``color_corrected_metrics``) ``cc_psnr cc_ssim cc_mse cc_l1``, the image scores of the
        colour-corrected render.  A view's scores do not depend on the batch it was in."""
        from .metrics import color_corrected_metrics, depth_metrics, image_metrics, normal_metrics
        if color_correct is None:
            color_correct = self.config.color_corrected_metrics
        cameras = list(cameras)
        V, bs = len(cameras), max(1, int(batch_size))
        for name, seq in (("images", images), ("normals", normals), ("depths", depths), ("valid", valid)):
            if seq is not None and len(seq) != V:
                raise ValueError(f"evaluate_views: {V} cameras but {len(seq)} {name}")
        if V == 0:
            raise ValueError("evaluate_views: no cameras")
        dev = self.device
        background = self._get_background_color()

        def stack(seq, lo, hi, prepare):
            return torch.stack([prepare(seq[i].to(dev)) for i in range(lo, hi)]).contiguous()

        per_view: Dict[str, List[Tensor]] = {}
        for lo in range(0, V, bs):
            hi = min(lo + bs, V)
            maps = self.render_views(cameras[lo:hi], batch_size=bs)
            gt = stack(images, lo, hi, lambda t: self.composite_with_background(self.get_gt_img(t), background).to(torch.float32))
            scores = dict(image_metrics(maps["rgb"], gt, ssim=True))
            if color_correct:
                scores.update(color_corrected_metrics(maps["rgb"], gt, ssim=True))
            mask = None if valid is None else stack(valid, lo, hi, lambda t: t.reshape(t.shape[0], t.shape[1]).bool())
            if normals is not None:
                n = normal_metrics(maps["normals"], stack(normals, lo, hi, lambda t: t.to(torch.float32)), mask, encoded=True)
                scores.update({"normal_" + k: v for k, v in n.items()})
            if depths is not None:
                d = depth_metrics(maps["depth"], stack(depths, lo, hi, lambda t: t.to(torch.float32).reshape(t.shape[0], t.shape[1])),
                                  mask)
                scores.update({"depth_" + k: v for k, v in d.items()})
            for k, v in scores.items():
                per_view.setdefault(k, []).append(v)
        result = {k: torch.cat(v) for k, v in per_view.items()}
        names = list(result)
        means = torch.stack([result[k].mean() for k in names]).tolist()                 # the one host read
        return {"per_view": result, "mean": {k: float(m) for k, m in zip(names, means)}}

    def get_gaussian_param_groups(self) -> Dict[str, List[nn.Parameter]]:
        """One optimizer group per Gaussian parameter (Splatfacto's ``get_gaussian_param_groups``)."""
        return {name: [self.gauss_params[name]] for name in self.gauss_params.keys()}

    def get_param_groups(self) -> Dict[str, List[nn.Parameter]]:
        """The Gaussian groups and, with ``use_bilateral_grid``, ``bilateral_grid`` (configs/rade_gs_method.py:78-83: Adam,
        lr 2e-3 falling to 1e-4 after 1000 warm-up steps; the schedule is the trainer's)."""
        groups = self.get_gaussian_param_groups()
        if self.config.use_bilateral_grid:
            groups["bilateral_grid"] = list(self.bil_grids.parameters())
        if self.config.camera_optimizer_mode != "off":
            self.camera_optimizer.get_param_groups(groups)              # "camera_opt" (configs/rade_gs_method.py:72-77)
        return groups


@dataclass
class RadegsFeaturesModelConfig(RadegsModelConfig):
    """rade_features_model.py:40-75: the fields of its config the model reads -- the width of the distilled feature vector a
    Gaussian carries (13 in the reference: 3 + 13 = 16 fused channels), the decoder's hidden width and the two weights of
    the feature loss (the reference's defaults), and the method of the text-query similarity map."""
    features_latent_dim: int = 13
    mlp_hidden_dim: int = 64
    features_loss_lambda: float = 1e-3
    features_regularization_lambda: float = 0.1
    similarity_method: str = "pairwise"          # rade_features_model.py:74: "standard" or "pairwise"


class RadegsFeaturesModel(RadegsModel):
    """``RadegsFeaturesModel`` (rade_features_model.py:78-596): every Gaussian carries ``distill_features`` [N, latent_dim]
    that are composited behind its SH colour; ``get_outputs`` returns them as ``outputs["features"]`` [H, W, latent_dim].
    With ``metadata`` (``feature_type``: the main feature model's name, ``feature_dims``: name -> (C, H, W)) the model also
    owns the decoder MLP (``self.decoder``, an optimizer group), ``decode_features`` (:149-189) and the cosine feature loss
    of ``get_loss_dict`` (:545-584), all on the kernels of csrc/featloss.hip.  The text encoder and
    its queries (CLIP) are foundation-model code outside the path."""

    def __init__(self, config: RadegsFeaturesModelConfig, means, scales, quats, opacities, features_dc, features_rest,
                 distill_features: Tensor, metadata: Optional[Dict] = None, num_train_data: int = 0):
        super().__init__(config, means, scales, quats, opacities, features_dc, features_rest, num_train_data=num_train_data)
        if distill_features.shape != (means.shape[0], config.features_latent_dim):
            raise ValueError(f"distill_features must be [N, {config.features_latent_dim}], got {tuple(distill_features.shape)}")
        self.gauss_params["distill_features"] = nn.Parameter(distill_features)
        self.metadata = None
        self.text_query = None                                          # the folded queries of ``set_text_queries``
        if metadata is not None:
            from .featureloss import TwoLayerMLP
            if "feature_type" not in metadata or "feature_dims" not in metadata:
                raise ValueError("RadegsFeaturesModel: metadata needs 'feature_type' and 'feature_dims'")
            dims = {name: tuple(int(v) for v in d) for name, d in metadata["feature_dims"].items()}
            if metadata["feature_type"] not in dims:
                raise ValueError(f"RadegsFeaturesModel: feature_type {metadata['feature_type']!r} is not among feature_dims "
                                 f"{sorted(dims)}")
            self.metadata = {"feature_type": metadata["feature_type"], "feature_dims": dims}
            self.main_features_name = metadata["feature_type"]
            self.main_features_dims = dims[self.main_features_name]                 # C, H, W
            self.decoder = TwoLayerMLP(config.features_latent_dim, config.mlp_hidden_dim, dims)

    distill_features = property(lambda self: self.gauss_params["distill_features"])

    def _features_for_render(self, pick):
        return pick(self.distill_features)

    def _need_decoder(self, what: str) -> None:
        if self.metadata is None:
            raise ValueError(f"{what}: the model was built without metadata (feature_type, feature_dims): it has no decoder")

    @torch.no_grad()
    def decode_features(self, features: Tensor, resize_factor: float = 1.0) -> Dict[str, Tensor]:
        """rade_features_model.py:149-189: ``features`` [H, W, latent_dim] -> name -> [C_b, h, w].  The features are resized to
        (int(H_main * resize_factor), int(W_main * resize_factor)) and decoded; the main branch comes back at that size, every
        other branch resized to its own (H_b, W_b).  Inference only (no gradient): training goes through ``get_loss_dict``."""
        from .featureloss import feature_decode
        self._need_decoder("decode_features")
        _, Hm, Wm = self.main_features_dims
        main_hw = (int(Hm * resize_factor), int(Wm * resize_factor))
        if min(main_hw) < 1:
            raise ValueError(f"decode_features: resize_factor {resize_factor} leaves an empty map {main_hw}")
        dims = {name: ((d[0],) + main_hw if name == self.main_features_name else d)
                for name, d in self.metadata["feature_dims"].items()}
        return feature_decode(features.detach(), self.decoder, dims, main_hw)

    SIMILARITY_RESIZE_FACTOR = 8.0                                      # rade_features_model.py:509-511

    @torch.no_grad()
    def set_text_queries(self, text_embeddings: Optional[Tensor], n_positive: int = 1) -> None:
        """The text queries of the similarity map (rade_features_model.py:484-491 ``set_text_queries``, with the embeddings
        in place of the strings: the text encoder is the caller's).  ``text_embeddings`` [Q, C_main] float32 on the model's
        device, unit-norm rows, the first ``n_positive`` positive and the others negative; they are folded into the main
        branch of the decoder once (``ops.fold_text_queries``) and kept as ``self.text_query``.  The fold is a SNAPSHOT of the
        decoder's weights at this call: call it again after the decoder has trained on.  None clears the queries."""
        if text_embeddings is None:
            self.text_query = None
            return
        self._need_decoder("set_text_queries")
        self.text_query = ops.fold_text_queries(self.decoder, self.main_features_name, text_embeddings, n_positive)

    @torch.no_grad()
    def get_outputs_for_camera(self, camera, obb_box=None) -> Dict[str, Union[Tensor, List, None]]:
        """rade_features_model.py:493-539: the base outputs and, with text queries set, ``outputs["similarity"]`` [H, W, 1]: the
        similarity (``config.similarity_method``, temperature 0.05) of the main branch at the working size (int(H_main * 8.0),
        int(W_main * 8.0)), resized bilinearly to the image -- on ``ops.similarity_map``, without the decoded features.  One
        deliberate difference: the reference assigns ``outs["similarity"]`` inside its "the shapes differ" block (:525-538), so
        a view already at the working size gets no map; here the map is always set.  Without queries, and for an empty crop
        (which renders no features): the base outputs."""
        outs = super().get_outputs_for_camera(camera, obb_box)
        if self.text_query is not None and "features" in outs:
            _, Hm, Wm = self.main_features_dims
            work_hw = (int(Hm * self.SIMILARITY_RESIZE_FACTOR), int(Wm * self.SIMILARITY_RESIZE_FACTOR))
            outs["similarity"] = ops.similarity_map(outs["features"], self.text_query, work_hw, tuple(outs["rgb"].shape[:2]),
                                                    method=self.config.similarity_method)
        return outs

    @torch.no_grad()
    def gaussian_similarity(self, softmax_temp: float = 0.05) -> Tensor:
        """The similarity of every Gaussian's ``distill_features`` to the text queries, [N] in 0..1 (the reference's
        commented-out ``similarity`` property, rade_features_model.py:143-147), ready for a threshold or a
        ``clean_gaussians``-style mask; no [N, C] decoded tensor is formed."""
        if self.text_query is None:
            raise ValueError("gaussian_similarity: no text queries are set (set_text_queries)")
        return ops.gaussian_similarity(self.distill_features.detach(), self.text_query, self.config.similarity_method, softmax_temp)

    def get_loss_dict(self, outputs, batch, metrics_dict=None) -> Dict[str, Tensor]:
        """rade_features_model.py:545-584: the base model's losses plus ``features_loss`` = features_loss_lambda * sum over
        the feature models of weight * mean(1 - cos(decoded, ground truth)), weight 1 for the main model and
        features_regularization_lambda for the others.  ``batch["features_dict"]`` (name -> [C, H, W]) may live on any device.
        One autograd node (``ops.feature_loss``).  A model without metadata returns the base dict, as before."""
        loss_dict = super().get_loss_dict(outputs, batch, metrics_dict)
        if self.metadata is None:
            return loss_dict
        if batch is None or "features_dict" not in batch:
            raise ValueError("get_loss_dict: the batch carries no 'features_dict'")
        features = outputs["features"]
        dims = self.metadata["feature_dims"]
        if set(batch["features_dict"]) != set(dims):
            raise ValueError(f"get_loss_dict: features_dict has {sorted(batch['features_dict'])}, the model's feature_dims "
                             f"{sorted(dims)}")
        gt = {}
        for name, d in dims.items():
            t = batch["features_dict"][name]
            if tuple(t.shape) != d:
                raise ValueError(f"get_loss_dict: features_dict[{name!r}] is {tuple(t.shape)}, feature_dims say {d}")
            gt[name] = t.to(device=features.device, dtype=torch.float32)
        loss_dict["features_loss"] = ops.feature_loss(features, self.decoder, gt, self.main_features_name,
                                                      self.config.features_regularization_lambda,
                                                      self.config.features_loss_lambda)
        return loss_dict

    def get_param_groups(self) -> Dict[str, List[nn.Parameter]]:
        """rade_features_model.py:591-596: the Gaussian groups (``distill_features`` among them, :586-589), for a model with a
        decoder ``decoder``, and with ``use_bilateral_grid`` ``bilateral_grid`` (configs/rade_features_method.py:89-94)."""
        groups = super().get_param_groups()
        if self.metadata is not None:
            groups["decoder"] = list(self.decoder.parameters())
        return groups
