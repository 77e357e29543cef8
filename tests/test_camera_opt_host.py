"""CPU: the camera optimizer (collab_splats_amd/camera_opt.py) -- exponential maps and their Jacobians against closed forms
written here and ``torch.linalg.matrix_exp``, the composition with a camera against ``torch.linalg.inv``, the regulariser,
metrics and ``state_dict``, the model wiring, and the C ABI of the view-matrix gradient (declared, exported, bound)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
MAGNITUDES = (0.0, 1e-8, 1e-3, 0.5, 3.0)


def _tangents(theta: float, n: int = 4, seed: int = 0):
    g = torch.Generator().manual_seed(seed + int(1e3 * theta) % 97)
    axis = torch.randn(n, 3, generator=g, dtype=F64)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    tau = torch.randn(n, 3, generator=g, dtype=F64)
    return torch.cat((tau, axis * theta), dim=-1)


def _hat(w):
    o = torch.zeros((), dtype=w.dtype)
    return torch.stack([torch.stack([o, -w[2], w[1]]), torch.stack([w[2], o, -w[0]]), torch.stack([-w[1], w[0], o])])


def _rodrigues_ref(x):
    """[6] -> [3,4]: closed-form Rodrigues rotation | raw translation.  (1 - cos th)/th^2 is written as sin^2(th/2) / (th^2 / 2):
    the same closed form without the cancellation that makes the textbook expression (and its derivative) meaningless at
    th = 1e-8.  th = 0 has no closed form (0/0): callers compare against the identity / the generators there."""
    tau, w = x[:3], x[3:]
    th = w.norm()
    K = _hat(w)
    R = torch.eye(3, dtype=x.dtype) + torch.sin(th) / th * K + 2.0 * torch.sin(0.5 * th) ** 2 / (th * th) * (K @ K)
    return torch.cat((R, tau[:, None]), dim=1)


def _se3_ref(x):
    T = torch.cat((torch.cat((_hat(x[3:]), x[:3, None]), dim=1), torch.zeros(1, 4, dtype=x.dtype)), dim=0)
    return torch.linalg.matrix_exp(T)[:3]


def _generators(mode: str, tau):
    """d adj / d xi at omega = 0, [3,4,6]: translation columns, then the so(3) generators (SE3: with their action on tau / 2)."""
    J = torch.zeros(3, 4, 6, dtype=F64)
    for i in range(3):
        J[i, 3, i] = 1.0
        e = torch.zeros(3, dtype=F64)
        e[i] = 1.0
        J[:, :3, 3 + i] = _hat(e)
        if mode == "SE3":
            J[:, 3, 3 + i] = 0.5 * (_hat(e) @ tau)
    return J


def _optimizer(mode, tangents):
    from collab_splats_amd import CameraOptimizer
    opt = CameraOptimizer(tangents.shape[0], mode).double()
    with torch.no_grad():
        opt.pose_adjustment.copy_(tangents)
    return opt


def test_zero_adjustment_is_the_identity():
    from collab_splats_amd import CameraOptimizer
    V = torch.eye(4, dtype=F64)[None].clone()
    V[0, :3, :] = torch.randn(3, 4, generator=torch.Generator().manual_seed(1), dtype=F64)
    for mode in ("SO3xR3", "SE3"):
        opt = CameraOptimizer(3, mode).double()
        assert opt.pose_adjustment.shape == (3, 6) and not opt.pose_adjustment.any()
        adj = opt(torch.tensor([0, 2]))
        assert adj.shape == (2, 3, 4) and torch.equal(adj, torch.eye(4, dtype=F64)[:3].expand(2, 3, 4))
        assert torch.equal(opt.apply_to_viewmat(V, 1), V)
        assert torch.equal(opt.apply_to_c2w(V[:, :3], 1), V[:, :3])
    off = CameraOptimizer(3, "off")
    assert off.apply_to_viewmat(V, 1) is V and torch.equal(off(torch.tensor([1])), torch.eye(4)[None, :3])
    with pytest.raises(ValueError, match="mode"):
        CameraOptimizer(3, "SO3")


@pytest.mark.parametrize("theta", MAGNITUDES)
def test_exponential_maps_values(theta):
    xs = _tangents(theta)
    so3 = _optimizer("SO3xR3", xs)(torch.arange(4)).detach()
    se3 = _optimizer("SE3", xs)(torch.arange(4)).detach()
    for i in range(4):
        if theta == 0.0:
            ref = torch.cat((torch.eye(3, dtype=F64), xs[i, :3, None]), dim=1)
        else:
            ref = _rodrigues_ref(xs[i])
        print(f"theta {theta}: SO3xR3 {float((so3[i] - ref).abs().max()):.2e}  SE3 {float((se3[i] - _se3_ref(xs[i])).abs().max()):.2e}")
        assert float((so3[i] - ref).abs().max()) <= 1e-12
        assert float((se3[i] - _se3_ref(xs[i])).abs().max()) <= 1e-10
        R = so3[i, :, :3]
        assert float((R @ R.T - torch.eye(3, dtype=F64)).abs().max()) <= 1e-12          # a rotation at every magnitude


@pytest.mark.parametrize("theta", MAGNITUDES)
def test_exponential_maps_jacobians(theta):
    from collab_splats_amd import camera_opt
    jac = torch.autograd.functional.jacobian
    xs = _tangents(theta, n=3, seed=5)
    for i in range(3):
        x = xs[i]
        got_so3 = jac(lambda t: camera_opt.exp_map_SO3xR3(t[None])[0], x)
        got_se3 = jac(lambda t: camera_opt.exp_map_SE3(t[None])[0], x)
        assert bool(torch.isfinite(got_so3).all()) and bool(torch.isfinite(got_se3).all())
        if theta == 0.0:
            assert float((got_so3 - _generators("SO3xR3", x[:3])).abs().max()) <= 1e-12
            assert float((got_se3 - _generators("SE3", x[:3])).abs().max()) <= 1e-12
        else:
            e1 = float((got_so3 - jac(_rodrigues_ref, x)).abs().max())
            print(f"theta {theta}: Jacobian SO3xR3 {e1:.2e}")
            assert e1 <= 1e-12
        e2 = float((got_se3 - jac(_se3_ref, x)).abs().max())
        print(f"theta {theta}: Jacobian SE3 {e2:.2e}")
        assert e2 <= 1e-10


@pytest.mark.parametrize("mode", ["SO3xR3", "SE3"])
def test_composition_with_a_rotated_translated_camera(mode):
    g = torch.Generator().manual_seed(3)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=F64))
    if torch.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    c2w = torch.eye(4, dtype=F64)
    c2w[:3, :3] = q
    c2w[:3, 3] = torch.tensor([0.7, -1.3, 2.1], dtype=F64)
    F = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=F64))
    V = (F @ torch.linalg.inv(c2w))[None]
    xs = torch.randn(3, 6, generator=g, dtype=F64) * torch.tensor([0.3] * 3 + [0.4] * 3, dtype=F64)
    opt = _optimizer(mode, xs)
    for i in range(3):
        adj = torch.eye(4, dtype=F64)
        adj[:3] = opt(torch.tensor([i]))[0]
        want = F @ torch.linalg.inv(c2w @ adj)
        got = opt.apply_to_viewmat(V, i)
        assert got.shape == (1, 4, 4) and float((got[0] - want).detach().abs().max()) <= 1e-12
        assert float((opt.apply_to_c2w(c2w[None, :3], i)[0] - (c2w @ adj)[:3]).detach().abs().max()) <= 1e-12
    # differentiable: the gradient reaches the rendered camera's row only
    opt.apply_to_viewmat(V, 1).square().sum().backward()
    grad = opt.pose_adjustment.grad
    assert bool(grad[1].abs().sum() > 0) and not grad[0].any() and not grad[2].any()


def test_regulariser_metrics_and_state_dict():
    from collab_splats_amd import CameraOptimizer
    opt = CameraOptimizer(2, "SO3xR3", trans_l2_penalty=0.5, rot_l2_penalty=0.25)
    with torch.no_grad():
        opt.pose_adjustment.copy_(torch.tensor([[3.0, 0, 4.0, 0, 0, 2.0], [0, 0, 1.0, 0.6, 0.8, 0]]))
    loss, metrics, groups = {"main_loss": torch.tensor(1.0)}, {}, {"means": []}
    opt.get_loss_dict(loss)
    opt.get_metrics_dict(metrics)
    opt.get_param_groups(groups)
    # mean(|tau|) = (5 + 1) / 2, mean(|omega|) = (2 + 1) / 2
    assert set(loss) == {"main_loss", "camera_opt_regularizer"}
    assert float(loss["camera_opt_regularizer"].detach()) == pytest.approx(3.0 * 0.5 + 1.5 * 0.25, rel=1e-6)
    assert float(metrics["camera_opt_translation"]) == pytest.approx(26.0 ** 0.5, rel=1e-6)
    assert float(metrics["camera_opt_rotation"]) == pytest.approx(5.0 ** 0.5, rel=1e-6)
    assert set(groups) == {"means", "camera_opt"} and groups["camera_opt"][0] is opt.pose_adjustment
    assert list(opt.state_dict()) == ["pose_adjustment"]
    fresh = CameraOptimizer(2, "SE3")
    fresh.load_state_dict(opt.state_dict())                                  # a nerfstudio checkpoint's key loads unchanged
    assert torch.equal(fresh.pose_adjustment, opt.pose_adjustment)
    # the regulariser is differentiable at the start of training (all zeros)
    start = CameraOptimizer(2, "SE3")
    d = {}
    start.get_loss_dict(d)
    d["camera_opt_regularizer"].backward()
    assert bool(torch.isfinite(start.pose_adjustment.grad).all())
    off = CameraOptimizer(2, "off")
    loss, metrics, groups = {"main_loss": torch.tensor(1.0)}, {}, {"means": []}
    off.get_loss_dict(loss), off.get_metrics_dict(metrics), off.get_param_groups(groups)
    assert not list(off.parameters()) and not off.state_dict()
    assert set(loss) == {"main_loss"} and metrics == {} and set(groups) == {"means"}


def _model(mode: str, features: bool = False, **kw):
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    sc = random_scene(40, 64, 48, seed=1)
    args = (sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0], sc["sh"][:, 1:])
    if features:
        cfg = radegs.RadegsFeaturesModelConfig(camera_optimizer_mode=mode, ssim_lambda=0.0)
        return radegs.RadegsFeaturesModel(cfg, *args, torch.rand(40, 13, generator=torch.Generator().manual_seed(2)), **kw)
    return radegs.RadegsModel(radegs.RadegsModelConfig(camera_optimizer_mode=mode, ssim_lambda=0.0), *args, **kw)


GAUSS = {"means", "scales", "quats", "opacities", "features_dc", "features_rest"}


def test_model_wiring():
    import collab_splats_amd as m
    from collab_splats_amd import radegs
    cfg = radegs.RadegsModelConfig()
    assert cfg.camera_optimizer_mode == "off" and radegs.RadegsFeaturesModelConfig().camera_optimizer_mode == "off"
    assert (cfg.camera_opt_trans_l2_penalty, cfg.camera_opt_rot_l2_penalty) == (1e-2, 1e-3)
    for features in (False, True):
        extra = {"distill_features"} if features else set()
        plain = _model("off", features, num_train_data=5)                              # ignored with the mode off
        assert not hasattr(plain, "camera_optimizer") and not any("camera_optimizer" in k for k in plain.state_dict())
        assert set(plain.get_param_groups()) == GAUSS | extra
        for mode in ("SO3xR3", "SE3"):
            with pytest.raises(ValueError, match="num_train_data"):
                _model(mode, features)
            with pytest.raises(ValueError, match="num_train_data"):
                _model(mode, features, num_train_data=0)
            model = _model(mode, features, num_train_data=3)
            assert isinstance(model.camera_optimizer, m.CameraOptimizer) and model.camera_optimizer.mode == mode
            assert model.camera_optimizer.pose_adjustment.shape == (3, 6)
            assert "camera_optimizer.pose_adjustment" in model.state_dict()
            groups = model.get_param_groups()
            assert set(groups) == GAUSS | extra | {"camera_opt"}
            assert groups["camera_opt"][0] is model.camera_optimizer.pose_adjustment
    # the regulariser joins the loss dict while training, and only then
    model = _model("SO3xR3", num_train_data=3).train()
    batch = {"image": torch.rand(8, 8, 3)}
    assert set(model.get_loss_dict({"rgb": torch.rand(8, 8, 3)}, batch)) == {"main_loss", "scale_reg", "camera_opt_regularizer"}
    assert set(model.eval().get_loss_dict({"rgb": torch.rand(8, 8, 3)}, batch)) == {"main_loss", "scale_reg"}
    assert set(_model("off").train().get_loss_dict({"rgb": torch.rand(8, 8, 3)}, batch)) == {"main_loss", "scale_reg"}
    with pytest.raises(ValueError, match="mode"):
        _model("SO3", num_train_data=3)


NEW_SYMBOLS = {"misplat_project_bwd_pose_workspace": 2, "misplat_project_bwd_pose": 17}


def test_abi_of_the_view_matrix_gradient(built_lib):
    """The two entry points are declared in include/misplat.h (with the argument counts the binding checks), exported by
    the built library and bound in _lib.py."""
    from collab_splats_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "misplat.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True).stdout
    lib = _lib.load()
    for name, n_args in NEW_SYMBOLS.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m is not None, name
        assert len(m.group(1).split(",")) == n_args, name
        assert re.search(r" T " + name + r"\b", exported), name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name].split(" ")[1]) == n_args
        assert hasattr(lib, name)
    assert _lib.SYMBOLS["misplat_project_bwd_pose_workspace"][0] == "q" and _lib._RET["q"] is C.c_int64
    # sizes need no GPU: 12 fp64 partials per workgroup and camera, a workgroup count that depends on N only and is capped
    ws = lambda n, c: int(lib.misplat_project_bwd_pose_workspace(n, c))
    assert ws(1, 1) >= 96 and ws(70001, 3) >= 3 * 274 * 96
    assert ws(10 ** 6, 1) == ws(10 ** 7, 1) <= 1024 * 96 + 256
    # bad sizes and a null workspace are refused before anything is launched
    P = _lib.make_params(4, 1, 16, 16)
    null = C.c_void_p(0)
    assert lib.misplat_project_bwd_pose(C.byref(P), *([null] * 16)) == -1
