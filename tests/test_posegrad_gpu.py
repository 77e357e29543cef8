"""GPU (-m gpu): the camera pose gradient -- ``viewmats.grad`` of ``fully_fused_projection`` and ``rasterization`` -- and the
camera optimizer on top of it, against the project's fp64 autograd oracle (``V.requires_grad_()`` there).  Error measure:
``helpers.rel_err`` (tensor-inf-norm).  Bars: 1e-4, the project's bar for every gradient; for the projection alone
``min(1e-4, max(8 e32, 1e-5))`` with e32 the error of the same oracle run in fp32 on the CPU against its fp64 self (the
factor 8 is the margin tests/test_adam_gpu.py gives a kernel whose operation order differs from torch's)."""
import functools

import numpy as np
import pytest
import torch

from helpers import rel_err, small_scene, upstream

pytestmark = pytest.mark.gpu
TOL = 1e-4
SHIFT = (0.2, 0.1, -0.1)
PROJ_KEYS = ("means2d", "depths", "conics", "compensations", "ray_ts", "ray_planes", "normals")
# The third camera of the projection test is the first pushed forward along its axis by PUSH: on small_scene(seed=1) (depths
# 1.8 .. 7.8 in that camera) the near plane then culls 36 % of the Gaussians (asserted below to lie in 1/4 .. 3/4).  The rows
# just in front of the plane (z ~ 0.01) carry gradients ~ 1 / z^3: that camera's sum is badly conditioned and e32 says by how much.
PUSH = 3.75


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from collab_splats_amd import load_library
    load_library()
    return torch.device("cuda:0")


def _views(sc, n):
    V0 = sc["viewmat"]
    V1 = V0.clone()
    V1[:3, 3] += torch.tensor(SHIFT, dtype=V0.dtype)
    V2 = V0.clone()
    V2[2, 3] -= PUSH
    return torch.stack([V0, V1, V2])[:n].contiguous()


# ----------------------------------------------------------------------------- 1. projection alone

def _oracle_project(sc, V, ups, masks, dt):
    """sum over cameras and the seven float outputs of <output, upstream> over the rows of ``masks``; gradients of it."""
    from oracle import torch_oracle as O
    ins = [sc[k].to(dt).clone().requires_grad_(True) for k in ("means", "quats", "scales")]
    Vl = V.to(dt).clone().requires_grad_(True)
    loss, valid = 0.0, []
    for c in range(V.shape[0]):
        pr = O.project(*ins, Vl[c], sc["K"].to(dt), sc["W"], sc["H"], None, O.RasterSpec(), calc_compensations=True)
        valid.append(pr["valid"])
        m = masks[c].to(dt)
        for k, u in zip(PROJ_KEYS, ups):
            loss = loss + (pr[k] * u[c].to(dt) * (m if pr[k].dim() == 1 else m[:, None])).sum()
    loss.backward()
    return Vl.grad, torch.stack(valid)


def _gpu_project(sc, V, ups, dev, pose: bool):
    from collab_splats_amd import fully_fused_projection
    ins = [sc[k].float().to(dev).requires_grad_(True) for k in ("means", "quats", "scales")]
    Vl = V.float().to(dev).requires_grad_(pose)
    C = V.shape[0]
    res = fully_fused_projection(ins[0], None, ins[1], ins[2], Vl, sc["K"].float()[None].expand(C, 3, 3).contiguous().to(dev),
                                 sc["W"], sc["H"], calc_compensations=True)
    torch.autograd.backward(list(res[1:]), [u.float().to(dev) for u in ups])
    return res[0], Vl.grad, [t.grad for t in ins]


@pytest.mark.parametrize("N,C,W,H", [(1, 1, 48, 40), (255, 1, 48, 40), (256, 1, 48, 40), (257, 1, 48, 40), (70001, 3, 640, 360)])
def test_projection_viewmat_gradient(dev, N, C, W, H):
    """Measured on MI355X (error of viewmats.grad per camera / e32 / bar): see DESIGN.md section 28."""
    sc = small_scene(n=N, W=W, H=H, seed=1)
    V = _views(sc, C)
    g = torch.Generator().manual_seed(11)
    shapes = [(C, N, 2), (C, N), (C, N, 3), (C, N), (C, N), (C, N, 2), (C, N, 3)]
    ups = [torch.rand(s, generator=g, dtype=torch.float64) - 0.5 for s in shapes]       # signed: the sums cancel
    radii, v_V, grads = _gpu_project(sc, V, ups, dev, True)
    vis = ((radii[..., 0] > 0) | (radii[..., 1] > 0)).cpu()
    # the oracle has no culling of its own in the backward: it is given the upstreams of the rows the forward kept (the
    # kernels get them unmasked -- culled rows must contribute nothing by themselves).  The forward's visibility is an
    # integer stage held elsewhere to the fp32 restatement; against fp64 it may differ on rounding boundaries only
    want, valid64 = _oracle_project(sc, V, ups, vis, torch.float64)
    assert int((valid64 != vis).sum()) <= 4
    assert int(vis[0].sum()) >= 1
    if C == 3:
        culled = 1.0 - float(valid64[2].sum()) / N
        assert 0.25 <= culled <= 0.75, culled
    want32, _ = _oracle_project(sc, V, ups, vis, torch.float32)
    assert v_V is not None and v_V.shape == (C, 4, 4) and v_V.dtype == torch.float32
    assert not v_V[:, 3, :].any()                                                      # the bottom row is written, as zeros
    for c in range(C):                                                                 # per camera: each against its own scale
        e32 = rel_err(want32[c], want[c])
        bar = min(1e-4, max(8 * e32, 1e-5))
        err = rel_err(v_V[c], want[c])
        print(f"[posegrad] projection N={N} camera {c}: err {err:.3e}  e32 {e32:.3e}  bar {bar:.3e}  visible {int(vis[c].sum())}")
        assert err <= bar, (c, err, e32, bar)
    assert rel_err(v_V, want) <= min(1e-4, max(8 * rel_err(want32, want), 1e-5))       # and the tensor as a whole
    # the other gradients of the same call are those of the call without a pose gradient, bit for bit
    _, none, plain = _gpu_project(sc, V, ups, dev, False)
    assert none is None
    for a, b in zip(grads, plain):
        assert torch.equal(a, b)
    # two runs give the same bits
    _, again, _ = _gpu_project(sc, V, ups, dev, True)
    assert torch.equal(again, v_V)


def test_projection_viewmat_gradient_of_an_empty_scene(dev):
    sc = small_scene(n=1, seed=1)
    sc = dict(sc, means=sc["means"][:0], quats=sc["quats"][:0], scales=sc["scales"][:0])
    V = _views(sc, 2)
    ups = [torch.zeros(s, dtype=torch.float64) for s in [(2, 0, 2), (2, 0), (2, 0, 3), (2, 0), (2, 0), (2, 0, 2), (2, 0, 3)]]
    _, v_V, _ = _gpu_project(sc, V, ups, dev, True)
    assert v_V.shape == (2, 4, 4) and not v_V.any()


# ----------------------------------------------------------------------------- 2. whole rasterizer

NAMES = ("means", "quats", "scales", "opacities", "sh")


def _scene():
    return small_scene(n=400, W=70, H=52, seed=1)


def _kw(mode="antialiased"):
    return dict(render_mode="RGB+ED", rasterize_mode=mode)


@functools.lru_cache(maxsize=None)
def _oracle_forward(C: int, variant: str):
    """The fp64 oracle's forward, once per (cameras, variant); ``leaves`` in NAMES order (+ extras), then V."""
    from oracle import torch_oracle as O
    sc = _scene()
    V = _views(sc, C).clone().requires_grad_(True)
    K = sc["K"][None].expand(C, 3, 3)
    lv = {k: sc[k].clone().requires_grad_(True) for k in NAMES}
    if variant == "sh3":
        ref = O.rasterization(*[lv[k] for k in NAMES], V, K, 70, 52, sh_degree=3, **_kw())
    elif variant == "rgb_classic":
        lv["sh"] = (sc["sh"][:, 0] * 0.5 + 0.5).clone().requires_grad_(True)            # [N,3] colours
        ref = O.rasterization(*[lv[k] for k in NAMES], V, K, 70, 52, sh_degree=None, **_kw("classic"))
    elif variant == "features":
        lv["features"] = torch.rand(400, 13, generator=torch.Generator().manual_seed(9), dtype=torch.float64).requires_grad_(True)
        cam_c = -(V[0, :3, :3].T @ V[0, :3, 3])
        rgb = torch.clamp_min(O.eval_sh(3, lv["means"] - cam_c, lv["sh"]) + 0.5, 0.0)
        cols = torch.cat((rgb, lv["features"]), dim=-1)
        ref = O.rasterization(lv["means"], lv["quats"], lv["scales"], lv["opacities"], cols, V, K, 70, 52, sh_degree=None, **_kw())
    elif variant == "raw":
        lv["scales"] = torch.log(sc["scales"]).clone().requires_grad_(True)
        lv["opacities"] = torch.logit(sc["opacities"]).clone().requires_grad_(True)
        ref = O.rasterization(lv["means"], lv["quats"], torch.exp(lv["scales"]), torch.sigmoid(lv["opacities"]), lv["sh"], V, K,
                              70, 52, sh_degree=3, **_kw())
    else:
        raise KeyError(variant)
    return ref[:5], lv, V


@functools.lru_cache(maxsize=None)
def _oracle_grads(C: int, variant: str, signed: bool):
    outs, lv, V = _oracle_forward(C, variant)
    ups = _ups(C, outs, signed)
    leaves = list(lv.values()) + [V]
    grads = torch.autograd.grad(list(outs), leaves, ups, retain_graph=True)
    return dict(zip(list(lv.keys()) + ["viewmats"], grads)), [o.detach() for o in outs]


def _ups(C, outs, signed):
    ups = upstream([t.shape for t in outs])
    return [u - 0.5 for u in ups] if signed else ups


def _gpu_leaves(lv, dev):
    return {k: v.detach().float().to(dev).requires_grad_(True) for k, v in lv.items()}


def _check(got: dict, want: dict, what):
    for k, w in want.items():
        err = rel_err(got[k], w)
        print(f"[posegrad] {what}: {k} err {err:.3e}")
        assert err < TOL, (what, k, err)


@pytest.mark.parametrize("C,signed", [(1, False), (1, True), (2, False), (2, True)])
def test_rasterization_viewmat_gradient(dev, C, signed):
    """Measured on MI355X: see DESIGN.md section 28 (the fp32 oracle's own error on viewmats.grad: 1.2e-6 for C = 1 and
    1.0e-6 for C = 2 with unsigned upstreams, 4.5e-6 for C = 1 signed)."""
    from collab_splats_amd import ops, rasterization
    want, ref_outs = _oracle_grads(C, "sh3", signed)
    _, lv, V64 = _oracle_forward(C, "sh3")
    sc = _scene()
    lf = _gpu_leaves(lv, dev)
    V = V64.detach().float().to(dev).requires_grad_(True)
    K = sc["K"].float()[None].expand(C, 3, 3).contiguous().to(dev)
    before = ops.PATH_STATS["forward"]
    out = rasterization(*[lf[k] for k in NAMES], V, K, 70, 52, sh_degree=3, return_depth_normal=True, **_kw())
    assert ops.PATH_STATS["forward"] == before                                         # not the fused node
    for got, w in zip(out[:5], ref_outs):
        assert rel_err(got, w) < TOL
    torch.autograd.backward(list(out[:5]), [u.float().to(dev) for u in _ups(C, ref_outs, signed)])
    got = {k: lf[k].grad for k in NAMES}
    got["viewmats"] = V.grad
    assert V.grad is not None and V.grad.shape == (C, 4, 4) and not V.grad[:, 3].any()
    _check(got, want, f"rasterization C={C} signed={signed}")
    if C == 1:
        # translating the camera is translating the scene: v_t = Rw sum_g v_mean[g] (exact in the oracle, SH term included)
        tie = V.detach()[0, :3, :3].double().cpu() @ lf["means"].grad.double().sum(0).cpu()
        err = rel_err(V.grad[0, :3, 3], tie)
        print(f"[posegrad] rasterization C=1 signed={signed}: translation identity err {err:.3e}")
        assert err < TOL
        assert rel_err(want["viewmats"][0, :3, 3], V64.detach()[0, :3, :3] @ want["means"].sum(0)) < 1e-10


def test_rasterization_viewmat_gradient_plain_colours_classic(dev):
    from collab_splats_amd import rasterization
    want, ref_outs = _oracle_grads(1, "rgb_classic", False)
    _, lv, V64 = _oracle_forward(1, "rgb_classic")
    lf = _gpu_leaves(lv, dev)
    V = V64.detach().float().to(dev).requires_grad_(True)
    K = _scene()["K"].float()[None].to(dev)
    out = rasterization(*[lf[k] for k in NAMES], V, K, 70, 52, sh_degree=None, return_depth_normal=True, **_kw("classic"))
    torch.autograd.backward(list(out[:5]), [u.float().to(dev) for u in _ups(1, ref_outs, False)])
    got = {k: lf[k].grad for k in NAMES}
    got["viewmats"] = V.grad
    _check(got, want, "plain colours, classic")


# ----------------------------------------------------------------------------- 3. routing

def test_routing_fused_node_without_pose_gradient_staged_path_with_it(dev):
    from collab_splats_amd import ops, rasterization
    _, lv, V64 = _oracle_forward(1, "sh3")
    K = _scene()["K"].float()[None].to(dev)
    ups = [u.float().to(dev) for u in _ups(1, _oracle_forward(1, "sh3")[0], False)]

    def step(pose):
        lf = _gpu_leaves(lv, dev)
        V = V64.detach().float().to(dev).requires_grad_(pose)
        before = dict(ops.PATH_STATS)
        out = rasterization(*[lf[k] for k in NAMES], V, K, 70, 52, sh_degree=3, return_depth_normal=True, **_kw())
        torch.autograd.backward(list(out[:5]), ups)
        took = {k: ops.PATH_STATS[k] - before.get(k, 0) for k in ops.PATH_STATS}
        return took, V, lf

    took, V, _ = step(False)
    assert took["forward"] == 1 and took.get("backward_one_call", 0) + took.get("backward_staged", 0) == 1, took
    assert V.grad is None
    took, V, _ = step(True)
    assert took["forward"] == 0 and took.get("backward_one_call", 0) + took.get("backward_staged", 0) == 0, took
    assert V.grad is not None
    # no gradient mode, no pose path: the fused node again
    before = ops.PATH_STATS["forward"]
    with torch.no_grad():
        lf = _gpu_leaves(lv, dev)
        rasterization(*[lf[k] for k in NAMES], V, K, 70, 52, sh_degree=3, return_depth_normal=True, **_kw())
    assert ops.PATH_STATS["forward"] == before + 1


def test_packed_nodes_refuse_a_pose_gradient(dev):
    from collab_splats_amd import _lib, ops
    _, lv, V64 = _oracle_forward(1, "sh3")
    lf = _gpu_leaves(lv, dev)
    V = V64.detach().float().to(dev).requires_grad_(True)
    K = _scene()["K"].float()[None].to(dev)
    P = _lib.make_params(400, 1, 70, 52, antialiased=True)
    args = [lf[k] for k in NAMES]
    with pytest.raises(NotImplementedError, match="staged path"):
        ops.raster_fused(*args, V, K, P, 3, False, 3, False)
    with pytest.raises(NotImplementedError, match="staged path"):
        ops.project_pack(*args, V, K, P, 3, False)
    wide = torch.rand(400, 16, device=dev)
    with pytest.raises(NotImplementedError, match="staged path"):
        ops.project_pack_x(*args[:4], wide, V, K, P, False, 3)


def test_features_call_with_a_pose_gradient(dev):
    """``features=`` (3 + 13 channels, 17 with the depth): the oracle is fed the concatenated colours."""
    from collab_splats_amd import ops, rasterization
    want, ref_outs = _oracle_grads(1, "features", False)
    _, lv, V64 = _oracle_forward(1, "features")
    lf = _gpu_leaves(lv, dev)
    V = V64.detach().float().to(dev).requires_grad_(True)
    K = _scene()["K"].float()[None].to(dev)
    before = ops.PATH_STATS["forward"]
    out = rasterization(*[lf[k] for k in NAMES], V, K, 70, 52, sh_degree=3, features=lf["features"], return_depth_normal=True,
                        **_kw())
    assert ops.PATH_STATS["forward"] == before and out[0].shape == (1, 52, 70, 17)
    for got, w in zip(out[:5], ref_outs):
        assert rel_err(got, w) < TOL
    torch.autograd.backward(list(out[:5]), [u.float().to(dev) for u in _ups(1, ref_outs, False)])
    got = {k: v.grad for k, v in lf.items()}
    got["viewmats"] = V.grad
    _check(got, want, "features=")


def test_split_colours_with_a_pose_gradient(dev):
    from collab_splats_amd import rasterization
    want, ref_outs = _oracle_grads(1, "sh3", False)
    _, lv, V64 = _oracle_forward(1, "sh3")
    lf = _gpu_leaves(lv, dev)
    dc = lv["sh"].detach()[:, 0].float().contiguous().to(dev).requires_grad_(True)
    rest = lv["sh"].detach()[:, 1:].float().contiguous().to(dev).requires_grad_(True)
    V = V64.detach().float().to(dev).requires_grad_(True)
    K = _scene()["K"].float()[None].to(dev)
    out = rasterization(lf["means"], lf["quats"], lf["scales"], lf["opacities"], (dc, rest), V, K, 70, 52, sh_degree=3,
                        return_depth_normal=True, **_kw())
    torch.autograd.backward(list(out[:5]), [u.float().to(dev) for u in _ups(1, ref_outs, False)])
    got = {k: lf[k].grad for k in NAMES[:4]}
    got["sh"] = torch.cat((dc.grad[:, None], rest.grad), dim=1)
    got["viewmats"] = V.grad
    _check(got, want, "(features_dc, features_rest)")


def test_raw_parameters_with_a_pose_gradient(dev):
    """``scales_are_log`` / ``opacities_are_logit``: off the one-node path the activations are torch's."""
    from collab_splats_amd import rasterization
    want, ref_outs = _oracle_grads(1, "raw", False)
    _, lv, V64 = _oracle_forward(1, "raw")
    lf = _gpu_leaves(lv, dev)
    V = V64.detach().float().to(dev).requires_grad_(True)
    K = _scene()["K"].float()[None].to(dev)
    out = rasterization(*[lf[k] for k in NAMES], V, K, 70, 52, sh_degree=3, scales_are_log=True, opacities_are_logit=True,
                        return_depth_normal=True, **_kw())
    torch.autograd.backward(list(out[:5]), [u.float().to(dev) for u in _ups(1, ref_outs, False)])
    got = {k: lf[k].grad for k in NAMES}
    got["viewmats"] = V.grad
    _check(got, want, "raw parameters")


def test_means2d_retain_grad_and_absgrad_on_the_pose_path(dev):
    from collab_splats_amd import rasterization
    _, lv, V64 = _oracle_forward(1, "sh3")
    K = _scene()["K"].float()[None].to(dev)

    def run(pose):
        lf = _gpu_leaves(lv, dev)
        V = V64.detach().float().to(dev).requires_grad_(pose)
        out = rasterization(*[lf[k] for k in NAMES], V, K, 70, 52, sh_degree=3, absgrad=True, return_depth_normal=True, **_kw())
        meta = out[5]
        meta["means2d"].retain_grad()
        out[0].sum().backward()
        return meta["means2d"].grad, meta["means2d"].absgrad, V.grad

    g, a, v_V = run(True)
    g0, a0, none = run(False)                                                          # the fused node's, same call
    assert v_V is not None and none is None
    assert g.shape == (1, 400, 2) and a.shape == (1, 400, 2) and float(a.sum()) > 0
    assert rel_err(g, g0) < TOL and rel_err(a, a0) < TOL


# ----------------------------------------------------------------------------- 4. pose recovery

def test_pose_recovery(dev):
    """80 Adam steps on a perturbed camera recover the pose the target was rendered from.  CONDITIONS, set from the fp64
    oracle run with exactly this set-up on the CPU (loss 0.0634 -> 0.00093, translation error 0.0399 -> 0.00074, rotation
    error 0.0194 -> 0.00024): a wrong sign, a transposed rotation block or a missing SH term does not get there."""
    from collab_splats_amd import CameraOptimizer, rasterization
    sc = _scene()
    args = [sc[k].float().to(dev) for k in NAMES]
    V0 = sc["viewmat"].float()[None].to(dev)
    K = sc["K"].float()[None].to(dev)
    kw = dict(sh_degree=3, render_mode="RGB", rasterize_mode="antialiased")
    target = rasterization(*args, V0, K, 70, 52, **kw)[0].detach()
    co = CameraOptimizer(1, "SO3xR3").to(dev)
    xi0 = torch.tensor([0.03, -0.02, 0.02, 0.01, -0.015, 0.01], device=dev)
    with torch.no_grad():
        co.pose_adjustment.copy_(xi0[None])
    opt = torch.optim.Adam(co.parameters(), lr=2e-3)
    losses = []
    for _ in range(80):
        opt.zero_grad()
        loss = (rasterization(*args, co.apply_to_viewmat(V0, 0), K, 70, 52, **kw)[0] - target).abs().mean()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    with torch.no_grad():
        end = (rasterization(*args, co.apply_to_viewmat(V0, 0), K, 70, 52, **kw)[0] - target).abs().mean()
    xi = co.pose_adjustment.detach()[0]
    start = float(losses[0])
    print(f"[posegrad] recovery: loss {start:.5f} -> {float(end):.5f}, translation {float(xi0[:3].norm()):.5f} -> "
          f"{float(xi[:3].norm()):.5f}, rotation {float(xi0[3:].norm()):.5f} -> {float(xi[3:].norm()):.5f}")
    assert float(end) < start / 10
    assert float(xi[:3].norm()) < float(xi0[:3].norm()) / 4
    assert float(xi[3:].norm()) < float(xi0[3:].norm()) / 4


# ----------------------------------------------------------------------------- 5. model

def _model(dev, **cfg):
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 240, 136, 6000
    sc = random_scene(N, W, H, seed=2)
    args = (sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0], sc["sh"][:, 1:])
    extra = {"num_train_data": 3} if cfg.get("camera_optimizer_mode", "off") != "off" else {}
    model = radegs.RadegsModel(radegs.RadegsModelConfig(rasterize_mode="antialiased", regularization_from_iter=0, **cfg),
                               *args, **extra).to(dev).train()
    model.step = 5000
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 0]])
    cam = radegs.PinholeCamera.make(c2w, 0.9 * W, 0.9 * W, W, H)
    cam.metadata = {"cam_idx": 1}
    return model, cam, (H, W)


def test_model_trains_the_pose_of_the_rendered_camera(dev):
    model, cam, (H, W) = _model(dev, camera_optimizer_mode="SO3xR3", camera_opt_trans_l2_penalty=0.0,
                                camera_opt_rot_l2_penalty=0.0)
    batch = {"image": torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5))}
    out = model.get_outputs(cam)
    loss = model.get_loss_dict(out, batch)
    assert "camera_opt_regularizer" in loss and float(loss["camera_opt_regularizer"].detach()) == 0.0
    sum(loss.values()).backward()
    g = model.camera_optimizer.pose_adjustment.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g[1].abs().sum()) > 0
    assert not g[0].any() and not g[2].any()                                           # exact zeros: the other cameras
    for k, p in model.gauss_params.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0, k
    # with the default penalties the regulariser is a finite number with a finite gradient at the start
    model2, _, _ = _model(dev, camera_optimizer_mode="SE3")
    loss2 = model2.get_loss_dict(model2.get_outputs(cam), batch)
    sum(loss2.values()).backward()
    g2 = model2.camera_optimizer.pose_adjustment.grad
    assert bool(torch.isfinite(g2).all()) and float(g2[1].abs().sum()) > 0
    # evaluation renders the stored pose: bitwise the outputs of a model without the optimizer
    with torch.no_grad():
        model.camera_optimizer.pose_adjustment[1] = torch.tensor([0.05, 0.0, -0.03, 0.01, 0.02, 0.0], device=dev)
    plain, _, _ = _model(dev)
    moved = model.get_outputs(cam)["rgb"].detach()
    assert not torch.equal(moved, plain.get_outputs(cam)["rgb"].detach())              # training: the refined pose
    model.eval(), plain.eval()
    with torch.no_grad():
        a, b = model.get_outputs(cam), plain.get_outputs(cam)
    for k in b:
        if torch.is_tensor(b[k]):
            assert torch.equal(a[k], b[k]), k


def test_model_with_the_mode_off_is_unchanged(dev):
    default, cam, _ = _model(dev)
    explicit, _, _ = _model(dev, camera_optimizer_mode="off")
    assert not hasattr(default, "camera_optimizer") and not hasattr(explicit, "camera_optimizer")
    a, b = default.get_outputs(cam), explicit.get_outputs(cam)
    cam.metadata = None
    c = default.get_outputs(cam)
    assert set(a) == set(b) == set(c)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    assert set(default.get_param_groups()) == set(explicit.get_param_groups())
