"""No GPU: the two references against each other under the cameras and parameters of camera_cases.py, and the floors that
keep every case of test_cameras_gpu.py from going empty."""
import numpy as np
import pytest
import torch

import camera_cases as cc
from helpers import rel_err, small_scene, upstream
from oracle import torch_oracle as O
from oracle.craster import CRaster

KEYS = ("means", "quats", "scales", "opacities", "sh")


def _c_port_vs_autograd_fp64(sc, K, V, W, H, mode, spec, min_isects):
    """The bars of test_oracle.py::test_c_port_matches_autograd_oracle_fp64: integer stages equal, images < 1e-12,
    gradients < 1e-11."""
    ins = [sc[k].double().clone().requires_grad_(True) for k in KEYS]
    Vt, Kt = torch.from_numpy(V).double(), torch.from_numpy(K).double()
    r, a, ed, md, n, meta = O.rasterization(*ins, Vt[None], Kt[None], W, H, sh_degree=3, render_mode="RGB+ED",
                                            rasterize_mode=mode, **cc.oracle_kwargs(spec))
    ups = upstream([t.shape for t in (r, a, ed, md, n)])
    torch.autograd.backward([r, a, ed, md, n], ups)
    cr = CRaster(np.float64)
    st = cr.forward(*[t.detach().numpy() for t in ins], Vt.numpy(), Kt.numpy(), W, H, sh_degree=3, render_mode="RGB+ED",
                    rasterize_mode=mode, **spec)
    assert np.array_equal(st["proj"]["radii"], meta["radii"][0].numpy())
    assert np.array_equal(st["bins"]["isect_ids"], meta["isect_ids"])
    assert np.array_equal(st["bins"]["flatten_ids"], meta["flatten_ids"])
    assert np.array_equal(st["bins"]["isect_offsets"], meta["isect_offsets"][0])
    for key in ("last_ids", "median_ids"):                  # (tile-sorted list there, depth-sorted visible list here: compare ids)
        c_idx = st["fwd"][key]
        c_gid = np.where(c_idx >= 0, st["bins"]["flatten_ids"][np.maximum(c_idx, 0)], -1)
        t_idx = meta[key][0].numpy()
        t_gid = np.where(t_idx >= 0, meta["order_ids"][0][np.maximum(t_idx, 0)], -1)
        assert np.array_equal(c_gid, t_gid), key
    assert st["bins"]["n_isects"] >= min_isects, st["bins"]["n_isects"]
    for got, ref in ((st["render"], r), (st["fwd"]["alpha"], a), (st["fwd"]["exp_depth"], ed),
                     (st["fwd"]["med_depth"], md), (st["fwd"]["normal"], n)):
        assert rel_err(got, ref[0]) < 1e-12
    gr = cr.backward(st, *[u[0].numpy() for u in ups])
    for name, t in zip(("v_means", "v_quats", "v_scales", "v_opacities", "v_colors"), ins):
        assert rel_err(gr[name], t.grad) < 1e-11, name
    return st


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("name", cc.CASES)
def test_cameras_c_port_matches_autograd_oracle_fp64(name, mode):
    W, H = 48, 40
    sc = small_scene(W=W, H=H)
    # small_scene was drawn for f = 1.25 W and lies between z = 1.5 and 7.5: behind_camera pulls it by 3
    K, V, spec = cc.case(name, W, H, f=1.25, z_shift=-3.0)
    st = _c_port_vs_autograd_fp64(sc, K, V, W, H, mode, spec, min_isects=80)
    cond = cc.conditions(name, st, CRaster(np.float64))
    if "near_plane" in spec or name == "behind_camera":
        assert cond["outside_planes"] >= 40, cond
    if "alpha_max" in spec:
        assert cond["alpha_share"] >= cc.MIN_ALPHA_SHARE, cond
    if name == "radius_clip":
        assert cond["clipped"] >= 50, cond


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("name", list(cc.GROWN_KS))
def test_cameras_grown_frame_c_port_matches_autograd_oracle_fp64(name, mode):
    """The Jacobian clamp on all four sides (the four limits differ with an off-centre principal point)."""
    W, H = 48, 40
    K, V, spec = cc.case(name, W, H)
    sc = cc.grown_frame_scene(600, W, H, K)
    st = _c_port_vs_autograd_fp64(sc, K, V, W, H, mode, spec, min_isects=100)
    cond = cc.conditions(name, st)
    assert min(cond["clamped"]) >= 1 and sum(cond["clamped"]) >= 15, cond    # (every side runs; the GPU size has >= 10 each)


@pytest.mark.parametrize("name", cc.CASES + tuple(cc.GROWN_KS))
def test_cameras_conditions_hold_at_the_gpu_tests_size(name):
    """fp32 C port, forward only, at the shapes of test_cameras_gpu.py: every case keeps what it is there to exercise."""
    W, H = 200, 120
    K, V, spec = cc.case(name, W, H)
    sc = cc.grown_frame_scene(3000, W, H, K) if name in cc.GROWN_KS else cc.posed_scene(4000, W, H)
    cr = CRaster(np.float32)
    st = cr.forward(*[sc[k].numpy() for k in KEYS], V, K, W, H, sh_degree=3, render_mode="RGB+ED",
                    rasterize_mode=cc.mode_of(name), **spec)
    cond = cc.check_conditions(name, cc.conditions(name, st, cr))
    print(cond)
    if name in cc.GROWN_KS:
        # the clamped rows carry gradients of the order of the tensor's maximum: a wrong clamp term cannot hide in them
        ups = upstream([(H, W, 4), (H, W, 1), (H, W, 1), (H, W, 1), (H, W, 3)], dtype=torch.float32)
        gr = cr.backward(st, *[u.numpy() for u in ups])
        P = st["P"]
        u_ = sc["means"][:, 0].numpy() / sc["means"][:, 2].numpy()
        v_ = sc["means"][:, 1].numpy() / sc["means"][:, 2].numpy()
        tx, ty = 0.5 * W / P.fx, 0.5 * H / P.fy
        cl = ((u_ > (W - P.cx) / P.fx + 0.3 * tx) | (u_ < -(P.cx / P.fx + 0.3 * tx))
              | (v_ > (H - P.cy) / P.fy + 0.3 * ty) | (v_ < -(P.cy / P.fy + 0.3 * ty))) & (st["proj"]["radii"] > 0).all(-1)
        assert np.abs(gr["v_means"][cl]).max() > 0.05 * np.abs(gr["v_means"]).max()


def test_cameras_make_params_refuses_another_tile_size():
    from collab_splats_amd._lib import make_params
    with pytest.raises(ValueError):
        make_params(10, 1, 64, 48, tile_size=8)
    assert make_params(10, 1, 64, 48, tile_size=16).tile_w == 4
