"""GPU (-m gpu): the colour configurations the reference trains with besides SH degree 3.

* ``spherical_harmonics`` (the drop-in the reference's features model calls when ``sh_degree > 0``), forward AND backward,
  against the fp64 autograd restatement ``oracle.torch_oracle.eval_sh``;
* SH degrees 0, 1 and 2 from 16-coefficient storage (the first 3 000 steps of every ``rade-gs`` run: ``sh_degree_to_use =
  min(step // 1000, 3)``) on the dense training path -- on-demand SH in the compositing forward, the sparse SH backward,
  rows cleared on touch, background fill -- in steady state against the C port; the degree switch under graph replay; the
  generic-K colour kernel (K = 1 / 4 / 9, and a misaligned K = 16 view);
* the degree-0 features call: ``rade-features`` trains at ``sh_degree=0``, so its call is ``rasterization(colors=
  cat(sigmoid(features_dc), features[N,13]), sh_degree=None)`` -- 16 pass-through channels, 17 with ``RGB+ED`` --, in steady
  state against the C port, and the degree-0 features model built around it.

Bars as in test_parity_gpu.py: integer stages bit-exact against the fp32 C port, images and gradients within 1e-4
tensor-inf-norm relative or a threshold flip proven by ``FlipProof``; every claim that a path ran is read off
``ops.PATH_STATS``.
"""
import math

import numpy as np
import pytest
import torch

from helpers import FULL_SIZE, FlipProof, assert_close_flips, rel_err, upstream

pytestmark = pytest.mark.gpu
TOL = 1e-4
F = 13                                   # the reference's distilled feature width (3 + 13 = 16 fused channels)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from collab_splats_amd import load_library
    load_library()
    return torch.device("cuda:0")


def _poison(dev, n_rows, widths=(48, 45, 16, 13, 4, 3)):
    """Seed the caching allocator with NaNs at the sizes of the per-Gaussian gradient tensors: a row that a kernel should
    have written (zeros included) and did not then shows up as NaN rather than as a lucky zero."""
    pool = [torch.full((n_rows * w + 64 * k,), float("nan"), device=dev) for w in widths for k in range(2)]
    del pool


def _sh_oracle(deg, dirs, coeffs, v_out):
    """fp64 autograd of eval_sh: (colours, v_coeffs, v_dirs) -- coeffs broadcast over leading camera axes, so v_coeffs is the
    sum over cameras."""
    from oracle.torch_oracle import eval_sh
    d64 = dirs.detach().double().cpu().requires_grad_(True)
    c64 = coeffs.detach().double().cpu().requires_grad_(True)
    out = eval_sh(deg, d64, c64)
    out.backward(v_out.detach().double().cpu())
    return out.detach(), c64.grad, d64.grad


# ================================================================ B. spherical_harmonics forward + backward vs fp64
@pytest.mark.parametrize("deg,K", [(0, 1), (0, 16), (1, 4), (1, 16), (1, 25), (2, 9), (2, 16), (3, 16), (3, 25), (0, 25)])
def test_spherical_harmonics_forward_backward_vs_fp64(dev, deg, K):
    """The wrapper with leading batch shapes [2, 3, 707]: colours within 1e-5, ``v_coeffs`` / ``v_dirs`` within 1e-4 of fp64
    autograd, and every coefficient above the active degree gets exactly 0.0 (the gradient tensor is allocated over NaNs)."""
    from collab_splats_amd import spherical_harmonics
    g = torch.Generator().manual_seed(10 * deg + K)
    lead = (2, 3, 707)
    dirs = (torch.randn(lead + (3,), generator=g) * torch.rand(lead + (1,), generator=g) * 4).to(dev).requires_grad_(True)
    coeffs = (torch.randn(lead + (K, 3), generator=g) * 0.5).to(dev).requires_grad_(True)
    v_out = torch.rand(lead + (3,), generator=g) - 0.3
    out = spherical_harmonics(deg, dirs, coeffs)
    assert out.shape == lead + (3,)
    ref, ref_vc, ref_vd = _sh_oracle(deg, dirs, coeffs, v_out)
    assert rel_err(out, ref) < 1e-5, rel_err(out, ref)
    _poison(dev, int(np.prod(lead)), widths=(3 * K, 3))
    out.backward(v_out.to(dev))
    nb = (deg + 1) ** 2
    assert rel_err(coeffs.grad[..., :nb, :], ref_vc[..., :nb, :]) < TOL
    assert rel_err(dirs.grad, ref_vd) < TOL if deg > 0 else not dirs.grad.any()     # (degree 0 does not see the direction)
    above = coeffs.grad[..., nb:, :]
    assert not torch.isnan(above).any() and not above.any(), "coefficients above the active degree must get exactly 0.0"


def test_spherical_harmonics_cameras_mask_and_empty(dev):
    """``spherical_harmonics_raw`` with [C, N, 3] directions and [N, K, 3] coefficients: ``v_coeffs`` is the sum over the
    cameras; under a ``radii`` mask the masked (camera, Gaussian) pairs give colour 0 and no gradient at all -- neither
    ``v_dirs`` nor a share of ``v_coeffs``; N = 0 runs forward and backward."""
    from collab_splats_amd import ops, spherical_harmonics
    g = torch.Generator().manual_seed(3)
    Cn, N, K, deg = 3, 4099, 16, 3
    dirs = (torch.randn(Cn, N, 3, generator=g) * 3).to(dev).requires_grad_(True)
    coeffs = (torch.randn(N, K, 3, generator=g) * 0.5).to(dev).requires_grad_(True)
    radii = torch.randint(0, 4, (Cn, N, 2), generator=g, dtype=torch.int32)
    radii[radii.sum(-1) > 0] += 1
    radii[0, :50] = 0                                             # and a stretch of rows masked in camera 0
    vis = (radii > 0).any(-1)
    assert 0.05 < float((~vis).float().mean()) < 0.5
    v_out = torch.rand(Cn, N, 3, generator=g) - 0.3
    for masked in (False, True):
        dirs.grad = coeffs.grad = None
        out = ops.spherical_harmonics_raw(deg, dirs, coeffs, radii.to(dev) if masked else None)
        m = vis[..., None].double() if masked else torch.ones(Cn, N, 1, dtype=torch.float64)
        ref, ref_vc, ref_vd = _sh_oracle(deg, dirs, coeffs, v_out * m)
        assert rel_err(out, ref * m) < 1e-5
        _poison(dev, Cn * N, widths=(3 * K, 3))
        out.backward(v_out.to(dev))
        assert rel_err(coeffs.grad, ref_vc) < TOL and rel_err(dirs.grad, ref_vd) < TOL
        if masked:
            assert not out[~vis.to(dev)].any() and not dirs.grad[~vis.to(dev)].any()
    # the wrapper's reference signature over the same cameras: the same bits as the raw entry without a mask
    out_w = spherical_harmonics(deg, dirs, coeffs[None].expand(Cn, N, K, 3))
    assert torch.equal(out_w, ops.spherical_harmonics_raw(deg, dirs, coeffs))
    # N = 0
    d0 = torch.zeros(0, 3, device=dev, requires_grad=True)
    c0 = torch.zeros(0, 16, 3, device=dev, requires_grad=True)
    o0 = spherical_harmonics(3, d0, c0)
    assert o0.shape == (0, 3)
    o0.sum().backward()
    assert d0.grad.shape == (0, 3) and c0.grad.shape == (0, 16, 3)


def test_spherical_harmonics_above_2_20_rows_and_zero_length_directions(dev):
    """N = 2^20 + 37 rows (an odd remainder of the 256-wide blocks), degree 3: forward and backward against fp64.  Rows with a
    ZERO-LENGTH direction get the DC term and ``v_dirs = 0`` (the kernel takes 1/|d| = 0 there, so every higher basis function
    is 0).  This differs from gsplat, which normalises the direction without a guard (1/|d| is infinite there, and the
    higher basis functions are not finite): the test pins the behaviour of this build."""
    from collab_splats_amd import spherical_harmonics
    from oracle.torch_oracle import SH_C0
    g = torch.Generator().manual_seed(21)
    N, K, deg = (1 << 20) + 37, 16, 3
    dirs_h = torch.randn(N, 3, generator=g) * 2
    zero = torch.zeros(N, dtype=torch.bool)
    zero[torch.randint(0, N, (500,), generator=g)] = True
    zero[-1] = True                                              # (the last row of the odd remainder)
    dirs_h[zero] = 0.0
    dirs = dirs_h.to(dev).requires_grad_(True)
    coeffs = (torch.randn(N, K, 3, generator=g) * 0.5).to(dev).requires_grad_(True)
    v_out = torch.rand(N, 3, generator=g) - 0.3
    out = spherical_harmonics(deg, dirs, coeffs)
    ref, ref_vc, ref_vd = _sh_oracle(deg, dirs, coeffs, v_out)
    assert rel_err(out, ref) < 1e-5
    zd = zero.to(dev)
    assert torch.allclose(out[zd], SH_C0 * coeffs[zd, 0], rtol=1e-6, atol=0)
    _poison(dev, N, widths=(3 * K, 3))
    out.backward(v_out.to(dev))
    assert rel_err(coeffs.grad, ref_vc) < TOL
    assert rel_err(dirs.grad[~zd], ref_vd[~zero]) < TOL
    assert not dirs.grad[zd].any() and not coeffs.grad[zd, 1:].any()
    assert torch.allclose(coeffs.grad[zd, 0], SH_C0 * v_out[zero].to(dev), rtol=1e-6, atol=0)


@pytest.mark.parametrize("deg", [1, 3])
def test_composed_reference_call_backward_equals_the_one_entry_call(dev, deg):
    """The reference's features call as it composes it -- ``spherical_harmonics`` -> ``clamp_min(+0.5)`` -> ``cat`` with the
    features -> ``rasterization(sh_degree=None)`` -- backpropagated, against the one-entry ``features=`` call on the same
    leaves: images within 1e-5 (geometry bit for bit), coefficient / feature / mean gradients within 1e-4."""
    from collab_splats_amd import rasterization, spherical_harmonics
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 200, 120, 4000
    sc = random_scene(N, W, H, seed=23)
    feats = torch.rand(N, F, generator=torch.Generator().manual_seed(2))
    sh = sc["sh"].clone()
    sh[:, 0] *= 0.4                                              # colours on both sides of the clamp at 0
    geo = [sc["means"], sc["quats"], torch.exp(sc["log_scales"]), torch.sigmoid(sc["opacity_logits"])]
    V, K = sc["viewmats"].to(dev), sc["Ks"].to(dev)
    ups = [u.to(dev) for u in upstream([(1, H, W, 3 + F + 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)],
                                       dtype=torch.float32)]
    kw = dict(render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True)
    res = []
    for composed in (True, False):
        leaves = [t.to(dev).requires_grad_(True) for t in geo]
        c_leaf, f_leaf = sh.to(dev).requires_grad_(True), feats.to(dev).requires_grad_(True)
        if composed:
            cam_c = -(V[0, :3, :3].T @ V[0, :3, 3])
            rgb = torch.clamp_min(spherical_harmonics(deg, leaves[0] - cam_c, c_leaf) + 0.5, 0.0)
            out = rasterization(*leaves, torch.cat((rgb, f_leaf), dim=-1), V, K, W, H, sh_degree=None, **kw)
        else:
            out = rasterization(*leaves, c_leaf, V, K, W, H, sh_degree=deg, features=f_leaf, **kw)
        torch.autograd.backward(list(out[:5]), ups)
        res.append(([t.detach() for t in out[:5]], (c_leaf.grad, f_leaf.grad, leaves[0].grad, leaves[3].grad)))
    (img_c, gr_c), (img_f, gr_f) = res
    for k, (a, b) in enumerate(zip(img_f, img_c)):
        assert torch.equal(a, b) if k > 0 else rel_err(a, b) < 1e-5, k
    for name, a, b in zip(("v_coeffs", "v_features", "v_means", "v_opacities"), gr_f, gr_c):
        assert rel_err(a, b) < TOL, (name, rel_err(a, b))
    nb = (deg + 1) ** 2
    assert not gr_f[0][:, nb:].any() and not gr_c[0][:, nb:].any()


# ================================================================ the steady-state runner and its C-port comparison
def _steady_vs_c_port(dev, craster, monkeypatch, N, W, H, *, deg, colour, lazy="auto", split=False, rm="RGB+ED", view=None,
                      seed=42, scale_mul=1.0, n_calls=8):
    """The training path's steady state -- ONE set of raw leaves (log-scales, logits) reused call after call, merged phases,
    speculative capacity, graph replay, the view's launch order -- compared with the C port on the ``n_calls``-th call.

    ``colour``: "sh" -- ``colors`` = SH coefficients [N,16,3] (or the (features_dc, features_rest) pair), ``sh_degree=deg``;
    "sh+features" -- the same plus ``features=[N,13]`` (the one-entry features call); "d0" -- the degree-0 features call,
    ``colors = cat(sigmoid(features_dc), features)`` [N,16], ``sh_degree=None``.  Returns the PATH_STATS deltas."""
    from collab_splats_amd import ops, rasterization
    from collab_splats_amd.synthetic import random_scene, view_matrix
    from oracle.torch_oracle import eval_sh
    monkeypatch.setattr(ops, "LAZY_SH", lazy)
    assert ops.GRAPHS and ops.MERGE_PHASES and ops.SPECULATE and ops.UNIT_ORDER and ops.FUSED_NODE
    assert not ops.DETERMINISTIC_BACKWARD
    sc = random_scene(N, W, H, seed=seed)
    if view is not None:
        sc["viewmats"] = view_matrix(view)
    sh = sc["sh"].clone()
    if colour != "sh":
        sh[:, 0] *= 0.4                                          # (SH colours on both sides of the clamp at 0)
    feats = torch.rand(N, F, generator=torch.Generator().manual_seed(seed + 1))
    log_s = (sc["log_scales"] + math.log(scale_mul)).contiguous()
    leaves = [t.to(dev).requires_grad_(True) for t in (sc["means"], sc["quats"], log_s, sc["opacity_logits"])]
    if colour == "d0":
        col_leaves = [sh[:, 0].contiguous().to(dev).requires_grad_(True)]          # features_dc: sigmoid logits
    elif split:
        col_leaves = [sh[:, 0].contiguous().to(dev).requires_grad_(True), sh[:, 1:].contiguous().to(dev).requires_grad_(True)]
    else:
        col_leaves = [sh.to(dev).requires_grad_(True)]
    f_leaf = feats.to(dev).requires_grad_(True) if colour != "sh" else None
    all_leaves = leaves + col_leaves + ([f_leaf] if f_leaf is not None else [])
    V, K = sc["viewmats"].to(dev), sc["Ks"].to(dev)
    n_col = 3 + (F if colour != "sh" else 0)
    Dp = n_col + (1 if rm == "RGB+ED" else 0)
    ups = upstream([(1, H, W, Dp), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)
    ups_dev = [u.to(dev) for u in ups]
    ops.reset_graph_cache(dev)
    ops._CAP_HINT.pop(ops._cap_key(ops._lib.make_params(N, 1, W, H), dev), None)
    before = dict(ops.PATH_STATS)
    out = None
    for call in range(n_calls):
        for l in all_leaves:
            l.grad = None
        del out
        _poison(dev, N)
        kw = dict(render_mode=rm, rasterize_mode="antialiased", return_depth_normal=True, scales_are_log=True,
                  opacities_are_logit=True)
        if colour == "d0":
            out = rasterization(*leaves, torch.cat((torch.sigmoid(col_leaves[0]), f_leaf), dim=-1), V, K, W, H,
                                sh_degree=None, **kw)
        else:
            colors = tuple(col_leaves) if split else col_leaves[0]
            out = rasterization(*leaves, colors, V, K, W, H, sh_degree=deg, features=f_leaf, **kw)
        torch.autograd.backward(list(out[:5]), ups_dev)
    torch.cuda.synchronize()
    took = {k: ops.PATH_STATS[k] - before.get(k, 0) for k in ops.PATH_STATS}
    # ---- the machinery was ON for the call that is compared
    assert took.get("forward") == n_calls and took.get("backward_one_call") == n_calls and took.get("backward_staged", 0) == 0, took
    assert took.get("forward_merged_phases", 0) == n_calls and took.get("forward_probe", 0) == 1, took
    assert took.get("forward_view_order", 0) == n_calls and took.get("capacity_redo", 0) == 0, took
    assert took.get("forward_nd", 0) == (n_calls if colour != "sh" else 0), took
    gs = ops.graph_cache_stats(dev)
    assert gs["hits"] >= 1 and gs["captures"] >= 1, gs
    r, a, ed, md, n, meta = out
    assert r.shape == (1, H, W, Dp)
    # ---- the C port on the activated values as the device computes them, colours as the reference would feed gsplat
    cr = craster.CRaster(np.float32)
    scales_np = torch.exp(leaves[2].detach()).cpu().numpy()
    op_np = torch.sigmoid(leaves[3].detach()).cpu().numpy()
    cam_c = -(sc["viewmats"][0, :3, :3].T @ sc["viewmats"][0, :3, 3])
    if colour == "sh":
        cols, c_deg = sh.numpy(), deg
    elif colour == "sh+features":
        means64, sh64, feats64 = (t.double().requires_grad_(True) for t in (sc["means"], sh, feats))
        fused64 = torch.cat((torch.clamp_min(eval_sh(deg, means64 - cam_c.double(), sh64) + 0.5, 0.0), feats64), dim=-1)
        cols, c_deg = fused64.detach().float().numpy(), None
    else:
        cols = torch.cat((torch.sigmoid(col_leaves[0].detach()), f_leaf.detach()), dim=-1).cpu().numpy()
        c_deg = None
    st = cr.forward(sc["means"].numpy(), sc["quats"].numpy(), scales_np, op_np, cols, sc["viewmats"][0].numpy(),
                    sc["Ks"][0].numpy(), W, H, sh_degree=c_deg, render_mode=rm, rasterize_mode="antialiased")
    assert np.array_equal(st["proj"]["radii"], meta["radii"][0].cpu().numpy())
    assert np.array_equal(st["proj"]["depths"].view(np.uint32), meta["depths"][0].detach().cpu().numpy().view(np.uint32))
    assert np.array_equal(st["proj"]["means2d"].view(np.uint32), meta["means2d"][0].detach().cpu().numpy().view(np.uint32))
    assert st["bins"]["n_isects"] == meta["n_isects"]
    assert np.array_equal(st["bins"]["flatten_ids"], meta["flatten_ids"].cpu().numpy())
    assert np.array_equal(st["bins"]["isect_offsets"], meta["isect_offsets"][0].cpu().numpy())
    assert np.array_equal(st["bins"]["isect_ids"], meta["isect_ids"].cpu().numpy().view(np.uint64))
    fw = st["fwd"]
    proof = FlipProof(cr.blend_margin(st), st["proj"]["means2d"], st["proj"]["radii"])
    for name, got, ref in (("render", r, st["render"]), ("alpha", a, fw["alpha"]), ("exp_depth", ed, fw["exp_depth"]),
                           ("med_depth", md, fw["med_depth"]), ("normal", n, fw["normal"])):
        assert_close_flips(got[0], ref, name, proof=proof)
    proof.check_ids(meta["last_ids"][0].cpu().numpy(), fw["last_ids"], meta["median_ids"][0].cpu().numpy(), fw["median_ids"])
    gr = cr.backward(st, *[u[0].numpy() for u in ups])
    want = dict(v_means=gr["v_means"], v_quats=gr["v_quats"], v_log_scales=gr["v_scales"] * scales_np,
                v_opacity_logits=gr["v_opacities"] * op_np * (1.0 - op_np))
    if colour == "sh":
        got_col = {"v_sh": torch.cat((col_leaves[0].grad[:, None, :], col_leaves[1].grad), dim=1) if split else col_leaves[0].grad}
        want_col = {"v_sh": gr["v_colors"]}
    elif colour == "sh+features":
        fused64.backward(torch.from_numpy(gr["v_colors"]).double())
        if deg > 0:                                              # + the SH view-direction term (none at degree 0)
            want["v_means"] = gr["v_means"] + means64.grad.float().numpy()
        got_col = {"v_sh": torch.cat((col_leaves[0].grad[:, None, :], col_leaves[1].grad), dim=1) if split else col_leaves[0].grad,
                   "v_features": f_leaf.grad}
        want_col = {"v_sh": sh64.grad.float().numpy(), "v_features": feats64.grad.float().numpy()}
    else:
        # the colour gradient chained through the sigmoid in fp64
        s64 = torch.sigmoid(col_leaves[0].detach().double().cpu())
        v_cols = torch.from_numpy(gr["v_colors"]).double()
        got_col = {"v_features_dc": col_leaves[0].grad, "v_features": f_leaf.grad}
        want_col = {"v_features_dc": (v_cols[:, :3] * s64 * (1.0 - s64)).numpy(), "v_features": v_cols[:, 3:].numpy()}
    for (name, ref), leaf in zip(want.items(), leaves):
        assert torch.isfinite(leaf.grad).all(), name
        assert_close_flips(leaf.grad, ref, name, proof=proof)
    for name, ref in want_col.items():
        assert torch.isfinite(got_col[name]).all(), name
        assert_close_flips(got_col[name], ref, name, proof=proof)
    assert_close_flips(meta["means2d"].grad[0], gr["v_means2d"], "v_means2d", proof=proof)
    if colour != "d0":
        nb = (deg + 1) ** 2                                      # above the active degree: exactly 0.0, over NaN-seeded memory
        above = got_col["v_sh"][:, nb:]
        assert not torch.isnan(above).any() and not above.any(), "coefficient gradients above the active degree"
    return took


# ================================================================ C. degrees 0, 1, 2 on the dense training path
@pytest.mark.parametrize("lazy", ["1", "auto"])
@pytest.mark.parametrize("deg", [0, 1, 2])
def test_low_sh_degrees_steady_state_dense_vs_c_port(dev, craster, monkeypatch, deg, lazy):
    """The progressive schedule's degrees 0, 1, 2 from 16-coefficient storage at 300 k Gaussians / 640 x 360: the on-demand
    SH of the compositing forward (a separate fetch at degree 0), the sparse SH backward that zeroes the coefficients above
    the active degree, rows cleared on touch and the background fill -- split (features_dc, features_rest) leaves for one
    of the two switch settings of each degree, the concatenated [N,16,3] tensor for the other."""
    split = (deg + (lazy == "1")) % 2 == 0
    took = _steady_vs_c_port(dev, craster, monkeypatch, 300_000, 640, 360, deg=deg, colour="sh", lazy=lazy, split=split,
                             scale_mul=1.5)
    assert took.get("forward_lazy_colour", 0) == 8 and took.get("forward_rows_on_touch", 0) == 8, took
    assert took.get("backward_background_fill", 0) == 8, took


@pytest.mark.parametrize("deg", [0, 2])
def test_features_one_entry_call_low_degrees_dense_vs_c_port(dev, craster, monkeypatch, deg):
    """The one-entry features call (SH colours + 13 features, RGB+ED: 17 channels) at degrees 0 and 2, 300 k Gaussians, the
    N-D records on demand."""
    took = _steady_vs_c_port(dev, craster, monkeypatch, 300_000, 640, 360, deg=deg, colour="sh+features", lazy="1",
                             split=deg == 0)
    assert took.get("forward_lazy_colour", 0) == 8 and took.get("forward_rows_on_touch", 0) == 8, took
    assert took.get("backward_background_fill", 0) == 8, took


@FULL_SIZE
def test_degree_1_full_size_steady_state_vs_c_port(dev, craster, monkeypatch):
    """The headline workload (1 M Gaussians, 1080p, its heaviest rotated view 3) at SH degree 1, the default switches."""
    took = _steady_vs_c_port(dev, craster, monkeypatch, 1_000_000, 1920, 1080, deg=1, colour="sh", view=3, split=True)
    assert took.get("forward_lazy_colour", 0) == 8 and took.get("backward_background_fill", 0) == 8, took


def test_degree_switch_never_replays_another_degrees_graph(dev, monkeypatch):
    """One set of leaves, graphs on, three calls at each of degrees 0, 1, 2, 3 in turn (the schedule's switches): the last
    call at each degree equals a fresh eager call (graphs off, fresh leaves) at that degree -- images bitwise, gradients
    within 2e-5 (the order of the atomic sums) -- so a graph captured at one degree never serves another."""
    from collab_splats_amd import ops, rasterization
    from collab_splats_amd.synthetic import random_scene
    monkeypatch.setattr(ops, "LAZY_SH", "1")
    N, W, H = 300_000, 640, 360
    sc = random_scene(N, W, H, seed=31)
    raw = [sc["means"], sc["quats"], sc["log_scales"], sc["opacity_logits"], sc["sh"]]
    V, K = sc["viewmats"].to(dev), sc["Ks"].to(dev)
    ups = [u.to(dev) for u in upstream([(1, H, W, 4), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)]

    def call(leaves, deg):
        for l in leaves:
            l.grad = None
        out = rasterization(*leaves, V, K, W, H, sh_degree=deg, render_mode="RGB+ED", rasterize_mode="antialiased",
                            return_depth_normal=True, scales_are_log=True, opacities_are_logit=True)
        torch.autograd.backward(list(out[:5]), ups)
        torch.cuda.synchronize()
        return [t.detach().clone() for t in out[:5]], [l.grad.clone() for l in leaves]

    ops.reset_graph_cache(dev)
    leaves = [t.to(dev).requires_grad_(True) for t in raw]
    before = dict(ops.PATH_STATS)
    got = {}
    for deg in (0, 1, 2, 3):
        for _ in range(3):
            got[deg] = call(leaves, deg)
    took = {k: ops.PATH_STATS[k] - before.get(k, 0) for k in ops.PATH_STATS}
    assert took.get("forward_lazy_colour", 0) == 12, took
    assert ops.graph_cache_stats(dev)["hits"] >= 4, ops.graph_cache_stats(dev)
    monkeypatch.setattr(ops, "GRAPHS", False)
    for deg in (0, 1, 2, 3):
        img, grad = call([t.to(dev).requires_grad_(True) for t in raw], deg)
        for k, (a, b) in enumerate(zip(got[deg][0], img)):
            assert torch.equal(a, b), (deg, k)
        for k, (a, b) in enumerate(zip(got[deg][1], grad)):
            assert rel_err(a, b) < 2e-5, (deg, k, rel_err(a, b))
        nb = (deg + 1) ** 2
        assert not got[deg][1][4][:, nb:].any()
    # the four degrees really render different colours
    assert not torch.equal(got[0][0][0], got[1][0][0]) and not torch.equal(got[2][0][0], got[3][0][0])


def _small_vs_c_port(dev, craster, cols_dev, cols_np, deg, sc, W, H):
    """One eager call against the C port (colour leaf given as a device tensor that may be a view)."""
    from collab_splats_amd import rasterization
    leaves = [sc["means"].to(dev).requires_grad_(True), sc["quats"].to(dev).requires_grad_(True),
              torch.exp(sc["log_scales"]).to(dev).requires_grad_(True),
              torch.sigmoid(sc["opacity_logits"]).to(dev).requires_grad_(True)]
    out = rasterization(*leaves, cols_dev, sc["viewmats"].to(dev), sc["Ks"].to(dev), W, H, sh_degree=deg,
                        render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True)
    cr = craster.CRaster(np.float32)
    st = cr.forward(sc["means"].numpy(), sc["quats"].numpy(), torch.exp(sc["log_scales"]).numpy(),
                    torch.sigmoid(sc["opacity_logits"]).numpy(), cols_np, sc["viewmats"][0].numpy(), sc["Ks"][0].numpy(),
                    W, H, sh_degree=deg, render_mode="RGB+ED", rasterize_mode="antialiased")
    meta = out[5]
    assert np.array_equal(st["proj"]["radii"], meta["radii"][0].cpu().numpy())
    assert np.array_equal(st["bins"]["flatten_ids"], meta["flatten_ids"].cpu().numpy())
    fw = st["fwd"]
    proof = FlipProof(cr.blend_margin(st), st["proj"]["means2d"], st["proj"]["radii"])
    for name, got, ref in (("render", out[0], st["render"]), ("alpha", out[1], fw["alpha"]), ("exp_depth", out[2], fw["exp_depth"]),
                           ("med_depth", out[3], fw["med_depth"]), ("normal", out[4], fw["normal"])):
        assert_close_flips(got[0], ref, name, proof=proof)
    proof.check_ids(meta["last_ids"][0].cpu().numpy(), fw["last_ids"], meta["median_ids"][0].cpu().numpy(), fw["median_ids"])
    ups = upstream([t.shape for t in out[:5]], dtype=torch.float32)
    torch.autograd.backward(list(out[:5]), [u.to(dev) for u in ups])
    gr = cr.backward(st, *[u[0].numpy() for u in ups])
    for name, leaf in zip(("v_means", "v_quats", "v_scales", "v_opacities"), leaves):
        assert_close_flips(leaf.grad, gr[name], name, proof=proof)
    return gr, proof


@pytest.mark.parametrize("deg,K", [(0, 1), (1, 4), (2, 9), (3, 16)])
def test_generic_k_colour_kernel_vs_c_port(dev, craster, deg, K):
    """The colour kernel's generic row length (KC = 0: every K other than an aligned 16): [N, K, 3] coefficients with
    K = (deg+1)^2 -- and, for degree 3, a K = 16 VIEW that starts 4 bytes into its buffer -- against the C port."""
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 320, 200, 6000
    sc = random_scene(N, W, H, seed=40 + K, sh_degree=deg)
    assert sc["sh"].shape == (N, K, 3)
    if K == 16:
        base = torch.zeros(N * K * 3 + 1, device=dev)
        base[1:] = sc["sh"].reshape(-1).to(dev)
        base.requires_grad_(True)
        cols = base[1:].view(N, K, 3)
        assert cols.data_ptr() % 16 == 4
    else:
        cols = sc["sh"].to(dev).requires_grad_(True)
    gr, proof = _small_vs_c_port(dev, craster, cols, sc["sh"].numpy(), deg, sc, W, H)
    v_sh = base.grad[1:].view(N, K, 3) if K == 16 else cols.grad
    assert_close_flips(v_sh, gr["v_colors"], "v_sh", proof=proof)
    if K == 16:
        assert base.grad[0] == 0


@pytest.mark.parametrize("step,moving", [(500, 0), (1500, 3)])
def test_model_fused_adam_leaves_inactive_coefficients_untouched(dev, monkeypatch, step, moving):
    """``RadegsModel`` (sh_degree 3, 300 k Gaussians: the on-demand SH path) trained three steps with ``FusedAdam`` at step 500
    (degree 0) leaves ``features_rest`` unchanged bit for bit, its Adam moments exactly zero; at step 1500 (degree 1) only
    ``features_rest[:, :3]`` moves.  A NaN or a stray non-zero in a gradient row above the active degree moves it."""
    from collab_splats_amd import FusedAdam, fused_adam_step_all, ops, radegs
    from collab_splats_amd.synthetic import random_scene
    monkeypatch.setattr(ops, "LAZY_SH", "1")
    W, H, N = 640, 360, 300_000
    sc = random_scene(N, W, H, seed=14)
    cfg = radegs.RadegsModelConfig(rasterize_mode="antialiased", output_depth_during_training=True)
    model = radegs.RadegsModel(cfg, sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0],
                               sc["sh"][:, 1:]).to(dev)
    model.train()
    model.step = step
    lrs = dict(means=1.6e-4, features_dc=0.0025, features_rest=0.0025 / 20, opacities=0.05, scales=0.005, quats=0.001)
    model.optimizers = {k: FusedAdam([p], lr=lrs[k], eps=1e-15) for k, p in model.gauss_params.items()}
    rest0 = model.features_rest.detach().clone()
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 0]])
    cam = radegs.PinholeCamera.make(c2w, 0.9 * W, 0.9 * W, W, H)
    gt = {"image": torch.rand(H, W, 3, generator=torch.Generator().manual_seed(6))}
    before = dict(ops.PATH_STATS)
    for it in range(3):
        for o in model.optimizers.values():
            o.zero_grad(set_to_none=True)
        _poison(dev, N)
        out = model.get_outputs(cam)
        loss = model.get_loss_dict(out, gt)
        sum(loss.values()).backward()
        fused_adam_step_all(model.optimizers)
    took = {k: ops.PATH_STATS[k] - before.get(k, 0) for k in ops.PATH_STATS}
    assert took.get("forward_lazy_colour", 0) == 3 and took.get("backward_background_fill", 0) == 3, took
    rest = model.features_rest.detach()
    assert torch.equal(rest[:, moving:], rest0[:, moving:])
    st = model.optimizers["features_rest"].state.get(model.features_rest, {})
    assert moving == 0 or "exp_avg" in st                       # (degree 0: a gradient of zeros, or none at all)
    if "exp_avg" in st:
        assert not st["exp_avg"][:, moving:].any() and not st["exp_avg_sq"][:, moving:].any()
    if moving:
        assert not torch.equal(rest[:, :moving], rest0[:, :moving]) and bool(st["exp_avg_sq"][:, :moving].any())
    assert not torch.equal(model.features_dc.detach(), sc["sh"][:, 0].to(dev))


# ================================================================ D. the degree-0 features call
@pytest.mark.parametrize("N,W,H,view,rm", [
    (30_000, 320, 192, None, "RGB+ED"), (30_000, 320, 192, None, "RGB"), (300_000, 640, 360, None, "RGB+ED"),
    (300_000, 640, 360, 2, "RGB"),
    pytest.param(1_000_000, 1920, 1080, 3, "RGB+ED", marks=FULL_SIZE)])
def test_degree0_features_call_steady_state_vs_c_port(dev, craster, monkeypatch, N, W, H, view, rm):
    """What ``rade-features`` (sh_degree=0) renders every step: ``cat(sigmoid(features_dc), features[N,13])`` with
    ``sh_degree=None`` -- 16 pass-through channels, 17 with RGB+ED -- antialiased, in steady state, against the C port; the
    colour gradient is chained through the sigmoid in fp64 to ``features_dc`` and to the features."""
    took = _steady_vs_c_port(dev, craster, monkeypatch, N, W, H, deg=None, colour="d0", rm=rm, view=view)
    assert took.get("forward_lazy_colour", 0) == 0, took


# ================================================================ E. the degree-0 features model
def test_degree0_features_model_vs_the_composed_reference_call(dev):
    """``RadegsFeaturesModel`` at ``sh_degree=0`` with ``features_rest`` [N,0,3], as the reference builds it: ``get_outputs``
    equals ``rasterization`` called with the reference's composed inputs (exp / sigmoid in front, ``cat(sigmoid(features_dc),
    distill_features)``, ``sh_degree=None``) plus the same epilogue -- images bitwise, gradients of all seven parameter groups
    within 2e-5 --; ``outputs["features"]`` is channels 3..15; training steps with ``step_all`` and a densification step keep
    every shape aligned (``features_rest`` stays [N',0,3]); ``render_views`` equals ``get_outputs`` in eval mode."""
    from collab_splats_amd import FusedAdam, fused_adam_step_all, ops, radegs, rasterization
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 320, 192, 30_000
    sc = random_scene(N, W, H, seed=27)
    feats = torch.rand(N, F, generator=torch.Generator().manual_seed(3))
    cfg = radegs.RadegsFeaturesModelConfig(sh_degree=0, output_depth_during_training=True, rasterize_mode="antialiased")
    model = radegs.RadegsFeaturesModel(cfg, sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0],
                                       torch.zeros(N, 0, 3), feats).to(dev)
    assert model.features_rest.shape == (N, 0, 3)
    model.train()
    model.step = 5000
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 0]])
    cam = radegs.PinholeCamera.make(c2w, 0.9 * W, 0.9 * W, W, H)
    keys = ("rgb", "depth", "median_depth", "accumulation", "normals", "depth_im", "features")
    g = torch.Generator().manual_seed(8)
    wts = {k: torch.rand(s, generator=g).to(dev) for k, s in
           (("rgb", (H, W, 3)), ("depth", (H, W, 1)), ("median_depth", (H, W, 1)), ("accumulation", (H, W, 1)),
            ("normals", (H, W, 3)), ("depth_im", (H, W, 1)), ("features", (H, W, F)))}
    out = model.get_outputs(cam)
    sum((out[k] * wts[k]).sum() for k in keys).backward()
    assert out["features"].shape == (H, W, F) and out["rgb"].shape == (H, W, 3)
    # ---- the reference's composition, restated (rade_features_model.py: colors = sigmoid(features_dc) at degree 0, cat with the
    # distilled features, rasterization(sh_degree=None), features = render[..., 3:3 + 13], then the colour post-processing)
    p = {k: v.detach().clone().requires_grad_(True) for k, v in model.gauss_params.items()}
    cp = model._get_camera_parameters(cam)
    colors = torch.cat((torch.sigmoid(p["features_dc"]), p["distill_features"]), dim=-1)
    render, alpha, ed, md, nrm, _ = rasterization(
        p["means"], p["quats"], torch.exp(p["scales"]), torch.sigmoid(p["opacities"]).squeeze(-1), colors, cp["viewmats"],
        cp["Ks"], W, H, sh_degree=None, render_mode="RGB+ED", rasterize_mode="antialiased", packed=False,
        return_depth_normal=True)
    assert render.shape[-1] == 3 + F + 1
    ep = ops.outputs_epilogue(torch.cat((render[..., :3], render[..., 3 + F:]), dim=-1), alpha, ed, md, nrm, [0.0, 0.0, 0.0], True)
    ref = {"rgb": ep[0][0], "depth": ep[1][0], "median_depth": ep[2][0], "accumulation": alpha[0], "normals": ep[3][0],
           "depth_im": ep[4][0], "features": render[0, ..., 3:3 + F]}
    for k in keys:
        assert torch.equal(out[k].detach(), ref[k].detach()), k
    sum((ref[k] * wts[k]).sum() for k in keys).backward()
    for k, q in model.gauss_params.items():
        if k == "features_rest":
            assert q.grad is None or not q.grad.any()            # (not read at degree 0: neither here nor in the reference)
            continue
        assert q.grad is not None and torch.isfinite(q.grad).all() and q.grad.abs().sum() > 0, k
        assert rel_err(q.grad, p[k].grad) < 2e-5, (k, rel_err(q.grad, p[k].grad))
    # ---- training steps with the fused optimizer, one densification step in between
    lrs = dict(means=1.6e-4, features_dc=0.0025, features_rest=0.0025 / 20, opacities=0.05, scales=0.005, quats=0.001,
               distill_features=0.0025)
    model.optimizers = {k: FusedAdam([q], lr=lrs[k], eps=1e-15) for k, q in model.gauss_params.items()}
    model.strategy.prune_opa, model.strategy.grow_grad2d = 0.2, 1e-7     # make the refinement step do something
    gt = {"image": torch.rand(H, W, 3, generator=g)}
    sizes = []
    for it in range(4):
        for o in model.optimizers.values():
            o.zero_grad(set_to_none=True)
        out = model.get_outputs(cam)
        loss = model.get_loss_dict(out, gt)
        (sum(loss.values()) + out["features"].square().mean()).backward()
        fused_adam_step_all(model.optimizers)
        model.strategy.step_post_backward(model.gauss_params, model.optimizers, model.strategy_state,
                                          model.step if it == 2 else model.step + 1, model.info)
        n_now = model.means.shape[0]
        sizes.append(n_now)
        for k, q in model.gauss_params.items():
            assert q.shape[0] == n_now, (it, k, q.shape)
            st = model.optimizers[k].state.get(q, {})
            assert all(st[m].shape == q.shape for m in ("exp_avg", "exp_avg_sq") if m in st), (it, k)
        assert model.features_rest.shape == (n_now, 0, 3)
        assert all(torch.isfinite(q).all() for q in model.gauss_params.values())
    assert sizes[2] != sizes[1], sizes                            # the refinement step resized the scene
    out = model.get_outputs(cam)
    assert out["features"].shape == (H, W, F) and float(out["accumulation"].detach().max()) > 0.5
    # ---- evaluation: render_views == get_outputs
    model.eval()
    with torch.no_grad():
        ev = model.get_outputs(cam)
        rv = model.render_views([cam], batch_size=1)
    assert ev["features"].shape == (H, W, F)
    for k in ("rgb", "depth", "median_depth", "accumulation", "normals"):
        assert rv[k].shape[1:] == ev[k].shape and rel_err(rv[k][0], ev[k]) < 1e-6, (k, rel_err(rv[k][0], ev[k]))
