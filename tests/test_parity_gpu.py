"""GPU (-m gpu): the HIP path, called through the C ABI, against the oracles.

Bars (BASELINE.json north_star): integer / index outputs bit-exact vs the fp32 CPU restatement;
colour / depth / normal and all gradients within 1e-4 relative (tensor-inf-norm, SURVEY.md
section 8(d)); at BASELINE's full size, size-independent properties (sortedness, determinism,
linearity of the backward, permutation invariance).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import FULL_SIZE, FlipProof, assert_close_flips, rel_err, small_scene, upstream

pytestmark = pytest.mark.gpu
TOL = 1e-4
GOLD = os.path.join(os.path.dirname(__file__), "golden", "camera_goldens.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from collab_splats_amd import load_library
    load_library()
    return torch.device("cuda:0")


def _scene_np(sc):
    return (sc["means"].numpy(), sc["quats"].numpy(), torch.exp(sc["log_scales"]).numpy(),
            torch.sigmoid(sc["opacity_logits"]).numpy(), sc["sh"].numpy(), sc["viewmats"][0].numpy(), sc["Ks"][0].numpy())


def _run_gpu(sc, dev, W, H, sh_degree=3, **kw):
    from collab_splats_amd import rasterization
    leaves = [sc["means"].to(dev).requires_grad_(True), sc["quats"].to(dev).requires_grad_(True),
              torch.exp(sc["log_scales"]).to(dev).requires_grad_(True),
              torch.sigmoid(sc["opacity_logits"]).to(dev).requires_grad_(True), sc["sh"].to(dev).requires_grad_(True)]
    out = rasterization(*leaves, sc["viewmats"].to(dev), sc["Ks"].to(dev), W, H, sh_degree=sh_degree,
                        return_depth_normal=True, **kw)
    return leaves, out


@pytest.fixture(params=[False, True], ids=["atomic", "deterministic"])
def grad_mode(request):
    """Both gradient-accumulation modes of the backward (ops.DETERMINISTIC_BACKWARD)."""
    from collab_splats_amd import ops
    old = ops.DETERMINISTIC_BACKWARD
    ops.set_deterministic(request.param)
    yield request.param
    ops.set_deterministic(old)


@pytest.mark.parametrize("N,W,H,mode,rm,deg,view", [
    (3000, 256, 256, "antialiased", "RGB+ED", 3, None),
    (10000, 256, 256, "antialiased", "RGB+ED", 3, None),     # BASELINE configs[0] at its stated size
    (20000, 640, 360, "classic", "RGB", 3, None),
    (5000, 333, 197, "antialiased", "RGB", 1, None),         # ragged: W, H not multiples of 16
    (100000, 1920, 1080, "antialiased", "RGB+ED", 3, None),  # BASELINE configs[1]
    (100000, 1920, 1080, "antialiased", "RGB+ED", 3, 5),     # configs[1] under a rotated view (configs[3]'s view 5)
])
def test_full_pipeline_vs_c_port(dev, craster, grad_mode, N, W, H, mode, rm, deg, view):
    from collab_splats_amd.synthetic import random_scene, view_matrix
    sc = random_scene(N, W, H, seed=42, sh_degree=3)
    if view is not None:
        sc["viewmats"] = view_matrix(view)
    leaves, out = _run_gpu(sc, dev, W, H, sh_degree=deg, render_mode=rm, rasterize_mode=mode, absgrad=True)
    r, a, ed, md, n, meta = out
    cr = craster.CRaster(np.float32)
    st = cr.forward(*_scene_np(sc), W, H, sh_degree=deg, render_mode=rm, rasterize_mode=mode)
    # ---- integer / index stages: bit-exact
    assert np.array_equal(st["proj"]["radii"], meta["radii"][0].cpu().numpy())
    assert np.array_equal(st["proj"]["depths"].view(np.uint32), meta["depths"][0].detach().cpu().numpy().view(np.uint32))
    assert np.array_equal(st["proj"]["means2d"].view(np.uint32), meta["means2d"][0].detach().cpu().numpy().view(np.uint32))
    assert np.array_equal(st["bins"]["tiles_per_gauss"], meta["tiles_per_gauss"][0].cpu().numpy())
    assert st["bins"]["n_isects"] == meta["n_isects"]
    assert np.array_equal(st["bins"]["isect_ids"], meta["isect_ids"].cpu().numpy().view(np.uint64))
    assert np.array_equal(st["bins"]["flatten_ids"], meta["flatten_ids"].cpu().numpy())
    assert np.array_equal(st["bins"]["isect_offsets"], meta["isect_offsets"][0].cpu().numpy())
    # ---- images: anything outside 1e-4 must be a PROVEN threshold flip (margin map of the C restatement)
    fw = st["fwd"]
    proof = FlipProof(cr.blend_margin(st), st["proj"]["means2d"], st["proj"]["radii"])
    for name, got, ref in (("render", r, st["render"]), ("alpha", a, fw["alpha"]), ("exp_depth", ed, fw["exp_depth"]),
                           ("med_depth", md, fw["med_depth"]), ("normal", n, fw["normal"])):
        assert_close_flips(got[0], ref, name, proof=proof)
    # contributor indices agree except at PROVEN fp32 threshold flips (alpha ~ 1/255, T ~ 1e-4, T ~ 0.5)
    proof.check_ids(meta["last_ids"][0].cpu().numpy(), fw["last_ids"], meta["median_ids"][0].cpu().numpy(), fw["median_ids"])
    # ---- gradients of every output to every parameter
    ups = upstream([t.shape for t in (r, a, ed, md, n)], dtype=torch.float32)
    meta["means2d"].retain_grad()
    torch.autograd.backward([r, a, ed, md, n], [u.to(dev) for u in ups])
    gr = cr.backward(st, *[u[0].numpy() for u in ups])
    for name, leaf in zip(("v_means", "v_quats", "v_scales", "v_opacities", "v_colors"), leaves):
        assert_close_flips(leaf.grad, gr[name], name, proof=proof)
    assert_close_flips(meta["means2d"].grad[0], gr["v_means2d"], "v_means2d", proof=proof)
    assert_close_flips(meta["means2d"].absgrad[0], gr["v_means2d_abs"], "v_means2d_abs", proof=proof)


def test_vs_fp64_autograd_oracle(dev):
    """Independent check against the dense fp64 autograd restatement (small scene)."""
    from oracle import torch_oracle as O
    from collab_splats_amd import rasterization
    sc = small_scene(n=400, W=70, H=52, seed=1)
    ins64 = [sc[k].clone().requires_grad_(True) for k in ("means", "quats", "scales", "opacities", "sh")]
    ref = O.rasterization(*ins64, sc["viewmat"][None], sc["K"][None], 70, 52, sh_degree=3, render_mode="RGB+ED",
                          rasterize_mode="antialiased")
    ins = [sc[k].float().to(dev).requires_grad_(True) for k in ("means", "quats", "scales", "opacities", "sh")]
    out = rasterization(*ins, sc["viewmat"][None].float().to(dev), sc["K"][None].float().to(dev), 70, 52, sh_degree=3,
                        render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True)
    ups = upstream([t.shape for t in ref[:5]])
    torch.autograd.backward(list(ref[:5]), ups)
    torch.autograd.backward(list(out[:5]), [u.float().to(dev) for u in ups])
    for got, want in zip(out[:5], ref[:5]):
        assert rel_err(got, want) < TOL
    for got, want in zip(ins, ins64):
        assert rel_err(got.grad, want.grad) < TOL
    assert np.array_equal(out[5]["radii"][0].cpu().numpy(), ref[5]["radii"][0].numpy())


def test_bins_vs_independent_fp64_oracle_rotated_view(dev):
    """The integer stages against the INDEPENDENT oracle (dense fp64 torch restatement, written separately from the C
    port): radii, tiles per Gaussian, the sorted (tile, depth, id) lists and the tile offsets at 8 000 Gaussians under a
    rotated camera.  Integer decisions taken in fp32 can differ from fp64 only on exact rounding boundaries (a radius
    sitting on an integer, a rectangle edge on a tile border), so rows where the two precisions disagree on the radii
    or tile counts are excluded -- and must stay a handful."""
    from oracle import torch_oracle as O
    from collab_splats_amd import rasterization
    from collab_splats_amd.synthetic import random_scene, view_matrix
    N, W, H = 8000, 320, 200
    sc = random_scene(N, W, H, seed=77)
    V = view_matrix(6)
    scales, op = torch.exp(sc["log_scales"]) * 6.0, torch.sigmoid(sc["opacity_logits"])
    pr = O.project(sc["means"].double(), sc["quats"].double(), scales.double(), V[0].double(), sc["Ks"][0].double(), W, H,
                   op.double(), O.RasterSpec(), calc_compensations=True)
    bs = O.bin_and_sort(pr["means2d"].numpy(), pr["radii"].numpy(), pr["depths"].numpy(), W, H)
    r = dict(radii=pr["radii"][None], tiles_per_gauss=bs["tiles_per_gauss"], isect_offsets=bs["isect_offsets"],
             flatten_ids=bs["flatten_ids"])
    out = rasterization(sc["means"].to(dev), sc["quats"].to(dev), scales.to(dev), op.to(dev), sc["sh"].to(dev), V.to(dev),
                        sc["Ks"].to(dev), W, H, sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased",
                        return_depth_normal=True)
    m = out[5]
    radii = m["radii"][0].cpu().numpy()
    tpg = m["tiles_per_gauss"][0].cpu().numpy()
    same = (radii == r["radii"][0].numpy()).all(-1) & (tpg == np.asarray(r["tiles_per_gauss"]).reshape(-1))
    assert (~same).sum() <= 8, int((~same).sum())                     # fp32-vs-fp64 rounding boundaries only
    assert tpg.sum() > 20_000
    # per tile: the same Gaussians in the same order, once the boundary rows are dropped from both
    offs_g = np.append(m["isect_offsets"][0].cpu().numpy().reshape(-1), m["n_isects"])
    fl_g = m["flatten_ids"].cpu().numpy()
    offs_r = np.append(np.asarray(r["isect_offsets"]).reshape(-1), len(r["flatten_ids"]))
    fl_r = np.asarray(r["flatten_ids"])
    dep = m["depths"][0].cpu().numpy()
    n_tiles = offs_g.size - 1
    checked = 0
    for t in range(n_tiles):
        a = fl_g[offs_g[t]:offs_g[t + 1]]
        b = fl_r[offs_r[t]:offs_r[t + 1]]
        a, b = a[same[a]], b[same[b]]
        if not np.array_equal(a, b):
            # the fp64 depth order may swap neighbours whose fp32 depths coincide: compare as (depth, id)-sorted sets
            assert np.array_equal(np.sort(a), np.sort(b)), t
            assert np.array_equal(a, a[np.lexsort((a, dep[a]))]), t      # ours IS in (fp32 depth, id) order
        checked += len(a)
    assert checked > 20_000


def test_kat_single_gaussian_on_gpu(dev):
    from collab_splats_amd import rasterization
    t = lambda x: torch.tensor(x, dtype=torch.float32, device=dev)
    z0, s, o, f = 4.0, 0.2, 0.8, 20.0
    K = t([[f, 0, 8.5], [0, f, 8.5], [0, 0, 1]])[None]
    r, a, ed, md, n, _ = rasterization(t([[0, 0, z0]]), t([[1, 0, 0, 0]]), t([[s, s, s]]), t([o]), t([[0.2, 0.5, 0.9]]),
                                       torch.eye(4, device=dev)[None], K, 17, 17, render_mode="RGB+ED",
                                       return_depth_normal=True)
    assert a[0, 8, 8, 0].item() == pytest.approx(o, rel=1e-6)
    assert r[0, 8, 8].tolist() == pytest.approx([o * 0.2, o * 0.5, o * 0.9, z0], rel=1e-5)
    assert md[0, 8, 8, 0].item() == pytest.approx(z0, rel=1e-6)
    assert n[0, 8, 8].tolist() == pytest.approx([0, 0, -o], abs=1e-6)
    var = (f * s / z0) ** 2 + 0.3
    assert a[0, 8, 10, 0].item() == pytest.approx(o * np.exp(-2.0 / var), rel=1e-5)


def test_edge_cases_empty_culled_and_two_cameras(dev, craster):
    from collab_splats_amd import rasterization
    from collab_splats_amd.synthetic import random_scene, view_matrix
    z = lambda *s: torch.zeros(*s, device=dev)
    eye, K = torch.eye(4, device=dev)[None], torch.tensor([[[20.0, 0, 8.5], [0, 20.0, 5.5], [0, 0, 1]]], device=dev)
    # empty scene and everything culled (behind the camera): zeros, last_ids == -1
    for means in (z(0, 3), torch.tensor([[0.0, 0, -2.0]] * 5, device=dev)):
        m = means.shape[0]
        quats = torch.ones(m, 4, device=dev)
        r, a, ed, md, n, meta = rasterization(means, quats, torch.ones(m, 3, device=dev) * 0.1, torch.ones(m, device=dev) * 0.5,
                                              z(m, 16, 3), eye, K, 17, 11, sh_degree=3, return_depth_normal=True)
        assert meta["n_isects"] == 0 and not a.any() and not r.any() and (meta["last_ids"] == -1).all()
        assert r.shape == (1, 11, 17, 3) and a.shape == (1, 11, 17, 1) and n.shape == (1, 11, 17, 3)
    # two cameras in one call == two single-camera calls (keys carry the camera index)
    W, H, N = 160, 96, 3000
    sc = random_scene(N, W, H, seed=7)
    V2 = torch.cat([sc["viewmats"], view_matrix(1)], 0).to(dev)
    K2 = sc["Ks"].expand(2, 3, 3).contiguous().to(dev)
    args = [sc["means"].to(dev), sc["quats"].to(dev), torch.exp(sc["log_scales"]).to(dev),
            torch.sigmoid(sc["opacity_logits"]).to(dev), sc["sh"].to(dev)]
    both = rasterization(*args, V2, K2, W, H, sh_degree=3, render_mode="RGB+ED", return_depth_normal=True)
    for ci in range(2):
        one = rasterization(*args, V2[ci:ci + 1], K2[ci:ci + 1], W, H, sh_degree=3, render_mode="RGB+ED",
                            return_depth_normal=True)
        for t2, t1 in zip(both[:5], one[:5]):
            assert torch.equal(t2[ci], t1[0])
    assert both[5]["radii"].shape == (2, N, 2) and both[5]["isect_offsets"].shape[0] == 2
    keys = both[5]["isect_ids"].cpu().numpy()
    assert np.all(np.diff(keys) >= 0)


@pytest.mark.parametrize("D,rm,det", [(7, "RGB+ED", False), (16, "RGB+ED", False), (16, "RGB", False), (5, "RGB", False),
                                      (19, "RGB+ED", False), (16, "RGB+ED", True), (23, "RGB", False)])
def test_feature_channels_backgrounds_and_render_modes(dev, craster, D, rm, det):
    """sh_degree=None with D 'fused feature' channels (rade_features_model.py:441-476: D = 16, 17 with ED):
    5..20 channels take the one-pass N-D kernels, anything else (or deterministic mode) the 4-channel passes;
    plus backgrounds and the 3-tuple return."""
    from collab_splats_amd import ops, rasterization
    from collab_splats_amd.synthetic import random_scene
    old = ops.DETERMINISTIC_BACKWARD
    ops.set_deterministic(det)
    try:
        _feature_case(dev, craster, D, rm)
    finally:
        ops.set_deterministic(old)


def test_absgrad_covers_every_channel_on_the_multi_pass_path(dev):
    """D = 16 colour channels: ``means2d.absgrad`` of the 4-channel-pass path (taken in deterministic mode) must count
    every pass -- it is the per-pass sum of |gradient|, an upper bound of the one-pass N-D kernel's |sum| that agrees
    with it wherever the passes' gradients share a sign -- and not just channels 0..3."""
    from collab_splats_amd import rendering, rasterization
    from collab_splats_amd.synthetic import random_scene
    W, H, N, D = 200, 120, 4000, 16
    sc = random_scene(N, W, H, seed=9)
    feats = torch.rand(N, D, generator=torch.Generator().manual_seed(4))
    scales, op = torch.exp(sc["log_scales"]), torch.sigmoid(sc["opacity_logits"])
    res = {}
    for one_pass in (True, False):
        old = rendering.ENABLE_ND_ONE_PASS
        rendering.ENABLE_ND_ONE_PASS = one_pass
        try:
            leaves = [t.to(dev).requires_grad_(True) for t in (sc["means"], sc["quats"], scales, op, feats)]
            out = rasterization(*leaves, sc["viewmats"].to(dev), sc["Ks"].to(dev), W, H, sh_degree=None, render_mode="RGB",
                                absgrad=True, return_depth_normal=True)
            out[5]["means2d"].retain_grad()
            out[0].sum().backward()                                  # positive upstream on every channel
            res[one_pass] = (out[5]["means2d"].absgrad.clone(), out[5]["means2d"].grad.clone())
        finally:
            rendering.ENABLE_ND_ONE_PASS = old
    (abs1, g1), (absm, gm) = res[True], res[False]
    assert rel_err(gm, g1) < TOL
    assert bool((absm >= abs1 * (1 - 1e-4) - 1e-7).all())                    # triangle inequality, never below
    assert float(absm.sum()) < 1.5 * float(abs1.sum())                       # ... and not wildly above
    # pass 0 alone would carry ~1/4 of it
    assert float(absm.sum()) > 0.9 * float(abs1.sum())


def _feature_case(dev, craster, D, rm):
    from collab_splats_amd import rasterization
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 200, 120, 4000
    sc = random_scene(N, W, H, seed=9)
    g = torch.Generator().manual_seed(4)
    feats = torch.rand(N, D, generator=g)
    scales, op = torch.exp(sc["log_scales"]), torch.sigmoid(sc["opacity_logits"])
    leaves = [t.to(dev).requires_grad_(True) for t in (sc["means"], sc["quats"], scales, op, feats)]
    Dp = D + (1 if rm == "RGB+ED" else 0)
    bg = torch.rand(1, Dp, generator=g).to(dev)
    out = rasterization(*leaves, sc["viewmats"].to(dev), sc["Ks"].to(dev), W, H, sh_degree=None, render_mode=rm,
                        rasterize_mode="classic", backgrounds=bg, return_depth_normal=True)
    assert out[0].shape == (1, H, W, Dp)
    cr = craster.CRaster(np.float32)
    st = cr.forward(sc["means"].numpy(), sc["quats"].numpy(), scales.numpy(), op.numpy(), feats.numpy(),
                    sc["viewmats"][0].numpy(), sc["Ks"][0].numpy(), W, H, sh_degree=None, render_mode=rm)
    want = st["render"] + (1 - st["fwd"]["alpha"]) * bg[0].cpu().numpy()
    assert rel_err(out[0][0], want) < TOL
    ups = upstream([t.shape for t in out[:5]], dtype=torch.float32)
    torch.autograd.backward(list(out[:5]), [u.to(dev) for u in ups])
    v_alpha = ups[1][0].numpy() - (ups[0][0].numpy() * bg[0].cpu().numpy()).sum(-1, keepdims=True)
    gr = cr.backward(st, ups[0][0].numpy(), v_alpha, ups[2][0].numpy(), ups[3][0].numpy(), ups[4][0].numpy())
    for name, leaf in zip(("v_means", "v_quats", "v_scales", "v_opacities", "v_colors"), leaves):
        assert rel_err(leaf.grad, gr[name]) < TOL, name
    r3 = rasterization(*[l.detach() for l in leaves[:4]], feats[:, :3].to(dev), sc["viewmats"].to(dev),
                       sc["Ks"].to(dev), W, H)
    assert len(r3) == 3 and r3[0].shape == (1, H, W, 3)


@pytest.mark.parametrize("rm,split,N,W,H,lazy", [("RGB+ED", False, 30_000, 320, 192, "auto"), ("RGB", True, 30_000, 320, 192, "auto"),
                                                 ("RGB+ED", True, 30_000, 320, 192, "1"), ("RGB+ED", False, 300_000, 640, 360, "1"),
                                                 ("RGB", True, 300_000, 640, 360, "1")])
def test_features_model_call_as_one_entry_steady_state_vs_c_port(dev, craster, monkeypatch, rm, split, N, W, H, lazy):
    """rade_features_model.py:427-476 as ONE product entry: ``rasterization(colors=SH coefficients, features=[N,13], sh_degree=3)``
    renders 16 (RGB) / 17 (RGB+ED) channels -- channels 0..2 = max(SH + 0.5, 0), channels 3..15 the features, no [N,16]
    concatenation, one autograd node, the one-entry forward / backward with graph replay and the view's launch order.  Steady
    state (the EIGHTH call on one set of leaves) against the C port fed what the reference would feed gsplat --
    ``cat(clamp_min(SH(dirs) + 0.5, 0), features)`` with ``sh_degree=None`` --, gradients chained back to the coefficients,
    the features and (through the view direction) the means with the fp64 torch oracle's SH.
    ``lazy`` = "1": the records ON DEMAND -- no colour kernel and no feature copy; the compositing forward evaluates SH, picks
    feature 0 and lays features 1.. (+ depth) into the featx row of the records it stages; from 262 144 Gaussians on also the
    gradient rows cleared on touch, the zeros of the untouched rows written in the background of the compositing backward and
    ONE kernel for the SH / feature / projection backward of the flagged rows."""
    from collab_splats_amd import ops, rasterization
    from collab_splats_amd.synthetic import random_scene
    from oracle.torch_oracle import eval_sh
    monkeypatch.setattr(ops, "LAZY_SH", lazy)
    F = 13
    sc = random_scene(N, W, H, seed=17)
    g = torch.Generator().manual_seed(5)
    feats = torch.rand(N, F, generator=g)
    scales, op = torch.exp(sc["log_scales"]), torch.sigmoid(sc["opacity_logits"])
    sh = sc["sh"].clone()
    sh[:, 0] *= 0.4                                              # (colours around the clamp at 0: both sides of it occur)
    leaves = [t.to(dev).requires_grad_(True) for t in (sc["means"], sc["quats"], scales, op)]
    if split:
        col_leaves = [sh[:, 0].contiguous().to(dev).requires_grad_(True), sh[:, 1:].contiguous().to(dev).requires_grad_(True)]
        colors = tuple(col_leaves)
    else:
        col_leaves = [sh.to(dev).requires_grad_(True)]
        colors = col_leaves[0]
    f_leaf = feats.to(dev).requires_grad_(True)
    V, K = sc["viewmats"].to(dev), sc["Ks"].to(dev)
    Dp = 3 + F + (1 if rm == "RGB+ED" else 0)
    ups = upstream([(1, H, W, Dp), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)
    ups_dev = [u.to(dev) for u in ups]
    ops.reset_graph_cache(dev)
    ops._CAP_HINT.pop(ops._cap_key(ops._lib.make_params(N, 1, W, H), dev), None)
    before = dict(ops.PATH_STATS)
    out = None
    for call in range(8):
        for l in leaves + col_leaves + [f_leaf]:
            l.grad = None
        del out
        out = rasterization(*leaves, colors, V, K, W, H, sh_degree=3, render_mode=rm, rasterize_mode="antialiased",
                            features=f_leaf, return_depth_normal=True)
        torch.autograd.backward(list(out[:5]), ups_dev)
    torch.cuda.synchronize()
    took = {k: ops.PATH_STATS[k] - before.get(k, 0) for k in ops.PATH_STATS}
    assert took.get("forward_nd") == 8 and took.get("backward_one_call") == 8 and took.get("forward_merged_phases") == 8 and took.get("forward_probe") == 1, took
    assert took.get("forward_lazy_colour", 0) == (8 if lazy == "1" else 0), took
    dense = lazy == "1" and N >= 262_144
    assert took.get("forward_rows_on_touch", 0) == (8 if dense else 0) and took.get("backward_background_fill", 0) == (8 if dense else 0), took
    assert took.get("forward_view_order") == 8 and ops.graph_cache_stats(dev)["hits"] >= 2
    assert out[0].shape == (1, H, W, Dp)
    # ---- what the reference feeds gsplat: colours evaluated on the host in fp32 exactly as the kernels do is not available
    # to the checker, so the C port gets the DEVICE's own fused colours (record slots + featx are not exposed either): it
    # is given cat(clamp(SH) from the fp64 oracle, features) and the images are compared at 1e-4 like everywhere else
    cam_c = -(sc["viewmats"][0, :3, :3].T @ sc["viewmats"][0, :3, 3])
    means64 = sc["means"].double().requires_grad_(True)
    sh64 = sh.double().requires_grad_(True)
    feats64 = feats.double().requires_grad_(True)
    rgb64 = torch.clamp_min(eval_sh(3, means64 - cam_c.double(), sh64) + 0.5, 0.0)
    fused64 = torch.cat((rgb64, feats64), dim=-1)
    cr = craster.CRaster(np.float32)
    st = cr.forward(sc["means"].numpy(), sc["quats"].numpy(), scales.numpy(), op.numpy(), fused64.detach().float().numpy(),
                    sc["viewmats"][0].numpy(), sc["Ks"][0].numpy(), W, H, sh_degree=None, render_mode=rm,
                    rasterize_mode="antialiased")
    meta = out[5]
    assert np.array_equal(st["bins"]["flatten_ids"], meta["flatten_ids"].cpu().numpy())
    fw = st["fwd"]
    proof = FlipProof(cr.blend_margin(st), st["proj"]["means2d"], st["proj"]["radii"])
    for name, got, ref in (("render", out[0], st["render"]), ("alpha", out[1], fw["alpha"]), ("exp_depth", out[2], fw["exp_depth"]),
                           ("med_depth", out[3], fw["med_depth"]), ("normal", out[4], fw["normal"])):
        assert_close_flips(got[0], ref, name, proof=proof)
    gr = cr.backward(st, *[u[0].numpy() for u in ups])
    fused64.backward(torch.from_numpy(gr["v_colors"]).double())
    want_means = gr["v_means"] + means64.grad.float().numpy()          # geometry + the SH view-direction term
    for name, leaf, ref in (("v_means", leaves[0], want_means), ("v_quats", leaves[1], gr["v_quats"]),
                            ("v_scales", leaves[2], gr["v_scales"]), ("v_opacities", leaves[3], gr["v_opacities"]),
                            ("v_features", f_leaf, feats64.grad.float().numpy())):
        assert_close_flips(leaf.grad, ref, name, proof=proof)
    got_sh = torch.cat((col_leaves[0].grad[:, None, :], col_leaves[1].grad), dim=1) if split else col_leaves[0].grad
    assert_close_flips(got_sh, sh64.grad.float().numpy(), "v_sh", proof=proof)
    # the reference's own composition (spherical_harmonics -> clamp -> cat -> rasterization(sh_degree=None)) through the same
    # library gives the same images (alpha / depths / normals bit for bit): the one-entry form is a fusion, not another algorithm
    from collab_splats_amd import spherical_harmonics
    with torch.no_grad():
        coeffs = torch.cat((col_leaves[0][:, None, :], col_leaves[1]), dim=1) if split else col_leaves[0]
        rgb = torch.clamp_min(spherical_harmonics(3, leaves[0] - cam_c.to(dev), coeffs) + 0.5, 0.0)
        ref_out = rasterization(*leaves, torch.cat((rgb, f_leaf), dim=-1), V, K, W, H, sh_degree=None, render_mode=rm,
                                rasterize_mode="antialiased", return_depth_normal=True)
    for k, (a, b) in enumerate(zip(out[:5], ref_out[:5])):              # (geometry identical; the two SH kernels may round differently)
        assert torch.equal(a.detach(), b) if k > 0 else rel_err(a, b) < 1e-5, ("fused entry differs from the composed call", k)


def _compare_with_c_port(dev, craster, means, quats, scales, opac, cols, V, K, W, H, sh_degree=None, rm="RGB+ED",
                         mode="antialiased", tol=TOL):
    from collab_splats_amd import rasterization
    leaves = [t.clone().to(dev).requires_grad_(True) for t in (means, quats, scales, opac, cols)]
    out = rasterization(*leaves, V[None].to(dev), K[None].to(dev), W, H, sh_degree=sh_degree, render_mode=rm,
                        rasterize_mode=mode, return_depth_normal=True)
    cr = craster.CRaster(np.float32)
    st = cr.forward(means.numpy(), quats.numpy(), scales.numpy(), opac.numpy(), cols.numpy(), V.numpy(), K.numpy(), W, H,
                    sh_degree=sh_degree, render_mode=rm, rasterize_mode=mode)
    assert np.array_equal(st["proj"]["radii"], out[5]["radii"][0].cpu().numpy())
    assert np.array_equal(st["bins"]["flatten_ids"], out[5]["flatten_ids"].cpu().numpy())
    assert np.array_equal(st["bins"]["isect_offsets"], out[5]["isect_offsets"][0].cpu().numpy())
    fw = st["fwd"]
    proof = FlipProof(cr.blend_margin(st), st["proj"]["means2d"], st["proj"]["radii"])
    for name, got, ref in (("render", out[0], st["render"]), ("alpha", out[1], fw["alpha"]), ("exp_depth", out[2], fw["exp_depth"]),
                           ("med_depth", out[3], fw["med_depth"]), ("normal", out[4], fw["normal"])):
        assert_close_flips(got[0], ref, name, tol=tol, proof=proof)
    proof.check_ids(out[5]["last_ids"][0].cpu().numpy(), fw["last_ids"], out[5]["median_ids"][0].cpu().numpy(), fw["median_ids"],
                    max_frac=1e-2)
    ups = upstream([t.shape for t in out[:5]], dtype=torch.float32)
    torch.autograd.backward(list(out[:5]), [u.to(dev) for u in ups])
    gr = cr.backward(st, *[u[0].numpy() for u in ups])
    for name, leaf in zip(("v_means", "v_quats", "v_scales", "v_opacities", "v_colors"), leaves):
        assert torch.isfinite(leaf.grad).all(), name
        assert_close_flips(leaf.grad, gr[name], name, tol=tol, proof=proof)
    return out, st


@pytest.mark.parametrize("W,H", [(1, 1), (5, 3), (16, 16), (17, 33), (130, 7)])
def test_tiny_and_odd_image_sizes(dev, craster, W, H):
    g = torch.Generator().manual_seed(W * 100 + H)
    n = 200
    means = torch.stack([(torch.rand(n, generator=g) - 0.5) * 2, (torch.rand(n, generator=g) - 0.5) * 2,
                         torch.rand(n, generator=g) * 3 + 1.5], -1)
    quats, scales = torch.randn(n, 4, generator=g), torch.exp(torch.rand(n, 3, generator=g) * 2 - 3.5)
    opac, cols = torch.rand(n, generator=g) * 0.9 + 0.05, torch.rand(n, 3, generator=g)
    K = torch.tensor([[1.2 * max(W, H), 0, W / 2], [0, 1.2 * max(W, H), H / 2], [0, 0, 1.0]])
    out, _ = _compare_with_c_port(dev, craster, means, quats, scales, opac, cols, torch.eye(4), K, W, H)
    assert out[0].shape == (1, H, W, 4)


def test_deep_stack_multi_batch_and_early_termination(dev, craster):
    """5000 Gaussians piled on the same few pixels: 70+ staging batches per tile, transmittance stop,
    median switch and the back-to-front re-traversal from the saved last index."""
    g = torch.Generator().manual_seed(77)
    n, W, H = 5000, 48, 32
    means = torch.stack([(torch.rand(n, generator=g) - 0.5) * 0.3, (torch.rand(n, generator=g) - 0.5) * 0.2,
                         2.0 + torch.arange(n).float() * 1e-3], -1)
    quats = torch.randn(n, 4, generator=g)
    scales = torch.exp(torch.rand(n, 3, generator=g) * 1.0 - 3.0)
    opac = torch.rand(n, generator=g) * 0.05 + 0.01                      # faint: hundreds contribute before T < 1e-4
    cols = torch.rand(n, 3, generator=g)
    K = torch.tensor([[60.0, 0, W / 2], [0, 60.0, H / 2], [0, 0, 1.0]])
    out, st = _compare_with_c_port(dev, craster, means, quats, scales, opac, cols, torch.eye(4), K, W, H, mode="classic", tol=2e-4)
    per_tile = np.diff(np.append(st["bins"]["isect_offsets"].reshape(-1), st["bins"]["n_isects"]))
    assert per_tile.max() > 2000                                          # >> 64: many batches
    assert float(out[1].detach().max()) > 0.99                            # pixels that saturate and stop early
    last = out[5]["last_ids"][0].cpu().numpy()
    assert (last >= 0).any() and last.max() < st["bins"]["n_isects"]


def test_screen_filling_and_degenerate_gaussians(dev, craster):
    """One Gaussian covering every tile, needle-like and pancake-like shapes, a Gaussian exactly on a tile corner,
    and a zero-opacity one; all gradients stay finite."""
    W, H = 96, 64
    means = torch.tensor([[0.0, 0.0, 1.0], [0.3, 0.1, 3.0], [-0.4, -0.2, 4.0], [0.0, 0.0, 5.0], [0.2, 0.2, 2.5], [0.1, -0.3, 6.0]])
    quats = torch.tensor([[1.0, 0, 0, 0], [0.3, 0.8, -0.2, 0.4], [0.0, 0.0, 1e-3, 0.0], [1, 1, 1, 1.0], [0.5, -0.5, 0.5, 0.5], [2.0, 0, 0, 0]])
    scales = torch.tensor([[5.0, 5.0, 5.0], [1.0, 1e-3, 1e-3], [1e-3, 0.7, 0.7], [0.05, 0.05, 0.05], [1e-4, 1e-4, 1e-4], [0.4, 0.2, 0.1]])
    opac = torch.tensor([0.3, 0.9, 0.8, 0.999, 0.5, 0.0])
    cols = torch.rand(6, 3, generator=torch.Generator().manual_seed(1))
    K = torch.tensor([[80.0, 0, 48.0], [0, 80.0, 32.0], [0, 0, 1.0]])           # mean 3 projects exactly onto a tile corner
    out, st = _compare_with_c_port(dev, craster, means, quats, scales, opac, cols, torch.eye(4), K, W, H)
    assert st["bins"]["tiles_per_gauss"][0] == (W // 16) * (H // 16)              # the big one hits every tile
    assert st["bins"]["tiles_per_gauss"][5] == 0                                  # zero opacity is culled
    # the sub-pixel Gaussian: antialiasing scales its opacity by sqrt(det0/det) ~ 0 -> below 1/255 -> culled ...
    assert out[5]["radii"][0, 4].max() == 0
    out_c, _ = _compare_with_c_port(dev, craster, means, quats, scales, opac, cols, torch.eye(4), K, W, H, mode="classic")
    assert out_c[5]["radii"][0, 4].min() > 0                                      # ... but survives in classic mode (eps2d)


def test_meta_serves_the_reference_consumers(dev):
    """`meta` must carry what the reference's consumers read: project_gaussians (utils/utils.py:13-40:
    radii, means2d, depths, width, height) and the prefilter mask (rade_gs_model.py:397)."""
    from collab_splats_amd import rasterization
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 320, 200, 4000
    sc = random_scene(N, W, H, seed=21)
    out = rasterization(sc["means"].to(dev), sc["quats"].to(dev), torch.exp(sc["log_scales"]).to(dev),
                        torch.sigmoid(sc["opacity_logits"]).to(dev), sc["sh"].to(dev), sc["viewmats"].to(dev),
                        sc["Ks"].to(dev), W, H, sh_degree=3, packed=False, return_depth_normal=True)
    meta = out[5]
    # --- the consumer's own steps (utils.py:19-37), on this build's meta
    Wm, Hm = meta["width"], meta["height"]
    radii = meta["radii"].squeeze()
    assert radii.shape == (N, 2)
    valid_mask = (radii > 1.0).sum(dim=1) > 0
    gaussian_ids = valid_mask.nonzero(as_tuple=False).squeeze()
    xy = torch.round(meta["means2d"]).squeeze().long()
    x, y = torch.clamp(xy[:, 0], 0, Wm - 1), torch.clamp(xy[:, 1], 0, Hm - 1)
    flat = x + y * Wm
    depths = meta["depths"].squeeze().detach().cpu()
    assert (Wm, Hm) == (W, H) and flat.shape == (N,) and depths.shape == (N,)
    assert 0 < gaussian_ids.numel() < N and int(flat.max()) < W * H
    assert torch.all(depths[valid_mask.cpu()] > 0)
    for key in ("conics", "opacities", "tile_width", "tile_height", "tiles_per_gauss", "isect_ids", "flatten_ids",
                "isect_offsets", "tile_size", "n_cameras", "ray_ts", "ray_planes", "normals"):
        assert meta[key] is not None, key
    assert meta["isect_offsets"].shape == (1, meta["tile_height"], meta["tile_width"])


def _assert_lists_in_depth_id_order(meta):
    """Every tile's list is its own members in (depth bits, Gaussian id) order -- the order of a one-shot 64-bit key sort,
    rebuilt here with numpy from the members the device reports (membership itself is checked against the C port)."""
    ids = meta["flatten_ids"].cpu().numpy().astype(np.int64)
    offs = meta["isect_offsets"].reshape(-1).cpu().numpy().astype(np.int64)
    n = int(meta["n_isects"])
    cnt = np.diff(np.concatenate([offs, [n]]))
    tile = np.repeat(np.arange(cnt.size), cnt)
    dbits = meta["depths"].flatten().cpu().numpy().view(np.uint32)[ids].astype(np.int64)
    want = np.lexsort((ids, dbits, tile))
    assert np.array_equal(ids[want], ids)
    keys = meta["isect_ids"].cpu().numpy().view(np.uint64)
    assert np.array_equal(keys, (tile.astype(np.uint64) << np.uint64(32)) | dbits.astype(np.uint64))


def test_both_gradient_modes_give_identical_bins(dev, monkeypatch):
    """Atomic and deterministic (emission-slot) binning produce the same tile lists, bit for bit, and each list is in the
    (depth, id) order of a global key sort."""
    from collab_splats_amd import ops, rasterization
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 640, 360, 50_000
    sc = random_scene(N, W, H, seed=12)
    args = [sc["means"].to(dev), sc["quats"].to(dev), torch.exp(sc["log_scales"]).to(dev),
            torch.sigmoid(sc["opacity_logits"]).to(dev), sc["sh"].to(dev), sc["viewmats"].to(dev), sc["Ks"].to(dev), W, H]
    outs = {}
    for det in (False, True):
        monkeypatch.setattr(ops, "DETERMINISTIC_BACKWARD", det)
        outs[det] = rasterization(*args, sh_degree=3, render_mode="RGB+ED", return_depth_normal=True)
    a, b = outs[False], outs[True]
    _assert_lists_in_depth_id_order(a[5])
    assert torch.equal(a[5]["flatten_ids"], b[5]["flatten_ids"])
    assert torch.equal(a[5]["isect_offsets"], b[5]["isect_offsets"])
    assert torch.equal(a[5]["isect_ids"], b[5]["isect_ids"])
    for x, y in zip(a[:5], b[:5]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("n,size", [(40_000, (320, 200)), (80_000, (48, 32))])
def test_depth_ties_and_long_buckets_come_out_in_id_order(dev, monkeypatch, n, size):
    """Buckets filled through atomic cursors arrive in arbitrary order: equal depths must still come out in
    Gaussian-id order (the tie path of the per-tile sort), for short buckets and for buckets longer than
    every LDS class (48x32 image: 6 tiles share 80k Gaussians, > 8192 entries each)."""
    from collab_splats_amd import ops, rasterization
    from collab_splats_amd.synthetic import random_scene
    W, H = size
    sc = random_scene(n, W, H, seed=21)
    means = sc["means"].clone()
    vm = sc["viewmats"][:1]
    # camera-space depth quantised to a handful of exactly equal values
    cam = means @ vm[0, :3, :3].T + vm[0, :3, 3]
    cam[:, 2] = torch.round(cam[:, 2] * 2.0) / 2.0
    means = (cam - vm[0, :3, 3]) @ vm[0, :3, :3]
    args = [means.to(dev), sc["quats"].to(dev), torch.exp(sc["log_scales"]).to(dev),
            torch.sigmoid(sc["opacity_logits"]).to(dev), sc["sh"].to(dev), vm.to(dev), sc["Ks"][:1].to(dev), W, H]
    outs = {}
    for det in (False, True):
        monkeypatch.setattr(ops, "DETERMINISTIC_BACKWARD", det)
        outs[det] = rasterization(*args, sh_degree=3, render_mode="RGB+ED", return_depth_normal=True)
    a = outs[False]
    d = a[5]["depths"].flatten()[a[5]["flatten_ids"].long()]
    assert (d[1:] == d[:-1]).float().mean() > 0.5                      # the scene really is full of ties
    offs = a[5]["isect_offsets"].reshape(-1).long()
    longest = int(torch.diff(offs, append=offs.new_tensor([a[5]["n_isects"]])).max())
    assert longest > (8192 if size == (48, 32) else 256)              # the global-scratch class is exercised
    _assert_lists_in_depth_id_order(a[5])
    b = outs[True]
    assert torch.equal(a[5]["flatten_ids"], b[5]["flatten_ids"])
    assert torch.equal(a[5]["isect_offsets"], b[5]["isect_offsets"])
    for x, y in zip(a[:5], b[:5]):
        assert torch.equal(x, y)


def test_split_sh_parameters_match_concatenated(dev):
    """colors=(features_dc, features_rest) (extension) == the reference's torch.cat path, values and gradients."""
    from collab_splats_amd import rasterization
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 320, 200, 6000
    sc = random_scene(N, W, H, seed=8)
    base = [sc["means"].to(dev), sc["quats"].to(dev), torch.exp(sc["log_scales"]).to(dev), torch.sigmoid(sc["opacity_logits"]).to(dev)]
    dc = sc["sh"][:, 0].contiguous().to(dev).requires_grad_(True)
    rest = sc["sh"][:, 1:].contiguous().to(dev).requires_grad_(True)
    cat = sc["sh"].to(dev).requires_grad_(True)
    kw = dict(sh_degree=2, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True)
    o1 = rasterization(*base, (dc, rest), sc["viewmats"].to(dev), sc["Ks"].to(dev), W, H, **kw)
    o2 = rasterization(*base, cat, sc["viewmats"].to(dev), sc["Ks"].to(dev), W, H, **kw)
    for a, b in zip(o1[:5], o2[:5]):
        assert torch.equal(a, b)
    ups = [u.to(dev) for u in upstream([t.shape for t in o1[:5]], dtype=torch.float32)]
    torch.autograd.backward(list(o1[:5]), ups)
    torch.autograd.backward(list(o2[:5]), ups)
    assert rel_err(dc.grad, cat.grad[:, 0]) < 1e-5 and rel_err(rest.grad, cat.grad[:, 1:]) < 1e-5
    assert not rest.grad[:, 8:].any()                                   # coefficients above the active degree


def test_projection_and_sh_wrappers(dev, craster):
    """fully_fused_projection 8-tuple (rade_gs_model.py:373-394) and spherical_harmonics
    (rade_features_model.py:430-438)."""
    from collab_splats_amd import fully_fused_projection, spherical_harmonics
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 320, 200, 5000
    sc = random_scene(N, W, H, seed=5)
    scales = torch.exp(sc["log_scales"])
    res = fully_fused_projection(sc["means"].to(dev), None, sc["quats"].to(dev), scales.to(dev), sc["viewmats"].to(dev),
                                 sc["Ks"].to(dev), W, H, eps2d=0.3, packed=False, near_plane=0.01, far_plane=1e10,
                                 radius_clip=0.0, sparse_grad=False, calc_compensations=False)
    radii, means2d, depths, conics, comps, ray_ts, ray_planes, normals = res
    assert comps is None and radii.shape == (1, N, 2) and normals.shape == (1, N, 3)
    cr = craster.CRaster(np.float32)
    P = cr.params(sc["Ks"][0].numpy(), W, H)
    ref = cr.project_fwd(sc["means"].numpy(), sc["quats"].numpy(), scales.numpy(), None, sc["viewmats"][0].numpy(), P)
    assert np.array_equal(radii[0].cpu().numpy(), ref["radii"])
    mask = torch.sum(radii, dim=-1).squeeze() > 0                       # rade_gs_model.py:397
    assert 0.5 * N < int(mask.sum()) < N
    for got, key in ((conics, "conics"), (ray_ts, "ray_ts"), (ray_planes, "ray_planes"), (normals, "normals")):
        assert rel_err(got[0], ref[key]) < 1e-5, key
    vis = mask.cpu().numpy()
    view_dir = sc["means"].numpy()[vis]                                  # camera at the origin (identity viewmat)
    assert np.all((normals[0].cpu().numpy()[vis] * view_dir).sum(-1) < 0)             # normals face the camera
    dirs = (sc["means"] - torch.tensor([0.0, 0.0, 0.0]))
    cols = spherical_harmonics(degrees_to_use=2, dirs=dirs.to(dev), coeffs=sc["sh"].to(dev))
    want = cr.sh_fwd(2, dirs.numpy(), sc["sh"].numpy())
    assert rel_err(cols, want) < 1e-5


@pytest.mark.parametrize("i", [0, 1, 2])
def test_depth_normal_kernel_vs_reference_goldens(dev, i):
    """The fused a4 stencil against vectors produced by the reference's own camera_utils.py."""
    from collab_splats_amd import ops
    g = np.load(GOLD)
    W, H = [int(v) for v in g[f"cam{i}_WH"]]
    fovx, fovy = g[f"cam{i}_fov"]
    fx, fy = W / (2 * np.tan(fovx / 2)), H / (2 * np.tan(fovy / 2))
    d1 = torch.from_numpy(g[f"dn{i}_d1"]).to(dev).requires_grad_(True)
    d2 = torch.from_numpy(g[f"dn{i}_d2"]).to(dev).requires_grad_(True)
    nr = torch.from_numpy(g[f"dn{i}_nrm"]).to(dev).requires_grad_(True)
    n2, err = ops.depth_normal(d1, d2, nr, fx, fy)
    assert np.abs(n2.detach().cpu().numpy() - g[f"dn{i}_normals2"]).max() < 2e-5
    assert np.abs(err.detach().cpu().numpy() - g[f"dn{i}_err"]).max() < 2e-5
    loss = 0.05 * ((1 - 0.6) * err[0].mean() + 0.6 * err[1].mean())
    assert abs(loss.item() - float(g[f"dn{i}_loss"])) < 1e-6
    loss.backward()
    assert rel_err(d1.grad, g[f"dn{i}_v_d1"]) < TOL
    assert rel_err(d2.grad, g[f"dn{i}_v_d2"]) < TOL
    assert rel_err(nr.grad, g[f"dn{i}_v_nrm"]) < TOL


@pytest.mark.parametrize("cd", [3, 4])
def test_outputs_epilogue_vs_reference_formulas(dev, cd):
    """Fused a3 kernels against the torch restatement of rade_gs_model.py:221-254, forward and backward."""
    from collab_splats_amd import ops
    from oracle import camera_oracle as co
    H, W = 37, 53
    g = torch.Generator().manual_seed(11)
    alpha = torch.rand(1, H, W, 1, generator=g)
    alpha[alpha < 0.3] = 0.0                                           # empty pixels exercise the where() branches
    render = torch.rand(1, H, W, cd, generator=g) * 1.4 - 0.2          # some values clamp at 0 and at 1
    ed, md = torch.rand(1, H, W, 1, generator=g) * 5, torch.rand(1, H, W, 1, generator=g) * 5
    nr = torch.randn(1, H, W, 3, generator=g) * 0.5
    bg = [0.2, 0.5, 0.9]
    ref_in = [t.clone().double().requires_grad_(True) for t in (render, alpha, ed, md, nr)]
    ref = co.outputs_post(*ref_in, torch.tensor(bg, dtype=torch.float64))
    got_in = [t.clone().to(dev).requires_grad_(True) for t in (render, alpha, ed, md, nr)]
    got = ops.outputs_epilogue(*got_in, bg, cd == 4)
    n_out = 5 if cd == 4 else 4
    ups = [torch.rand(t.shape, generator=g) for t in got[:n_out]]
    for a, b in zip(got[:n_out], ref[:n_out]):
        assert rel_err(a, b) < 1e-6
    torch.autograd.backward(list(ref[:n_out]), [u.double() for u in ups])
    torch.autograd.backward(list(got[:n_out]), [u.to(dev) for u in ups])
    for a, b, name in zip(got_in, ref_in, ("render", "alpha", "expected_depths", "median_depths", "expected_normals")):
        assert rel_err(a.grad, b.grad) < 1e-6, name


def test_model_get_outputs_and_loss(dev):
    """Host mirror of RadegsModel.get_outputs / get_loss_dict (rade_gs_model.py:80-309): keys, shapes,
    masking conventions and the depth-normal loss, end to end with backward."""
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 240, 136, 6000
    sc = random_scene(N, W, H, seed=2)
    cfg = radegs.RadegsModelConfig(rasterize_mode="antialiased", regularization_from_iter=0, absgrad=True)
    model = radegs.RadegsModel(cfg, sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0],
                               sc["sh"][:, 1:]).to(dev)
    model.train()
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 0]])         # OpenGL camera looking down +z (OpenCV)
    cam = radegs.PinholeCamera.make(c2w, 0.9 * W, 0.9 * W, W, H)
    model.step = 5000
    out = model.get_outputs(cam)
    assert set(out) == {"rgb", "depth", "median_depth", "depth_im", "accumulation", "normals",
                        "depth_normal_error_map", "middepth_normal_error_map", "background"}
    assert out["rgb"].shape == (H, W, 3) and out["depth"].shape == (H, W, 1) and out["normals"].shape == (H, W, 3)
    assert out["depth_im"] is None and out["depth_normal_error_map"].shape == (H, W, 1)
    assert 0 <= out["rgb"].min() and out["rgb"].max() <= 1
    acc = out["accumulation"]
    empty = acc[..., 0] == 0
    assert empty.any() and torch.all(out["depth"][..., 0][empty] == out["depth"].max())   # where(alpha>0, x, max)
    loss = model.get_loss_dict(out, {"image": torch.rand(H, W, 3)})
    assert set(loss) == {"main_loss", "scale_reg", "depth_normal_loss"}       # Splatfacto's keys + the depth-normal term
    sum(loss.values()).backward()
    for k, p in model.gauss_params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert model.info["means2d"].grad is not None and model.info["means2d"].absgrad is not None
    model.strategy.step_post_backward(model.gauss_params, {}, model.strategy_state, model.step + 1, model.info)
    assert model.strategy_state["count"].sum() > 0                       # statistics gathered (no refinement at this step)
    n_before = model.means.shape[0]
    model.strategy.prune_opa, model.strategy.grow_grad2d = 0.2, 1e-7     # make this refinement step do something
    d, sp, pr = model.strategy.step_post_backward(model.gauss_params, {}, model.strategy_state, model.step, model.info)
    assert model.means.shape[0] == n_before + d + sp - pr and (d + sp + pr) > 0   # a refinement step resizes the scene
    model.get_outputs(cam)                                               # ... and the resized scene renders
    model.eval()
    with torch.no_grad():
        ev = model.get_outputs(cam)
    assert ev["depth_im"].shape == (H, W, 1) and ev["background"].shape == (H, W, 3)
    mask = model._prefilter_voxel(model._get_camera_parameters(cam))
    n_now = model.means.shape[0]
    assert mask.shape == (n_now,) and mask.dtype == torch.bool and 0 < int(mask.sum()) < n_now


def test_resolution_schedule_renders_the_downscaled_camera(dev):
    """rade_gs_model.py:132-136, 223 at a downscale factor of 2: a training step under the schedule renders what a camera of
    half the resolution renders (same intrinsics / 2), bit for bit, and the caller's camera is untouched afterwards."""
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 256, 144, 5000
    sc = random_scene(N, W, H, seed=6)
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 0]])

    def model(**kw):
        cfg = radegs.RadegsModelConfig(rasterize_mode="antialiased", regularization_from_iter=0, **kw)
        m = radegs.RadegsModel(cfg, sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0],
                               sc["sh"][:, 1:]).to(dev)
        m.train()
        m.step = 4000
        return m

    full = radegs.PinholeCamera.make(c2w, 0.9 * W, 0.9 * W, W, H)
    half = radegs.PinholeCamera.make(c2w, 0.45 * W, 0.45 * W, W // 2, H // 2)
    m1 = model(num_downscales=3, resolution_schedule=2000)                      # 2^(3 - 4000 // 2000) = 2
    a = m1.get_outputs(full)
    b = model().get_outputs(half)
    assert a["rgb"].shape == (H // 2, W // 2, 3)
    for k in ("rgb", "depth", "median_depth", "accumulation", "normals", "depth_normal_error_map"):
        assert torch.equal(a[k], b[k]), k
    assert (int(full.width.item()), int(full.height.item()), full.fx, full.cx) == (W, H, 0.9 * W, W / 2.0)
    # the data manager hands out the FULL-resolution image whatever the schedule says (advisor, round 4): get_loss_dict
    # box-filters it by the same factor, as Splatfacto's get_gt_img does -- float and uint8 alike -- and takes the fused path
    gt_full = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(4))
    gt_half = gt_full.view(H // 2, 2, W // 2, 2, 3).mean(dim=(1, 3))
    l_full = m1.get_loss_dict(a, {"image": gt_full})
    l_u8 = m1.get_loss_dict(a, {"image": (gt_full * 255).round().to(torch.uint8)})
    m1.step = 6000                                                   # (factor 1: the pre-shrunk image is taken as it is)
    l_half = m1.get_loss_dict(a, {"image": gt_half})
    m1.step = 4000
    assert set(l_full) == {"main_loss", "scale_reg", "depth_normal_loss"}
    assert abs(float(l_full["main_loss"]) - float(l_half["main_loss"])) < 1e-5
    assert abs(float(l_u8["main_loss"]) - float(l_full["main_loss"])) < 5e-3
    sum(l_full.values()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m1.gauss_params.values())


def test_features_model_mirror_outputs(dev):
    """``RadegsFeaturesModel`` (rade_features_model.py:195-478, rasterizer side): the distilled features are composited
    behind the SH colours in the same call -- ``outputs["features"]`` [H, W, 13] --, the colour / depth / normal outputs
    are those of the base model on the same Gaussians, and the backward reaches the feature parameters too."""
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 208, 128, 5000
    sc = random_scene(N, W, H, seed=8)
    feats = torch.rand(N, 13, generator=torch.Generator().manual_seed(2))
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 0]])
    cam = radegs.PinholeCamera.make(c2w, 0.9 * W, 0.9 * W, W, H)
    args = (sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0], sc["sh"][:, 1:])
    kw = dict(rasterize_mode="antialiased", regularization_from_iter=0, output_depth_during_training=True)
    fm = radegs.RadegsFeaturesModel(radegs.RadegsFeaturesModelConfig(**kw), *args, feats).to(dev)
    bm = radegs.RadegsModel(radegs.RadegsModelConfig(**kw), *args).to(dev)
    fm.train(); bm.train()
    fm.step = bm.step = 5000
    fo, bo = fm.get_outputs(cam), bm.get_outputs(cam)
    assert fo["features"].shape == (H, W, 13) and "features" not in bo
    for k in ("rgb", "depth", "median_depth", "accumulation", "normals", "depth_im", "depth_normal_error_map"):
        assert rel_err(fo[k], bo[k]) < 1e-6, k
    acc = fo["accumulation"]                                         # features in [0, 1]: sum w f <= sum w = alpha, pixel by pixel
    assert float(fo["features"].min()) >= 0.0 and bool((fo["features"].amax(-1, keepdim=True) <= acc + 1e-5).all())
    assert float(fo["features"].max()) > 0.1
    loss = fm.get_loss_dict(fo, {"image": torch.rand(H, W, 3)})
    (sum(loss.values()) + fo["features"].square().mean()).backward()
    for k, p in fm.gauss_params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all() and (k != "distill_features" or p.grad.abs().sum() > 0), k


def test_features_model_mirror_dense_scene_records_on_demand_equal_the_dense_stages(dev, monkeypatch):
    """``RadegsFeaturesModel`` on a dense scene (300 k Gaussians: the training path takes the N-D records ON DEMAND -- no colour
    kernel, no feature copy, rows cleared on touch, flagged-row backward; activations inside the kernels): the outputs are
    bit for bit those of the dense colour stages (``MISPLAT_LAZY_ND=0``) and the gradients of all seven parameter groups agree to
    the order of the atomic sums, steady state (third step of each)."""
    from collab_splats_amd import ops, radegs
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 640, 360, 300_000
    sc = random_scene(N, W, H, seed=12)
    feats = torch.rand(N, 13, generator=torch.Generator().manual_seed(4))
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 0]])
    cam = radegs.PinholeCamera.make(c2w, 0.9 * W, 0.9 * W, W, H)
    args = (sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0], sc["sh"][:, 1:])
    kw = dict(rasterize_mode="antialiased", regularization_from_iter=0, output_depth_during_training=True)
    gt = {"image": torch.rand(H, W, 3, generator=torch.Generator().manual_seed(6))}
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setattr(ops, "LAZY_ND", mode)
        monkeypatch.setattr(ops, "LAZY_SH", "1")
        m = radegs.RadegsFeaturesModel(radegs.RadegsFeaturesModelConfig(**kw), *args, feats).to(dev)
        m.train()
        m.step = 5000
        before = dict(ops.PATH_STATS)
        for it in range(3):
            for p in m.gauss_params.values():
                p.grad = None
            out = m.get_outputs(cam)
            loss = m.get_loss_dict(out, gt)
            (sum(loss.values()) + out["features"].square().mean()).backward()
        took = {k: ops.PATH_STATS[k] - before.get(k, 0) for k in ops.PATH_STATS}
        assert took.get("forward_nd") == 3 and took.get("forward_lazy_colour", 0) == (3 if mode == "1" else 0), took
        assert took.get("backward_background_fill", 0) == (3 if mode == "1" else 0), took
        res[mode] = ({k: out[k].detach().clone() for k in ("rgb", "features", "depth", "accumulation", "normals")},
                     {k: p.grad.clone() for k, p in m.gauss_params.items()})
    for k, v in res["1"][0].items():
        assert torch.equal(v, res["0"][0][k]), k
    for k, g in res["1"][1].items():
        assert torch.isfinite(g).all() and rel_err(g, res["0"][1][k]) < 2e-5, (k, rel_err(g, res["0"][1][k]))


def test_crop_box_renders_exactly_the_cropped_subset(dev):
    """rade_gs_model.py:96-119 (evaluation only): a crop box selects Gaussians by ``within(means)``; the outputs are those
    of a model that holds only the selected ones, and an empty crop returns ``get_empty_outputs``."""
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 200, 120, 5000
    sc = random_scene(N, W, H, seed=4)
    cfg = radegs.RadegsModelConfig(rasterize_mode="antialiased")

    def make(sel):
        return radegs.RadegsModel(cfg, sc["means"][sel], sc["log_scales"][sel], sc["quats"][sel], sc["opacity_logits"][sel],
                                  sc["sh"][sel, 0], sc["sh"][sel, 1:]).to(dev).eval()

    class Box:
        def __init__(self, lo):
            self.lo = lo

        def within(self, pts):
            return (pts[:, 0] > self.lo)[:, None]

    c2w = torch.tensor([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 0]])
    cam = radegs.PinholeCamera.make(c2w, 0.9 * W, 0.9 * W, W, H)
    full = make(slice(None))
    sel = sc["means"][:, 0] > 0.0
    part = make(sel)
    # (the meshing loop hands the box to get_outputs_for_camera, which installs it as the crop box: mesh.py:1581-1584)
    a, b = full.get_outputs_for_camera(cam, obb_box=Box(0.0)), part.get_outputs_for_camera(cam)
    for k in ("rgb", "depth", "median_depth", "accumulation", "normals", "depth_im"):
        assert torch.equal(a[k], b[k]), k
    full.set_crop(Box(0.0))                                               # ... or set_crop + get_outputs in evaluation mode
    c = full.get_outputs(cam)
    assert torch.equal(c["rgb"], b["rgb"])
    e = full.get_outputs_for_camera(cam, obb_box=Box(1e9))
    assert set(e) == {"rgb", "depth", "accumulation", "background"} and e["rgb"].shape == (H, W, 3)


def test_end_to_end_optimisation_recovers_a_scene(dev):
    """Independent of every oracle: perturb a scene, fit it back to its own renders (colour + expected depth +
    normals) with Adam through the HIP backward.  Wrong-signed or mis-scaled gradients cannot pass this."""
    from collab_splats_amd import rasterization
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 160, 96, 1500
    sc = random_scene(N, W, H, seed=31)
    V, K = sc["viewmats"].to(dev), sc["Ks"].to(dev)

    def render(p):
        return rasterization(p["means"], p["quats"], torch.exp(p["log_scales"]), torch.sigmoid(p["opacity_logits"]), p["sh"],
                             V, K, W, H, sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased",
                             return_depth_normal=True)

    truth = {k: sc[k].to(dev) for k in ("means", "log_scales", "quats", "opacity_logits", "sh")}
    with torch.no_grad():
        target = [t.clone() for t in render(truth)[:5]]
    g = torch.Generator().manual_seed(5)
    noise = {"means": 0.03, "log_scales": 0.3, "quats": 0.2, "opacity_logits": 0.8, "sh": 0.3}
    params = {k: (v + noise[k] * torch.randn(v.shape, generator=g).to(dev)).requires_grad_(True) for k, v in truth.items()}
    lrs = {"means": 2e-3, "log_scales": 1e-2, "quats": 5e-3, "opacity_logits": 5e-2, "sh": 2e-2}
    opt = torch.optim.Adam([{"params": [params[k]], "lr": lrs[k]} for k in params])

    def loss_fn():
        out = render(params)
        return sum((o - t).abs().mean() * wgt for o, t, wgt in zip(out[:5], target, (1.0, 1.0, 0.1, 0.0, 0.5)))

    first = loss_fn().item()
    for _ in range(150):
        opt.zero_grad(set_to_none=True)
        loss = loss_fn()
        loss.backward()
        opt.step()
    last = loss_fn().item()
    assert np.isfinite(last) and last < 0.35 * first, (first, last)
    assert all(torch.isfinite(p).all() for p in params.values())


def test_training_loop_with_densification(dev):
    """Model mirror + one Adam per parameter group + DefaultStrategy refinement every 25 steps, multi-view: the loss
    falls, the scene is resized, and parameters / optimizer moments stay aligned throughout."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "train_synthetic", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    log = mod.train(steps=120, n=3000, W=160, H=96, n_views=4, refine_every=25, verbose=False)
    losses = [l for l, _, _ in log]
    assert all(np.isfinite(losses))
    assert np.mean(losses[-8:]) < 0.75 * np.mean(losses[:8]), (losses[:8], losses[-8:])     # L1 colour loss
    sizes = {n for _, n, _ in log}
    assert len(sizes) > 1                                                 # densification resized the scene
    assert sum(sum(c) for _, _, c in log) > 0


# ---------------------------------------------------------------- BASELINE full size: properties
@pytest.fixture(scope="module")
def full(dev):
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 1920, 1080, 1_000_000
    sc = random_scene(N, W, H, seed=42)
    return sc, W, H, N


def test_full_size_properties(dev, full, grad_mode):
    """1 M Gaussians, 1080p (BASELINE configs[2]): sortedness, tile ranges, invariants, bitwise
    determinism (forward always; backward in deterministic mode) and linearity of the backward."""
    sc, W, H, N = full
    leaves, out = _run_gpu(sc, dev, W, H, render_mode="RGB+ED", rasterize_mode="antialiased")
    r, a, ed, md, n, meta = out
    keys = meta["isect_ids"]
    I = meta["n_isects"]
    assert I == int(meta["tiles_per_gauss"].sum()) and I > 4_000_000
    assert bool((keys[1:] >= keys[:-1]).all())                                        # sorted
    offs = meta["isect_offsets"].reshape(-1).long()
    assert bool((offs[1:] >= offs[:-1]).all()) and int(offs[0]) == 0 and int(offs[-1]) <= I
    tiles = (keys >> 32)
    probe = torch.randint(0, offs.numel() - 1, (2000,), device=dev)
    nonempty = offs[probe + 1] > offs[probe]
    p = probe[nonempty]
    assert bool((tiles[offs[p]] == p).all()) and bool((tiles[offs[p + 1] - 1] == p).all())
    fl = meta["flatten_ids"].long()
    assert int(fl.min()) >= 0 and int(fl.max()) < N
    vis = (meta["radii"][0] > 0).any(-1)
    assert bool(vis[fl].all())                                                        # only visible Gaussians are binned
    assert float(a.detach().min()) >= 0 and float(a.detach().max()) < 1.0                              # alpha = 1 - T, T > t_stop
    assert bool((n.norm(dim=-1, keepdim=True) <= a + 1e-5).all())                    # |sum w n| <= sum w
    assert bool(torch.isfinite(r).all() and torch.isfinite(ed).all() and torch.isfinite(md).all())
    zmin, zmax = float(meta["depths"][0][vis].detach().min()), float(meta["depths"][0][vis].detach().max())
    has = a[..., 0] > 0.5
    assert float(md[..., 0][has].min()) > 0.5 * zmin and float(md[..., 0][has].max()) < 2.0 * zmax
    ups1 = [u.to(dev) for u in upstream([t.shape for t in (r, a, ed, md, n)], seed=1, dtype=torch.float32)]
    ups2 = [u.to(dev) for u in upstream([t.shape for t in (r, a, ed, md, n)], seed=2, dtype=torch.float32)]

    def grads(ups):
        for l in leaves:
            l.grad = None
        torch.autograd.backward([r, a, ed, md, n], ups, retain_graph=True)
        return [l.grad.clone() for l in leaves]

    g1, g1b, g2 = grads(ups1), grads(ups1), grads(ups2)
    g12 = grads([x + y for x, y in zip(ups1, ups2)])
    for x, y in zip(g1, g1b):
        if grad_mode:
            assert torch.equal(x, y)                                                  # bitwise reproducible backward
        else:
            assert rel_err(x, y) < 1e-4, rel_err(x, y)                                # atomics: order-dependent rounding
    for x, y, s in zip(g1, g2, g12):
        assert rel_err(x + y, s) < 1e-4                                               # backward is linear in the upstream
    _, out2 = _run_gpu(sc, dev, W, H, render_mode="RGB+ED", rasterize_mode="antialiased")
    for t1, t2 in zip(out[:5], out2[:5]):
        assert torch.equal(t1, t2)                                                    # bitwise reproducible forward


def test_full_size_permutation_invariance(dev, full):
    """Re-ordering the Gaussians (distinct depths) must not change any image: per pixel the
    compositing order is by depth, so the fp32 operation sequence is identical."""
    from collab_splats_amd import rasterization
    sc, W, H, N = full
    n = 200_000
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(n, generator=g)
    means = sc["means"][:n].clone()
    zs = 2.0 + 10.0 * (torch.randperm(n, generator=g).float() + 0.5) / n          # distinct depths by construction
    means[:, :2] *= (zs / means[:, 2])[:, None]
    means[:, 2] = zs
    base = [means, sc["quats"][:n], torch.exp(sc["log_scales"][:n]), torch.sigmoid(sc["opacity_logits"][:n]), sc["sh"][:n]]
    o1 = rasterization(*[t.to(dev) for t in base], sc["viewmats"].to(dev), sc["Ks"].to(dev), W, H, sh_degree=3,
                       render_mode="RGB+ED", return_depth_normal=True)
    o2 = rasterization(*[t[perm].to(dev) for t in base], sc["viewmats"].to(dev), sc["Ks"].to(dev), W, H, sh_degree=3,
                       render_mode="RGB+ED", return_depth_normal=True)
    d = o1[5]["depths"][0][(o1[5]["radii"][0] > 0).any(-1)]
    assert d.unique().numel() == d.numel()
    for t1, t2 in zip(o1[:5], o2[:5]):
        assert torch.equal(t1, t2)
    assert torch.equal(o1[5]["radii"][0][perm], o2[5]["radii"][0])


def test_fused_adam_matches_torch_adam(dev):
    """misplat_adam_step vs torch.optim.Adam on the six parameter groups with the reference's learning rates
    (rade_gs_method.py:44-71, eps = 1e-15): 25 steps, odd sizes (scalar tail), one fused launch for all groups."""
    from collab_splats_amd import FusedAdam, fused_adam_step_all
    g = torch.Generator().manual_seed(3)
    shapes = dict(means=(10007, 3), features_dc=(10007, 3), features_rest=(10007, 15, 3), opacities=(10007, 1),
                  scales=(10007, 3), quats=(10007, 4))
    lrs = dict(means=1.6e-4, features_dc=0.0025, features_rest=0.0025 / 20, opacities=0.05, scales=0.005, quats=0.001)
    init = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
    ref_p = {k: v.clone().to(dev).requires_grad_(True) for k, v in init.items()}
    our_p = {k: v.clone().to(dev).requires_grad_(True) for k, v in init.items()}
    ref_o = {k: torch.optim.Adam([ref_p[k]], lr=lrs[k], eps=1e-15) for k in shapes}
    our_o = {k: FusedAdam([our_p[k]], lr=lrs[k], eps=1e-15) for k in shapes}
    for step in range(25):
        for k in shapes:
            gr = (torch.randn(shapes[k], generator=g) * (10.0 ** float(torch.randint(-6, 1, (1,), generator=g)))).to(dev)
            if step == 7 and k == "quats":
                gr = None                                            # a group without a gradient is skipped
            ref_p[k].grad = None if gr is None else gr.clone()
            our_p[k].grad = None if gr is None else gr.clone()
        for o in ref_o.values():
            o.step()
        fused_adam_step_all(our_o)
    for k in shapes:
        assert rel_err(our_p[k], ref_p[k]) < 2e-6, k
        assert rel_err(our_o[k].state[our_p[k]]["exp_avg"], ref_o[k].state[ref_p[k]]["exp_avg"]) < 2e-6, k
        assert rel_err(our_o[k].state[our_p[k]]["exp_avg_sq"], ref_o[k].state[ref_p[k]]["exp_avg_sq"]) < 2e-6, k
        assert int(our_o[k].state[our_p[k]]["step"]) == int(ref_o[k].state[ref_p[k]]["step"])
    # single-optimizer step() and more than MISPLAT_ADAM_MAX_TENSORS parameters in one optimizer
    many = [torch.randn(33 + i, generator=g).to(dev).requires_grad_(True) for i in range(11)]
    many_ref = [m.detach().clone().requires_grad_(True) for m in many]
    o1, o2 = FusedAdam(many, lr=1e-2), torch.optim.Adam(many_ref, lr=1e-2)
    for _ in range(3):
        for a, b in zip(many, many_ref):
            gr = torch.randn(a.shape, generator=g).to(dev)
            a.grad, b.grad = gr.clone(), gr.clone()
        o1.step(); o2.step()
    for a, b in zip(many, many_ref):
        assert rel_err(a, b) < 2e-6


def test_render_views_batch_equals_single_view_outputs(dev):
    """Eval-time batch rendering (section 8(f) rank 4): V views through the camera batch dimension of the kernels
    give, view by view, exactly what get_outputs_for_camera gives one at a time; tsdf_frame reproduces the
    extrinsic / intrinsic the reference hands to Open3D (mesh.py:1591-1604, 1626-1630)."""
    import math
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene, view_matrix
    W, H, N = 200, 120, 8000
    sc = random_scene(N, W, H, seed=5)
    cfg = radegs.RadegsModelConfig(rasterize_mode="antialiased")
    model = radegs.RadegsModel(cfg, sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0],
                               sc["sh"][:, 1:]).to(dev).eval()
    model.step = 10_000
    flip = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0]))
    cams = []
    for i in range(5):
        c2w = torch.linalg.inv(view_matrix(i)[0]) @ flip                 # OpenCV w2c -> OpenGL c2w
        cams.append(radegs.PinholeCamera.make(c2w[:3, :4], 0.9 * W, 0.9 * W, W, H))
    batched = model.render_views(cams, batch_size=3)                        # batches of 3 + 2
    assert batched["rgb"].shape == (5, H, W, 3) and batched["depth"].shape == (5, H, W, 1)
    for i, cam in enumerate(cams):
        one = model.get_outputs_for_camera(cam)
        for k in ("rgb", "depth", "median_depth", "accumulation", "normals"):
            assert torch.equal(batched[k][i], one[k]), (i, k)
    assert (batched["accumulation"] > 0).float().mean() > 0.5
    ext, intr = radegs.tsdf_frame(cams[1])
    assert np.allclose(ext, view_matrix(1)[0].double().numpy(), atol=1e-6)  # world -> OpenCV camera
    assert intr == dict(width=W, height=H, fx=0.9 * W, fy=0.9 * W, cx=W / 2.0, cy=H / 2.0)


def test_many_tiles_fall_back_to_32bit_tile_keys(dev):
    """C * tiles > 65536 (5 cameras x 128 x 128 tiles) takes the 32-bit tile-key path of the bucket sort; every
    camera of the batch must still equal its own single-camera render bit for bit."""
    from collab_splats_amd import rasterization
    from collab_splats_amd.synthetic import random_scene, view_matrix
    W = H = 2048
    N = 3000
    sc = random_scene(N, W, H, seed=9)
    base = [sc["means"].to(dev), sc["quats"].to(dev), torch.exp(sc["log_scales"]).to(dev) * 4.0,
            torch.sigmoid(sc["opacity_logits"]).to(dev), sc["sh"].to(dev)]
    V = torch.cat([view_matrix(i) for i in range(5)], dim=0).to(dev)
    K = sc["Ks"].to(dev).expand(5, 3, 3).contiguous()
    kw = dict(sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True)
    full = rasterization(*base, V, K, W, H, **kw)
    assert full[5]["isect_offsets"].numel() == 5 * 128 * 128 > 65536
    for c in (0, 3, 4):
        one = rasterization(*base, V[c:c + 1], K[c:c + 1], W, H, **kw)
        for a, b in zip(full[:5], one[:5]):
            assert torch.equal(a[c], b[0]), c
        assert (one[1] > 0).any()


@pytest.mark.parametrize("lazy", ["0", "1"])
def test_shared_gaussians_multi_view_gradients_add_up(dev, monkeypatch, lazy):
    """(also with the on-demand colours forced on: several cameras in one call)
    BASELINE configs[4]/[5] semantics: with C views in one call the parameter gradients are the SUM of the
    per-view gradients (what data-parallel ranks all-reduce), and the per-view images equal the single-view ones."""
    from collab_splats_amd import ops, rasterization
    from collab_splats_amd.synthetic import random_scene, view_matrix
    monkeypatch.setattr(ops, "LAZY_SH", lazy)
    W, H, N, C = 480, 270, 60_000, 4
    sc = random_scene(N, W, H, seed=17)
    V = torch.cat([view_matrix(i) for i in range(C)], dim=0).to(dev)
    K = sc["Ks"].to(dev).expand(C, 3, 3).contiguous()
    kw = dict(sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True)

    def leaves():
        return [sc["means"].to(dev).requires_grad_(True), sc["quats"].to(dev).requires_grad_(True),
                torch.exp(sc["log_scales"]).to(dev).requires_grad_(True),
                torch.sigmoid(sc["opacity_logits"]).to(dev).requires_grad_(True), sc["sh"].to(dev).requires_grad_(True)]

    lb = leaves()
    full = rasterization(*lb, V, K, W, H, **kw)
    ups = [u.to(dev) for u in upstream([t.shape for t in full[:5]], dtype=torch.float32)]
    torch.autograd.backward(list(full[:5]), ups)
    acc = None
    for c in range(C):
        lc = leaves()
        one = rasterization(*lc, V[c:c + 1], K[c:c + 1], W, H, **kw)
        for a, b in zip(full[:5], one[:5]):
            assert torch.equal(a[c], b[0]), c
        torch.autograd.backward(list(one[:5]), [u[c:c + 1] for u in ups])
        acc = [l.grad.clone() for l in lc] if acc is None else [x + l.grad for x, l in zip(acc, lc)]
    for name, l, s in zip(("means", "quats", "scales", "opacities", "sh"), lb, acc):
        assert rel_err(l.grad, s) < 1e-4, (name, rel_err(l.grad, s))


def test_five_million_gaussians_bins_and_images(dev):
    """BASELINE configs[4] size (5 M Gaussians, 1080p, ~32 M intersections; buckets of ~4 000 entries take the large
    size classes of the per-tile sort): sorted keys, monotone offsets, finite images, bitwise reproducible forward."""
    from collab_splats_amd import rasterization
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 1920, 1080, 5_000_000
    sc = random_scene(N, W, H, seed=42)
    args = [sc["means"].to(dev), sc["quats"].to(dev), torch.exp(sc["log_scales"]).to(dev),
            torch.sigmoid(sc["opacity_logits"]).to(dev), sc["sh"].to(dev), sc["viewmats"].to(dev), sc["Ks"].to(dev), W, H]
    kw = dict(sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True)
    with torch.no_grad():
        o1 = rasterization(*args, **kw)
        o2 = rasterization(*args, **kw)
    meta = o1[5]
    I = meta["n_isects"]
    assert I > 25_000_000 and I == int(meta["tiles_per_gauss"].sum())
    keys = meta["isect_ids"]
    assert bool((keys[1:] >= keys[:-1]).all())                        # (tile, depth) order
    same = keys[1:] == keys[:-1]
    fl = meta["flatten_ids"]
    assert bool((fl[1:][same] > fl[:-1][same]).all())                 # ties broken by Gaussian id
    offs = meta["isect_offsets"].reshape(-1).long()
    assert bool((offs[1:] >= offs[:-1]).all()) and int(offs[0]) == 0
    cnt = torch.diff(offs, append=offs.new_tensor([I]))
    assert int(cnt.max()) > 4096                                       # the 8192-entry class is exercised
    for a, b in zip(o1[:5], o2[:5]):
        assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("view", range(8))
def test_full_size_rotated_views_properties(dev, full, view):
    """BASELINE configs[3]: the per-GPU workload of the 8-view run -- 1 M Gaussians at 1080p under each of the eight
    rotated ``view_matrix(i)`` cameras (rank i renders view i) -- through the size-independent properties: sorted
    keys with id-ordered ties, consistent tile ranges, only visible Gaussians binned, |sum w n| <= alpha, finite
    images and gradients, a bitwise reproducible forward, and a backward that is linear in the upstream gradients."""
    from collab_splats_amd.synthetic import view_matrix
    sc, W, H, N = full
    scv = dict(sc)
    scv["viewmats"] = view_matrix(view)
    leaves, out = _run_gpu(scv, dev, W, H, render_mode="RGB+ED", rasterize_mode="antialiased")
    r, a, ed, md, n, meta = out
    keys, I = meta["isect_ids"], meta["n_isects"]
    assert I == int(meta["tiles_per_gauss"].sum()) and I > 3_000_000
    assert bool((keys[1:] >= keys[:-1]).all())
    fl = meta["flatten_ids"].long()
    same = keys[1:] == keys[:-1]
    assert bool((fl[1:][same] > fl[:-1][same]).all())
    offs = meta["isect_offsets"].reshape(-1).long()
    assert bool((offs[1:] >= offs[:-1]).all()) and int(offs[0]) == 0 and int(offs[-1]) <= I
    cnt = torch.diff(offs, append=offs.new_tensor([I]))
    tiles_of = torch.repeat_interleave(torch.arange(offs.numel(), device=dev), cnt)
    assert torch.equal(tiles_of, (keys >> 32))                                        # every tile range holds its own keys
    vis = (meta["radii"][0] > 0).any(-1)
    assert int(fl.min()) >= 0 and int(fl.max()) < N and bool(vis[fl].all())
    assert float(a.detach().min()) >= 0 and float(a.detach().max()) < 1.0
    assert bool((n.norm(dim=-1, keepdim=True) <= a + 1e-5).all())
    for t in (r, ed, md, n):
        assert bool(torch.isfinite(t).all())
    ups1 = [u.to(dev) for u in upstream([t.shape for t in (r, a, ed, md, n)], seed=1, dtype=torch.float32)]
    ups2 = [u.to(dev) for u in upstream([t.shape for t in (r, a, ed, md, n)], seed=2, dtype=torch.float32)]

    def grads(ups):
        for l in leaves:
            l.grad = None
        torch.autograd.backward([r, a, ed, md, n], ups, retain_graph=True)
        return [l.grad.clone() for l in leaves]

    g1, g2 = grads(ups1), grads(ups2)
    g12 = grads([x + y for x, y in zip(ups1, ups2)])
    for x, y, s_ in zip(g1, g2, g12):
        assert bool(torch.isfinite(x).all())
        assert rel_err(x + y, s_) < 1e-4
    _, out2 = _run_gpu(scv, dev, W, H, render_mode="RGB+ED", rasterize_mode="antialiased")
    for t1, t2 in zip(out[:5], out2[:5]):
        assert torch.equal(t1, t2)


def test_config5_five_million_model_step_with_depth_normal_loss(dev):
    """BASELINE configs[4] minus the collective: 5 M shared Gaussians at 1080p through the product model mirror --
    ``RadegsModel.get_outputs`` (step >= regularization_from_iter, so a3 + a4 run) -> ``get_loss_dict`` (L1 + the
    depth-normal consistency term, rade_gs_model.py:202-214, 292-307) -> backward.  Finite gradients on all six
    parameter groups, linear in the loss scale, and bitwise repeatable in deterministic mode."""
    from collab_splats_amd import ops, radegs
    from collab_splats_amd.synthetic import random_scene
    W, H, N = 1920, 1080, 5_000_000
    sc = random_scene(N, W, H, seed=42)
    cfg = radegs.RadegsModelConfig(rasterize_mode="antialiased", regularization_from_iter=0)
    model = radegs.RadegsModel(cfg, sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0],
                               sc["sh"][:, 1:]).to(dev)
    model.train()
    model.step = 20000
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 0]])
    cam = radegs.PinholeCamera.make(c2w, 0.9 * W, 0.9 * W, W, H)
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(9)).to(dev)

    def step(scale):
        for p in model.gauss_params.values():
            p.grad = None
        out = model.get_outputs(cam)
        loss = model.get_loss_dict(out, {"image": target})
        assert set(loss) == {"main_loss", "scale_reg", "depth_normal_loss"}
        (scale * sum(loss.values())).backward()
        return {k: float(v) for k, v in loss.items()}, {k: p.grad.clone() for k, p in model.gauss_params.items()}

    old = ops.DETERMINISTIC_BACKWARD
    try:
        ops.set_deterministic(True)
        l1, g1 = step(1.0)
        l1b, g1b = step(1.0)
        _, g2 = step(2.0)
    finally:
        ops.set_deterministic(old)
    assert model.info["n_isects"] > 25_000_000
    assert l1 == l1b and 0 < l1["depth_normal_loss"] < 0.05 and 0 < l1["main_loss"] < 1
    assert set(g1) == {"means", "scales", "quats", "opacities", "features_dc", "features_rest"}
    for k in g1:
        assert bool(torch.isfinite(g1[k]).all()) and float(g1[k].abs().max()) > 0, k
        assert torch.equal(g1[k], g1b[k]), k                                          # deterministic mode: bitwise repeat
        assert rel_err(g2[k], 2.0 * g1[k]) < 1e-5, k                                  # linear in the loss scale
    _, ga = step(1.0)                                                                 # default (atomic) mode agrees
    for k in g1:
        assert rel_err(ga[k], g1[k]) < 1e-4, (k, rel_err(ga[k], g1[k]))


@pytest.mark.parametrize("i", [0, 1, 2])
def test_get_loss_dict_depth_normal_term_vs_reference_goldens(dev, i):
    """a5 through the PRODUCT function: the error maps of the fused a4 kernel go into ``RadegsModel.get_loss_dict``
    (rade_gs_model.py:289-307) and its value and gradients are compared with what the reference's own code produced
    (tests/golden/make_camera_goldens.py)."""
    from collab_splats_amd import ops, radegs
    g = np.load(GOLD)
    W, H = [int(v) for v in g[f"cam{i}_WH"]]
    fovx, fovy = g[f"cam{i}_fov"]
    fx, fy = W / (2 * np.tan(fovx / 2)), H / (2 * np.tan(fovy / 2))
    d1 = torch.from_numpy(g[f"dn{i}_d1"]).to(dev).requires_grad_(True)
    d2 = torch.from_numpy(g[f"dn{i}_d2"]).to(dev).requires_grad_(True)
    nr = torch.from_numpy(g[f"dn{i}_nrm"]).to(dev).requires_grad_(True)
    _, err = ops.depth_normal(d1, d2, nr, fx, fy)
    one = torch.zeros(1, 3)
    model = radegs.RadegsModel(radegs.RadegsModelConfig(regularization_from_iter=15000), one, one, torch.ones(1, 4),
                               torch.zeros(1), one, torch.zeros(1, 15, 3))
    outputs = {"rgb": torch.zeros(H, W, 3, device=dev), "depth_normal_error_map": err[0].unsqueeze(-1),
               "middepth_normal_error_map": err[1].unsqueeze(-1)}
    model.step = 14999
    assert "depth_normal_loss" not in model.get_loss_dict(outputs, None)             # inactive before regularization_from_iter
    model.step = 15000
    loss = model.get_loss_dict(outputs, None)
    assert set(loss) == {"depth_normal_loss"}
    assert abs(loss["depth_normal_loss"].item() - float(g[f"dn{i}_loss"])) < 1e-6
    loss["depth_normal_loss"].backward()
    assert rel_err(d1.grad, g[f"dn{i}_v_d1"]) < TOL
    assert rel_err(d2.grad, g[f"dn{i}_v_d2"]) < TOL
    assert rel_err(nr.grad, g[f"dn{i}_v_nrm"]) < TOL


@pytest.mark.parametrize("H,W", [(7, 5), (270, 480), (1080, 1920)])
def test_fused_loss_node_equals_the_torch_formulas(dev, H, W):
    """ops.mean_losses (misplat_loss_fwd / misplat_loss_bwd): the L1 term and the depth-normal term of get_loss_dict
    (rade_gs_model.py:289-307) with their gradients, against the reference's torch expressions; reproducible bit for
    bit; error maps packed in one [2,H,W] tensor (what get_outputs hands over) or given separately; either term alone."""
    from collab_splats_amd import ops
    g = torch.Generator().manual_seed(H * W)
    rgb0 = torch.rand(H, W, 3, generator=g).to(dev)
    gt = torch.rand(H, W, 3, generator=g).to(dev)
    gt[0, 0] = rgb0[0, 0]                                      # sign(0) = 0 in the backward
    err0 = torch.rand(2, H, W, generator=g).to(dev)
    r, lam = 0.6, 0.05

    def reference():
        rgb, err = rgb0.clone().requires_grad_(True), err0.clone().requires_grad_(True)
        l1 = torch.abs(gt - rgb).mean()
        dn = lam * ((1 - r) * err[0].unsqueeze(-1).mean() + r * err[1].unsqueeze(-1).mean())
        (1.7 * l1 + 0.3 * dn).backward()
        return l1.detach(), dn.detach(), rgb.grad, err.grad

    l1_ref, dn_ref, vrgb_ref, verr_ref = reference()
    seen = []
    for packed in (True, False):
        rgb, err = rgb0.clone().requires_grad_(True), err0.clone().requires_grad_(True)
        if packed:
            l1, dn = ops.mean_losses(rgb, gt, err=err, depth_ratio=r, depth_normal_lambda=lam)
        else:
            l1, dn = ops.mean_losses(rgb, gt, e1=err[0].unsqueeze(-1), e2=err[1].unsqueeze(-1), depth_ratio=r,
                                     depth_normal_lambda=lam)
        (1.7 * l1 + 0.3 * dn).backward()
        assert abs(float(l1) - float(l1_ref)) <= 2e-6 * float(l1_ref) and abs(float(dn) - float(dn_ref)) <= 2e-6 * float(dn_ref)
        assert torch.allclose(rgb.grad, vrgb_ref, rtol=1e-6, atol=0) and torch.allclose(err.grad, verr_ref, rtol=1e-6, atol=0)
        assert float(rgb.grad[0, 0].abs().sum()) == 0.0
        seen.append((l1.detach().clone(), dn.detach().clone()))
    assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1])
    rgb = rgb0.clone().requires_grad_(True)                    # one term alone
    l1, none = ops.mean_losses(rgb, gt)
    assert none is None and torch.equal(l1.detach(), seen[0][0])
    l1.backward()
    assert torch.allclose(rgb.grad * 1.7, vrgb_ref, rtol=1e-6, atol=0)
    err = err0.clone().requires_grad_(True)
    none, dn = ops.mean_losses(None, None, err=err, depth_ratio=r, depth_normal_lambda=lam)
    assert none is None and torch.equal(dn.detach(), seen[0][1])
    dn.backward()
    assert torch.allclose(err.grad * 0.3, verr_ref, rtol=1e-6, atol=0)


@pytest.mark.parametrize("H,W", [(11, 11), (37, 53), (120, 200), (1080, 1920)])
def test_main_loss_l1_plus_ssim_vs_the_pytorch_msssim_restatement(dev, H, W):
    """The image term the model inherits from Splatfacto (rade_gs_model.py:289 -> nerfstudio, third-party)
    [UNVERIFIED-UPSTREAM]: main_loss = 0.8 L1 + 0.2 (1 - SSIM), SSIM as pytorch_msssim computes it (11-tap gaussian,
    valid region).  ``ops.mean_losses(..., ssim_lambda=...)`` (misplat_loss_fwd + misplat_ssim_fwd / misplat_ssim_bwd)
    against oracle/ssim_oracle.py in fp64 with autograd: value within 2e-6, gradient image within 1e-4 of its own
    scale; twice the same bits; the gradient scales with the upstream gradient; identical images give exactly 0 loss
    and 0 gradient... up to rounding of 1 - SSIM; the depth-normal half of the node is unchanged by the SSIM half."""
    from collab_splats_amd import ops
    from oracle import ssim_oracle
    g = torch.Generator().manual_seed(H * 7 + W)
    gt = torch.rand(H, W, 3, generator=g)
    # a prediction correlated with the target (a training image, not noise): SSIM well inside (0, 1)
    pred = (gt + 0.15 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
    lam = 0.2
    p64 = pred.double().requires_grad_(True)
    ref = ssim_oracle.main_loss(p64, gt.double(), lam)
    ref.backward()
    rgb = pred.to(dev).requires_grad_(True)
    gtd = gt.to(dev)
    main, none = ops.mean_losses(rgb, gtd, ssim_lambda=lam)
    assert none is None
    (3.0 * main).backward()
    assert abs(float(main) - float(ref)) < 2e-6, (float(main), float(ref))
    got = rgb.grad.cpu().double() / 3.0
    scale = float(p64.grad.abs().max())
    assert float((got - p64.grad).abs().max()) < 1e-4 * scale, float((got - p64.grad).abs().max()) / scale
    rgb2 = pred.to(dev).requires_grad_(True)
    main2, _ = ops.mean_losses(rgb2, gtd, ssim_lambda=lam)
    (3.0 * main2).backward()
    assert torch.equal(main2, main) and torch.equal(rgb2.grad, rgb.grad)
    # with the depth-normal maps in the same node
    err = torch.rand(2, H, W, generator=g).to(dev).requires_grad_(True)
    main3, dn = ops.mean_losses(rgb2.detach().requires_grad_(True), gtd, err=err, depth_ratio=0.6, depth_normal_lambda=0.05,
                                ssim_lambda=lam)
    _, dn_ref = ops.mean_losses(None, None, err=err.detach().requires_grad_(True), depth_ratio=0.6, depth_normal_lambda=0.05)
    assert torch.equal(main3, main) and torch.equal(dn, dn_ref)
    # identical images
    same = gtd.clone().requires_grad_(True)
    zero, _ = ops.mean_losses(same, gtd, ssim_lambda=lam)
    zero.backward()
    assert abs(float(zero)) < 1e-6 and float(same.grad.abs().max()) < 1e-6 * float(rgb.grad.abs().max())


def test_main_loss_rejects_images_smaller_than_the_ssim_window(dev):
    from collab_splats_amd import ops
    rgb, gt = torch.rand(10, 40, 3, device=dev), torch.rand(10, 40, 3, device=dev)
    with pytest.raises(ValueError, match="11 x 11"):
        ops.mean_losses(rgb, gt, ssim_lambda=0.2)
    l1, _ = ops.mean_losses(rgb, gt)                                   # the L1 term alone has no such limit
    assert abs(float(l1) - float((gt - rgb).abs().mean())) < 1e-6


def _bench_like_scene(dev, N, W, H, seed, scale_mul=1.0):
    from collab_splats_amd.synthetic import random_scene
    sc = random_scene(N, W, H, seed=seed)
    return [sc["means"].to(dev), sc["quats"].to(dev), (torch.exp(sc["log_scales"]) * scale_mul).to(dev),
            torch.sigmoid(sc["opacity_logits"]).to(dev), sc["sh"].to(dev), sc["viewmats"].to(dev), sc["Ks"].to(dev), W, H]


def _fwd_bwd(args, leaves=None, **flags):
    """One forward + backward under temporary ``ops`` switches; returns (images, gradients, meta).  ``leaves``: the
    parameter tensors to use (and reuse: a training loop's addresses repeat, fresh clones' do not)."""
    from collab_splats_amd import ops, rasterization
    old = {k: getattr(ops, k) for k in flags}
    for k, v in flags.items():
        setattr(ops, k, v)
    try:
        if leaves is None:
            leaves = [t.clone().requires_grad_(True) for t in args[:5]]
        for l in leaves:
            l.grad = None
        out = rasterization(*leaves, *args[5:], sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased",
                            return_depth_normal=True)
        ups = [u.to(out[0].device) for u in upstream([t.shape for t in out[:5]], dtype=torch.float32)]
        torch.autograd.backward(list(out[:5]), ups)
        torch.cuda.synchronize()
        return [t.detach().clone() for t in out[:5]], [l.grad.clone() for l in leaves], out[5]
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


def test_one_entry_forward_speculation_and_graph_replay_change_nothing(dev):
    """The host-side machinery of the default path -- one C entry per phase (misplat_raster_fwd), the speculative
    intersection capacity, hipGraph replay, longest-first launch order -- must be invisible in the results: the images
    are bitwise those of the stage-by-stage path, the bins identical, the gradients equal up to atomic summation order."""
    args = _bench_like_scene(dev, 30_000, 640, 360, seed=5)
    ref_img, ref_grad, ref_meta = _fwd_bwd(args, FUSED_ENTRY=False, UNIT_ORDER=False)
    variants = [dict(FUSED_ENTRY=True, SPECULATE=False, GRAPHS=False, UNIT_ORDER=False),
                dict(FUSED_ENTRY=True, SPECULATE=True, GRAPHS=False, UNIT_ORDER=True),
                dict(FUSED_ENTRY=True, SPECULATE=True, GRAPHS=True, UNIT_ORDER=True),
                dict(FUSED_ENTRY=False, UNIT_ORDER=True)]
    from collab_splats_amd import ops
    for flags in variants:
        leaves = None
        if flags.get("GRAPHS"):
            ops.reset_graph_cache()                        # (earlier tests' many shapes may have paused captures)
            leaves = [t.clone().requires_grad_(True) for t in args[:5]]     # one set of parameters, as a training loop has
        for rep in range(6 if leaves else 3):              # repeats: capacity hints, cached launch orders and graphs are reused
            img, grad, meta = _fwd_bwd(args, leaves, **flags)
            for a, b in zip(img, ref_img):
                assert torch.equal(a, b), (flags, rep)
            assert meta["n_isects"] == ref_meta["n_isects"]
            assert torch.equal(meta["flatten_ids"], ref_meta["flatten_ids"]), (flags, rep)
            assert torch.equal(meta["isect_offsets"], ref_meta["isect_offsets"]), (flags, rep)
            for a, b in zip(grad, ref_grad):
                assert rel_err(a, b) < 1e-5, (flags, rep)
            del img, grad, meta, a, b                      # (nothing of this repeat stays allocated: the next one sees the same addresses)
        if flags.get("GRAPHS"):
            stats = ops.graph_cache_stats()
            assert stats["captures"] >= 1 and stats["hits"] >= 1, stats     # graphs were captured AND replayed above


def test_speculative_capacity_overflow_is_detected_and_redone_exactly(dev):
    """A capacity guessed from the previous call that turns out too small must not change anything: the second scene
    has the same shape but several times the intersections of the first, so the speculative launch overflows and phase B runs
    again with the exact size."""
    from collab_splats_amd import ops
    small = _bench_like_scene(dev, 20_000, 480, 270, seed=8)
    big = _bench_like_scene(dev, 20_000, 480, 270, seed=8, scale_mul=5.0)
    ref_img, ref_grad, ref_meta = _fwd_bwd(big, FUSED_ENTRY=False)
    ops._CAP_HINT.clear()
    ops._CAP_CHOSEN.clear()
    _, _, m_small = _fwd_bwd(small, FUSED_ENTRY=True, SPECULATE=True)
    assert ref_meta["n_isects"] > 1.5 * ops._quantise_cap(int(m_small["n_isects"] * ops.CAP_FIRST_MARGIN))   # it WILL overflow
    img, grad, meta = _fwd_bwd(big, FUSED_ENTRY=True, SPECULATE=True)
    assert meta["n_isects"] == ref_meta["n_isects"] == int(meta["tiles_per_gauss"].sum())
    assert torch.equal(meta["flatten_ids"], ref_meta["flatten_ids"])
    for a, b in zip(img, ref_img):
        assert torch.equal(a, b)
    for a, b in zip(grad, ref_grad):
        assert rel_err(a, b) < 1e-5
    img2, _, _ = _fwd_bwd(small, FUSED_ENTRY=True, SPECULATE=True)          # and back down (hint now too large: harmless)
    img3, _, _ = _fwd_bwd(small, FUSED_ENTRY=False)
    for a, b in zip(img2, img3):
        assert torch.equal(a, b)


@pytest.mark.parametrize("lazy", ["0", "1"])
def test_whole_step_graph_replays_equal_eager_steps(dev, monkeypatch, lazy):
    """(also with the on-demand colours forced on: the unset pattern, the flags and the sparse backward kernels inside a
    captured graph)
    graphs.GraphedStep: activations + forward + backward captured once with a fixed intersection capacity (no host
    synchronisation inside), replayed after the parameters changed in place: same images (bitwise) and gradients as an
    eager step on the same values; a capacity that is too small is reported, not silently truncated."""
    from collab_splats_amd import graphs, ops, rasterization, MisplatError
    from collab_splats_amd.synthetic import random_scene
    monkeypatch.setattr(ops, "LAZY_SH", lazy)
    N, W, H = 10_000, 256, 256
    sc = random_scene(N, W, H, seed=3)
    names = ("means", "log_scales", "quats", "opacity_logits", "sh")
    params = {k: sc[k].to(dev).requires_grad_(True) for k in names}
    V, K = sc["viewmats"].to(dev), sc["Ks"].to(dev)
    ups = [u.to(dev) for u in upstream([(1, H, W, 4), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)]

    def run(p):
        for t in p.values():
            t.grad = None
        out = rasterization(p["means"], p["quats"], torch.exp(p["log_scales"]), torch.sigmoid(p["opacity_logits"]), p["sh"],
                            V, K, W, H, sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased",
                            return_depth_normal=True)
        torch.autograd.backward(list(out[:5]), ups)
        # (nothing with autograd history may outlive the call: a graph kept alive from the previous iteration on another
        # stream breaks the capture -- PyTorch's AccumulateGrad stream rule)
        return [t.detach() for t in out[:5]], out[5]["n_isects"]

    _, n0 = run(params)
    torch.cuda.synchronize()
    n0 = int(n0)
    with pytest.raises(MisplatError):
        graphs.GraphedStep(lambda: run(params), capacity=n0 // 3)
    g = graphs.GraphedStep(lambda: run(params), capacity=2 * n0)
    static_grads = [params[k].grad for k in names]            # the graph writes these tensors on every replay
    for rep in range(3):
        with torch.no_grad():                                  # the optimiser's in-place update
            params["means"].add_(0.01 * (rep + 1))
            params["log_scales"].add_(0.02)
        imgs, n_dev = g.replay()
        n_graph = g.check()                                    # synchronises
        assert n_graph == int(n_dev)
        ref = {k: params[k].detach().clone().requires_grad_(True) for k in names}   # eager, same values, other tensors
        ref_imgs, ref_n = run(ref)
        torch.cuda.synchronize()
        assert n_graph == int(ref_n)
        for a, b in zip(imgs, ref_imgs):
            assert torch.equal(a, b), rep
        for a, k in zip(static_grads, names):
            assert rel_err(a, ref[k].grad) < 1e-5, (rep, k)
    # The launch-order feedback survives the capture: the captured step uses the warm-up stream's table (no zero-fill node
    # inside the graph that would wipe it on every replay), the projection kernel FOUND the record of this camera in the last
    # replay (selector word 1) and the record carries the camera's tag and a valid permutation.
    assert ops.PATH_STATS["capture_reused_order_table"] >= 1
    found = False
    for key, (table, sel, stride) in ops._ORDER_TABLES.items():
        if key[2:5] != (1, (W + 15) // 16, (H + 15) // 16):
            continue
        sel_h, head = sel.cpu(), table.view(-1, stride)[:, :3].cpu()
        hit = (head[:, 2] != 0) & ((head[:, 0] != 0) | (head[:, 1] != 0))
        found |= bool(sel_h[1] == 1) and bool(hit[int(sel_h[0])]) and (int(head[int(sel_h[0]), 0]), int(head[int(sel_h[0]), 1])) == (int(sel_h[2]), int(sel_h[3]))
    assert found


def test_one_whole_step_graph_per_resident_camera(dev):
    """graphs.GraphedViews: a trainer with its views resident on the device replays activations + forward + backward of view v
    as one hipGraph per view, in any order, while the parameters move in place.  The gradients live in STATIC tensors that every
    graph accumulates into (``p.grad.zero_()`` inside the step, not ``p.grad = None``: a replay does not run Python, so a
    ``.grad`` attribute assigned during one graph's capture would not follow the replays of another): every replay gives bitwise
    the images and (to 1e-5) the gradients of an eager step of that view on the same values."""
    from collab_splats_amd import graphs, ops, rasterization
    from collab_splats_amd.synthetic import random_scene, view_matrix
    N, W, H = 10_000, 256, 256
    sc = random_scene(N, W, H, seed=5)
    names = ("means", "log_scales", "quats", "opacity_logits", "sh")
    params = {k: sc[k].to(dev).requires_grad_(True) for k in names}
    views = [view_matrix(v).to(dev) for v in range(3)]
    K = sc["Ks"].to(dev)
    ups = [u.to(dev) for u in upstream([(1, H, W, 4), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)]

    def run(p, v):
        for t in p.values():
            if t.grad is None:
                t.grad = None
            else:
                t.grad.zero_()
        out = rasterization(p["means"], p["quats"], torch.exp(p["log_scales"]), torch.sigmoid(p["opacity_logits"]), p["sh"],
                            views[v], K, W, H, sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased",
                            return_depth_normal=True)
        torch.autograd.backward(list(out[:5]), ups)
        return [t.detach() for t in out[:5]], out[5]["n_isects"]

    n_max = 0
    for v in range(3):
        _, n = run(params, v)                                     # (leaves .grad tensors behind: the static ones from here on)
        torch.cuda.synchronize()
        n_max = max(n_max, int(n))
    static = {k: params[k].grad for k in names}
    gv = graphs.GraphedViews(lambda v: run(params, v), 3, capacity=2 * n_max)
    assert len(gv) == 3 and all(params[k].grad is static[k] for k in names)
    for rep, v in enumerate((2, 0, 1, 1, 2, 0)):
        with torch.no_grad():
            params["means"].add_(0.004)
            params["log_scales"].add_(0.01)
        imgs, n_dev = gv.replay(v)
        n_graph = gv.check(v)
        ref = {k: params[k].detach().clone().requires_grad_(True) for k in names}
        ref_imgs, ref_n = run(ref, v)
        torch.cuda.synchronize()
        assert n_graph == int(n_dev) == int(ref_n), (rep, v)
        for a, b in zip(imgs, ref_imgs):
            assert torch.equal(a, b), (rep, v)
        for k in names:
            assert rel_err(static[k], ref[k].grad) < 1e-5, (rep, v, k)
    # An overflow of ONE view must not be hidden by the replays of the others (advisor, round 4: one pinned count per device
    # was overwritten by whichever graph ran last).  Grow the Gaussians until the densest view outgrows the shared capacity
    # while another still fits, replay the dense view FIRST and the other one after it: check() raises all the same.
    from collab_splats_amd._lib import MisplatError
    cap = gv.capacity
    for _ in range(40):
        with torch.no_grad():
            params["log_scales"].add_(0.05)
        counts = []
        for v in range(3):
            ref = {k: params[k].detach().clone().requires_grad_(True) for k in names}
            counts.append(int(run(ref, v)[1]))
        if max(counts) > cap:
            break
    torch.cuda.synchronize()
    assert max(counts) > cap > min(counts), (counts, cap)
    dense, sparse = counts.index(max(counts)), counts.index(min(counts))
    gv.replay(dense)
    gv.replay(sparse)
    assert gv.steps[sparse].check() == counts[sparse]              # that view's own replay is fine ...
    with pytest.raises(MisplatError, match="exceed the fixed capacity"):
        gv.check()                                                 # ... the set of views is not


@pytest.mark.parametrize("N,W,H,scale_mul", [(30_000, 640, 360, 1.0), (5_000, 333, 197, 1.0), (60_000, 320, 200, 2.0)])
def test_on_demand_colours_equal_the_colour_kernel(dev, N, W, H, scale_mul):
    """MISPLAT_LAZY_SH: the compositing forward evaluates a record's SH colour when it first stages it (and the backward
    recomputes the Jacobian for the rows that have a gradient) instead of a colour kernel over all visible rows: the
    same images bit for bit (which of the two runs is a speed decision), the same bins, gradients equal up to rounding."""
    args = _bench_like_scene(dev, N, W, H, seed=21, scale_mul=scale_mul)
    ref_img, ref_grad, ref_meta = _fwd_bwd(args, LAZY_SH="0")
    for rep in range(2):
        img, grad, meta = _fwd_bwd(args, LAZY_SH="1")
        assert torch.equal(meta["flatten_ids"], ref_meta["flatten_ids"])
        for k, (a, b) in enumerate(zip(img, ref_img)):
            assert torch.equal(a, b), k                        # same colour bits from either evaluation: same images
        for k, (a, b) in enumerate(zip(grad, ref_grad)):
            assert torch.isfinite(a).all()
            assert rel_err(a, b) < 2e-5, (k, rel_err(a, b))


def test_background_fill_and_sparse_backward_equal_the_dense_backward(dev):
    """From 262 144 Gaussians the fused node's backward writes only the rows the compositing backward flagged, over
    zeros that extra workgroups of the compositing kernel's own grid wrote into the (uninitialised) gradient tensors:
    every row without a gradient must be exactly zero -- the allocator is seeded with NaNs first -- and the others equal
    the dense per-Gaussian backward of the two-node form (no row flags) up to the order of the atomic sums."""
    from collab_splats_amd import ops
    args = _bench_like_scene(dev, 300_000, 640, 360, seed=9, scale_mul=1.5)
    ref_img, ref_grad, _ = _fwd_bwd(args, FUSED_NODE=False)
    before = dict(ops.PATH_STATS)
    for rep in range(3):                                       # (capacity hint, merged phases, graph replay; lazy colours once dense)
        # the next allocations of these sizes come back full of NaNs: the output gradients, and the packed gradient rows
        # [N,16] -- which, with on-demand colours, nothing clears as a whole: the forward clears the row of each record
        # whose colour it sets (misplat_raster_args.lazy_colour = 2), and those are the only rows the backward reads
        poison = [torch.full((300_000 * 48 + 64 * k,), float("nan"), device=dev) for k in range(4)]
        poison += [torch.full((300_000 * 16,), float("nan"), device=dev) for k in range(3)]
        del poison
        img, grad, _ = _fwd_bwd(args)
        for a, b in zip(img, ref_img):
            assert torch.equal(a, b)
        for k, (a, b) in enumerate(zip(grad, ref_grad)):
            assert torch.isfinite(a).all(), (rep, k)
            assert rel_err(a, b) < 2e-5, (rep, k, rel_err(a, b))
            dead = b.reshape(b.shape[0], -1).abs().sum(1) == 0
            assert bool(dead.any()) and float(a.reshape(a.shape[0], -1)[dead].abs().sum()) == 0.0, (rep, k)
    took = {k: v - before.get(k, 0) for k, v in ops.PATH_STATS.items()}
    assert took.get("forward_lazy_colour", 0) >= 1 and took.get("forward_rows_on_touch", 0) == took["forward_lazy_colour"], took
    assert took.get("backward_rows_refilled", 0) == 0, took


def test_scene_above_2_5M_rows_head_fill_and_rows_on_touch_equal_the_dense_backward(dev):
    """From 2.5 M rows the zeros of the sparse backward are written by the FIRST workgroups of the compositing backward's
    grid (the tail is too short for 0.6 GB), the launch order table, the on-touch row clears and the flagged-rows
    backward all run at a size the rest of the suite does not reach: 2.6 M Gaussians at 640 x 360.  Images bitwise and
    gradients (to the order of the atomic sums) those of the two-node form with its dense per-Gaussian backward; rows
    without a gradient exactly zero over a NaN-seeded allocator; two identical steady-state calls give identical images."""
    from collab_splats_amd import ops
    N = 2_600_000
    args = _bench_like_scene(dev, N, 640, 360, seed=21, scale_mul=0.6)
    ref_img, ref_grad, _ = _fwd_bwd(args, FUSED_NODE=False)
    before = dict(ops.PATH_STATS)
    leaves = [t.clone().requires_grad_(True) for t in args[:5]]
    imgs = []
    for rep in range(3):
        poison = [torch.full((N * 48 + 64 * k,), float("nan"), device=dev) for k in range(2)]
        poison += [torch.full((N * 16,), float("nan"), device=dev) for k in range(2)]
        del poison
        img, grad, meta = _fwd_bwd(args, leaves)
        imgs.append(img)
        for a, b in zip(img, ref_img):
            assert torch.equal(a, b), rep
        for k, (a, b) in enumerate(zip(grad, ref_grad)):
            assert torch.isfinite(a).all(), (rep, k)
            assert rel_err(a, b) < 2e-5, (rep, k, rel_err(a, b))
            dead = b.reshape(b.shape[0], -1).abs().sum(1) == 0
            assert bool(dead.any()) and float(a.reshape(a.shape[0], -1)[dead].abs().sum()) == 0.0, (rep, k)
    took = {k: v - before.get(k, 0) for k, v in ops.PATH_STATS.items()}
    assert took.get("backward_background_fill", 0) == 3 and took.get("forward_view_order", 0) == 3, took
    assert took.get("forward_lazy_colour", 0) >= 2 and took.get("forward_rows_on_touch", 0) == took["forward_lazy_colour"], took
    keys = meta["isect_ids"]
    assert bool((keys[1:] >= keys[:-1]).all()) and meta["n_isects"] == int(meta["tiles_per_gauss"].sum())


def test_rows_cleared_on_first_touch_are_refilled_for_a_backward_that_reads_every_row(dev):
    """A forward that cleared the packed gradient rows only where it set a colour (on-demand colours, >= 262 144
    Gaussians), followed by a backward that is NOT the flagged-rows one: a loss on ``meta["means2d"]`` sends the call down
    the stage-by-stage backward, whose per-Gaussian kernels read every visible row -- the rows are then cleared as a
    whole first (the allocator is seeded with NaNs).  Gradients equal those of the same loss with the scheme switched off."""
    from collab_splats_amd import ops, rasterization
    args = _bench_like_scene(dev, 300_000, 640, 360, seed=9, scale_mul=1.5)
    kw = dict(sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True)

    def run(on_touch):
        old = ops.ROWS_ON_TOUCH
        ops.ROWS_ON_TOUCH = on_touch
        try:
            res = None
            for rep in range(3):                               # (on-demand colours start once the capacity hint says "dense")
                poison = [torch.full((300_000 * 16,), float("nan"), device=dev) for k in range(3)]
                del poison
                leaves = [t.clone().requires_grad_(True) for t in args[:5]]
                out = rasterization(*leaves, *args[5:], **kw)
                ups = [u.to(dev) for u in upstream([t.shape for t in out[:5]], dtype=torch.float32)]
                loss = sum((o * u).sum() for o, u in zip(out[:5], ups)) + (out[5]["means2d"] * 1e-3).sum()
                loss.backward()
                torch.cuda.synchronize()
                res = [l.grad.clone() for l in leaves]
            return res
        finally:
            ops.ROWS_ON_TOUCH = old

    before = dict(ops.PATH_STATS)
    got = run(True)
    took = {k: v - before.get(k, 0) for k, v in ops.PATH_STATS.items()}
    assert took.get("forward_rows_on_touch", 0) >= 1 and took.get("backward_rows_refilled", 0) == took["forward_rows_on_touch"], took
    ref = run(False)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert torch.isfinite(a).all(), k
        assert rel_err(a, b) < 2e-5, (k, rel_err(a, b))


@pytest.mark.parametrize("N,W,H,scale_mul,two_cams", [(30_000, 640, 360, 1.0, False), (300_000, 640, 360, 1.5, False),
                                                     (4_000, 200, 120, 1.0, True)])
def test_activations_inside_the_projection_kernels_equal_torch_activations(dev, N, W, H, scale_mul, two_cams):
    """rasterization(..., scales_are_log=True, opacities_are_logit=True): exp / sigmoid (rade_gs_model.py:443-444) run
    inside the projection kernels and the gradients come back for the raw parameters -- the same images and the same
    gradients as with torch.exp / torch.sigmoid in front (sparse and one-launch per-Gaussian backward; two cameras fall
    back to the torch activations)."""
    from collab_splats_amd import rasterization
    args = _bench_like_scene(dev, N, W, H, seed=13, scale_mul=scale_mul)
    raw = [args[0], args[1], torch.log(args[2]), torch.logit(args[3].clamp(1e-4, 1 - 1e-4)), args[4]]
    viewmats, Ks = args[5], args[6]
    if two_cams:
        viewmats, Ks = torch.cat([viewmats, viewmats]), torch.cat([Ks, Ks])
    kw = dict(sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True, absgrad=True)
    ups = None
    results = []
    for inside in (False, True, True):                          # (third run: capacity hint, graphs, on-demand colours)
        leaves = [t.clone().requires_grad_(True) for t in raw]
        if inside:
            out = rasterization(*leaves, viewmats, Ks, W, H, scales_are_log=True, opacities_are_logit=True, **kw)
        else:
            out = rasterization(leaves[0], leaves[1], torch.exp(leaves[2]), torch.sigmoid(leaves[3]), leaves[4], viewmats, Ks,
                                W, H, **kw)
        if ups is None:
            ups = [u.to(dev) for u in upstream([t.shape for t in out[:5]], dtype=torch.float32)]
        torch.autograd.backward(list(out[:5]), ups)
        torch.cuda.synchronize()
        results.append(([t.detach().clone() for t in out[:5]], [l.grad.clone() for l in leaves]))
    (ref_img, ref_grad) = results[0]
    for img, grad in results[1:]:
        for name, a, b in zip(("render", "alpha", "exp_depth", "med_depth", "normal"), img, ref_img):
            assert_close_flips(a, b, name, tol=1e-5)            # (expf in the kernel vs torch.exp: last-bit differences)
        for name, a, b in zip(("v_means", "v_quats", "v_log_scales", "v_opacity_logits", "v_sh"), grad, ref_grad):
            assert torch.isfinite(a).all(), name
            assert_close_flips(a, b, name, tol=5e-5)


@pytest.mark.parametrize("N", [30_000, 300_000])
def test_gradient_sink_with_activations_inside_the_kernels(dev, N):
    """parallel.GradientBuckets (the data-parallel path: the backward kernels write the parameters' gradients straight into
    ONE flat buffer, stage by stage so that the colour bucket's all-reduce can start early) together with raw log-scales /
    logits as inputs: every parameter is then a direct input of the rasterizer, so all five gradients land in the buffer
    without a copy, and they equal the ordinary backward's."""
    from collab_splats_amd import ops, parallel, rasterization
    W, H = 640, 360
    args = _bench_like_scene(dev, N, W, H, seed=17, scale_mul=1.5 if N > 100_000 else 1.0)
    raw = [args[0], args[1], torch.log(args[2]), torch.logit(args[3].clamp(1e-4, 1 - 1e-4)), args[4]]
    kw = dict(sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True,
              scales_are_log=True, opacities_are_logit=True)
    ups = None
    grads = []
    for sink in (False, True, True):
        leaves = [t.clone().requires_grad_(True) for t in raw]
        bucket = parallel.GradientBuckets(leaves, geometry=[0, 1, 2, 3], colour=[4]) if sink else None
        if bucket is not None:
            bucket.attach()
        try:
            out = rasterization(*leaves, args[5], args[6], W, H, **kw)
            if ups is None:
                ups = [u.to(dev) for u in upstream([t.shape for t in out[:5]], dtype=torch.float32)]
            torch.autograd.backward(list(out[:5]), ups)
        finally:
            if bucket is not None:
                bucket.allreduce()
            assert ops.GRAD_SINK is None
        if bucket is not None:
            for l, v in zip(leaves, bucket.views):
                assert l.grad.data_ptr() == v.data_ptr()                     # the gradients ARE the buffer's slices
        grads.append([l.grad.clone() for l in leaves])
    for got in grads[1:]:
        for name, a, b in zip(("v_means", "v_quats", "v_log_scales", "v_opacity_logits", "v_sh"), got, grads[0]):
            assert torch.isfinite(a).all(), name
            assert rel_err(a, b) < 2e-5, (name, rel_err(a, b))


def test_sparse_reduce_without_a_host_read_and_its_overflow_fallback(dev, monkeypatch):
    """The sparse shared-Gaussian reduce on the device (one GPU, rehearsal mode: every step of the multi-rank path except the
    collective itself): from a sink's second step on, bitmap -> union -> pack -> unpack run with a row CAPACITY from the earlier
    steps and the union's size is read only after everything has been waited for (no host read inside the step); a union
    that outgrows the capacity leaves the dense buffer untouched and is reduced densely.  In every case the gradients are
    those of a step without a sink (atomic backward: to the order of its sums)."""
    from collab_splats_amd import ops, parallel, rasterization
    monkeypatch.setattr(parallel, "REHEARSE", True)
    monkeypatch.setattr(parallel, "SPARSE", "1")
    N, W, H = 300_000, 640, 360
    args = _bench_like_scene(dev, N, W, H, seed=17, scale_mul=1.5)
    raw = [args[0], args[1], torch.log(args[2]), torch.logit(args[3].clamp(1e-4, 1 - 1e-4)), args[4]]
    kw = dict(sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True,
              scales_are_log=True, opacities_are_logit=True)
    leaves = [t.clone().requires_grad_(True) for t in raw]
    ups = None

    def step(bucket):
        nonlocal ups
        for l in leaves:
            l.grad = None
        if bucket is not None:
            bucket.attach()
        try:
            out = rasterization(*leaves, args[5], args[6], W, H, **kw)
            if ups is None:
                ups = [u.to(dev) for u in upstream([t.shape for t in out[:5]], dtype=torch.float32)]
            torch.autograd.backward(list(out[:5]), ups)
        finally:
            if bucket is not None:
                bucket.allreduce(average=False)
        return [l.grad.clone() for l in leaves]

    def same(g, ref):
        for name, a, b in zip(("v_means", "v_quats", "v_log_scales", "v_opacity_logits", "v_sh"), g, ref):
            assert torch.isfinite(a).all() and rel_err(a, b) < 2e-5, (name, rel_err(a, b))

    try:
        ref = step(None)
        bucket = parallel.GradientBuckets(leaves, geometry=[0, 1, 2, 3], colour=[4])
        stats0 = dict(parallel.STATS)
        got = [step(bucket) for _ in range(3)]
        took = {k: parallel.STATS[k] - stats0.get(k, 0) for k in parallel.STATS}
        # step 1 reads the union's size once; steps 2 and 3 run on the capacity it left
        assert took["host_reads_in_step"] == 1 and took["union_overflow"] == 0 and took["sparse"] >= 3, took
        assert bucket._row_cap is not None and bucket._row_cap < N
        for g in got:
            same(g, ref)
        bucket._row_cap = 1024                                    # far too small: the scatter must do nothing, dense fallback
        g = step(bucket)
        assert parallel.STATS["union_overflow"] - stats0.get("union_overflow", 0) >= 1 and bucket._row_cap > 1024
        same(g, ref)
        same(step(bucket), ref)                                   # and sparse again on the corrected capacity
    finally:
        assert ops.GRAD_SINK is None


@pytest.mark.timeout(900)
def test_rccl_world_of_one_runs_every_collective_of_the_gradient_buckets(dev):
    """BASELINE configs[4] / SURVEY.md section 8(e): the device branch of ``parallel.GradientBuckets`` through RCCL.  One GPU
    cannot measure scaling, but it can put every collective the N > 1 path issues through the ``nccl`` backend: a process
    group of ONE rank with ``parallel.FORCE_COLLECTIVES`` (tests/rccl_world1.py, a child process: the group is initialised
    before anything else touches the card; the child is started, not exec'd) -- uint8 bitmap all-gather, packed sparse
    all-reduce (host-sized first step, capacity-sized later steps, overflow fallback), rs_ag's reduce-scatter + all-gather,
    the dense all-reduce, the early colour launch from inside backward(), a late regulariser gradient on the geometry slices
    (advisor, round 4: such a step must go dense).  Sum over one rank = identity: results equal what was written, bit for
    bit, and the rasterizer's own no-collective gradients to the order of its atomic sums."""
    import json
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rccl_world1.py")
    r = subprocess.run([sys.executable, child, str(port)], env=env, capture_output=True, text=True, timeout=800)
    tail = (r.stdout[-3000:] + "\n---- stderr ----\n" + r.stderr[-3000:])
    assert r.returncode == 0, tail
    lines = [l for l in r.stdout.splitlines() if l.startswith("RCCL_WORLD1 ")]
    assert lines, tail
    res = json.loads(lines[-1][len("RCCL_WORLD1 "):])
    assert res["ok"] and res["backend"] == "nccl"
    assert res["rasterizer_max_rel_err_vs_no_sink"] < 2e-5
    assert all(c["stats"]["collectives"] > 0 for c in res["cases"].values())


def test_model_step_into_the_gradient_sink_goes_sparse_for_both_buckets(dev, monkeypatch):
    """configs[4] per rank: the model mirror's step (``get_outputs`` -> ``get_loss_dict`` -> backward) with its six parameters
    in a ``GradientBuckets`` sink.  The model hands the rasterizer ``opacities.squeeze(-1)`` (rade_gs_model.py:444) -- a view
    of the whole parameter: its gradient is written into the parameter's slice all the same, so EVERY slice is written in
    place and both buckets can travel as touched rows only (round 4 copied that one gradient in, which silently sent the
    geometry bucket densely: 220 MB instead of a few at 5 M).  Gradients equal those of a step without a sink."""
    from collab_splats_amd import ops, parallel, radegs
    from collab_splats_amd.synthetic import random_scene
    monkeypatch.setattr(parallel, "REHEARSE", True)
    monkeypatch.setattr(parallel, "SPARSE", "1")
    N, W, H = 300_000, 640, 360
    sc = random_scene(N, W, H, seed=23)
    cfg = radegs.RadegsModelConfig(rasterize_mode="antialiased", regularization_from_iter=0, ssim_lambda=0.2)
    model = radegs.RadegsModel(cfg, sc["means"], sc["log_scales"] + 0.405, sc["quats"], sc["opacity_logits"], sc["sh"][:, 0],
                               sc["sh"][:, 1:]).to(dev)
    model.train()
    model.step = 20000
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 0]])
    cam = radegs.PinholeCamera.make(c2w, 0.9 * W, 0.9 * W, W, H)
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    leaves = [model.gauss_params[k] for k in parallel.GRAD_KEYS]

    def step(bucket):
        if bucket is None:
            for p in leaves:
                p.grad = None
        else:
            bucket.attach()
        try:
            loss = model.get_loss_dict(model.get_outputs(cam), {"image": target})
            sum(loss.values()).backward()
        finally:
            if bucket is not None:
                bucket.allreduce()
        return [p.grad.clone() for p in leaves]

    ref = step(None)
    bucket = parallel.GradientBuckets(leaves)
    before = dict(parallel.STATS)
    for it in range(3):
        got = step(bucket)
        for name, a, b in zip(parallel.GRAD_KEYS, got, ref):
            assert torch.isfinite(a).all() and rel_err(a, b) < 2e-5, (it, name, rel_err(a, b))
        for p, v in zip(leaves, bucket.views):
            assert p.grad.data_ptr() == v.data_ptr()
    took = {k: parallel.STATS[k] - before.get(k, 0) for k in parallel.STATS}
    assert took["sparse"] == 6 and took["dense"] == 0 and took["geometry_touched_late"] == 0, took
    assert ops.GRAD_SINK is None


def test_large_scene_entirely_out_of_view_gives_zero_gradients(dev):
    """No intersection at all in a scene large enough for the background-fill path (>= 262 144 Gaussians): the compositing
    backward has no grid to carry the fill, the zeros are then written by plain fill launches -- every gradient is
    exactly zero (the allocator is seeded with NaNs first), the images are empty."""
    from collab_splats_amd import rasterization
    N, W, H = 300_000, 320, 200
    args = _bench_like_scene(dev, N, W, H, seed=3)
    viewmats = args[5].clone()
    viewmats[:, 2, 3] -= 1.0e4                                  # the whole scene behind the camera
    for rep in range(2):
        poison = [torch.full((N * 48 + 64 * k,), float("nan"), device=dev) for k in range(4)]
        del poison
        leaves = [t.clone().requires_grad_(True) for t in args[:5]]
        out = rasterization(*leaves, viewmats, args[6], W, H, sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased",
                            return_depth_normal=True, absgrad=True)
        assert int(out[5]["n_isects"]) == 0 and float(out[1].detach().abs().sum()) == 0.0
        ups = [u.to(dev) for u in upstream([t.shape for t in out[:5]], dtype=torch.float32)]
        torch.autograd.backward(list(out[:5]), ups)
        for l in leaves:
            assert l.grad is not None and float(l.grad.abs().sum()) == 0.0
        assert float(out[5]["means2d"].absgrad.abs().sum()) == 0.0


@pytest.mark.parametrize("F,rm", [(12, "RGB+ED"), (13, "RGB+ED"), (9, "RGB")])
def test_feature_records_on_demand_other_widths_and_an_empty_view(dev, monkeypatch, F, rm):
    """N-D records on demand beside the features model's own 13 channels: F = 12 with a depth channel (D' = 16, three quads,
    none of them padded), F = 9 (D' = 12: two quads -- not an on-demand width, the dense stages must serve it), and a scene
    that is entirely out of view (no intersection: the zeros of every gradient, v_features included, come from plain fills)."""
    from collab_splats_amd import ops, rasterization
    from collab_splats_amd.synthetic import random_scene
    N, W, H = 300_000, 480, 270
    sc = random_scene(N, W, H, seed=23)
    feats = torch.rand(N, F, generator=torch.Generator().manual_seed(9))
    V, K = sc["viewmats"].to(dev), sc["Ks"].to(dev)
    Dp = 3 + F + (1 if rm == "RGB+ED" else 0)
    ups = [u.to(dev) for u in upstream([(1, H, W, Dp), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)]
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setattr(ops, "LAZY_ND", mode)
        monkeypatch.setattr(ops, "LAZY_SH", "1")
        leaves = [sc[k].to(dev).requires_grad_(True) for k in ("means", "quats", "log_scales", "opacity_logits", "sh")]
        f_leaf = feats.to(dev).requires_grad_(True)
        before = dict(ops.PATH_STATS)
        for it in range(3):
            for l in leaves + [f_leaf]:
                l.grad = None
            out = rasterization(*leaves, V, K, W, H, sh_degree=3, render_mode=rm, rasterize_mode="antialiased", features=f_leaf,
                                return_depth_normal=True, scales_are_log=True, opacities_are_logit=True)
            torch.autograd.backward(list(out[:5]), ups)
        took = {k: ops.PATH_STATS[k] - before.get(k, 0) for k in ops.PATH_STATS}
        on_demand = mode == "1" and (Dp - 4 + 3) // 4 in (3, 4)
        assert took.get("forward_nd") == 3 and took.get("forward_lazy_colour", 0) == (3 if on_demand else 0), took
        res[mode] = ([t.detach().clone() for t in out[:5]], [l.grad.clone() for l in leaves + [f_leaf]])
    for a, b in zip(res["1"][0], res["0"][0]):
        assert torch.equal(a, b)
    for a, b in zip(res["1"][1], res["0"][1]):
        assert torch.isfinite(a).all() and rel_err(a, b) < 2e-5
    # nothing in view: every gradient exactly zero (the allocator is seeded with NaNs first)
    monkeypatch.setattr(ops, "LAZY_ND", "1")
    Vb = V.clone()
    Vb[:, 2, 3] -= 1.0e4
    for rep in range(2):
        poison = [torch.full((N * 48 + 64 * k,), float("nan"), device=dev) for k in range(4)]
        del poison
        leaves = [sc[k].to(dev).requires_grad_(True) for k in ("means", "quats", "log_scales", "opacity_logits", "sh")]
        f_leaf = feats.to(dev).requires_grad_(True)
        out = rasterization(*leaves, Vb, K, W, H, sh_degree=3, render_mode=rm, rasterize_mode="antialiased", features=f_leaf,
                            return_depth_normal=True, scales_are_log=True, opacities_are_logit=True)
        assert int(out[5]["n_isects"]) == 0 and float(out[0].detach().abs().sum()) == 0.0
        torch.autograd.backward(list(out[:5]), ups)
        for l in leaves + [f_leaf]:
            assert l.grad is not None and float(l.grad.abs().sum()) == 0.0


def test_two_node_form_backpropagates_a_loss_on_projection_outputs(dev, monkeypatch):
    """MISPLAT_FUSED_NODE=0: the projection's own outputs in ``meta`` are differentiable, and a loss on them reaches the
    projection backward WITHOUT passing the compositing kernels -- the `touched` row flags (set by the compositing
    backward) must not be in play there.  The gradient of a loss on the per-Gaussian normals equals the one the projection
    wrapper gives."""
    from collab_splats_amd import ops, rasterization, fully_fused_projection
    monkeypatch.setattr(ops, "FUSED_NODE", False)
    N, W, H = 20_000, 320, 200
    args = _bench_like_scene(dev, N, W, H, seed=4)
    for rep in range(2):                                       # (second call: capacity hint, merged phases, graphs)
        leaves = [t.clone().requires_grad_(True) for t in args[:5]]
        out = rasterization(*leaves, *args[5:], sh_degree=3, render_mode="RGB+ED", rasterize_mode="classic",
                            return_depth_normal=True)        # (classic: the wrapper has no anti-aliasing compensation)
        (out[5]["normals"] * out[5]["normals"].new_tensor([0.3, -0.7, 1.1])).sum().backward()
        ref = [t.clone().requires_grad_(True) for t in args[:3]]
        proj = fully_fused_projection(ref[0], None, ref[1], ref[2], args[5], args[6], W, H, opacities=args[3])
        (proj[7] * proj[7].new_tensor([0.3, -0.7, 1.1])).sum().backward()
        assert float(leaves[0].grad.abs().sum()) > 0
        assert rel_err(leaves[0].grad, ref[0].grad) < 1e-5, rep
        assert leaves[4].grad is None or float(leaves[4].grad.abs().sum()) == 0.0


def test_unit_order_is_a_permutation_sorted_by_measured_work(dev):
    """misplat_unit_order: every unit exactly once, heaviest first inside each XCD strip, padding = units."""
    from collab_splats_amd import _lib
    lib = _lib.load()
    P = _lib.make_params(10, 1, 1000, 700)                 # 63 x 44 tiles, 2 bands each: 5544 units (not a multiple of 8)
    units = P.tile_w * P.tile_h * 2
    g = torch.Generator().manual_seed(2)
    work = torch.randint(0, 3000, (units,), generator=g, dtype=torch.int32).to(dev)
    per = (units + 7) // 8
    perm = torch.full((per * 8,), -7, dtype=torch.int32, device=dev)
    _lib.check(lib.misplat_unit_order(C.byref(P), _lib.ptr(work), _lib.ptr(perm), _lib.stream_ptr()), "unit_order")
    perm = perm.cpu().numpy()
    work = work.cpu().numpy()
    real = perm[perm < units]
    assert np.array_equal(np.sort(real), np.arange(units)) and (perm[perm >= units] == units).all()
    for x in range(8):
        strip = perm[x::8]
        strip = strip[strip < units]
        assert ((strip >= x * per) & (strip < (x + 1) * per)).all()                  # strips keep their XCD
        top = max(int(work[x * per:min((x + 1) * per, units)].max()), 1)              # classes are relative to the strip's maximum
        cls = (work[strip].astype(np.float32) * np.float32(255.0 / top)).astype(np.int64)
        assert (np.diff(cls) <= 0).all()                                               # descending work classes


@pytest.mark.parametrize("case", range(24))
def test_random_configurations_vs_c_port(dev, craster, case):
    """Seeded fuzz over the keyword space the reference can reach (render mode, rasterize mode, SH degree or
    pass-through colours, ragged sizes, both gradient modes): images and every gradient
    against the fp32 C port, integer stages bit-exact."""
    from collab_splats_amd import ops, rasterization, _lib
    from collab_splats_amd.synthetic import random_scene
    rng = np.random.default_rng(1000 + case)
    W, H = int(rng.integers(17, 300)), int(rng.integers(17, 220))
    N = int(rng.integers(50, 6000))
    mode = ["classic", "antialiased"][int(rng.integers(2))]
    rm = ["RGB", "RGB+ED", "RGB+D", "ED", "D"][int(rng.integers(5))]
    deg = [None, 0, 1, 2, 3][int(rng.integers(5))]
    det = bool(rng.integers(2))
    rng.choice([1, 2, 4]), rng.choice([1, 2, 4])                             # (keeps the cases of earlier rounds: two draws less otherwise)
    sc = random_scene(N, W, H, seed=int(rng.integers(1 << 30)), sh_degree=3)
    scales, op = torch.exp(sc["log_scales"]), torch.sigmoid(sc["opacity_logits"])
    if rng.integers(3) == 0:
        scales = scales * float(rng.uniform(2.0, 6.0))                       # large footprints: many tiles per Gaussian
    colors = sc["sh"] if deg is not None else torch.sigmoid(sc["sh"][:, 0])    # [N,16,3] or [N,3]
    old_det = ops.DETERMINISTIC_BACKWARD
    try:
        ops.set_deterministic(det)
        leaves = [t.to(dev).requires_grad_(True) for t in (sc["means"], sc["quats"], scales, op, colors)]
        out = rasterization(*leaves, sc["viewmats"].to(dev), sc["Ks"].to(dev), W, H, sh_degree=deg, render_mode=rm,
                            rasterize_mode=mode, return_depth_normal=True, absgrad=True)
        r, a, ed, md, n, meta = out
        cr = craster.CRaster(np.float32)
        st = cr.forward(sc["means"].numpy(), sc["quats"].numpy(), scales.numpy(), op.numpy(), colors.numpy(),
                        sc["viewmats"][0].numpy(), sc["Ks"][0].numpy(), W, H, sh_degree=deg, render_mode=rm,
                        rasterize_mode=mode)
        tag = f"case {case}: {W}x{H} N={N} {mode} {rm} deg={deg} det={det}"
        assert np.array_equal(st["proj"]["radii"], meta["radii"][0].cpu().numpy()), tag
        assert st["bins"]["n_isects"] == meta["n_isects"], tag
        assert np.array_equal(st["bins"]["flatten_ids"], meta["flatten_ids"].cpu().numpy()), tag
        assert np.array_equal(st["bins"]["isect_offsets"], meta["isect_offsets"][0].cpu().numpy()), tag
        fw = st["fwd"]
        proof = FlipProof(cr.blend_margin(st), st["proj"]["means2d"], st["proj"]["radii"])
        for name, got, ref in (("render", r, st["render"]), ("alpha", a, fw["alpha"]), ("exp_depth", ed, fw["exp_depth"]),
                               ("med_depth", md, fw["med_depth"]), ("normal", n, fw["normal"])):
            assert_close_flips(got[0], ref, f"{tag} {name}", proof=proof)
        proof.check_ids(meta["last_ids"][0].cpu().numpy(), fw["last_ids"], meta["median_ids"][0].cpu().numpy(), fw["median_ids"],
                        max_frac=1e-2)
        ups = upstream([t.shape for t in (r, a, ed, md, n)], seed=case, dtype=torch.float32)
        meta["means2d"].retain_grad()
        torch.autograd.backward([r, a, ed, md, n], [u.to(dev) for u in ups])
        gr = cr.backward(st, *[u[0].numpy() for u in ups])
        for name, leaf in zip(("v_means", "v_quats", "v_scales", "v_opacities", "v_colors"), leaves):
            if leaf.grad is None:                                   # "D" / "ED": the colours take no part
                assert name == "v_colors" and rm in ("D", "ED") and not np.any(gr[name]), tag
                continue
            assert_close_flips(leaf.grad, gr[name], f"{tag} {name}", proof=proof)
        assert_close_flips(meta["means2d"].absgrad[0], gr["v_means2d_abs"], f"{tag} absgrad", proof=proof)
    finally:
        ops.set_deterministic(old_det)


def test_fused_get_outputs_node_matches_separate_nodes(dev):
    """The one-node a3 + a4 epilogue (ops.get_outputs_epilogue) against the two separate nodes: same outputs, same
    gradients for every input, also when only some outputs take part in the loss (absent upstream gradients)."""
    from collab_splats_amd import ops
    g = torch.Generator().manual_seed(11)
    H, W = 57, 83
    base = [torch.rand(1, H, W, 4, generator=g), torch.rand(1, H, W, 1, generator=g),
            2.0 + torch.rand(1, H, W, 1, generator=g), 2.0 + torch.rand(1, H, W, 1, generator=g),
            torch.randn(1, H, W, 3, generator=g)]
    base[1][0, :9, :11] = 0.0                                           # an empty region: where(alpha > 0, ...)
    fx, fy, bg = 70.0, 66.0, (1.0, 1.0, 1.0)

    def run(fused: bool, use):
        ins = [t.clone().to(dev).requires_grad_(True) for t in base]
        if fused:
            rgb, dep, med, nrm, err, dim = ops.get_outputs_epilogue(*ins, bg, True, fx, fy)
        else:
            _, err = ops.depth_normal(ins[2].reshape(H, W), ins[3].reshape(H, W), ins[4].reshape(H, W, 3), fx, fy)
            rgb, dep, med, nrm, dim = ops.outputs_epilogue(*ins, bg, True)
        outs = dict(rgb=rgb, dep=dep, med=med, nrm=nrm, err=err, dim=dim)
        gg = torch.Generator().manual_seed(5)
        loss = sum((outs[k] * torch.rand(outs[k].shape, generator=gg).to(dev)).sum() for k in use)
        loss.backward()
        return outs, [t.grad for t in ins]

    for use in (("rgb", "dep", "med", "nrm", "err", "dim"), ("rgb", "err"), ("err",), ("rgb",)):
        o1, g1 = run(True, use)
        o2, g2 = run(False, use)
        for k in o1:
            assert torch.allclose(o1[k], o2[k], rtol=1e-6, atol=1e-7), (use, k)
        for a, b in zip(g1, g2):
            if a is None or b is None:
                assert (a is None or not a.any()) and (b is None or not b.any()), use
            else:
                assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), use


# ---------------------------------------------------------------- the TIMED path itself against the oracle
_FULL_SIZE = FULL_SIZE


@pytest.mark.parametrize("lazy", ["1", "auto"])
@pytest.mark.parametrize("N,W,H,view,scale_mul,absgrad,opac_shift", [
    (100_000, 1920, 1080, None, 1.0, True, 0.0), (100_000, 1920, 1080, 5, 1.0, True, 0.0), (300_000, 640, 360, None, 1.5, True, 0.0),
    # without absgrad the flagged-row backward takes the SUMS form (csrc/blend.hip MSUM: the mean2d and opacity gradients are
    # finished per row by the per-Gaussian kernel) -- the bench's and the model's default; the second case shifts the opacity
    # logits up by 3 (a third of the Gaussians above alpha_max = 0.99): the trips that keep the clamp and its test
    (300_000, 640, 360, None, 1.5, False, 0.0), (300_000, 640, 360, 2, 1.5, False, 3.0),
    # (a negative shift selects rasterize_mode="classic" for the same form: no compensation factor in the opacity the row's
    #  sixth slot is divided by)
    (300_000, 640, 360, 4, 1.5, False, -0.5),
    # BASELINE configs[2] / [3] at full size: the headline workload on its heaviest rotated view, every gradient (round 4 had
    # this comparison in bench.py's post-timing leg only)
    pytest.param(1_000_000, 1920, 1080, 3, 1.0, False, 0.0, marks=_FULL_SIZE),
    # BASELINE configs[4] at full size (minus the collective): 5 M Gaussians, where front-only ordering, the 8 192-entry sort
    # class, indexed buckets and head-of-grid fills are the DEFAULT path (nothing forced here)
    pytest.param(5_000_000, 1920, 1080, None, 1.0, True, 0.0, marks=_FULL_SIZE)])
def test_steady_state_training_path_vs_c_port(dev, craster, monkeypatch, N, W, H, view, scale_mul, absgrad, opac_shift, lazy):
    _steady_state_vs_c_port(dev, craster, monkeypatch, N, W, H, view, scale_mul, absgrad, opac_shift, lazy)


@pytest.mark.parametrize("case", ["roll_translate", "combined"])
def test_steady_state_training_path_cameras_vs_c_port(dev, craster, monkeypatch, case):
    """The dense machinery -- background fill, rows cleared on touch, front-only pivots, the one-launch per-Gaussian
    backward: all from 262 144 rows on -- under a rolled, translated, anisotropic camera and under an off-centre one with
    near / far planes, ``radius_clip`` and ``alpha_max`` off their defaults (tests/camera_cases.py, scaled to 640 x 360).
    Both cameras leave a sixth to a fifth of the tiles empty and a third below FRONT_MIN_BUCKET entries, and the buckets are
    half as long as under the scene's own camera, so fewer pixels saturate before the end of their list: the share of tiles
    that front-only ordering cuts is only asked to be 5 % here -- some tiles, so that the pivots of these cameras are in use;
    front-only itself is asserted ON for all eight calls either way (152 and 112 of the 920 tiles were cut on the MI355X)."""
    import camera_cases as cc
    from collab_splats_amd import ops
    N, W, H = 300_000, 640, 360
    K, V, spec = cc.case(case, W, H)
    # the launch-order records of this tile grid are left as they were found (test_cycling_views_... counts the records of its
    # own eight views in the same table)
    mine = lambda k: k[0] == dev.index and k[2:5] == (1, (W + 15) // 16, (H + 15) // 16)
    saved = {k: (v[0].clone(), v[1].clone()) for k, v in ops._ORDER_TABLES.items() if mine(k)}
    try:
        st = _steady_state_vs_c_port(dev, craster, monkeypatch, N, W, H, None, 1.5, True, 0.0, "1", K=torch.from_numpy(K),
                                     V=torch.from_numpy(V), front_share=0.05, **spec)
    finally:
        torch.cuda.synchronize()
        for k in [k for k in ops._ORDER_TABLES if mine(k)]:
            if k in saved:
                ops._ORDER_TABLES[k][0].copy_(saved[k][0])
                ops._ORDER_TABLES[k][1].copy_(saved[k][1])
            else:
                del ops._ORDER_TABLES[k]
        ops.reset_graph_cache(dev)
    cond = cc.conditions(case, st)
    print(cond)
    assert cond["visible"] > 60_000 and cond["n_isects"] > 200_000, cond     # (half of what the C port measured: 120 593 / 423 435 for combined)
    if case == "combined":
        assert cond["outside_planes"] > 30_000 and cond["alpha_share"] >= cc.MIN_ALPHA_SHARE, cond


def _steady_state_vs_c_port(dev, craster, monkeypatch, N, W, H, view, scale_mul, absgrad, opac_shift, lazy, K=None, V=None,
                            front_share=0.5, **spec):
    """What ``bench.py --ext-activations`` and the model mirror run from their second step on -- ONE set of raw leaves
    (log-scales, logits) reused call after call with ``scales_are_log`` / ``opacities_are_logit``, both phases in one
    launch with a speculative capacity, graph replay, the previous step's launch order, on-demand SH colours, ``touched``
    row flags + background fill + the one-launch per-Gaussian backward -- compared DIRECTLY with the C restatement on the
    EIGHTH call (graphs are captured when an argument block is seen a second time and replayed from the third; the
    allocator may alternate between two or three sets of addresses, each an argument block of its own): integer
    stages bit for bit, images and the gradients of the RAW parameters within 1e-4 or a proven
    threshold flip.  The C port is given the activated values as the device computes them (expf / sigmoid: the kernels use
    the expressions of torch's own device kernels, so torch.exp / torch.sigmoid on the GPU yield the same bits); its
    gradients are chained through exp / sigmoid in numpy."""
    import math
    from collab_splats_amd import ops, rasterization
    from collab_splats_amd.synthetic import random_scene, view_matrix
    full_size = N >= 1_000_000
    if (full_size or not absgrad) and lazy != "auto":
        pytest.skip("full size / the sums form: the default switches only")
    monkeypatch.setattr(ops, "LAZY_SH", lazy)
    if 262_144 <= N < 1_000_000:
        monkeypatch.setattr(ops, "FRONT_ONLY", "1")             # ("auto" takes it from a typical bucket of 1 024 entries: 5 M Gaussians)
    assert ops.FRONT_ONLY == ("1" if 262_144 <= N < 1_000_000 else "auto")
    assert ops.GRAPHS and ops.MERGE_PHASES and ops.SPECULATE and ops.UNIT_ORDER and ops.FUSED_NODE
    assert not ops.DETERMINISTIC_BACKWARD
    sc = random_scene(N, W, H, seed=42)
    if view is not None:
        sc["viewmats"] = view_matrix(view)
    if K is not None:                                           # a camera of the caller's (and ``spec``: keywords off their defaults)
        sc["Ks"], sc["viewmats"] = K[None].contiguous(), V[None].contiguous()
    log_s = (sc["log_scales"] + math.log(scale_mul)).contiguous()
    sc["opacity_logits"] = (sc["opacity_logits"] + opac_shift).contiguous()
    mode = "classic" if opac_shift < 0 else "antialiased"
    if opac_shift > 0:
        assert 0.2 < float((torch.sigmoid(sc["opacity_logits"]) > 0.99).float().mean()) < 0.6
    leaves = [t.to(dev).requires_grad_(True) for t in (sc["means"], sc["quats"], log_s, sc["opacity_logits"], sc["sh"])]
    V, K = sc["viewmats"].to(dev), sc["Ks"].to(dev)
    cd_shapes = [(1, H, W, 4), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)]
    ups = upstream(cd_shapes, dtype=torch.float32)
    ups_dev = [u.to(dev) for u in ups]
    ops.reset_graph_cache(dev)                                  # (earlier tests' many shapes may have paused captures)
    ops._CAP_HINT.pop(ops._cap_key(ops._lib.make_params(N, 1, W, H), dev), None)
    before = dict(ops.PATH_STATS)
    out = None
    n_calls = 8
    for call in range(n_calls):
        for l in leaves:
            l.grad = None
        del out
        out = rasterization(*leaves, V, K, W, H, sh_degree=3, render_mode="RGB+ED", rasterize_mode=mode,
                            absgrad=absgrad, return_depth_normal=True, scales_are_log=True, opacities_are_logit=True, **spec)
        torch.autograd.backward(list(out[:5]), ups_dev)
    torch.cuda.synchronize()
    took = {k: ops.PATH_STATS[k] - before.get(k, 0) for k in ops.PATH_STATS}
    # ---- the machinery was ON for the call that is compared
    assert took.get("forward") == n_calls and took.get("backward_one_call") == n_calls and took.get("backward_staged", 0) == 0
    assert took.get("forward_merged_phases", 0) == n_calls and took.get("forward_probe", 0) == 1   # (a counting pass first)
    assert took.get("forward_view_order", 0) == n_calls             # the launch order comes from the record of this view
    assert took.get("capacity_redo", 0) == 0
    gs = ops.graph_cache_stats(dev)
    assert gs["hits"] >= 1 and gs["captures"] >= 1, gs
    dense = N >= 262_144
    n_lazy = took.get("forward_lazy_colour", 0)
    assert n_lazy == (n_calls if (lazy == "1" or dense) else 0), took   # "auto": a dense scene (known from the counting pass on)
    if dense:                                                   # background fill + one-launch per-Gaussian backward
        assert took.get("backward_background_fill", 0) == n_lazy, took
    r, a, ed, md, n, meta = out
    if N == 1_000_000:
        assert took.get("forward_front_only", 0) == 0, took     # (typical bucket ~800 entries: below the 1 024 of "auto")
    elif dense:
        # front-only ordering (forced on above for the small dense scene, the default at 5 M): from the first call (the
        # counting pass has left the capacity hint), with the view's own pivots from the second; meta["flatten_ids"] below is
        # completed on access
        assert took.get("forward_front_only", 0) == n_calls, took
        assert meta["_bins"]["partial"] is not None and not meta._has("flatten_ids") and "flatten_ids" in meta
        fn = meta["_bins"]["partial"]["front_n"].cpu().numpy()
        cnt = np.diff(np.concatenate([meta["isect_offsets"].reshape(-1).cpu().numpy(), [meta["n_isects"]]]))
        # (front_share: 0.5 under the scene's own camera, which fills the frame)
        assert ((fn >= 0) & (fn < cnt)).sum() > front_share * fn.size, "most tiles should have been sorted in front only"
    # ---- the C restatement on the same raw parameters
    cr = craster.CRaster(np.float32)
    scales_np = torch.exp(leaves[2].detach()).cpu().numpy()
    op_np = torch.sigmoid(leaves[3].detach()).cpu().numpy()
    st = cr.forward(sc["means"].numpy(), sc["quats"].numpy(), scales_np, op_np, sc["sh"].numpy(), sc["viewmats"][0].numpy(),
                    sc["Ks"][0].numpy(), W, H, sh_degree=3, render_mode="RGB+ED", rasterize_mode=mode, **spec)
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
                v_opacity_logits=gr["v_opacities"] * op_np * (1.0 - op_np), v_sh=gr["v_colors"])
    for (name, ref), leaf in zip(want.items(), leaves):
        assert torch.isfinite(leaf.grad).all(), name
        assert_close_flips(leaf.grad, ref, name, proof=proof)
    assert_close_flips(meta["means2d"].grad[0], gr["v_means2d"], "v_means2d", proof=proof)
    if absgrad:
        assert_close_flips(meta["means2d"].absgrad[0], gr["v_means2d_abs"], "v_means2d_abs", proof=proof)
    return st


@pytest.mark.parametrize("margin,expect_flags", [(1.05, False), (0.6, True)])
def test_front_only_ordering_is_exact_and_flags_the_tiles_it_cut_too_short(dev, craster, monkeypatch, margin, expect_flags):
    """Front-only ordering (dense scenes): only the part of every bucket in front of the depth the view's last visit reached
    is sorted.  With the default margin no tile runs out of sorted entries; with a pivot that is far too shallow
    (margin 0.6) most tiles do: they are flagged, sorted in full and composited again.  Either way the images are bitwise
    those of a run that sorts everything, the lists completed on access are the C port's bit for bit, and the gradients
    agree with the C port."""
    from collab_splats_amd import ops, rasterization
    from collab_splats_amd.synthetic import random_scene
    N, W, H = 200_000, 480, 272
    sc = random_scene(N, W, H, seed=9)
    scales, op = torch.exp(sc["log_scales"]) * 1.5, torch.sigmoid(sc["opacity_logits"])
    leaves = [t.to(dev).requires_grad_(True) for t in (sc["means"], sc["quats"], scales, op, sc["sh"])]
    V, K = sc["viewmats"].to(dev), sc["Ks"].to(dev)
    ups = upstream([(1, H, W, 4), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)
    ups_dev = [u.to(dev) for u in ups]

    def run(n_calls):
        out = None
        for _ in range(n_calls):
            for l in leaves:
                l.grad = None
            out = rasterization(*leaves, V, K, W, H, sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased",
                                return_depth_normal=True)
            torch.autograd.backward(list(out[:5]), ups_dev)
        torch.cuda.synchronize()
        return out, [l.grad.clone() for l in leaves]

    monkeypatch.setattr(ops, "FRONT_ONLY", "0")
    ops.reset_graph_cache(dev)
    ref, ref_g = run(2)
    assert ref[5]["_bins"]["partial"] is None
    ref_ids = ref[5]["flatten_ids"].clone()
    monkeypatch.setattr(ops, "FRONT_ONLY", "1")
    monkeypatch.setattr(ops, "FRONT_MARGIN", margin)
    before = ops.PATH_STATS["forward_front_only"]
    out, g = run(4)                                   # (the view's record carries pivots from its first visit on)
    assert ops.PATH_STATS["forward_front_only"] - before == 4
    part = out[5]["_bins"]["partial"]
    assert part is not None
    fn, flags = part["front_n"].cpu().numpy(), part["tile_flag"].cpu().numpy()
    cnt = np.diff(np.concatenate([out[5]["isect_offsets"].reshape(-1).cpu().numpy(), [out[5]["n_isects"]]]))
    cut = (fn >= 0) & (fn < cnt)
    assert cut.sum() > 0.3 * fn.size, (cut.sum(), fn.size)       # the scene is dense enough for the test to mean something
    assert (flags != 0).any() == expect_flags, int((flags != 0).sum())
    if expect_flags:
        assert (flags[cut] != 0).mean() > 0.2                 # a pivot at 0.6 x the reach cuts many tiles too short
    for a, b in zip(out[:5], ref[:5]):
        assert torch.equal(a, b)
    assert torch.equal(out[5]["last_ids"], ref[5]["last_ids"]) and torch.equal(out[5]["median_ids"], ref[5]["median_ids"])
    for a, b in zip(g, ref_g):
        assert rel_err(a, b) < 2e-5                           # (atomic summation order)
    # the lists, completed on access, against the full sort and the C port
    ids = out[5]["flatten_ids"]
    assert out[5]["_bins"]["partial"] is None and torch.equal(ids, ref_ids)
    cr = craster.CRaster(np.float32)
    st = cr.forward(sc["means"].numpy(), sc["quats"].numpy(), scales.numpy(), op.numpy(), sc["sh"].numpy(),
                    sc["viewmats"][0].numpy(), sc["Ks"][0].numpy(), W, H, sh_degree=3, render_mode="RGB+ED",
                    rasterize_mode="antialiased")
    assert np.array_equal(st["bins"]["flatten_ids"], ids.cpu().numpy())
    assert np.array_equal(st["bins"]["isect_ids"], out[5]["isect_ids"].cpu().numpy().view(np.uint64))
    proof = FlipProof(cr.blend_margin(st), st["proj"]["means2d"], st["proj"]["radii"])
    fw = st["fwd"]
    for name, got, want in (("render", out[0], st["render"]), ("alpha", out[1], fw["alpha"]), ("exp_depth", out[2], fw["exp_depth"]),
                            ("med_depth", out[3], fw["med_depth"]), ("normal", out[4], fw["normal"])):
        assert_close_flips(got[0], want, name, proof=proof)
    gr = cr.backward(st, *[u[0].numpy() for u in ups])
    for name, leaf in zip(("v_means", "v_quats", "v_scales", "v_opacities", "v_colors"), leaves):
        assert_close_flips(leaf.grad, gr[name], name, proof=proof)


def test_graphs_replay_while_the_scene_is_being_trained(dev):
    """What a graph key may depend on: a training loop updates its parameters IN PLACE every step, so the intersection count of
    a view changes from visit to visit -- and so did, until round 4, the backward's argument block (it carried this call's
    exact count), which therefore never replayed outside a benchmark with frozen parameters.  The backward is keyed on the
    forward's CAPACITY now (every list range comes from ``offsets``).  Eight cycling views, parameters moved a little after
    every step: from the fourth round on every forward and every backward is a replay, nothing is captured any more, and the
    gradients are those of a cold call on the same values."""
    from collab_splats_amd import ops, rasterization
    from collab_splats_amd.synthetic import random_scene, view_matrix
    N, W, H = 60_000, 640, 360
    sc = random_scene(N, W, H, seed=13)
    leaves = [sc[k].to(dev).requires_grad_(True) for k in ("means", "quats", "log_scales", "opacity_logits", "sh")]
    views = [view_matrix(v).to(dev) for v in range(8)]
    K = sc["Ks"].to(dev)
    ups = [u.to(dev) for u in upstream([(1, H, W, 4), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)]
    kw = dict(sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True,
              scales_are_log=True, opacities_are_logit=True)

    def step(v, ls):
        for l in ls:
            l.grad = None
        out = rasterization(*ls, views[v], K, W, H, **kw)
        torch.autograd.backward(list(out[:5]), ups)
        return int(out[5]["n_isects"])

    ops.reset_graph_cache(dev)
    ops._CAP_HINT.pop(ops._cap_key(ops._lib.make_params(N, 1, W, H), dev), None)
    counts = set()
    for rnd in range(5):
        if rnd == 3:
            g0 = ops.graph_cache_stats(dev)
        for v in range(8):
            n = step(v, leaves)
            if v == 0:
                counts.add(n)
            with torch.no_grad():                                     # the optimiser: a bounded in-place step
                for l in leaves:
                    l.add_(torch.sign(l.grad), alpha=-2e-3)
    g1 = ops.graph_cache_stats(dev)
    assert len(counts) >= 4, counts                                   # the count of view 0 really moved from visit to visit
    assert g1["captures"] == g0["captures"] and g1["hits"] - g0["hits"] == 32, (g0, g1)
    # and the replayed step computes what a cold call computes on the same values
    n = step(3, leaves)
    got = [l.grad.clone() for l in leaves]
    cold = [l.detach().clone().requires_grad_(True) for l in leaves]
    old = (ops.GRAPHS, ops.SPECULATE)
    try:
        ops.GRAPHS, ops.SPECULATE = False, False
        assert step(3, cold) == n
    finally:
        ops.GRAPHS, ops.SPECULATE = old
    for a, b in zip(got, cold):
        assert rel_err(a, b.grad) < 2e-5


def test_graph_cache_smaller_than_the_working_set_stops_capturing(dev, monkeypatch):
    """More resident camera tensors than the cache holds graphs for (here: 4 entries, 8 views x 2 calls): every graph is evicted
    before its block comes round again, so every capture would be wasted.  The cache counts graphs evicted without a replay and
    goes quiet (plain launches) after 32 of them; the images stay those of a cold call throughout."""
    from collab_splats_amd import ops, rasterization
    from collab_splats_amd.synthetic import random_scene, view_matrix
    N, W, H = 20_000, 320, 192
    sc = random_scene(N, W, H, seed=19)
    leaves = [sc[k].to(dev).requires_grad_(True) for k in ("means", "quats", "log_scales", "opacity_logits", "sh")]
    views = [view_matrix(v).to(dev) for v in range(8)]
    K = sc["Ks"].to(dev)
    ups = [u.to(dev) for u in upstream([(1, H, W, 4), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)]
    kw = dict(sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True,
              scales_are_log=True, opacities_are_logit=True)

    def call(v):
        for l in leaves:
            l.grad = None
        out = rasterization(*leaves, views[v], K, W, H, **kw)
        torch.autograd.backward(list(out[:5]), ups)
        return [t.detach().clone() for t in out[:5]]

    old = (ops.GRAPHS, ops.SPECULATE)
    try:
        ops.GRAPHS, ops.SPECULATE = False, False
        cold = [call(v) for v in range(8)]
    finally:
        ops.GRAPHS, ops.SPECULATE = old
    monkeypatch.setattr(ops, "GRAPH_CACHE_ENTRIES", 4)
    ops.reset_graph_cache(dev)
    try:
        marks = []
        for rnd in range(14):
            for v in range(8):
                img = call(v)
                for x, y in zip(img, cold[v]):
                    assert torch.equal(x, y), (rnd, v)
            marks.append(ops.graph_cache_stats(dev)["captures"])
        # captures stop: 32 wasted graphs after the first 4 fill the cache, then silence for 4 096 lookups
        assert marks[-1] == marks[-4] and marks[-1] <= 4 + 32 + 4, marks
    finally:
        ops.reset_graph_cache(dev)                                # (the next test gets a cache of the default size)


def test_cycling_views_reuse_graphs_without_capacity_redo(dev):
    """A training loop renders a different camera every step (rade_gs_model.py:94-95).  Eight resident view matrices
    cycled over one set of leaves with graphs, merged phases and the speculative capacity on: the decaying-maximum
    capacity hint never falls short although the views differ in their counts, and every view's images and gradients equal
    those of a cold call (no graphs, no speculation) whatever launch order and graph the call happened to get."""
    from collab_splats_amd import ops, rasterization
    from collab_splats_amd.synthetic import random_scene, view_matrix
    N, W, H = 60_000, 640, 360
    sc = random_scene(N, W, H, seed=11)
    leaves = [sc[k].to(dev).requires_grad_(True) for k in ("means", "quats", "log_scales", "opacity_logits", "sh")]
    views = [view_matrix(v).to(dev) for v in range(8)]
    K = sc["Ks"].to(dev)
    ups = [u.to(dev) for u in upstream([(1, H, W, 4), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)]
    kw = dict(sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True)

    def call(v):
        for l in leaves:
            l.grad = None
        out = rasterization(leaves[0], leaves[1], torch.exp(leaves[2]), torch.sigmoid(leaves[3]), leaves[4], views[v], K, W, H, **kw)
        torch.autograd.backward(list(out[:5]), ups)
        return [t.detach().clone() for t in out[:5]], [l.grad.clone() for l in leaves], int(out[5]["n_isects"])

    old = (ops.GRAPHS, ops.SPECULATE)
    try:
        ops.GRAPHS, ops.SPECULATE = False, False
        cold = [call(v) for v in range(8)]
    finally:
        ops.GRAPHS, ops.SPECULATE = old
    counts = [c[2] for c in cold]
    assert max(counts) > 1.05 * min(counts)                       # the views really differ in their intersection counts
    ops.reset_graph_cache(dev)
    ops._CAP_HINT.pop(ops._cap_key(ops._lib.make_params(N, 1, W, H), dev), None)
    for rnd in range(5):
        if rnd == 3:
            before, g0 = dict(ops.PATH_STATS), ops.graph_cache_stats(dev)
        for v in range(8):
            img, grad, n_is = call(v)
            assert n_is == counts[v]
            for x, y in zip(img, cold[v][0]):
                assert torch.equal(x, y), (rnd, v)
            for x, y in zip(grad, cold[v][1]):
                assert rel_err(x, y) < 2e-5, (rnd, v)
    took = {k: ops.PATH_STATS[k] - before.get(k, 0) for k in ops.PATH_STATS}
    g1 = ops.graph_cache_stats(dev)
    assert took.get("capacity_redo", 0) == 0 and took.get("forward_merged_phases", 0) == 16, took
    # Rounds 4 - 5 (the capacity hint has seen the largest view in round 1, the arena slot its final size in round 2, every
    # steady-state argument block has been sighted twice by the end of round 3): the call's own arrays come from its arena
    # slot -- the same addresses every time a view comes back --, so all 16 forwards and 16 backwards replay their graphs
    # and nothing is captured any more
    assert g1["captures"] == g0["captures"] and g1["hits"] - g0["hits"] >= 32, (g0, g1)
    assert took.get("forward_arena_slot", 0) == 16, took
    # ---- every view found its own launch order: eight valid records with eight different tags in the view-keyed table,
    # each one a permutation of the units (padding entries = units), and from the second round on the selector said "found"
    assert took.get("forward_view_order", 0) == 16, took
    tables = [v for k, v in ops._ORDER_TABLES.items() if k[3:5] == ((W + 15) // 16, (H + 15) // 16) and k[0] == torch.device(dev).index]
    assert len(tables) == 1
    table, sel, stride = tables[0]
    units = ((W + 15) // 16) * ((H + 15) // 16) * 2
    recs = table.view(-1, stride).cpu()
    valid = recs[recs[:, 2] != 0]
    assert valid.shape[0] == 8 and len({(int(r[0]), int(r[1])) for r in valid}) == 8
    for r in valid:
        perm = r[ops.ORDER_HEADER:ops.ORDER_HEADER + 8 * ((units + 7) // 8)]
        assert torch.equal(torch.sort(perm[perm < units]).values, torch.arange(units, dtype=torch.int32))
        assert int((perm == units).sum()) == perm.numel() - units
    assert int(sel.cpu()[1]) == 1


def test_arena_slots_are_not_recycled_under_tensors_that_are_still_held(dev):
    """The arrays of a call are views of a persistent arena slot (arena.py).  A caller that keeps ``meta`` (or any output)
    across later calls must still find its values there: a slot is handed out again only when nothing refers to its storage.
    Three more calls run while the first call's outputs are held; a released slot IS reused (same addresses)."""
    from collab_splats_amd import arena, ops, rasterization
    from collab_splats_amd.synthetic import random_scene
    N, W, H = 20_000, 256, 160
    sc = random_scene(N, W, H, seed=11)
    leaves = [t.to(dev).requires_grad_(True) for t in (sc["means"], sc["quats"], torch.exp(sc["log_scales"]),
                                                       torch.sigmoid(sc["opacity_logits"]), sc["sh"])]
    V, K = sc["viewmats"].to(dev), sc["Ks"].to(dev)
    kw = dict(sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True)
    ups = [u.to(dev) for u in upstream([(1, H, W, 4), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)]

    def call(scale=1.0):
        return rasterization(leaves[0] * scale, *leaves[1:], V, K, W, H, **kw)

    call(); call()                                               # (the ring learns the call's demand, then owns a slot)
    torch.cuda.synchronize()
    before = dict(arena.STATS)
    held = call()
    assert ops.PATH_STATS["forward_arena_slot"] > 0
    ptr0 = held[0].data_ptr()
    snap = [t.detach().clone() for t in held[:5]] + [held[5]["means2d"].detach().clone(), held[5]["radii"].clone(),
                                                      held[5]["flatten_ids"].clone()]
    others = []
    for k in range(3):                                           # different scenes: a recycled slot would be overwritten
        o = call(scale=1.0 + 0.05 * (k + 1))
        assert o[0].data_ptr() != ptr0
        torch.autograd.backward(list(o[:5]), ups)
        others.append(o[0].data_ptr())
        del o
    torch.cuda.synchronize()
    now = list(held[:5]) + [held[5]["means2d"], held[5]["radii"], held[5]["flatten_ids"]]
    for a, b in zip(now, snap):
        assert torch.equal(a.detach(), b)
    torch.autograd.backward(list(held[:5]), ups)                 # the held call's backward still finds its saved tensors intact
    assert all(torch.isfinite(l.grad).all() for l in leaves)
    assert others[0] == others[1] == others[2]                   # the other slot was free again each time: same addresses
    del held, now
    for l in leaves:
        l.grad = None
    again = call()
    assert again[0].data_ptr() in (ptr0, others[0])
    # (one more forward slot while the first is held, and the backward ring's first slot -- it owns one from its first call)
    assert arena.STATS["slots_created"] - before.get("slots_created", 0) <= 3


def test_plan_cache_changes_nothing_and_keeps_held_tensors_intact(dev, monkeypatch):
    """A steady-state call finds its carved views and its filled argument blocks on its arena slot (``ops._FwdPlan`` /
    ``_BwdPlan``: what a small scene's eager step spent most of its host time rebuilding).  The plan is pure plumbing: the same
    images bit for bit and the same gradients as a loop that rebuilds everything, plan hits from the third step on; and the
    plan's own references to the slot are counted EXACTLY -- a caller that keeps a single tensor of a call (here ``radii`` alone)
    keeps that slot out of circulation, its values stay what they were while other calls run."""
    from collab_splats_amd import arena, ops, rasterization
    from collab_splats_amd.synthetic import random_scene, view_matrix
    N, W, H = 20_000, 320, 192
    sc = random_scene(N, W, H, seed=13)
    leaves = [sc[k].to(dev).requires_grad_(True) for k in ("means", "quats", "log_scales", "opacity_logits", "sh")]
    views = [view_matrix(v).to(dev) for v in range(2)]
    K = sc["Ks"].to(dev)
    kw = dict(sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True, scales_are_log=True,
              opacities_are_logit=True, absgrad=True)
    ups = [u.to(dev) for u in upstream([(1, H, W, 4), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)]

    def loop(n_steps):
        res = []
        for it in range(n_steps):
            for l in leaves:
                l.grad = None
            out = rasterization(*leaves, views[it % 2], K, W, H, **kw)
            m2d = out[5]["means2d"]
            m2d.retain_grad()
            torch.autograd.backward(list(out[:5]), ups)
            res.append(([t.detach().clone() for t in out[:5]], [l.grad.clone() for l in leaves], m2d.grad.clone(), m2d.absgrad.clone(),
                        out[5]["flatten_ids"].clone()))
            del out, m2d
        torch.cuda.synchronize()
        return res

    arena.reset()
    monkeypatch.setattr(ops, "PLAN_CACHE", False)
    ref = loop(6)
    arena.reset()
    monkeypatch.setattr(ops, "PLAN_CACHE", True)
    before = dict(ops.PATH_STATS)
    got = loop(10)
    took = {k: ops.PATH_STATS[k] - before.get(k, 0) for k in ops.PATH_STATS}
    assert took.get("forward_plan_hit", 0) >= 6 and took.get("backward_plan_hit", 0) >= 6, took
    for it in (4, 5, 8, 9):
        r = ref[4 + it % 2]
        for a, b in zip(got[it][0], r[0]):
            assert torch.equal(a, b), it
        for a, b in zip(got[it][1], r[1]):
            assert rel_err(a, b) < 2e-5, it
        assert rel_err(got[it][2], r[2]) < 2e-5 and rel_err(got[it][3], r[3]) < 2e-5 and torch.equal(got[it][4], r[4])
    # ---- one tensor of a call held across later calls: the slot it lives in is not handed out again
    for l in leaves:
        l.grad = None
    out = rasterization(*leaves, views[0], K, W, H, **kw)
    held = out[5]["radii"]
    snap = held.clone()
    del out
    with torch.no_grad():
        leaves[0].add_(0.3)                                          # another scene: a recycled slot would show other radii
    later = loop(4)
    assert not torch.equal(later[-2][4], got[8][4])                  # (the scene did change)
    assert torch.equal(held, snap)
    del held
    loop(2)


def test_arena_memory_stays_bounded_while_the_scene_grows(dev):
    """densification only ever grows N, so every arena ring becomes obsolete sooner or later.  Each ring has a
    memory pool of its own that dies with it, and the memory of dropped rings goes back to the device (``arena.trim``): after
    eight growths of 20 % the memory the process holds must be what the LAST shape needs (times a constant), not the sum over
    every shape there ever was."""
    import math
    from collab_splats_amd import arena, ops, rasterization
    from collab_splats_amd.synthetic import random_scene
    W, H = 640, 360
    kw = dict(sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True,
              scales_are_log=True, opacities_are_logit=True)
    ups = [u.to(dev) for u in upstream([(1, H, W, 4), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)]
    torch.cuda.synchronize()
    arena.reset()
    torch.cuda.empty_cache()
    base_reserved = torch.cuda.memory_reserved()
    before = dict(arena.STATS)
    reserved, held = [], []
    n = 200_000
    for growth in range(9):
        sc = random_scene(n, W, H, seed=3)
        leaves = [sc[k].to(dev).requires_grad_(True) for k in ("means", "quats", "log_scales", "opacity_logits", "sh")]
        V, K = sc["viewmats"].to(dev), sc["Ks"].to(dev)
        for step in range(arena.IDLE_LOOKUPS // 2 + 8):           # (two ring lookups per step: the old shape's rings go idle)
            for l in leaves:
                l.grad = None
            out = rasterization(*leaves, V, K, W, H, **kw)
            torch.autograd.backward(list(out[:5]), ups)
            del out
        torch.cuda.synchronize()
        held.append(torch.cuda.memory_allocated())
        reserved.append(torch.cuda.memory_reserved() - base_reserved)
        del leaves
        n = int(n * 1.2)
    took = {k: arena.STATS[k] - before.get(k, 0) for k in arena.STATS}
    assert took.get("rings_dropped_idle", 0) >= 8 and took.get("trims", 0) >= 2, took   # (a trim per >= 256 MB of dropped slots)
    assert len(arena._RINGS) <= 4
    # what the first shape cost, scaled by the growth of N (x 4.3 over the run), bounds the last one -- the sum over all nine
    # shapes would be ~ 4.8 x that
    assert reserved[-1] < 1.5 * reserved[0] * (1.2 ** 8), (reserved, held)
    assert reserved[-1] < 0.45 * sum(reserved), (reserved, held)


def test_sparse_reduce_kernels_bitmaps_union_pack_unpack(dev):
    """csrc/optim.hip, the device half of the sparse shared-Gaussian reduce (parallel.GradientBuckets): flags -> bitmap,
    OR of several ranks' bitmaps -> ascending row ids, rows packed side by side and scattered back -- against numpy."""
    from collab_splats_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(3)
    for n, world in ((5, 1), (2051, 3), (1_000_003, 8)):
        flags = (rng.random((world, n)) < 0.04).astype(np.uint8) * rng.integers(1, 255, (world, n), dtype=np.uint8)
        nbytes = (n + 7) // 8
        gathered = torch.empty(world, nbytes, dtype=torch.uint8, device=dev)
        for w in range(world):
            f = torch.zeros((n + 7) // 8 * 8, dtype=torch.uint8, device=dev)         # (8-byte aligned, like the forward's carve)
            f[:n] = torch.from_numpy(flags[w]).to(dev)
            _lib.check(lib.misplat_touched_bits(_lib.ptr(f), C.c_int64(n), C.c_void_p(gathered[w].data_ptr()), _lib.stream_ptr()), "bits")
        want_bits = np.stack([np.packbits(flags[w] != 0, bitorder="little") for w in range(world)])
        assert np.array_equal(gathered.cpu().numpy(), want_bits)
        n_blocks = (nbytes + 255) // 256
        counts = torch.empty(n_blocks, dtype=torch.int32, device=dev)
        _lib.check(lib.misplat_union_count(_lib.ptr(gathered), C.c_int32(world), C.c_int64(nbytes), _lib.ptr(counts), _lib.stream_ptr()), "count")
        rows = np.flatnonzero((flags != 0).any(0))
        incl = torch.cumsum(counts, 0, dtype=torch.int64)
        assert int(incl[-1]) == rows.size
        offs_k = torch.full((n_blocks,), -1, dtype=torch.int64, device=dev)          # the library's own one-workgroup scan
        total_k = torch.full((1,), -1, dtype=torch.int64, device=dev)
        _lib.check(lib.misplat_union_scan(_lib.ptr(counts), C.c_int64(n_blocks), _lib.ptr(offs_k), _lib.ptr(total_k), _lib.stream_ptr()), "scan")
        assert torch.equal(offs_k, incl - counts) and int(total_k) == rows.size
        ids = torch.empty(max(rows.size, 1), dtype=torch.int32, device=dev)
        _lib.check(lib.misplat_union_ids(_lib.ptr(gathered), C.c_int32(world), C.c_int64(nbytes), _lib.ptr((incl - counts).contiguous()),
                                         _lib.ptr(ids), C.c_int64(ids.numel()), _lib.stream_ptr()), "ids")
        assert np.array_equal(ids[:rows.size].cpu().numpy(), rows.astype(np.int32))
        widths = [3, 45, 3, 3, 4, 1]
        tens = [torch.randn(n, w, device=dev) for w in widths]
        W = sum(widths)
        packed = torch.empty(rows.size * W, device=dev)
        ptrs = (C.c_void_p * 6)(*[t.data_ptr() for t in tens])
        wid = (C.c_int32 * 6)(*widths)
        idt = ids[:rows.size].contiguous()
        _lib.check(lib.misplat_rows_pack(C.c_int32(6), ptrs, wid, _lib.ptr(idt), C.c_int64(rows.size), None, _lib.ptr(packed), _lib.stream_ptr()), "pack")
        want = torch.cat([t[idt.long()] for t in tens], dim=1)
        assert torch.equal(packed.view(rows.size, W), want)
        # the sync-free form: buffers sized from an earlier step (larger or smaller than this union), the count on the device
        count_dev = incl[-1:].contiguous()
        for cap in (rows.size + 37, max(rows.size - 3, 0)):
            ids_c = torch.full((max(cap, 1),), -1, dtype=torch.int32, device=dev)
            _lib.check(lib.misplat_union_ids(_lib.ptr(gathered), C.c_int32(world), C.c_int64(nbytes), _lib.ptr((incl - counts).contiguous()),
                                             _lib.ptr(ids_c), C.c_int64(cap), _lib.stream_ptr()), "ids capped")
            m = min(cap, rows.size)
            assert np.array_equal(ids_c[:m].cpu().numpy(), rows[:m].astype(np.int32)) and bool((ids_c[m:cap] == -1).all())
            packed_c = torch.full((max(cap, 1) * W,), 5.0, device=dev)
            outs_c = [torch.full_like(t, 7.0) for t in tens]
            optrs_c = (C.c_void_p * 6)(*[t.data_ptr() for t in outs_c])
            if cap > 0:
                _lib.check(lib.misplat_rows_pack(C.c_int32(6), ptrs, wid, _lib.ptr(ids_c), C.c_int64(cap), _lib.ptr(count_dev), _lib.ptr(packed_c),
                                                 _lib.stream_ptr()), "pack counted")
                _lib.check(lib.misplat_rows_unpack(C.c_int32(6), optrs_c, wid, _lib.ptr(ids_c), C.c_int64(cap), _lib.ptr(count_dev),
                                                   _lib.ptr(packed_c), _lib.stream_ptr()), "unpack counted")
            if cap >= rows.size:                                   # fits: rows behind the count are zeros, the scatter is exact
                pc = packed_c[:cap * W].view(cap, W)
                assert torch.equal(pc[:rows.size], want) and bool((pc[rows.size:] == 0).all())
                for o, t in zip(outs_c, tens):
                    assert torch.equal(o[idt.long()], t[idt.long()])
            else:                                                  # too small: the scatter must not have touched anything
                for o in outs_c:
                    assert bool((o == 7.0).all())
        outs = [torch.full_like(t, 7.0) for t in tens]
        optrs = (C.c_void_p * 6)(*[t.data_ptr() for t in outs])
        _lib.check(lib.misplat_rows_unpack(C.c_int32(6), optrs, wid, _lib.ptr(idt), C.c_int64(rows.size), None, _lib.ptr(packed * 2), _lib.stream_ptr()), "unpack")
        torch.cuda.synchronize()
        keep = np.ones(n, bool)
        keep[rows] = False
        for o, t in zip(outs, tens):
            assert torch.equal(o[idt.long()], 2 * t[idt.long()]) and bool((o[torch.from_numpy(keep).to(dev)] == 7.0).all())


def test_sparse_reduce_union_scan_takes_a_second_trip(dev):
    """1 025 block counts (one per 2 048 rows): the one-workgroup scan of 1 024 counts a trip carries its sum into a second
    trip.  The same chain and the same assertions as the test above, without the packing."""
    from collab_splats_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(4)
    n, world = 1025 * 2048 - 5, 2
    flags = (rng.random((world, n)) < 0.04).astype(np.uint8)
    nbytes = (n + 7) // 8
    gathered = torch.from_numpy(np.stack([np.packbits(flags[w], bitorder="little") for w in range(world)])).to(dev)
    n_blocks = (nbytes + 255) // 256
    assert n_blocks == 1025
    counts = torch.empty(n_blocks, dtype=torch.int32, device=dev)
    _lib.check(lib.misplat_union_count(_lib.ptr(gathered), C.c_int32(world), C.c_int64(nbytes), _lib.ptr(counts), _lib.stream_ptr()), "count")
    rows = np.flatnonzero(flags.any(0))
    incl = torch.cumsum(counts, 0, dtype=torch.int64)
    assert int(incl[-1]) == rows.size and int(counts[-1]) > 0
    offs_k = torch.full((n_blocks,), -1, dtype=torch.int64, device=dev)
    total_k = torch.full((1,), -1, dtype=torch.int64, device=dev)
    _lib.check(lib.misplat_union_scan(_lib.ptr(counts), C.c_int64(n_blocks), _lib.ptr(offs_k), _lib.ptr(total_k), _lib.stream_ptr()), "scan")
    assert torch.equal(offs_k, incl - counts) and int(total_k) == rows.size
    ids = torch.empty(rows.size, dtype=torch.int32, device=dev)
    _lib.check(lib.misplat_union_ids(_lib.ptr(gathered), C.c_int32(world), C.c_int64(nbytes), _lib.ptr(offs_k), _lib.ptr(ids),
                                     C.c_int64(ids.numel()), _lib.stream_ptr()), "ids")
    assert np.array_equal(ids.cpu().numpy(), rows.astype(np.int32))


def test_memset_node_in_a_captured_sequence_is_applied_on_every_replay(dev):
    """Round 2 saw a replayed forward return "garbage + n" intersections when its captured sequence began with a 16-byte
    hipMemsetAsync of the counters, and removed every memset from the library without finding out why.  The same construct in
    miniature (memset 16 B + a kernel that adds into the counters, captured on a private non-blocking stream in thread-local
    mode, the counters overwritten with garbage between replays): on this ROCm the memset node IS applied on every replay --
    so the node itself was not what failed (DESIGN.md section 8 has the reading of the round-2 evidence).  Kept as a canary:
    if a ROCm update breaks memset nodes, a caller's whole-step capture that contains torch memsets would be affected."""
    from collab_splats_amd import _lib
    lib = _lib.load()
    counters = torch.zeros(2, dtype=torch.int64, device=dev)
    add = torch.zeros(1, dtype=torch.int64, device=dev)
    n = 12
    out = (C.c_int64 * n)()
    torch.cuda.synchronize()
    rc = lib.misplat_debug_memset_replay(_lib.ptr(counters), _lib.ptr(add), C.c_int32(n), out, _lib.stream_ptr())
    assert rc == 0
    assert list(out) == [1000 + k for k in range(n)], list(out)


def test_view_keyed_orders_survive_eviction_and_collisions(dev, monkeypatch):
    """Two slots for five views: every call evicts somebody's record.  The order is a speed hint -- the images stay
    bitwise those of a run without any launch order, the gradients equal up to the order of the atomic sums, and
    whatever the table holds is a valid permutation under its tag."""
    from collab_splats_amd import ops, rasterization
    from collab_splats_amd.synthetic import random_scene, view_matrix
    N, W, H = 30_000, 320, 208
    sc = random_scene(N, W, H, seed=3)
    leaves = [sc[k].to(dev).requires_grad_(True) for k in ("means", "quats", "log_scales", "opacity_logits", "sh")]
    views = [view_matrix(v).to(dev) for v in range(5)]
    K = sc["Ks"].to(dev)
    ups = [u.to(dev) for u in upstream([(1, H, W, 4), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)]
    kw = dict(sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True)

    def call(v):
        for l in leaves:
            l.grad = None
        out = rasterization(leaves[0], leaves[1], torch.exp(leaves[2]), torch.sigmoid(leaves[3]), leaves[4], views[v], K, W, H, **kw)
        torch.autograd.backward(list(out[:5]), ups)
        return [t.detach().clone() for t in out[:5]], [l.grad.clone() for l in leaves]

    monkeypatch.setattr(ops, "UNIT_ORDER", False)
    ref = [call(v) for v in range(5)]
    monkeypatch.setattr(ops, "UNIT_ORDER", True)
    monkeypatch.setattr(ops, "ORDER_SLOTS", 2)
    for rnd in range(3):
        for v in range(5):
            img, grad = call(v)
            for x, y in zip(img, ref[v][0]):
                assert torch.equal(x, y), (rnd, v)
            for x, y in zip(grad, ref[v][1]):
                assert rel_err(x, y) < 2e-5, (rnd, v)
    (table, sel, stride), = [v for k, v in ops._ORDER_TABLES.items() if k[-1] == 2 and k[3:5] == ((W + 15) // 16, (H + 15) // 16)]
    units = ((W + 15) // 16) * ((H + 15) // 16) * 2
    recs = table.view(-1, stride).cpu()
    assert recs.shape[0] == 2 and bool((recs[:, 2] != 0).all())
    for r in recs:
        perm = r[ops.ORDER_HEADER:ops.ORDER_HEADER + 8 * ((units + 7) // 8)]
        assert torch.equal(torch.sort(perm[perm < units]).values, torch.arange(units, dtype=torch.int32))


# ---------------------------------------------------------------- f3 / f4 on the device, against their oracles
@pytest.mark.parametrize("step", [10, 3010])
def test_strategy_on_device_matches_the_numpy_restatement_unverified_upstream(dev, step):
    """[UNVERIFIED-UPSTREAM] f3 with DEVICE tensors: ``DefaultStrategy.step_post_backward`` (clone / split / prune, the
    optimizer moments carried along) on the GPU against the independent fp64 numpy restatement of tests/test_host.py, on the
    same 12-Gaussian state: same survivors in the same order, same children, same counts, moments of the survivors kept
    and of the children zero."""
    import test_host as TH
    from collab_splats_amd.strategy import DefaultStrategy
    n = 12
    params, optimizers = TH._toy_training_state(n)
    with torch.no_grad():
        params["scales"][4:8] = float(np.log(0.05))
        params["scales"][8] = float(np.log(0.2))
        params["opacities"][10:12] = -9.0
    params = torch.nn.ParameterDict({k: torch.nn.Parameter(v.detach().to(dev)) for k, v in params.items()})
    optimizers = {k: torch.optim.Adam([params[k]], lr=1e-3) for k in params}
    for k in params:                                                      # one step so that the moments exist and differ per row
        params[k].grad = torch.arange(params[k].numel(), device=dev, dtype=torch.float32).reshape(params[k].shape) * 1e-3
        optimizers[k].step()
        params[k].grad = None
    before = {k: v.detach().double().cpu().numpy().copy() for k, v in params.items()}
    m_before = optimizers["means"].state[params["means"]]["exp_avg"].detach().cpu().clone()
    cfg = dict(grow_grad2d=0.5, grow_scale3d=0.01, prune_opa=0.005, prune_scale3d=0.1, reset_every=3000, scene_scale=1.0)
    s = DefaultStrategy(refine_start_iter=0, refine_every=10, reset_every=3000, grow_grad2d=0.5, grow_scale3d=0.01,
                        prune_opa=0.005, seed=7)
    st = s.initialize_state(scene_scale=1.0)
    grad = torch.zeros(1, n, 2)
    grad[0, [0, 1, 4, 5], 0] = 1.0
    m2d = torch.zeros(1, n, 2, device=dev, requires_grad=True)
    m2d.grad = grad.to(dev)
    info = {"means2d": m2d, "radii": torch.ones(1, n, 2, dtype=torch.int32, device=dev), "width": 2, "height": 2, "n_cameras": 1}
    noise = torch.randn(2, 2, 3, generator=s._generator(step)).double().numpy()
    avg = np.hypot(grad[0, :, 0].numpy() * 2 / 2.0, 0.0)
    want, counts = TH._np_refine(before, avg, noise, step, cfg)
    got_counts = s.step_post_backward(params, optimizers, st, step, info)
    assert tuple(got_counts) == counts
    for k in params:
        assert params[k].is_cuda and params[k].shape == want[k].shape, k
        assert np.abs(params[k].detach().double().cpu().numpy() - want[k]).max() < 1e-6, k
    # optimizer moments: survivors keep theirs (in order), children start from zero
    # (this state: rows 0, 1 are cloned, 4, 5 split, 10, 11 transparent, 8 oversized -- pruned only after the first reset)
    m_after = optimizers["means"].state[params["means"]]["exp_avg"].detach().cpu()
    kept_src = [i for i in range(n) if i not in (4, 5, 10, 11) and not (i == 8 and step > 3000)]
    assert counts == (2, 2, 2 + int(step > 3000)) and m_after.shape[0] == len(kept_src) + 2 + 4
    assert torch.equal(m_after[:len(kept_src)], m_before[kept_src])
    assert not m_after[len(kept_src):].any()


def test_eval_render_handoff_vs_oracle_post_processing(dev, craster):
    """f4 on the device (mesh.py:1568-1630): ``render_views`` maps for two rotated views against
    ``camera_oracle.outputs_post`` (the restatement of rade_gs_model.py:221-254) applied to the C port's images of the
    same views; ``tsdf_frame`` of those cameras equals the reference-generated camera goldens' convention; an ``obb_box``
    handed to ``get_outputs_for_camera`` (mesh.py:1581-1584) crops exactly as a model of the selected Gaussians renders."""
    from oracle import camera_oracle as CO
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene, view_matrix
    W, H, N = 320, 200, 12_000
    sc = random_scene(N, W, H, seed=19)
    cfg = radegs.RadegsModelConfig(rasterize_mode="antialiased")
    model = radegs.RadegsModel(cfg, sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0],
                               sc["sh"][:, 1:]).to(dev).eval()
    model.step = 10_000
    flip = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0]))
    views = (3, 6)
    cams = [radegs.PinholeCamera.make((torch.linalg.inv(view_matrix(v)[0]) @ flip)[:3, :4], 0.9 * W, 0.9 * W, W, H) for v in views]
    maps = model.render_views(cams, batch_size=2)
    cr = craster.CRaster(np.float32)
    scales_np = torch.exp(model.scales.detach()).cpu().numpy()                    # (as the device computes them)
    op_np = torch.sigmoid(model.opacities.detach().squeeze(-1)).cpu().numpy()
    for i, v in enumerate(views):
        # the model's camera parameters are rebuilt from the field of view (rade_gs_model.py:322-334): use what it used
        cp = model._get_camera_parameters(cams[i])
        Vm, Km = cp["viewmats"][0].cpu().numpy(), cp["Ks"][0].cpu().numpy()
        st = cr.forward(sc["means"].numpy(), sc["quats"].numpy(), scales_np, op_np, sc["sh"].numpy(), Vm, Km, W, H,
                        sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased")
        fw = st["fwd"]
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x))[None]
        rgb, depth, median, normals, _ = CO.outputs_post(t(st["render"]), t(fw["alpha"]), t(fw["exp_depth"]), t(fw["med_depth"]),
                                                         t(fw["normal"]), torch.zeros(3))
        proof = FlipProof(cr.blend_margin(st), st["proj"]["means2d"], st["proj"]["radii"])
        for name, got, ref in (("rgb", maps["rgb"][i], rgb[0]), ("accumulation", maps["accumulation"][i], t(fw["alpha"])[0]),
                               ("normals", maps["normals"][i], normals[0])):
            assert_close_flips(got, ref.numpy(), f"view {v} {name}", proof=proof)
        # masked depths: where(alpha > 0, x, max(x)) -- a flipped pixel may move the fill value, compare the hit pixels
        hit = fw["alpha"][..., 0] > 0
        for name, got, ref in (("depth", maps["depth"][i], fw["exp_depth"]), ("med_depth", maps["median_depth"][i], fw["med_depth"])):
            g = got.cpu().numpy()
            assert_close_flips(np.where(hit[..., None], g, 0.0), np.where(hit[..., None], ref, 0.0), f"view {v} {name}", proof=proof)
            assert np.isclose(g[~hit].max() if (~hit).any() else g.max(), ref.max(), rtol=1e-5) or (~hit).sum() == 0
        ext, intr = radegs.tsdf_frame(cams[i])
        assert np.abs(ext - view_matrix(v)[0].double().numpy()).max() < 1e-6          # OpenGL c2w -> OpenCV world-to-camera
        assert np.abs(ext - Vm.astype(np.float64)).max() < 1e-5                        # ... the matrix the rasterizer was given
        assert intr == dict(width=W, height=H, fx=0.9 * W, fy=0.9 * W, cx=W / 2.0, cy=H / 2.0)
    # golden-pinned extrinsics (reference-generated) on the device path too
    g = np.load(GOLD)
    for i in range(3):
        Wg, Hg = [int(x) for x in g[f"cam{i}_WH"]]
        Kg = g[f"cam{i}_K"]
        cam = radegs.PinholeCamera.make(torch.from_numpy(g[f"cam{i}_c2w"]), Kg[0, 0], Kg[1, 1], Wg, Hg, cx=Kg[0, 2], cy=Kg[1, 2])
        ext, _ = radegs.tsdf_frame(cam)
        assert np.abs(ext - g[f"cam{i}_viewmat"]).max() < 1e-5
        cp = radegs.camera_parameters(cam, dev)
        assert np.abs(cp["viewmats"][0].cpu().numpy() - g[f"cam{i}_viewmat"]).max() < 1e-5

    # obb_box (mesh.py:1581-1584 passes the crop box): the same maps as a model that holds only the selected Gaussians
    class Box:
        def within(self, pts):
            return (pts[:, 1] < 0.3)[:, None]

    sel = sc["means"][:, 1] < 0.3
    part = radegs.RadegsModel(cfg, sc["means"][sel], sc["log_scales"][sel], sc["quats"][sel], sc["opacity_logits"][sel],
                              sc["sh"][sel, 0], sc["sh"][sel, 1:]).to(dev).eval()
    part.step = model.step
    a, b = model.get_outputs_for_camera(cams[0], obb_box=Box()), part.get_outputs_for_camera(cams[0])
    for k in ("rgb", "depth", "median_depth", "accumulation", "normals", "depth_im"):
        assert torch.equal(a[k], b[k]), k
    model.set_crop(None)


def test_graphed_step_rejects_a_result_with_autograd_history_before_capturing(dev):
    """graphs.GraphedStep: an ``fn`` that RETURNS tensors with autograd history would keep the previous iteration's graph
    alive and take the process down inside capture_end; it must raise MisplatError during the warm-up instead."""
    from collab_splats_amd import graphs, rasterization, MisplatError
    args = _bench_like_scene(dev, 3_000, 160, 96, seed=2)
    leaves = [t.clone().requires_grad_(True) for t in args[:5]]

    def bad():
        for l in leaves:
            l.grad = None
        out = rasterization(*leaves, *args[5:], sh_degree=3, render_mode="RGB+ED", return_depth_normal=True)
        sum(o.sum() for o in out[:5]).backward()
        return out[:2]                                           # (attached to the graph of this call)

    with pytest.raises(MisplatError, match="autograd history"):
        graphs.GraphedStep(bad, capacity=400_000)
    assert not torch.cuda.is_current_stream_capturing()


def test_unit_order_survives_garbage_work_counts(dev):
    """misplat_unit_order with work counts that are negative, huge or NaN-patterned (a hint from another launch must never
    be trusted): still a permutation of every XCD strip's units plus padding, nothing written outside the buffer."""
    import ctypes as C
    from collab_splats_amd import _lib
    lib = _lib.load()
    W, H = 1920, 1080
    P = _lib.make_params(1000, 1, W, H)
    units = P.tile_w * P.tile_h * 2
    per = (units + 7) // 8
    g = torch.Generator().manual_seed(3)
    work = torch.randint(-2 ** 31, 2 ** 31 - 1, (units,), generator=g, dtype=torch.int64).to(torch.int32).to(dev)
    guard = 4096
    buf = torch.full((8 * per + 2 * guard,), -7, dtype=torch.int32, device=dev)
    perm = buf[guard:guard + 8 * per]
    _lib.check(lib.misplat_unit_order(C.byref(P), _lib.ptr(work), C.c_void_p(perm.data_ptr()), _lib.stream_ptr()),
               "misplat_unit_order")
    torch.cuda.synchronize()
    assert (buf[:guard] == -7).all() and (buf[guard + 8 * per:] == -7).all()
    p = perm.cpu().numpy().reshape(per, 8)
    for x in range(8):
        lo, hi = x * per, min((x + 1) * per, units)
        col = p[:, x]
        assert np.array_equal(np.sort(col[col < units]), np.arange(lo, hi)), x
        assert (col[col >= units] == units).all()
