"""GPU (-m gpu): ``rasterization()`` under the cameras and parameters of camera_cases.py -- off-centre and anisotropic
intrinsics, rolled / translated poses, near / far planes, ``radius_clip``, ``eps2d``, ``radius_sigma``, ``alpha_max`` --
on every path of rendering.py, against the fp32 C port called with the same keywords.  Bars as in test_parity_gpu.py:
integer / index stages bit for bit, images and gradients within 1e-4 or a proven threshold flip."""
import numpy as np
import pytest
import torch

import camera_cases as cc
from helpers import FlipProof, assert_close_flips, rel_err, upstream

pytestmark = pytest.mark.gpu
TOL = 1e-4
W, H, N, N_GROWN = 200, 120, 4000, 3000
GROWN = tuple(cc.GROWN_KS)
PATHS = ("one_node", "two_node", "deterministic", "nd_one_pass", "features_entry", "generic")
GEOM = ("means", "quats", "scales", "opacities")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from collab_splats_amd import load_library
    load_library()
    return torch.device("cuda:0")


def _scene(name):
    K, V, spec = cc.case(name, W, H)
    sc = cc.grown_frame_scene(N_GROWN, W, H, K) if name in GROWN else cc.posed_scene(N, W, H)
    return sc, K, V, spec


def _spy(monkeypatch, ops):
    """Counts the entries of ops that rendering.py chooses between: which path a call really took."""
    calls = {}
    for fn in ("raster_fused", "project_pack", "blend_packed", "project_pack_x", "blend_packed_x", "project", "blend"):
        def wrap(*a, _f=getattr(ops, fn), _n=fn, **kw):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, fn, wrap)
    return calls


_REFS = {}


def _reference(craster, key, cols, sc, V, K, mode, spec, sh_degree, geom=None, size=(W, H)):
    """C port forward + backward + margin map, computed once per ``key`` and shared (never modified)."""
    if key not in _REFS:
        cr = craster.CRaster(np.float32)
        geom = [sc[k].numpy() for k in GEOM] if geom is None else geom
        W, H = size
        st = cr.forward(*geom, cols, V, K, W, H, sh_degree=sh_degree, render_mode="RGB+ED", rasterize_mode=mode, **spec)
        Dp = st["render"].shape[-1]
        ups = upstream([(1, H, W, Dp), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)
        gr = cr.backward(st, *[u[0].numpy() for u in ups])
        _REFS[key] = (cr, st, ups, gr, cr.blend_margin(st))
    return _REFS[key]


def _assert_forward(out, st, margin, cam=0, n_cams=1, ids=True):
    """The forward half of test_full_pipeline_vs_c_port's assertions; returns the FlipProof for the gradients."""
    r, a, ed, md, n, meta = out
    assert np.array_equal(st["proj"]["radii"], meta["radii"][cam].cpu().numpy())
    assert np.array_equal(st["proj"]["depths"].view(np.uint32), meta["depths"][cam].detach().cpu().numpy().view(np.uint32))
    assert np.array_equal(st["proj"]["means2d"].view(np.uint32), meta["means2d"][cam].detach().cpu().numpy().view(np.uint32))
    assert np.array_equal(st["bins"]["tiles_per_gauss"], meta["tiles_per_gauss"][cam].cpu().numpy())
    if n_cams == 1 and ids:
        assert st["bins"]["n_isects"] == int(meta["n_isects"])
        assert np.array_equal(st["bins"]["isect_ids"], meta["isect_ids"].cpu().numpy().view(np.uint64))
        assert np.array_equal(st["bins"]["flatten_ids"], meta["flatten_ids"].cpu().numpy())
        assert np.array_equal(st["bins"]["isect_offsets"], meta["isect_offsets"][0].cpu().numpy())
    fw = st["fwd"]
    proof = FlipProof(margin, st["proj"]["means2d"], st["proj"]["radii"])
    for name, got, ref in (("render", r, st["render"]), ("alpha", a, fw["alpha"]), ("exp_depth", ed, fw["exp_depth"]),
                           ("med_depth", md, fw["med_depth"]), ("normal", n, fw["normal"])):
        assert_close_flips(got[cam], ref, name, proof=proof)
    if n_cams == 1:
        proof.check_ids(meta["last_ids"][0].cpu().numpy(), fw["last_ids"], meta["median_ids"][0].cpu().numpy(), fw["median_ids"])
    return proof


def _assert_means2d_grads(meta, gr, proof, absgrad_exact=True):
    assert_close_flips(meta["means2d"].grad[0], gr["v_means2d"], "v_means2d", proof=proof)
    got_abs = meta["means2d"].absgrad[0]
    if absgrad_exact:
        assert_close_flips(got_abs, gr["v_means2d_abs"], "v_means2d_abs", proof=proof)
    else:
        # 4-channel passes: the per-pass sum of |gradient| -- an upper bound of the C port's one-pass |sum| (see
        # test_absgrad_covers_every_channel_on_the_multi_pass_path), never below it and not wildly above
        ga, ra = got_abs.cpu().numpy().astype(np.float64), gr["v_means2d_abs"].astype(np.float64)
        assert (ga >= ra * (1 - 1e-3) - 1e-4 * ra.max()).all() and ga.sum() < 3.0 * ra.sum()


CASE_PATHS = [(n, p) for n in cc.CASES for p in PATHS] + \
             [(n, p) for n in GROWN for p in ("one_node", "two_node", "nd_one_pass", "generic")]


@pytest.mark.parametrize("name,path", CASE_PATHS, ids=[f"{n}-{p}" for n, p in CASE_PATHS])
def test_cameras_every_case_on_every_path_vs_c_port(dev, craster, monkeypatch, name, path):
    """(a) every case x every path: one forward + backward with ``absgrad``, the assertion set of
    test_full_pipeline_vs_c_port, which path was taken and that the case still exercises what it is for."""
    from collab_splats_amd import ops, rasterization
    from oracle.torch_oracle import eval_sh
    sc, K, V, spec = _scene(name)
    mode = cc.mode_of(name)
    old_det = ops.DETERMINISTIC_BACKWARD
    if path == "two_node":
        monkeypatch.setattr(ops, "FUSED_NODE", False)
    calls = _spy(monkeypatch, ops)
    g = torch.Generator().manual_seed(4)
    feats, sh_degree, chain = None, 3, None
    if path in ("nd_one_pass", "generic"):
        cols_t = torch.rand(sc["means"].shape[0], 16 if path == "nd_one_pass" else 23, generator=g)
        cols_np, sh_degree, ref_deg = cols_t.numpy(), None, None
    elif path == "features_entry":
        # the C port is fed what the reference would feed gsplat: cat(clamp_min(SH(dirs) + 0.5, 0), features), sh_degree=None
        cols_t, feats = sc["sh"].clone(), torch.rand(sc["means"].shape[0], 13, generator=g)
        cols_t[:, 0] *= 0.4                                       # (colours on both sides of the clamp at 0)
        cam_c = torch.from_numpy(-(V[:3, :3].T.astype(np.float64) @ V[:3, 3].astype(np.float64)))
        means64, sh64, feats64 = (t.double().requires_grad_(True) for t in (sc["means"], cols_t, feats))
        fused64 = torch.cat((torch.clamp_min(eval_sh(3, means64 - cam_c, sh64) + 0.5, 0.0), feats64), dim=-1)
        cols_np, ref_deg, chain = fused64.detach().float().numpy(), None, (fused64, means64, sh64, feats64)
    else:
        cols_t, cols_np, ref_deg = sc["sh"], sc["sh"].numpy(), 3
    kind = {"one_node": "sh", "two_node": "sh", "deterministic": "sh"}.get(path, path)
    cr, st, ups, gr, margin = _reference(craster, (name, kind), cols_np, sc, V, K, mode, spec, ref_deg)
    cond = cc.check_conditions(name, cc.conditions(name, st, cr))
    print(path, cond)
    leaves = [sc[k].to(dev).requires_grad_(True) for k in GEOM] + [cols_t.to(dev).requires_grad_(True)]
    f_leaf = None if feats is None else feats.to(dev).requires_grad_(True)
    before = dict(ops.PATH_STATS)
    try:
        if path == "deterministic":
            ops.set_deterministic(True)
        out = rasterization(*leaves, torch.from_numpy(V)[None].to(dev), torch.from_numpy(K)[None].to(dev), W, H,
                            sh_degree=sh_degree, render_mode="RGB+ED", rasterize_mode=mode, absgrad=True,
                            return_depth_normal=True, features=f_leaf, **spec)
        took = {k: ops.PATH_STATS[k] - before.get(k, 0) for k in ops.PATH_STATS}
        # ---- which path
        if path in ("one_node", "nd_one_pass", "features_entry"):
            assert calls.get("raster_fused") == 1 and not {"blend", "blend_packed", "blend_packed_x"} & set(calls), calls
            assert took.get("forward") == 1, took
            assert took.get("forward_nd", 0) == (0 if path == "one_node" else 1), took
        elif path in ("two_node", "deterministic"):
            assert calls.get("project_pack") == 1 and calls.get("blend_packed") == 1, calls
            assert not {"raster_fused", "blend", "blend_packed_x"} & set(calls) and took.get("forward", 0) == 0, (calls, took)
            assert ops.DETERMINISTIC_BACKWARD == (path == "deterministic") and ops.FUSED_NODE == (path == "deterministic")
        else:
            assert calls.get("project") == 1 and calls.get("blend") == 6, calls       # (24 channels: six 4-channel passes)
            assert not {"raster_fused", "blend_packed", "blend_packed_x"} & set(calls) and took.get("forward", 0) == 0, (calls, took)
        meta = out[5]
        assert out[0].shape == (1, H, W, st["render"].shape[-1])
        proof = _assert_forward(out, st, margin)
        meta["means2d"].retain_grad()
        torch.autograd.backward(list(out[:5]), [u.to(dev) for u in ups])
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(old_det)
    want = dict(v_means=gr["v_means"], v_quats=gr["v_quats"], v_scales=gr["v_scales"], v_opacities=gr["v_opacities"],
                v_colors=gr["v_colors"])
    if chain is not None:                                         # back through cat / clamp / SH in fp64
        fused64, means64, sh64, feats64 = chain
        means64.grad = sh64.grad = feats64.grad = None
        fused64.backward(torch.from_numpy(gr["v_colors"]).double(), retain_graph=True)
        want["v_means"] = gr["v_means"] + means64.grad.float().numpy()
        want["v_colors"] = sh64.grad.float().numpy()
        assert_close_flips(f_leaf.grad, feats64.grad.float().numpy(), "v_features", proof=proof)
    for (gname, ref), leaf in zip(want.items(), leaves):
        assert torch.isfinite(leaf.grad).all(), gname
        assert_close_flips(leaf.grad, ref, gname, proof=proof)
    _assert_means2d_grads(meta, gr, proof, absgrad_exact=path != "generic")
    if name in GROWN:                                              # the clamped rows are not the small ones
        assert np.abs(gr["v_means"]).max() > 0


@pytest.mark.parametrize("name", ["offcentre_pp", "near_far", "combined"])
def test_cameras_activations_inside_the_kernels_vs_c_port(dev, craster, name):
    """(b) ``scales_are_log`` / ``opacities_are_logit``: gradients of the RAW leaves, chained through exp / sigmoid as the
    steady-state test does; the C port gets the activated values as the device computes them."""
    from collab_splats_amd import ops, rasterization
    sc, K, V, spec = _scene(name)
    mode = cc.mode_of(name)
    leaves = [sc[k].to(dev).requires_grad_(True) for k in ("means", "quats", "log_scales", "opacity_logits", "sh")]
    scales_np = torch.exp(leaves[2].detach()).cpu().numpy()
    op_np = torch.sigmoid(leaves[3].detach()).cpu().numpy()
    cr, st, ups, gr, margin = _reference(craster, (name, "activations"), sc["sh"].numpy(), sc, V, K, mode, spec, 3,
                                         geom=[sc["means"].numpy(), sc["quats"].numpy(), scales_np, op_np])
    cc.check_conditions(name, cc.conditions(name, st, cr))
    before = dict(ops.PATH_STATS)
    out = rasterization(*leaves, torch.from_numpy(V)[None].to(dev), torch.from_numpy(K)[None].to(dev), W, H, sh_degree=3,
                        render_mode="RGB+ED", rasterize_mode=mode, absgrad=True, return_depth_normal=True,
                        scales_are_log=True, opacities_are_logit=True, **spec)
    assert ops.PATH_STATS["forward"] - before.get("forward", 0) == 1          # (the one node: the activations are in its kernels)
    proof = _assert_forward(out, st, margin)
    out[5]["means2d"].retain_grad()
    torch.autograd.backward(list(out[:5]), [u.to(dev) for u in ups])
    want = dict(v_means=gr["v_means"], v_quats=gr["v_quats"], v_log_scales=gr["v_scales"] * scales_np,
                v_opacity_logits=gr["v_opacities"] * op_np * (1.0 - op_np), v_sh=gr["v_colors"])
    for (gname, ref), leaf in zip(want.items(), leaves):
        assert torch.isfinite(leaf.grad).all(), gname
        assert_close_flips(leaf.grad, ref, gname, proof=proof)
    _assert_means2d_grads(out[5], gr, proof)


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
def test_cameras_two_different_cameras_in_one_call(dev, craster, det):
    """(c) two cameras with different K AND different V in one call: compositing reads the intrinsics of its own camera.
    Camera i of the pair equals the single-camera call bit for bit and the C port (keys with the camera's tile base); the
    gradient of the pair is the sum of the two single-camera gradients."""
    from collab_splats_amd import ops, rasterization
    names = ("offcentre_pp", "anisotropic_f")
    sc = cc.posed_scene(N, W, H)
    cams = [cc.case(n, W, H) for n in names]
    assert not np.array_equal(cams[0][0], cams[1][0]) and not np.array_equal(cams[0][1], cams[1][1])
    K2 = torch.from_numpy(np.stack([c[0] for c in cams])).to(dev)
    V2 = torch.from_numpy(np.stack([c[1] for c in cams])).to(dev)
    mode = "antialiased"
    old = ops.DETERMINISTIC_BACKWARD
    ops.set_deterministic(det)
    try:
        def run(Vs, Ks):
            leaves = [sc[k].to(dev).requires_grad_(True) for k in GEOM + ("sh",)]
            out = rasterization(*leaves, Vs, Ks, W, H, sh_degree=3, render_mode="RGB+ED", rasterize_mode=mode,
                                return_depth_normal=True)
            return leaves, out
        leaves2, both = run(V2, K2)
        assert both[0].shape == (2, H, W, 4) and both[5]["radii"].shape == (2, N, 2)
        ups = upstream([(2, H, W, 4), (2, H, W, 1), (2, H, W, 1), (2, H, W, 1), (2, H, W, 3)], dtype=torch.float32)
        grads1, keys, flat, n_before = [], [], [], 0
        tiles = both[5]["tile_width"] * both[5]["tile_height"]
        for ci, name in enumerate(names):
            leaves1, one = run(V2[ci:ci + 1], K2[ci:ci + 1])
            for k, (t2, t1) in enumerate(zip(both[:5], one[:5])):
                assert torch.equal(t2[ci], t1[0]), (name, k)
            for key in ("radii", "means2d", "depths", "tiles_per_gauss"):
                assert torch.equal(both[5][key][ci], one[5][key][0]), (name, key)
            for key in ("last_ids", "median_ids"):               # (indices into the call's own list: compare the Gaussians)
                gids = []
                for m, c in ((both[5], ci), (one[5], 0)):
                    idx = m[key][c].long()
                    gids.append(torch.where(idx >= 0, m["flatten_ids"].long()[idx.clamp(min=0)] % N, idx))
                assert torch.equal(gids[0], gids[1]), (name, key)
            cr, st, _, _, margin = _reference(craster, (name, "sh", mode), sc["sh"].numpy(), sc, cams[ci][1], cams[ci][0], mode, {}, 3)
            cc.check_conditions(name, cc.conditions(name, st, cr))
            _assert_forward(both, st, margin, cam=ci, n_cams=2)
            _assert_forward(one, st, margin)
            bs = cr.bin_sort(st["proj"]["means2d"], st["proj"]["radii"], st["proj"]["depths"], st["P"], cam_tile_base=ci * tiles)
            keys.append(bs["isect_ids"])
            flat.append(bs["flatten_ids"] + ci * N)
            assert np.array_equal(bs["isect_offsets"] + n_before, both[5]["isect_offsets"][ci].cpu().numpy())
            n_before += st["bins"]["n_isects"]
            torch.autograd.backward(list(one[:5]), [u[ci:ci + 1].to(dev) for u in ups])
            grads1.append([l.grad.clone() for l in leaves1])
        assert int(both[5]["n_isects"]) == n_before
        assert np.array_equal(np.concatenate(keys), both[5]["isect_ids"].cpu().numpy().view(np.uint64))
        assert np.array_equal(np.concatenate(flat), both[5]["flatten_ids"].cpu().numpy())
        torch.autograd.backward(list(both[:5]), [u.to(dev) for u in ups])
        for k, leaf in enumerate(leaves2):
            assert rel_err(leaf.grad, grads1[0][k] + grads1[1][k]) < TOL, k
    finally:
        ops.set_deterministic(old)


def _variants(kind, W, H):
    """Two calls that present the same bit patterns of everything the view-keyed records and capacity hints are keyed by,
    or cameras that differ in one number only."""
    Kc, Vc, _ = cc.case("near_far", W, H)                         # the centred camera
    if kind in ("spec_near_far", "spec_near_far_dense"):
        return [(Kc, Vc, {}), (Kc, Vc, dict(near_plane=4.0, far_plane=9.0))]
    if kind == "spec_clip_alpha":
        return [(Kc, Vc, {}), (Kc, Vc, dict(radius_clip=4.0, alpha_max=0.7))]
    if kind == "cam_cy":
        K0, V0, _ = cc.case("offcentre_pp", W, H)
        K1 = K0.copy()
        K1[1, 2] -= 37.5
        return [(K0, V0, {}), (K1, V0, {})]
    K0, _, _ = cc.case("roll_translate", W, H)
    return [(K0, cc.pose(0.1, -0.1, 0.5), {}), (K0, cc.pose(0.1, -0.1, -0.5), {})]


@pytest.mark.parametrize("kind", ["spec_near_far", "spec_clip_alpha", "cam_cy", "cam_roll", "spec_near_far_dense"])
def test_cameras_records_keyed_by_camera_alone_stay_exact(dev, craster, monkeypatch, kind):
    """(d) launch orders and front-only pivots are looked up by the bits of ``viewmats`` and ``Ks``, capacity hints by the
    shape: eight forward + backward calls on ONE set of raw leaves with the steady-state switches alternate between two
    variants that share those records (or differ in one number of the camera); the seventh and the eighth call are each
    compared with the C port under their own variant.  The pivots of front-only ordering only mean something in a dense scene
    (buckets of FRONT_MIN_BUCKET entries and more): ``spec_near_far_dense`` is the smallest the suite has for them (the shape
    of test_front_only_ordering_is_exact_...).  ``capacity_redo`` is reported, not asserted: a redo is the designed
    answer to a stale hint."""
    from collab_splats_amd import ops, rasterization
    monkeypatch.setattr(ops, "LAZY_SH", "1")
    dense = kind.endswith("_dense")
    N, W, H, scale_mul = (200_000, 480, 272, 1.5) if dense else (4000, 200, 120, 4.0)
    if dense:
        monkeypatch.setattr(ops, "FRONT_ONLY", "1")
    assert ops.GRAPHS and ops.MERGE_PHASES and ops.SPECULATE and ops.UNIT_ORDER and ops.FUSED_NODE
    assert not ops.DETERMINISTIC_BACKWARD
    variants = _variants(kind, W, H)
    sc = cc.posed_scene(N, W, H, scale_mul=scale_mul)
    mode = "antialiased"
    leaves = [sc[k].to(dev).requires_grad_(True) for k in ("means", "quats", "log_scales", "opacity_logits", "sh")]
    scales_np = torch.exp(leaves[2].detach()).cpu().numpy()
    op_np = torch.sigmoid(leaves[3].detach()).cpu().numpy()
    cams = [(torch.from_numpy(V)[None].to(dev), torch.from_numpy(K)[None].to(dev)) for K, V, _ in variants]
    ups = upstream([(1, H, W, 4), (1, H, W, 1), (1, H, W, 1), (1, H, W, 1), (1, H, W, 3)], dtype=torch.float32)
    ups_dev = [u.to(dev) for u in ups]
    ops.reset_graph_cache(dev)
    ops._CAP_HINT.pop(ops._cap_key(ops._lib.make_params(N, 1, W, H), dev), None)
    before = dict(ops.PATH_STATS)
    kept = {}
    for call in range(8):
        for l in leaves:
            l.grad = None
        K, V, spec = variants[call % 2]
        Vd, Kd = cams[call % 2]
        out = rasterization(*leaves, Vd, Kd, W, H, sh_degree=3, render_mode="RGB+ED", rasterize_mode=mode, absgrad=True,
                            return_depth_normal=True, scales_are_log=True, opacities_are_logit=True, **spec)
        out[5]["means2d"].retain_grad()
        torch.autograd.backward(list(out[:5]), ups_dev)
        if call >= 6:
            torch.cuda.synchronize()
            m = out[5]
            meta = {k: (m[k].detach().clone() if torch.is_tensor(m[k]) else m[k]) for k in
                    ("radii", "depths", "means2d", "tiles_per_gauss", "n_isects", "isect_ids", "flatten_ids", "isect_offsets",
                     "last_ids", "median_ids")}
            kept[call] = ([t.detach().clone() for t in out[:5]] + [meta], [l.grad.clone() for l in leaves],
                          m["means2d"].grad.clone(), m["means2d"].absgrad.clone())
        del out
    took = {k: ops.PATH_STATS[k] - before.get(k, 0) for k in ops.PATH_STATS}
    print(kind, "capacity_redo", took.get("capacity_redo", 0), "view_order", took.get("forward_view_order", 0),
          "graph", ops.graph_cache_stats(dev))
    assert took.get("forward") == 8 and took.get("backward_one_call") == 8 and took.get("forward_lazy_colour") == 8, took
    assert took.get("forward_view_order", 0) >= 6, took           # (the records the two variants share were in use)
    assert took.get("forward_front_only", 0) >= (6 if dense else 0), took
    for call in (6, 7):
        K, V, spec = variants[call % 2]
        cr, st, _, gr, margin = _reference(craster, (kind, call % 2), sc["sh"].numpy(), sc, V, K, mode, spec, 3,
                                           geom=[sc["means"].numpy(), sc["quats"].numpy(), scales_np, op_np], size=(W, H))
        assert st["bins"]["n_isects"] >= cc.MIN_ISECTS and (st["proj"]["radii"] > 0).all(-1).sum() >= cc.MIN_VISIBLE
        outs, grads, g2d, gabs = kept[call]
        proof = _assert_forward(outs, st, margin)
        want = dict(v_means=gr["v_means"], v_quats=gr["v_quats"], v_log_scales=gr["v_scales"] * scales_np,
                    v_opacity_logits=gr["v_opacities"] * op_np * (1.0 - op_np), v_sh=gr["v_colors"])
        for (gname, ref), got in zip(want.items(), grads):
            assert torch.isfinite(got).all(), gname
            assert_close_flips(got, ref, f"call {call + 1} {gname}", proof=proof)
        assert_close_flips(g2d[0], gr["v_means2d"], "v_means2d", proof=proof)
        assert_close_flips(gabs[0], gr["v_means2d_abs"], "v_means2d_abs", proof=proof)
    # the two variants really differ: the second reference is not the first
    assert not np.array_equal(_REFS[(kind, 0)][1]["proj"]["radii"], _REFS[(kind, 1)][1]["proj"]["radii"])


# ---------------------------------------------------------------- (f) small surfaces

def test_cameras_normalised_expected_depth_vs_c_port(dev, craster):
    """``normalise_expected_depth=True``: exp_depth / max(alpha, 1e-10) of the C port's maps, gradients by its chain rule."""
    from collab_splats_amd import rasterization
    name = "roll_translate"
    sc, K, V, spec = _scene(name)
    mode = cc.mode_of(name)
    cr, st, ups, _, margin = _reference(craster, (name, "sh"), sc["sh"].numpy(), sc, V, K, mode, spec, 3)
    cc.check_conditions(name, cc.conditions(name, st, cr))
    leaves = [sc[k].to(dev).requires_grad_(True) for k in GEOM + ("sh",)]
    out = rasterization(*leaves, torch.from_numpy(V)[None].to(dev), torch.from_numpy(K)[None].to(dev), W, H, sh_degree=3,
                        render_mode="RGB+ED", rasterize_mode=mode, return_depth_normal=True, normalise_expected_depth=True)
    fw = st["fwd"]
    a = np.maximum(fw["alpha"], np.float32(1e-10))
    proof = FlipProof(margin, st["proj"]["means2d"], st["proj"]["radii"])
    for nm, got, ref in (("render", out[0], st["render"]), ("alpha", out[1], fw["alpha"]), ("exp_depth", out[2], fw["exp_depth"] / a),
                         ("med_depth", out[3], fw["med_depth"]), ("normal", out[4], fw["normal"])):
        assert_close_flips(got[0], ref, nm, proof=proof)
    assert rel_err(fw["exp_depth"] / a, fw["exp_depth"]) > 0.05       # (the division shows)
    torch.autograd.backward(list(out[:5]), [u.to(dev) for u in ups])
    u = [x[0].numpy() for x in ups]
    v_alpha = u[1] + np.where(fw["alpha"] > 1e-10, -u[2] * fw["exp_depth"] / (a * a), 0.0).astype(np.float32)
    gr = cr.backward(st, u[0], v_alpha, (u[2] / a).astype(np.float32), u[3], u[4])
    for gname, leaf in zip(("v_means", "v_quats", "v_scales", "v_opacities", "v_colors"), leaves):
        assert_close_flips(leaf.grad, gr[gname], gname, proof=proof)


def test_cameras_projection_wrapper_off_the_defaults(dev, craster):
    """``fully_fused_projection`` with near / far planes, ``radius_clip`` and ``eps2d`` off their defaults, under an
    off-centre anisotropic rolled camera, against ``CRaster.project_fwd``."""
    from collab_splats_amd import fully_fused_projection
    sc = cc.posed_scene(N, W, H)
    K, V, _ = cc.case("combined", W, H)
    kw = dict(near_plane=3.0, far_plane=10.0, radius_clip=3.0, eps2d=0.8)
    cr = craster.CRaster(np.float32)
    for aa in (False, True):
        res = fully_fused_projection(sc["means"].to(dev), None, sc["quats"].to(dev), sc["scales"].to(dev),
                                     torch.from_numpy(V)[None].to(dev), torch.from_numpy(K)[None].to(dev), W, H, packed=False,
                                     sparse_grad=False, calc_compensations=aa, **kw)
        radii, means2d, depths, conics, comps, ray_ts, ray_planes, normals = res
        P = cr.params(K, W, H, antialiased=aa, **kw)
        ref = cr.project_fwd(sc["means"].numpy(), sc["quats"].numpy(), sc["scales"].numpy(), None, V, P)
        assert np.array_equal(radii[0].cpu().numpy(), ref["radii"])
        vis = (ref["radii"] > 0).all(-1)
        P0 = cr.params(K, W, H, antialiased=aa)
        vis0 = (cr.project_fwd(sc["means"].numpy(), sc["quats"].numpy(), sc["scales"].numpy(), None, V, P0)["radii"] > 0).all(-1)
        assert 300 < vis.sum() < vis0.sum() - 300                  # the parameters cut a real share, and leave one
        assert np.array_equal(means2d[0].cpu().numpy()[vis].view(np.uint32), ref["means2d"][vis].view(np.uint32))
        assert np.array_equal(depths[0].cpu().numpy()[vis].view(np.uint32), ref["depths"][vis].view(np.uint32))
        got = dict(conics=conics, ray_ts=ray_ts, ray_planes=ray_planes, normals=normals)
        if aa:
            got["compensations"] = comps
        else:
            assert comps is None
        for key, t in got.items():
            assert rel_err(t[0].cpu().numpy()[vis], ref[key][vis]) < 1e-5, key


def test_cameras_rasterization_refuses_another_tile_size(dev):
    from collab_splats_amd import rasterization
    sc = cc.posed_scene(64, 32, 32)
    K, V, _ = cc.case("offcentre_pp", 32, 32)
    with pytest.raises(ValueError):
        rasterization(*[sc[k].to(dev) for k in GEOM + ("sh",)], torch.from_numpy(V)[None].to(dev),
                      torch.from_numpy(K)[None].to(dev), 32, 32, sh_degree=3, tile_size=8)


def test_cameras_model_outputs_under_an_anisotropic_rolled_camera(dev, craster):
    """``RadegsModel.get_outputs`` on a non-square PinholeCamera with fx != fy, an off-centre principal point and a rolled,
    translated pose, against the C port fed ``model._get_camera_parameters(cam)`` and the restated post-processing.  The model
    rebuilds K from the field of view: the principal point is centred there by design."""
    from oracle import camera_oracle as CO
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    Wm, Hm, Nm = 232, 136, 6000
    sc = random_scene(Nm, Wm, Hm, seed=19)
    cfg = radegs.RadegsModelConfig(rasterize_mode="antialiased")
    model = radegs.RadegsModel(cfg, sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0],
                               sc["sh"][:, 1:]).to(dev).eval()
    model.step = 10_000
    flip = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0]))
    Vw = torch.from_numpy(cc.pose(0.2, -0.12, 0.5, shift=(0.3, -0.2, 0.8)))
    fx, fy = 0.8 * Wm, 0.55 * Wm
    cam = radegs.PinholeCamera.make((torch.linalg.inv(Vw) @ flip)[:3, :4], fx, fy, Wm, Hm, cx=0.3 * Wm, cy=0.7 * Hm)
    with torch.no_grad():
        out = model.get_outputs(cam)
    cp = model._get_camera_parameters(cam)
    Vm, Km = cp["viewmats"][0].cpu().numpy(), cp["Ks"][0].cpu().numpy()
    assert Km[0, 2] == Wm / 2.0 and Km[1, 2] == Hm / 2.0           # by design (the reference forces it)
    assert abs(Km[0, 0] - fx) < 1e-3 * fx and abs(Km[1, 1] - fy) < 1e-3 * fy and Km[0, 0] > 1.4 * Km[1, 1]
    assert np.abs(Vm - Vw.numpy()).max() < 1e-5
    cr = craster.CRaster(np.float32)
    scales_np = torch.exp(model.scales.detach()).cpu().numpy()
    op_np = torch.sigmoid(model.opacities.detach().squeeze(-1)).cpu().numpy()
    st = cr.forward(sc["means"].numpy(), sc["quats"].numpy(), scales_np, op_np, sc["sh"].numpy(), Vm, Km, Wm, Hm,
                    sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased")
    assert st["bins"]["n_isects"] > 2000
    fw = st["fwd"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))[None]
    rgb, depth, median, normals, _ = CO.outputs_post(t(st["render"]), t(fw["alpha"]), t(fw["exp_depth"]), t(fw["med_depth"]),
                                                     t(fw["normal"]), out["background"].reshape(-1, 3)[0].cpu())
    proof = FlipProof(cr.blend_margin(st), st["proj"]["means2d"], st["proj"]["radii"])
    for nm, got, ref in (("rgb", out["rgb"], rgb[0]), ("accumulation", out["accumulation"], t(fw["alpha"])[0]),
                         ("normals", out["normals"], normals[0])):
        assert_close_flips(got, ref.numpy(), nm, proof=proof)
    hit = fw["alpha"][..., 0] > 0
    for nm, got, ref in (("depth", out["depth"], fw["exp_depth"]), ("med_depth", out["median_depth"], fw["med_depth"])):
        gnp = got.cpu().numpy()
        assert_close_flips(np.where(hit[..., None], gnp, 0.0), np.where(hit[..., None], ref, 0.0), nm, proof=proof)
