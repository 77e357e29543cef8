"""GPU: dense-grid screened Poisson reconstruction (csrc/poisson.hip, collab_splats_amd/poisson.py) against the numpy restatement
(tests/poisson_restatement.py).  The splat's int64 grids, b and D are compared for equality; chi through fp64 residuals against
what the fp32 restatement reaches on the same scene (computed here, never taken from the code under test); the mesh against the
restatement's extraction of the GPU's own chi."""
import functools

import numpy as np
import pytest
import torch

import poisson_restatement as R
import poisson_scenes as S
import tsdf_scenes as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(x, dtype=None):
    if x is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _np(x):
    return None if x is None else x.cpu().numpy()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _close(a, b, rel=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and (a.size == 0 or np.abs(a - b).max() <= rel * max(np.abs(b).max(), 1e-30))


@functools.lru_cache(maxsize=None)
def host(name):
    """The restatement's whole pipeline on a scene, its fp64 solve and the two figures the GPU's chi is held to."""
    p, n, c, depth = S.scene(name)
    out = R.reconstruct(p, n, c, depth)
    x64 = R.cg(out["b"], out["D"], 1e-12, 50 * out["G"], np.float64)[0]
    out.update(points=p, normals=n, colours=c, depth=depth, chi64=x64, true32=R.true_residual(out["b"], out["D"], out["chi"]),
               err32=float(np.abs(out["chi"] - x64).max() / np.abs(x64).max()))
    return out


@functools.lru_cache(maxsize=None)
def device(name):
    import collab_splats_amd as m
    h = host(name)
    return m.poisson_reconstruct(_t(h["points"]), _t(h["normals"]), _t(h["colours"]), depth=h["depth"])


def _radial_error(v, h):
    return np.abs(np.linalg.norm(np.asarray(v, np.float64) - S.CENTRE, axis=1) - S.RADIUS) / float(h)


# ------------------------------------------------------------------------------------------------------------- 1 splat
def _check_splat(p, n, c, depth, scale):
    import collab_splats_amd as m
    o, h, G = R.grid(p, depth, scale)
    g = m.poisson_grid(_t(p), depth=depth, scale=scale)
    assert _bits(g["origin"], o) and _bits(g["h"], h) and g["G"] == G
    Wq, Vq, Cq = R.splat(p, n, c, o, h, G)
    W, V, C = m.poisson_splat(_t(p), _t(n), _t(c), depth=depth, scale=scale)
    assert W.dtype == torch.int64 and np.array_equal(_np(W), Wq) and np.array_equal(_np(V), Vq)
    assert (C is None and Cq is None) or np.array_equal(_np(C), Cq)
    Wf, b, D = R.system(Wq, Vq, 1.0)
    gW, gb, gD = m.poisson_system(W, V)
    assert _bits(_np(gW), Wf) and _bits(_np(gb), b) and _bits(_np(gD), D)
    gb2, gD2 = m.poisson_system(W, V, point_weight=2.5)[1:]
    assert _bits(_np(gb2), b) and _bits(_np(gD2), R.system(Wq, Vq, 2.5)[2])


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_splat_and_system_equal_the_restatement(name):
    h = host(name)
    _check_splat(h["points"], h["normals"], h["colours"], h["depth"], 1.1)


@pytest.mark.parametrize("name", ["cell_centres", "duplicates", "extremes", "no_colours", "zero_normal"])
def test_splat_edge_cases(name):
    p, n, c, scale = S.splat_edge_cases()[name]
    _check_splat(p, n, c, 5, scale)
    _check_splat(p, n, c, 4, scale)


# ------------------------------------------------------------------------------------------------------------- 2 solve
@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_solve_reaches_what_the_fp32_restatement_reaches(name):
    """Measured on the MI355X (true residual / chi error; the restatement's own in brackets): see DESIGN.md section 20.2."""
    import collab_splats_amd as m
    h = host(name)
    W, V = _t(h["Wq"]), _t(h["Vq"])
    chi, info = m.poisson_solve(W, V)
    G = h["G"]
    assert info["converged"] is True and 0 < info["iterations"] <= 8 * G and info["residual"] <= 1e-5
    x = _np(chi)
    true_gpu = R.true_residual(h["b"], h["D"], x)
    err_gpu = float(np.abs(x - h["chi64"]).max() / np.abs(h["chi64"]).max())
    print(name, "iterations", info["iterations"], "(", h["iterations"], ") true residual", true_gpu, "(", h["true32"], ") chi error",
          err_gpu, "(", h["err32"], ")")
    assert true_gpu <= 3 * h["true32"]
    assert err_gpu <= 4 * h["err32"]
    chi2, info2 = m.poisson_solve(W, V)                                            # two runs: bitwise
    assert torch.equal(chi.view(torch.int32), chi2.view(torch.int32)) and info == info2


def test_iteration_cap_and_zero_right_hand_side():
    import collab_splats_amd as m
    h = host("sphere5")
    W, V = _t(h["Wq"]), _t(h["Vq"])
    chi, info = m.poisson_solve(W, V, max_iters=10)                                # the cap is exact although the host looks every 16
    assert info["iterations"] == 10 and info["converged"] is False and 1e-5 < info["residual"] < 1.0
    assert np.isfinite(_np(chi)).all()
    chi, info = m.poisson_solve(W, V, max_iters=0)
    assert info["iterations"] == 0 and info["converged"] is False and not _np(chi).any()
    chi, info = m.poisson_solve(W, torch.zeros_like(V))                            # b = 0: no 0 / 0
    assert info == {"iterations": 0, "residual": 0.0, "converged": True} and not _np(chi).any()
    chi, info = m.poisson_solve(W, V, tol=1e-3)
    assert info["converged"] and info["iterations"] < h["iterations"] and info["residual"] <= 1e-3


# ----------------------------------------------------------------------------------------------------- 3 iso, 4 mesh
@pytest.mark.parametrize("name", ["sphere5", "cap5", "sparse5"])
def test_iso_and_mesh_equal_the_restatement_on_the_gpus_chi(name):
    h = host(name)
    v, t, c, d, info = device(name)
    chi = _np(info["chi"])
    o, hh, G = h["o"], h["h"], h["G"]
    assert _bits(info["origin"], o) and _bits(info["h"], hh) and info["G"] == G
    iso = R.iso_value(chi, o, hh, G, h["points"])
    assert abs(info["iso"] - iso) <= 1e-6 * abs(iso)
    C = R.to_float(h["Cq"])
    rv, rt, rc, rd = R.extract(chi, info["iso"], o, hh, G, h["W"], C)
    assert t.dtype == torch.int32 and np.array_equal(_np(t), rt) and len(rt) > 0
    assert _close(_np(v), rv) and _close(_np(c), rc) and _close(_np(d), rd)


@pytest.mark.parametrize("value, iso", [(1.0, 0.0), (-1.0, 0.0), (0.25, 0.25)])
def test_extract_of_a_constant_chi_is_the_four_empty_tensors(value, iso):
    """No crossed edge (one unit at depth 4, all positive, all negative or all zero): the driver's M = 0 path."""
    from collab_splats_amd import poisson
    chi = torch.full((16, 16, 16), value, dtype=torch.float32, device=DEV)
    v, t, c, d = poisson._extract(chi, iso, 4, np.zeros(3, np.float32), np.float32(1.0), torch.ones_like(chi), None)
    assert v.shape == (0, 3) and v.dtype == torch.float32 and t.shape == (0, 3) and t.dtype == torch.int32
    assert c.shape == (0, 3) and c.dtype == torch.float32 and d.shape == (0,) and d.dtype == torch.float32
    assert all(x.device == chi.device for x in (v, t, c, d))


# ----------------------------------------------------------------------------------------------------------- 5 sphere
@pytest.mark.parametrize("name", ["sphere5", "sphere6"])
def test_sphere_end_to_end(name):
    import collab_splats_amd as m
    h = host(name)
    v, t, c, d, info = device(name)
    assert info["converged"]
    err = _radial_error(_np(v), h["h"])
    assert err.max() <= 0.5
    assert m.mesh_holes(v, t)[0].shape[0] == 0 and m.mesh_components(v, t)[1].shape[0] == 1
    st = m.mesh_edge_stats(v, t)
    assert v.shape[0] - st["n_edges"] + t.shape[0] == 2 and st["n_nonmanifold"] == 0
    sphere = 4.0 / 3.0 * np.pi * S.RADIUS ** 3
    vol = R.signed_volume(_np(v), _np(t))
    ref = R.signed_volume(h["vertices"], h["triangles"])
    print(name, "max error / h", err.max(), "volume ratio", vol / sphere, "(", ref / sphere, ")")
    assert abs(ref / sphere - 1.0) <= 0.02                                         # the restatement's own triangles meet the 2 %
    assert vol > 0 and abs(vol / sphere - 1.0) <= 0.02
    col = _np(c)
    assert np.abs(col - (0.5 + 0.5 * (_np(v) - S.CENTRE) / S.RADIUS)).max() <= 0.1  # the scene's colour field, smoothed over a cell
    assert (_np(d) > 0).all()


# -------------------------------------------------------------------------------------------------------------- 6 cap
def test_open_cap_and_its_trim():
    import collab_splats_amd as m
    h = host("cap5")
    v, t, c, d, info = device("cap5")
    err = _radial_error(_np(v), h["h"])
    assert (err > 2.0).any()                                                       # the sheet that closes the cap is there
    dn = _np(d)
    thr = 0.25 * float(np.median(dn[dn > 0]))
    tv, tt, td, (tc,), index = m.poisson_trim(v, t, d, quantile=0.0, min_density=thr, attributes=(c,))
    assert 0 < tv.shape[0] < v.shape[0] and _radial_error(_np(tv), h["h"]).max() <= 0.5
    ti = _np(tt)
    assert ti.min() == 0 and ti.max() == tv.shape[0] - 1 and len(np.unique(ti)) == tv.shape[0]
    assert (_np(td) >= thr).all() and torch.equal(tv, v[index]) and torch.equal(tc, c[index]) and torch.equal(td, d[index])


# ------------------------------------------------------------------------------------------------------------- 7 trim
def test_trim_rule_attributes_and_order():
    import collab_splats_amd as m
    v, t, c, d, info = device("sphere5")
    dn = _np(d).astype(np.float64)
    tag = torch.arange(v.shape[0], device=DEV)
    for q, md in ((0.01, None), (0.25, None), (0.0, float(np.median(dn))), (0.1, float(np.quantile(dn, 0.05)))):
        tv, tt, td, (tc, tg), index = m.poisson_trim(v, t, d, quantile=q, min_density=md, attributes=(c, tag))
        rv, rt, rd, rindex = R.trim(_np(v), _np(t), _np(d), q, md)
        assert np.array_equal(_np(index), rindex) and np.array_equal(_np(tt), rt) and tt.dtype == t.dtype
        assert _bits(_np(tv), rv) and _bits(_np(td), rd) and torch.equal(tg, index) and torch.equal(tc, c[index])
        drop = dn < np.quantile(dn, q)                                             # the reference's expression (mesh.py:817-818)
        if md is not None:
            drop |= dn < md
        assert not drop[rindex].any() and (np.diff(rindex) > 0).all()
        kept = ~drop[_np(t).astype(np.int64)].any(1)
        assert np.array_equal(rindex[_np(tt).astype(np.int64)], _np(t)[kept])      # the kept faces, in their order
    tv, tt, td, (tc,), index = m.poisson_trim(v, t, d, quantile=0.0, min_density=None, attributes=(c,))        # the identity
    assert torch.equal(tv, v) and torch.equal(tt, t) and torch.equal(td, d) and torch.equal(tc, c)
    assert torch.equal(index, torch.arange(v.shape[0], device=DEV))


# ------------------------------------------------------------------------------------------------------ 8 determinism
def test_two_runs_are_bitwise_equal():
    import collab_splats_amd as m
    h = host("cap5")
    a = device("cap5")
    b = m.poisson_reconstruct(_t(h["points"]), _t(h["normals"]), _t(h["colours"]), depth=h["depth"])
    for x, y in zip(a[:4], b[:4]):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(a[4]["chi"].view(torch.int32), b[4]["chi"].view(torch.int32))
    assert {k: a[4][k] for k in ("iterations", "residual", "converged", "iso")} == {k: b[4][k] for k in
                                                                                     ("iterations", "residual", "converged", "iso")}


# ------------------------------------------------------------------------------------------------------------ 9 model
@functools.lru_cache(maxsize=None)
def _model():
    model = T.sphere_gaussians(20000).to(DEV)
    model.eval()
    W, H = 96, 72
    _, vms, _, _ = T.sphere_views(8, 8, 8)
    K = T.intrinsics(W, H, 60.0)
    return model, [T.pinhole_camera(M, K, W, H) for M in vms]


@pytest.mark.parametrize("source", ["depth_normal", "gaussians"])
def test_model_poisson_mesh_is_the_composition_of_the_public_calls(source):
    import collab_splats_amd as m
    model, cams = _model()
    if source == "depth_normal":
        kw = dict(total_points=20000, min_accumulation=0.5, seed=1)
        cloud = model.depth_normal_points(cams, **kw)
        args = (cams,)
    else:
        kw = {}
        cloud = model.gaussian_points()
        args = (None,)
    assert cloud["points"].shape[0] > 5000
    v, t, c, d, info = m.poisson_reconstruct(cloud["points"], cloud["normals"], cloud["colors"], depth=6)
    for q in (0.01, 0.0):
        want_v, want_t, want_d, (want_c,), _ = m.poisson_trim(v, t, d, quantile=q, attributes=(c,))
        got = model.poisson_mesh(*args, source=source, depth=6, trim_quantile=q, **kw)
        assert len(got) == 4 and got[0].shape[0] > 1000 and got[1].shape[0] > 2000
        for x, y in zip(got, (want_v, want_t, want_c, want_d)):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
    lv, lt = m.filter_mesh_components(got[0], got[1], use_largest=True)[:2]       # untrimmed: its largest component is closed
    assert lt.shape[0] > 0.9 * got[1].shape[0] and m.mesh_edge_stats(lv, lt)["n_boundary"] == 0
    r = (lv.double().cpu().numpy() - np.array([0.1, -0.05, 0.2]))
    assert abs(np.median(np.linalg.norm(r, axis=1)) - 0.3) < 0.02                  # tsdf_scenes' sphere
    with pytest.raises(ValueError, match="source"):
        model.poisson_mesh(cams, source="tsdf")


# ------------------------------------------------------------------------------------------------------- 10 validation
def test_validation():
    import collab_splats_amd as m
    p, n, c = (_t(x) for x in S.sphere(100, seed=4))
    for depth in (3, 10):
        with pytest.raises(ValueError, match="depth"):
            m.poisson_reconstruct(p, n, c, depth=depth)
        with pytest.raises(ValueError, match="depth"):
            m.poisson_splat(p, n, c, depth=depth)
    with pytest.raises(ValueError, match="normals"):
        m.poisson_reconstruct(p, n[:50], c, depth=5)
    with pytest.raises(ValueError, match="colors"):
        m.poisson_reconstruct(p, n, c[:, :2], depth=5)
    with pytest.raises(m.MisplatError):
        m.poisson_reconstruct(p.cpu(), n.cpu(), depth=5)
    with pytest.raises(m.MisplatError):
        m.poisson_trim(p.cpu(), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(100))
    bad = p.clone()
    bad[7, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        m.poisson_reconstruct(bad, n, c, depth=5)
    with pytest.raises(ValueError, match="finite"):
        m.poisson_reconstruct(p, bad, c, depth=5)
    with pytest.raises(ValueError, match="extent"):
        m.poisson_reconstruct(p[:1], n[:1], c[:1], depth=5)
    with pytest.raises(ValueError, match="extent"):
        m.poisson_grid(p[:1].expand(5, 3), depth=5)
    with pytest.raises(ValueError, match="max_iters"):
        m.poisson_reconstruct(p, n, c, depth=5, max_iters=-1)
    with pytest.raises(ValueError, match="point_weight"):
        m.poisson_reconstruct(p, n, c, depth=5, point_weight=-1.0)
    v, t, col, d, info = m.poisson_reconstruct(p, n, None, depth=4)               # the smallest grid, no colours
    assert v.shape[0] > 0 and not _np(col).any() and info["G"] == 16
