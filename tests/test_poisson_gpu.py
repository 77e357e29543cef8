"""GPU: dense-grid screened Poisson reconstruction (csrc/poisson.hip, collab_splats_amd/poisson.py) against the numpy restatement
(tests/poisson_restatement.py).  The splat's int64 grids, b and D are compared for equality; chi through fp64 residuals against
what the fp32 restatement reaches on the same scene (computed here, never taken from the code under test) and, from section 11 on,
bit for bit with the restatement in the device's own order (``cg_exact``), iteration by iteration and up to the default depth 8;
the mesh against the restatement's extraction of the GPU's own chi."""
import ctypes as C
import functools
import math

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


def _bits64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


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
    assert _bits64(info["iso"], R.mean_exact(R.sample(chi, o, hh, G, h["points"])))  # the sampler and the mean in the device's order
    C = R.to_float(h["Cq"])
    rv, rt, rc, rd = R.extract(chi, info["iso"], o, hh, G, h["W"], C)
    assert t.dtype == torch.int32 and np.array_equal(_np(t), rt) and len(rt) > 0
    assert _close(_np(v), rv) and _close(_np(c), rc) and _close(_np(d), rd)
    # The density is the sampler alone: on the GPU's own vertices it is the restatement's bits.  The vertices come out of the TSDF
    # extraction and the colour goes through a torch division, so those two stay at 1e-6.
    assert _bits(_np(d), R.sample(h["W"], o, hh, G, _np(v)))


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


# ------------------------------------------------------------------------------------------ 11 the solver, bit for bit
# The CG's every sum has a written order (csrc/wgprims.h), its products are exact and alpha, beta are rounded at one place: the
# vectors and the solver state equal ``R.cg_exact``'s after every iteration.  The references are built once per process.
@functools.lru_cache(maxsize=None)
def grids(name):
    """The restatement's grid, splat and system of a scene (no solve): any of SCENES, LARGE, SMALL."""
    if name in S.SCENES:
        return host(name)
    p, n, c, depth = S.any_scene(name)
    o, h, G = R.grid(p, depth)
    Wq, Vq, Cq = R.splat(p, n, c, o, h, G)
    W, b, D = R.system(Wq, Vq)
    return dict(points=p, normals=n, colours=c, depth=depth, o=o, h=h, G=G, Wq=Wq, Vq=Vq, Cq=Cq, W=W, b=b, D=D)


@functools.lru_cache(maxsize=None)
def linear_system(name):
    """(b, D): "dense4" / "dense5" are the dense random systems, anything else a scene's."""
    if name.startswith("dense"):
        b, D = S.dense_random_system(int(name[5:]))
        assert np.array_equal(D >= R.neighbours(b.shape[0]), np.ones_like(D, bool)) and (b != 0).all()
        return b, D
    g = grids(name)
    return g["b"], g["D"]


@functools.lru_cache(maxsize=None)
def exact(name, n_steps=None, max_iters=None):
    b, D = linear_system(name)
    return R.cg_exact(b, D, 1e-5, max_iters, n_steps)


class Solver:
    """misplat_poisson_cg_init / _iterate driven as ``poisson._solve`` drives them, with x, r, z, p, ap and the workspace kept."""

    def __init__(self, b, D, max_iters=None, tol=1e-5):
        from collab_splats_amd import poisson as P
        from collab_splats_amd._lib import check, load, ptr, stream_ptr
        self._call = (check, load(), ptr, stream_ptr)
        self.depth = int(b.shape[0]).bit_length() - 1
        self.cap = (8 << self.depth) if max_iters is None else int(max_iters)
        self.tol = float(tol)
        self.b, self.D = _t(np.ascontiguousarray(b, np.float32)), _t(np.ascontiguousarray(D, np.float32))
        self.ws = P._workspace(self.depth, 0, DEV)
        self.x, self.r, self.z, self.p = (torch.empty_like(self.b) for _ in range(4))
        self.ap = torch.zeros_like(self.b)
        check(load().misplat_poisson_cg_init(ptr(self.b), ptr(self.D), self.depth, self.cap, ptr(self.ws), C.c_int64(self.ws.numel()),
                                             ptr(self.x), ptr(self.r), ptr(self.z), ptr(self.p), stream_ptr()), "misplat_poisson_cg_init")

    def iterate(self, n):
        check, lib, ptr, stream_ptr = self._call
        check(lib.misplat_poisson_cg_iterate(ptr(self.D), self.depth, int(n), C.c_double(self.tol), self.cap, ptr(self.ws),
                                             C.c_int64(self.ws.numel()), ptr(self.x), ptr(self.r), ptr(self.z), ptr(self.p),
                                             ptr(self.ap), stream_ptr()), "misplat_poisson_cg_iterate")
        return self

    def state(self):
        return self.ws[:64].view(torch.float64).cpu().numpy().copy()

    def snapshot(self):
        """x, r, z, p, ap as uint32 bits and the eight state doubles as uint64 bits."""
        return [_np(v).view(np.uint32).copy() for v in (self.x, self.r, self.z, self.p, self.ap)] + [self.state().view(np.uint64)]


def _same_snapshot(a, b):
    return [k for k, (u, v) in enumerate(zip(a, b)) if not np.array_equal(u, v)] == []


def _differences(solver, ref):
    """What differs from a ``cg_exact`` result, by bits: [] when x, r, z, p and the eight state values are the same."""
    out = []
    for name, got, want in zip("xrzp", (solver.x, solver.r, solver.z, solver.p), ref[:4]):
        g = _np(got)
        bad = g.view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32)
        if bad.any():
            out.append((name, int(bad.sum()), np.argwhere(bad)[0].tolist(), float(np.abs(g.astype(np.float64) - want).max())))
    st = solver.state()
    for k, label in enumerate(("rz", "pAp", "rr", "bb", "alpha", "beta", "done", "iters")):
        if st[k:k + 1].view(np.uint64)[0] != np.asarray(ref[4], np.float64)[k:k + 1].view(np.uint64)[0]:
            out.append((label, float(st[k]), float(ref[4][k])))
    return out


STEP_CASES = [(name, k) for name in ("dense4", "dense5", "sphere5") for k in (1, 2, 3, 17)] + [("sphere7", 20), ("sphere8", 3)]


@pytest.mark.parametrize("name, k", STEP_CASES)
def test_cg_steps_equal_the_exact_order_restatement(name, k):
    """dense4 / dense5: no cell of b is zero, so every face, edge and corner of the stencil counts.  sphere7: 2 048 partials, two
    trips per thread of the second level; sphere8: 16 384, sixteen trips (the unrolled body twice)."""
    b, D = linear_system(name)
    ref = exact(name, k)
    assert ref[5] == k and ref[6] == 0                                             # still running: every kernel did its work k times
    s = Solver(b, D).iterate(k)
    assert _differences(s, ref) == []


@pytest.mark.parametrize("name", ["sphere4", "sphere5", "cap5", "sparse5", "sphere6"])
def test_whole_solve_equals_the_exact_order_restatement(name):
    import collab_splats_amd as m
    g = grids(name)
    ref = exact(name)
    assert ref[6] == 1
    chi, info = m.poisson_solve(_t(g["Wq"]), _t(g["Vq"]))
    assert _bits(_np(chi), ref[0])
    assert info == R.exact_info(ref[4]) and info["iterations"] == ref[5] and info["converged"] is True


def test_chunking_the_iterations_changes_nothing():
    b, D = linear_system("sphere5")
    one = Solver(b, D)
    for _ in range(17):
        one.iterate(1)
    two = Solver(b, D).iterate(16).iterate(1)
    three = Solver(b, D).iterate(17)
    assert _same_snapshot(one.snapshot(), three.snapshot()) and _same_snapshot(two.snapshot(), three.snapshot())
    assert three.state()[R.S_ITERS] == 17.0 and _differences(three, exact("sphere5", 17)) == []
    assert _np(three.ap).any() and _bits(_np(three.ap), R.apply_A32(D, exact("sphere5", 16)[3]))     # ap = A p of the last iteration


def test_check_every_changes_no_result():
    import collab_splats_amd as m
    from collab_splats_amd import poisson
    g = grids("sphere5")
    W, V = _t(g["Wq"]), _t(g["Vq"])
    ref = exact("sphere5")
    before = poisson.CHECK_EVERY
    assert before == 16
    try:
        for every in (1, 5, 16, 64):
            poisson.CHECK_EVERY = every
            chi, info = m.poisson_solve(W, V)
            assert _bits(_np(chi), ref[0]) and info == R.exact_info(ref[4]), every
            chi, info = m.poisson_solve(W, V, max_iters=10)                        # the cap is exact whatever the host's stride
            assert _bits(_np(chi), exact("sphere5", None, 10)[0]) and info == R.exact_info(exact("sphere5", None, 10)[4]), every
    finally:
        poisson.CHECK_EVERY = before


@pytest.mark.parametrize("stop", ["converged", "cap", "max_iters_0", "zero_rhs"])
def test_the_kernels_are_no_ops_after_the_stop(stop):
    b, D = linear_system("sphere5")
    cap = {"converged": None, "cap": 10, "max_iters_0": 0, "zero_rhs": None}[stop]
    if stop == "zero_rhs":
        b = np.zeros_like(b)
    ref = R.cg_exact(b, D, 1e-5, cap) if stop == "zero_rhs" else exact("sphere5", None, cap)
    s = Solver(b, D, cap)
    for _ in range(8 * 32 // 16 + 1):                                              # poisson._solve's loop, bounded by the default cap
        if s.state()[R.S_DONE] != 0:
            break
        s.iterate(16)
    assert s.state()[R.S_DONE] == {"converged": 1.0, "cap": 2.0, "max_iters_0": 2.0, "zero_rhs": 1.0}[stop] == ref[6]
    assert _differences(s, ref) == []
    before = s.snapshot()
    s.iterate(16)
    assert _same_snapshot(before, s.snapshot())
    assert _differences(s, ref) == []


# ------------------------------------------------------------------------------------------------- 12 the mean alone
MEAN_SIZES = [1, 3, 1023, 1024, 1025, (1 << 20) + 1, 9 * (1 << 20) + 5]


@pytest.mark.parametrize("wide", [False, True], ids=["offset", "wide"])
@pytest.mark.parametrize("n", MEAN_SIZES)
def test_mean_equals_the_exact_order_restatement(n, wide):
    """2^20 + 1 values are 1 025 partials (thread 0 makes a second trip), 9 2^20 + 5 are 9 217 (the unrolled body and a remainder).
    offset: normal deviates around 1000, the issue's values; they share an exponent, so every order sums them exactly and only the
    count, the ragged block and the division are tested.  wide: 60 binades, where the order shows (tests/test_poisson_host.py).
    Bound against math.fsum: as in test_poisson_host.test_exact_sums_are_within_the_path_bound_of_fsum, gamma_(d + 3) sum |v| / n with
    d = 4 + 9 + trips + 21."""
    from collab_splats_amd import poisson as P
    from collab_splats_amd._lib import check, load, ptr, stream_ptr
    x = S.mean_values(n, wide)
    ws = P._workspace(4, n, DEV)
    vals = _t(x)
    out = torch.zeros(1, dtype=torch.float64, device=DEV)
    check(load().misplat_poisson_mean(ptr(vals), C.c_int64(n), ptr(ws), C.c_int64(ws.numel()), ptr(out), stream_ptr()),
          "misplat_poisson_mean")
    got = float(out.item())
    want = R.mean_exact(x)
    x64 = x.astype(np.float64)
    d = R.sum_path_length(n, lane_adds=4) + 3
    bound = d * 2.0 ** -53 / (1 - d * 2.0 ** -53) * math.fsum(np.abs(x64)) / n
    print(n, wide, "mean", got, "restatement", want, "fsum", math.fsum(x64) / n, "bound", bound)
    assert _bits64(got, want)
    assert abs(got - math.fsum(x64) / n) <= bound


# ------------------------------------------------------------------------------------------------ 13 the sampler alone
@pytest.mark.parametrize("nch", [1, 3, 16])
@pytest.mark.parametrize("depth", [4, 6])
def test_sampler_equals_the_restatement_bit_for_bit(depth, nch):
    from collab_splats_amd import poisson as P
    G = 1 << depth
    rng = np.random.default_rng(100 * depth + nch)
    field = rng.standard_normal((nch, G, G, G)).astype(np.float32)
    # a general frame, and a dyadic one in which cell centres, faces and the last centre are exact in fp32
    frames = [(np.array([-0.3, 0.2, 0.1], np.float32), np.float32(np.float32(1.1) / np.float32(G)), False),
              (np.array([-0.25, 0.5, 0.125], np.float32), np.float32(1.0 / G), True)]
    for o, h, dyadic in frames:
        q = S.sampler_queries(o, h, G)
        g = (q - o) / h - np.float32(0.5)                                          # the queries reach every clamp, on every axis
        fl = np.floor(g)
        t = g - np.clip(fl, 0, G - 2)
        assert (fl < 0).any(0).all() and (fl > G - 2).any(0).all() and (g < -3).any(0).all() and (g > G + 1.5).any(0).all()
        assert (t < 0).any(0).all() and (t > 1).any(0).all()
        if dyadic:
            assert (t == 1).any(0).all() and ((g == fl) & (fl >= 0) & (fl <= G - 1)).all(1).sum() >= 500
        got = P._sample(_t(field), depth, o, h, _t(q))
        want = R.sample(field, o, h, G, q)
        assert got.shape == (len(q), nch) and _bits(_np(got), want)


# -------------------------------------------------------------------------------------------------- 14 the clamped splat
def _face_mass(Wq):
    return [int(np.take(Wq, k, axis=2 - a).sum()) for a in range(3) for k in (0, -1)]           # x-, x+, y-, y+, z-, z+


# (scene, scale) -> the faces that take clamped mass.  The sphere (radius 0.5 in a cube of half side 0.25 or 0.125) lies wholly
# outside the cube: all six.  The box of "extremes" spans +-1, +-0.5, +-0.25: at scale 0.5 the cube's half side is 0.5, x is beyond
# it, y is on it (f = 0.5 of the upper corner is clamped) and z is 4 or 8 cells inside: no point can reach a z face; at 0.25 all do.
CLAMPED = {("sphere", 0.5): 6, ("sphere", 0.25): 6, ("extremes", 0.5): 4, ("extremes", 0.25): 6}


@pytest.mark.parametrize("depth", [4, 5])
@pytest.mark.parametrize("name, scale", sorted(CLAMPED))
def test_clamped_splat_equals_the_restatement(name, scale, depth):
    p, n, c = S.sphere(5000, seed=6) if name == "sphere" else S.splat_edge_cases()["extremes"][:3]
    o, h, G = R.grid(p, depth, scale)
    g = (p - o) / h - np.float32(0.5)
    inside = ((g >= -0.5) & (g <= G - 0.5)).all(1)                                 # the points of the closed cube
    assert inside.sum() < 0.5 * len(p)                                             # most points lie outside the cube
    Wq = R.splat(p, n, None, o, h, G)[0]
    Win = R.splat(p[inside], n[inside], None, o, h, G)[0] if inside.any() else np.zeros_like(Wq)
    clamped = [a > b for a, b in zip(_face_mass(Wq), _face_mass(Win))]
    assert sum(clamped) == CLAMPED[name, scale] and clamped[:4] == [True] * 4      # before relying on the restatement
    _check_splat(p, n, c, depth, scale)


# ------------------------------------------------------------------------------------------------- 15 the default depth
def _gpu_residual_ratio(name):
    """true fp64 residual / recurrence residual of the GPU's chi on a scene."""
    import collab_splats_amd as m
    g = grids(name)
    chi, info = m.poisson_solve(_t(g["Wq"]), _t(g["Vq"]))
    assert info["converged"]
    return R.true_residual(g["b"], g["D"], _np(chi)) / info["residual"], info


def test_default_depth_end_to_end():
    """depth = 8 is poisson_reconstruct's default.  The restatement cannot solve it in test time, so chi is held to the project's
    own bar one level down: true residual / recurrence residual of the GPU's chi at depths 5, 6 and 7 (where the solve equals
    cg_exact bit for bit, or step for step), 3 x the largest, the factor test_solve_reaches_what_the_fp32_restatement_reaches grants.
    Measured on the MI355X: see DESIGN.md section 20.2.  No geometric figure is asserted here: the restatement shows none at this
    depth."""
    import collab_splats_amd as m
    g = grids("sphere8")
    G = g["G"]
    assert G == 256 and m.poisson_grid(_t(g["points"]))["G"] == 256                # the default depth
    p, n, c = _t(g["points"]), _t(g["normals"]), _t(g["colours"])
    a = m.poisson_reconstruct(p, n, c, depth=8)
    info = a[4]
    assert info["converged"] is True and 0 < info["iterations"] <= 8 * G and info["residual"] <= 1e-5 and info["G"] == G
    b = m.poisson_reconstruct(p, n, c)                                             # the default, and the second run
    for x, y in zip(a[:4], b[:4]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.shape[0] > 0 and torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(info["chi"].view(torch.int32), b[4]["chi"].view(torch.int32))
    keys = ("iterations", "residual", "converged", "iso")
    assert {k: info[k] for k in keys} == {k: b[4][k] for k in keys}
    chi = _np(info["chi"])
    del a, b
    W, V, Cq = m.poisson_splat(p, n, c, depth=8)
    assert np.array_equal(_np(W), g["Wq"]) and np.array_equal(_np(V), g["Vq"]) and np.array_equal(_np(Cq), g["Cq"])
    gW, gb, gD = m.poisson_system(W, V)
    assert _bits(_np(gW), g["W"]) and _bits(_np(gb), g["b"]) and _bits(_np(gD), g["D"])
    del W, V, Cq, gW, gb, gD
    assert _bits64(info["iso"], R.mean_exact(R.sample(chi, g["o"], g["h"], G, g["points"])))
    true8 = R.true_residual(g["b"], g["D"], chi)
    ratios = {name: _gpu_residual_ratio(name)[0] for name in ("sphere5", "sphere6", "sphere7")}
    print("depth 8: iterations", info["iterations"], "recurrence residual", info["residual"], "true residual", true8, "ratio",
          true8 / info["residual"], "ratios at depth 5, 6, 7", ratios)
    assert true8 / info["residual"] <= 3 * max(ratios.values())
