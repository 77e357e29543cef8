"""CPU: the yardsticks of the level-set search and of the Laplacian smoothing (tests/levelset_restatement.py) checked against
closed forms, and the Python surface's argument errors with no GPU present."""
import numpy as np
import pytest
import torch

import density_scenes as S
import levelset_restatement as LR
import levelset_scenes as LS


# ------------------------------------------------------------------------------------------------------- the search
@pytest.mark.parametrize("name", sorted(LS.LONG))
def test_oracle_hit_counts(name):
    """The fp64 search's hits per level on the long ray sets; every set has hits and misses at every level; a ray is left out
    of the GPU comparison only if a coarse sample lies within 1e-4 of the level: at most 16 of 1024 (`random` at 0.1)."""
    O = LS.long_oracle(name)
    assert tuple(int(n) for n in O["hit"].sum(1)) == LS.HITS[name]
    assert all(0 < n < 1024 for n in LS.HITS[name])
    near = [int((np.abs(O["D"] - lev) < 1e-4).any(1).sum()) for lev in LS.LEVELS]
    print(name, "rays with a coarse sample within 1e-4 of the level:", near)
    assert max(near) <= 16 and (name == "random" or max(near) <= 3)
    assert len(LS.short_set(name)["t0"]) == LS.HITS[name][1]


def test_single_hits_the_closed_form_radius():
    """One isotropic Gaussian (s = 0.1, o = 1, cut-off r = 3): d = l on the sphere of radius rho = s sqrt(-2 ln(l / o + e^{-r^2/2}))
    (0.11586 at l = 0.5).  The search interpolates d linearly between fine samples h_f = (t1 - t0) / 63^2 apart along a unit
    direction: the interpolant errs by at most h_f^2 / 8 max |d''|, and along any direction |d''| <= o / s^2 (the maximum of
    |(x^2 - 1) e^{-x^2/2}| is 1, at the centre).  d depends on the radius alone, so an error of e in d moves the radius by
    e / |d'(rho)|, d'(rho) = -o rho / s^2 exp(-rho^2 / 2 s^2), up to a second-order term e^2 |d''| / (2 |d'|^3) that the factor 1.01
    covers; 1e-12 for the fp64 arithmetic.  (The fp32 directions are unit to 6e-8; the hit point is o + t v with the same v.)"""
    sc = S.scene("single")
    s, o, mu = 0.1, 1.0, sc["means"][0].astype(np.float64)
    assert np.allclose(sc["scales"], s) and sc["opacities"][0] == o
    r, O = LS.long_set("single"), LS.long_oracle("single")
    h_f = float(r["t1"][0] - r["t0"][0]) / 63.0 / 63.0
    for li, lev in enumerate(LS.LEVELS):
        e = lev / o + np.exp(-4.5)
        rho = s * np.sqrt(-2.0 * np.log(e))
        slope = o * rho / s ** 2 * e
        tol = 1.01 * (h_f ** 2 / 8.0) * (o / s ** 2) / slope + 1e-12
        hit = O["hit"][li]
        p = r["origins"][hit].astype(np.float64) + O["t"][li][hit][:, None] * r["dirs"][hit].astype(np.float64)
        err = np.abs(np.linalg.norm(p - mu[None, :], axis=1) - rho).max()
        print(f"level {lev}: rho = {rho:.5f}, {int(hit.sum())} hits, max |radius - rho| = {err:.3e}, tol = {tol:.3e}")
        assert err <= tol, (lev, err, tol)
        if lev == 0.5:
            assert abs(rho - 0.11586) < 5e-6


def test_search_side_paths():
    """A ray that starts inside a level hits only after the density has dipped below it; invalid rays miss every level."""
    d = LR.oracle_density(S.oracle("single"))
    mu = S.scene("single")["means"][0]
    inside = LR.search(d, [mu], [[1.0, 0.0, 0.0]], [0.0], [0.6], (0.5,))
    assert not inside["hit"].any() and inside["D"][0, 0] > 0.5 and inside["t"][0, 0] == 0
    through = LR.search(d, [mu - [0.6, 0, 0]], [[1.0, 0.0, 0.0]], [0.0], [1.2], (0.5,))
    rho = 0.1 * np.sqrt(-2.0 * np.log(0.5 + np.exp(-4.5)))
    assert through["hit"].all() and abs(through["t"][0, 0] - (0.6 - rho)) < 1e-6
    bad = LR.search(d, [mu - [0.6, 0, 0]] * 3, [[1.0, 0.0, 0.0]] * 3, [0.0, 1.2, np.nan], [0.0, 0.0, 1.2], (0.5, 0.1))
    assert not bad["hit"].any() and not bad["t"].any()


# ---------------------------------------------------------------------------------------------------- the smoothing
def test_smoothing_restatement_on_a_tetrahedron():
    """Every vertex of the regular tetrahedron has the other three at one distance: x' = x + lam (-x / 3 - x); the centroid of a
    closed mesh with equal edge lengths stays."""
    v, t = LS.tetrahedron()
    out, (att,) = LR.smooth_laplacian(v, t, 1, 0.5, [v[:, :2] * 2])
    assert np.allclose(out, v / 3.0, atol=1e-7) and np.allclose(att, v[:, :2] * 2 / 3.0, atol=1e-7)
    assert np.abs(out.mean(0)).max() < 1e-7
    out2 = LR.smooth_laplacian(v, t, 2, 0.5)[0]
    assert np.allclose(out2, v / 9.0, atol=1e-7)
    assert np.array_equal(LR.smooth_laplacian(v, t, 1, 0.0)[0], v)


def test_smoothing_restatement_on_a_grid_patch():
    """3 x 3 patch, centre lifted to z = 1: its six neighbours (four at sqrt 2, two at sqrt 3) balance around (1, 1, 0); corner 0
    has the two neighbours (1, 0, 0) and (0, 1, 0) at distance 1; the vertex no triangle names does not move."""
    v, t = LS.grid_patch()
    out = LR.smooth_laplacian(v, t, 1, 0.5)[0]
    assert np.allclose(out[4], [1.0, 1.0, 0.5], atol=1e-7)
    assert np.allclose(out[0], [0.25, 0.25, 0.0], atol=1e-7)
    assert np.array_equal(out[9], v[9])
    w1, w2 = 1.0 / (1.0 + 1e-12), 1.0 / (np.sqrt(2.0) + 1e-12)                           # vertex 1: 0, 2 at 1; 3 at sqrt 2; 4 at sqrt 2
    mean = (w1 * v[0] + w1 * v[2] + w2 * v[3] + w2 * v[4]).astype(np.float64) / (2 * w1 + 2 * w2)
    assert np.allclose(out[1], v[1] + 0.5 * (mean - v[1]), atol=1e-7)


# ------------------------------------------------------------------------------------------------ argument errors
def _field():
    from collab_splats_amd.density import DensityField
    f = DensityField.__new__(DensityField)
    f.n_gauss, f.n_units, f.device = 4, 0, torch.device("cpu")
    return f


def test_raycast_argument_errors_without_a_gpu():
    import collab_splats_amd as m
    from collab_splats_amd.density import level_surface_points
    assert m.level_surface_points is level_surface_points
    f = _field()
    o, v, a, b = torch.zeros(5, 3), torch.ones(5, 3), torch.zeros(5), torch.ones(5)
    with pytest.raises(ValueError, match="origins"):
        f.raycast(torch.zeros(5, 2), v, a, b, (0.3,))
    with pytest.raises(ValueError, match="origins"):
        f.raycast(torch.zeros(5, 3, dtype=torch.int32), v, a, b, (0.3,))
    with pytest.raises(ValueError, match="dirs"):
        f.raycast(o, torch.ones(4, 3), a, b, (0.3,))
    with pytest.raises(ValueError, match="t_near"):
        f.raycast(o, v, torch.zeros(4), b, (0.3,))
    with pytest.raises(ValueError, match="t_far"):
        f.raycast(o, v, a, torch.ones(5, 1), (0.3,))
    for levels in ((), (0.1, 0.2, 0.3, 0.4, 0.5), (0.0,), (-0.1,), (float("nan"),), (float("inf"),), (1e-60,), 0.3, ("a",)):
        with pytest.raises(ValueError, match="level"):
            f.raycast(o, v, a, b, levels)
        with pytest.raises(ValueError, match="level"):
            level_surface_points(f, o, v, a, b, levels)
    with pytest.raises(ValueError, match="values"):
        level_surface_points(f, o, v, a, b, (0.3,), values=torch.zeros(3, 2))
    with pytest.raises(ValueError, match="DensityField"):
        level_surface_points(None, o, v, a, b, (0.3,))
    with pytest.raises(m.MisplatError, match="no CPU fallback"):
        f.raycast(o, v, a, b, (0.3,))


def test_model_argument_errors_without_a_gpu():
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    sc = random_scene(30, 64, 48, seed=1)
    model = radegs.RadegsModel(radegs.RadegsModelConfig(), sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"],
                               sc["sh"][:, 0], sc["sh"][:, 1:])
    cam = radegs.PinholeCamera.make(torch.eye(4)[:3], 50.0, 50.0, 64, 48)
    for call in (model.level_set_points, model.level_set_mesh):
        with pytest.raises(ValueError, match="no cameras"):
            call([], 0.02)
        with pytest.raises(ValueError, match="return_normal"):
            call([cam], 0.02, return_normal="nearest")
        with pytest.raises(ValueError, match="total_points"):
            call([cam], 0.02, total_points=-1)
        with pytest.raises(ValueError, match="voxel_size"):
            call([cam], 0.0)
        with pytest.raises(ValueError, match="search_radius"):
            call([cam], 0.02, search_radius=0.0)
    with pytest.raises(ValueError, match="level"):
        model.level_set_points([cam], 0.02, surface_levels=(0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError, match="level"):
        model.level_set_points([cam], 0.02, surface_levels=(0.0,))
    with pytest.raises(ValueError, match="level"):
        model.level_set_mesh([cam], 0.02, surface_level=-1.0)
    with pytest.raises(ValueError, match="surface_level"):
        model.level_set_mesh([cam], 0.02, surface_level="x")
    with pytest.raises(ValueError, match="surface_level"):
        model.level_set_mesh([cam], 0.02, surface_levels=(0.3,))
    with pytest.raises(ValueError, match="smooth_iterations"):
        model.level_set_mesh([cam], 0.02, smooth_iterations=-1)
    with pytest.raises(radegs.MisplatError):
        model.level_set_points([cam], 0.02)


def test_smooth_laplacian_argument_errors_without_a_gpu():
    import collab_splats_amd as m
    from collab_splats_amd import meshclean
    assert m.smooth_laplacian is meshclean.smooth_laplacian and "smooth_laplacian" in meshclean.__all__
    v, t = (torch.from_numpy(x) for x in LS.tetrahedron())
    with pytest.raises(ValueError, match="vertices"):
        m.smooth_laplacian(v[:, :2], t)
    with pytest.raises(ValueError, match="triangles"):
        m.smooth_laplacian(v, t[:, :2])
    with pytest.raises(ValueError, match="triangles"):
        m.smooth_laplacian(v, t.float())
    with pytest.raises(ValueError, match="indices"):
        m.smooth_laplacian(v, t + 1)
    for it in (-1, 1.5, True):
        with pytest.raises(ValueError, match="iterations"):
            m.smooth_laplacian(v, t, iterations=it)
    for lam in (float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="lam"):
            m.smooth_laplacian(v, t, lam=lam)
    with pytest.raises(ValueError, match="attribute"):
        m.smooth_laplacian(v, t, attributes=(torch.zeros(3, 2),))
    with pytest.raises(ValueError, match="attribute"):
        m.smooth_laplacian(v, t, attributes=(torch.zeros(4, 2, dtype=torch.float64),))
    with pytest.raises(m.MisplatError, match="no CPU fallback"):
        m.smooth_laplacian(v, t)
