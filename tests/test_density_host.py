"""CPU: the Gaussian density field's yardsticks (tests/density_restatement.py) checked against each other, and the Python
surface's argument errors with no GPU present.

  * the oracle's gradient against central differences of its own density;
  * the restatement's lists are conservative: no (voxel, Gaussian) pair the oracle needs is missing from the voxel's unit list;
  * the restatement's fp32 field stays within the project's standing 1e-4 of the oracle;
  * no voxel of a mesh scene lies within 1e-3 of the iso it is extracted at (the GPU mesh test counts crossings from the oracle);
  * the scenes exercise what they are there for."""
import numpy as np
import pytest
import torch

import density_scenes as S
from density_restatement import Oracle


# ------------------------------------------------------------------------------------------------------- the yardsticks
@pytest.mark.parametrize("name", ["negative", "tilted_disc", "culled"])
def test_oracle_gradient_matches_central_differences(name):
    """Step and tolerance from fp64 and the field's third derivative, not from any code under test.  Along a unit direction n the
    third derivative of o exp(-|A x|^2 / 2) is o |A n|^3 He3(u) exp(-u^2 / 2) exp(-rest / 2) with |A n| <= 1 / s_min and
    max |He3(u) exp(-u^2 / 2)| = 1.3801, so M3 = sum_g 1.3801 o_g / s_min,g^3 bounds it.  A central difference of step t errs by at
    most t^2 M3 / 6 + eps_d / t, eps_d = 1e-12 the evaluation error of d (the oracle's A x - A mu cancellation, |A mu| < 1e3);
    the step t = (3 eps_d / M3)^(1/3) minimises that.  The field has a kink at each cut-off surface: points within 2 t / s_min of
    one (in the Gaussian's own metric) are not differentiated."""
    sc = S.scene(name)
    O = S.oracle(name)
    s_min = np.asarray(sc["scales"], np.float64)[O.ids].min(1)
    M3 = float((1.3801 * O.o / s_min ** 3).sum())
    eps_d = 1e-12
    t = (3 * eps_d / M3) ** (1.0 / 3.0)
    tol = 2.0 * (t * t * M3 / 6.0 + eps_d / t)
    rng = np.random.default_rng(5)
    lo, hi = O.mu.min(0) - 0.1, O.mu.max(0) + 0.1
    p = rng.uniform(lo, hi, (2000, 3))
    _, tt, _, _ = O.terms(p)
    root_m = np.sqrt((tt * tt).sum(-1))
    clear = (np.abs(root_m - 3.0) > 2 * t / s_min[None, :]).all(1)
    assert clear.mean() > 0.9
    p = p[clear]
    g = O.evaluate(p)["grad"]
    assert np.abs(g).max() > 1.0                                  # (the points see the field)
    for a in range(3):
        e = np.zeros(3)
        e[a] = t
        fd = (O.evaluate(p + e)["density"] - O.evaluate(p - e)["density"]) / (2 * t)
        assert np.abs(fd - g[:, a]).max() <= tol, (name, a, np.abs(fd - g[:, a]).max(), tol)


@pytest.mark.parametrize("name", S.NAMES)
def test_lists_are_conservative(name):
    """Every (voxel, Gaussian) with oracle m < r^2 has the Gaussian in the list of the voxel's unit, except pairs whose term is
    below 2^-23 max d (inclusion at the cut-off may round either way: the term is continuous there)."""
    R = S.restated(name)
    d, alloc, kmax, ids = S.oracle_map(name)
    if d.size == 0:
        assert not R.lists
        return
    thr = 2.0 ** -23 * d.max()
    for m in range(d.shape[0]):
        needed = set(int(g) for g in ids[kmax[m] >= max(thr, 1e-300)])
        have = set(R.lists.get(m, ()))
        assert needed <= have, (name, m, sorted(needed - have))


@pytest.mark.parametrize("name", S.NAMES)
def test_restatement_within_the_standing_bound(name):
    """max |fp32 - oracle| / max |oracle| <= 1e-4 over every voxel of the map (a voxel of an unallocated unit counts as 0)."""
    d, _, _, _ = S.oracle_map(name)
    if d.size == 0:
        return
    f = S.restated_map(name)
    e32 = np.abs(f - d).max() / np.abs(d).max()
    print(f"{name}: e32 = {e32:.3e}")
    assert e32 <= 1e-4


@pytest.mark.parametrize("name,iso", S.MESH)
def test_iso_margin(name, iso):
    """No voxel's oracle density lies within 1e-3 of the iso; and the level set does not reach the map's outermost voxels, so
    the mesh is closed."""
    R = S.restated(name)
    d = S.to_dense(S.oracle_map(name)[0], R.dims)
    assert np.abs(d - iso).min() > 1e-3, (name, iso, np.abs(d - iso).min())
    above = d > iso
    assert above.any() and above[1:-1, 1:-1, 1:-1].sum() == above.sum()


# --------------------------------------------------------------------------------------------- the scenes do their job
def test_scenes_exercise_their_mechanisms():
    R = S.restated("single")                                     # all 8 units around the corner, stitched across three faces
    have = {tuple(c) for c in R.unit_coords()}
    assert {(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)} <= have
    R = S.restated("tilted_disc")                                # the slab test drops units of the AABB; thinner than a voxel
    assert 0 < R.n_pairs < R.aabb_pairs and S.scene("tilted_disc")["scales"].min() < S.H
    R = S.restated("tiny")                                       # the voxel next door lies in the next unit
    assert {tuple(c) for c in R.unit_coords()} == {(0, 0, 0), (1, 0, 0)}
    d = S.to_dense(S.oracle_map("tiny")[0], R.dims)
    assert (d > 0.5).sum() == 1 and d[8, 8, 15] > 0.5
    for n in S.BATCH_SIZES:                                      # one unit, one list of n
        R = S.restated(f"batches_{n}")
        assert list(R.lists) == [0] and len(R.lists[0]) == n and tuple(R.dims) == (1, 1, 1)
    R = S.restated("negative")
    assert (R.lo < 0).all() and (R.lo + R.dims > 0).all()
    R = S.restated("clipped")                                    # one unit; the Gaussian outside makes no pair
    assert tuple(R.dims) == (1, 1, 1) and R.lists == {0: [0, 2]}
    assert (R.E[0] * 2 > 0.32).all()                             # (wider than the whole map)
    R = S.restated("culled")
    assert R.ok.tolist() == [False, False, True, False, True, True]
    q = S.scene("culled")["quats"]
    assert not np.array_equal(q[4], q[5]) and abs(np.linalg.norm(q[5].astype(np.float64)) - 3.7) < 1e-5
    assert np.array_equal(R.records[4].view(np.uint32), R.records[5].view(np.uint32))     # the twins, bit for bit
    R = S.restated("empty")
    assert not R.ok.any() and not R.lists and R.n_pairs == 0
    R = S.restated("random")
    assert len(R.lists) == 64 and tuple(R.dims) == (4, 4, 4) and R.n_pairs < R.aabb_pairs


def test_oracle_dominant_and_values():
    """Two Gaussians by hand: the lowest g wins a tie, -1 and 0 where d = 0, values are the term-weighted mean."""
    means = np.array([[0, 0, 0], [0.2, 0, 0], [5, 5, 5]], np.float32)
    quats = np.tile(np.array([[1, 0, 0, 0]], np.float32), (3, 1))
    scales = np.full((3, 3), 0.1, np.float32)
    O = Oracle(means, quats, scales, np.array([0.5, 0.5, 1.0], np.float32))
    vals = np.array([[1.0, 0.0], [0.0, 1.0], [7.0, 7.0]])
    out = O.evaluate(np.array([[0.1, 0, 0], [0.05, 0, 0], [2.0, 2.0, 2.0]]), vals)
    assert out["dominant"].tolist() == [0, 0, -1]
    assert np.allclose(out["values"][0], [0.5, 0.5]) and out["values"][1][0] > 0.5 and np.all(out["values"][2] == 0)
    assert out["density"][2] == 0 and np.all(out["grad"][2] == 0) and abs(out["grad"][0][0]) < 1e-12


# ----------------------------------------------------------------------------------------------------- Python surface
def _args(n=4):
    return torch.zeros(n, 3), torch.tensor([[1.0, 0, 0, 0]]).repeat(n, 1), torch.full((n, 3), 0.1), torch.full((n,), 0.5)


def test_argument_errors_are_raised_without_a_gpu():
    import collab_splats_amd as m
    from collab_splats_amd.density import DensityField, gaussian_density, gaussian_density_grad
    assert m.DensityField is DensityField and m.gaussian_density is gaussian_density
    mu, q, s, o = _args()
    with pytest.raises(ValueError, match="means"):
        DensityField(torch.zeros(4, 2), q, s, o, 0.02)
    with pytest.raises(ValueError, match="quats"):
        DensityField(mu, torch.zeros(4, 3), s, o, 0.02)
    with pytest.raises(ValueError, match="scales"):
        DensityField(mu, q, torch.zeros(3, 3), o, 0.02)
    with pytest.raises(ValueError, match="opacities"):
        DensityField(mu, q, s, torch.zeros(5), 0.02)
    for h in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            DensityField(mu, q, s, o, h)
    for r in (0.0, -1.0, 6.5, float("nan")):
        with pytest.raises(ValueError, match="cutoff"):
            DensityField(mu, q, s, o, 0.02, cutoff=r)
    with pytest.raises(ValueError, match="min_opacity"):
        DensityField(mu, q, s, o, 0.02, min_opacity=1.5)
    with pytest.raises(ValueError, match="bounds"):
        DensityField(mu, q, s, o, 0.02, bounds=[[0, 0, 0], [1, -1, 1]])
    with pytest.raises(ValueError, match="bounds"):
        DensityField(mu, q, s, o, 0.02, bounds=[[0, 0, 0]])
    with pytest.raises(ValueError, match="points"):
        gaussian_density(torch.zeros(5, 2), mu, q, s, o, 0.02)
    with pytest.raises(ValueError, match="cutoff"):
        gaussian_density_grad(torch.zeros(5, 3), mu, q, s, o, 0.02, cutoff=7.0)
    # CPU tensors: there is no CPU fallback
    with pytest.raises(m.MisplatError, match="no CPU fallback"):
        DensityField(mu, q, s, o, 0.02)
    with pytest.raises(m.MisplatError, match="no CPU fallback"):
        gaussian_density(torch.zeros(5, 3), mu, q, s, o, 0.02)


def test_query_and_mesh_argument_errors_without_a_gpu():
    """The checks of query / extract_mesh come before anything touches the device: exercised on an object built by hand."""
    from collab_splats_amd.density import MAX_CHANNELS, DensityField
    f = DensityField.__new__(DensityField)
    f.n_gauss, f.n_units, f.device = 4, 0, torch.device("cpu")
    with pytest.raises(ValueError, match="points"):
        f.query(torch.zeros(3))
    with pytest.raises(ValueError, match="values"):
        f.query(torch.zeros(2, 3), values=torch.zeros(3, 2))
    with pytest.raises(ValueError, match="channels"):
        f.query(torch.zeros(2, 3), values=torch.zeros(4, MAX_CHANNELS + 1))
    with pytest.raises(ValueError, match="channels"):
        f.extract_mesh(0.5, values=torch.zeros(4, 17))
    with pytest.raises(ValueError, match="iso"):
        f.extract_mesh(float("nan"))


def test_model_surface_without_a_gpu():
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    sc = random_scene(30, 64, 48, seed=1)
    args = (sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"], sc["sh"][:, 0], sc["sh"][:, 1:])
    model = radegs.RadegsModel(radegs.RadegsModelConfig(), *args)
    c = model.colors.detach()
    assert c.shape == (30, 3) and float(c.min()) >= 0 and float(c.max()) <= 1
    assert torch.equal(c, torch.clamp(sc["sh"][:, 0] * 0.28209479177387814 + 0.5, 0, 1))
    m0 = radegs.RadegsModel(radegs.RadegsModelConfig(sh_degree=0), *args[:4], sc["sh"][:, 0], sc["sh"][:, 1:1])
    assert torch.equal(m0.colors, torch.sigmoid(sc["sh"][:, 0]))
    with pytest.raises(ValueError, match="cameras"):
        model.marching_cubes_mesh()
    with pytest.raises(ValueError, match="no cameras"):
        model.marching_cubes_mesh(cameras=[])
    cam = radegs.PinholeCamera.make(torch.eye(4)[:3], 50.0, 50.0, 64, 48)
    with pytest.raises(ValueError, match="resolution"):
        model.marching_cubes_mesh(cameras=[cam], resolution=1)
    with pytest.raises(ValueError, match="span no volume"):
        model.marching_cubes_mesh(cameras=[cam])
    with pytest.raises(radegs.MisplatError):
        model.get_density(torch.zeros(3, 3))
