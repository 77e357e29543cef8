"""GPU: the density field (csrc/density.hip) off its defaults and at workload coordinates, on the two-unit scenes of
tests/density_regimes_scenes.py: a cut-off of 1.5 and of 6, min_opacity 0 and 0.5, the bench's voxel
size at unit coordinates (46, -27, 72), a lattice hundreds of metres out, Gaussians a hundredth of a voxel thick.

Two error bars.  The standing rule of test_density_gpu.py: err = max |got - oracle| / max |oracle| over everything compared,
bound = min(8 max(e32, 2^-23), 1e-4), e32 the fp32 restatement's own error by the same formula.  The local-scale rule beside it:
err_loc = max over the entries with S > 0 of |got - oracle| / S, with S = Oracle.scale (the size of the terms the entry is made
of, each with the factor 1 + m / 2 by which an error of the exponent's argument grows), e32_loc the restatement's, the same
bound and the same multiple for the same reason (same terms, same order, a few more roundings per term); an entry with S = 0
must be exactly 0.  Under it a unit that holds only the tail of a faint Gaussian is measured against that tail, not against the
steepest Gaussian of the scene: a wrongly skipped record or a term lost at a brick's corner shows."""
import numpy as np
import pytest
import torch

import density_regimes_scenes as RS
import density_scenes as S
from test_density_gpu import DEV, EPS, _bits, _field, _scatter, _t

pytestmark = pytest.mark.gpu


def _build(name, **kw):
    from collab_splats_amd import DensityField
    sc = S.scene(name)
    return DensityField(_t(sc["means"]), _t(sc["quats"]), _t(sc["scales"]), _t(sc["opacities"]), sc["h"], cutoff=sc["cutoff"],
                        min_opacity=sc["min_opacity"], bounds=sc["bounds"], **kw)


def _planes(f):
    """The pool [n, 5, 4096] in map order."""
    return f._pool[f._slot_map[f._map_order()].long()].cpu().numpy()


# ---------------------------------------------------------------------------------------------------- integer structures
@pytest.mark.parametrize("name", RS.NAMES)
def test_integer_structures_bit_for_bit(name):
    f, R = _field(name), S.restated(name)
    assert np.array_equal(f.lo, R.lo) and np.array_equal(f.dims, R.dims)
    coords, _, (offsets, ids) = f.units()
    assert np.array_equal(coords, R.unit_coords()), f"allocated units differ: {len(coords)} vs {len(R.lists)}"
    ro, ri = R.unit_lists()
    assert np.array_equal(offsets, ro) and np.array_equal(ids, ri)
    assert f.n_units == len(R.lists) == 2 and f.n_pairs == R.n_pairs
    assert np.array_equal(_bits(f._records.cpu().numpy()), _bits(R.records))


# -------------------------------------------------------------------------------------------------------------- field
@pytest.mark.parametrize("name", RS.NAMES + ("random", "tilted_disc"))
def test_field_under_both_rules(name):
    f, R = _field(name), S.restated(name)
    ref, scale, r32 = S.oracle_map(name)[0], RS.scale_map(name), S.restated_map(name)
    coords, d, _ = f.units()
    got = _scatter(d, coords, R)
    assert np.array_equal(_bits(S.to_dense(got, R.dims)), _bits(f.dense().cpu().numpy()))     # units() and dense() agree
    e32, err = RS.rel(r32, ref), RS.rel(got, ref)
    e32_loc, err_loc = RS.rel_local(r32, ref, scale), RS.rel_local(got, ref, scale)
    print(f"field {name}: err = {err:.3e}  e32 = {e32:.3e}  bound = {RS.bound(e32):.3e}   local scale: err = {err_loc:.3e}  "
          f"e32 = {e32_loc:.3e}  bound = {RS.bound(e32_loc):.3e}")
    assert err <= RS.bound(e32), (name, err, e32, RS.bound(e32))
    assert err_loc <= RS.bound(e32_loc), (name, err_loc, e32_loc, RS.bound(e32_loc))


# ------------------------------------------------------------------------------------------ skipping against no skipping
@pytest.mark.parametrize("name", RS.NAMES + ("random",))
def test_skipping_drops_only_zero_terms(name):
    """The kernel that passes over the records whose slabs miss a wave's brick (_flags = 0) against the one that evaluates
    every record at every voxel (_flags = 1): plane 0 bitwise equal wherever the oracle puts no Gaussian of the unit's list
    within |m - r^2| <= 1e-4 r^2 (at most 0.2 % of the voxels lie in such a shell), there within 8 * 2^-23 S; planes 1 to 4
    bitwise equal everywhere."""
    a, b, R = _field(name), _build(name, _flags=1), S.restated(name)
    assert a.n_units == b.n_units and torch.equal(a._slot_map, b._slot_map) and torch.equal(a._ids, b._ids)
    pa, pb = _planes(a), _planes(b)
    assert np.array_equal(_bits(pa[:, 1:]), _bits(pb[:, 1:]))
    assert (pa[:, 1] == 1).all() and not pa[:, 2:].any()
    coords = a.units()[0]
    da, db = _scatter(pa[:, 0], coords, R), _scatter(pb[:, 0], coords, R)
    shell, scale = RS.shell_map(name), RS.scale_map(name)
    assert shell.mean() <= RS.SHELL_SHARE, (name, shell.mean())
    differ = _bits(da) != _bits(db)
    gap = np.abs(da.astype(np.float64) - db.astype(np.float64))
    print(f"skip {name}: {int(differ.sum())} voxels differ, {int((differ & ~shell).sum())} of them outside the shells "
          f"({int(shell.sum())} voxels, {shell.mean():.2e}); largest difference {gap.max():.3e}")
    assert not (differ & ~shell).any(), (name, int((differ & ~shell).sum()), float(gap[~shell].max()))
    assert (gap[shell] <= 8 * EPS * scale[shell]).all(), name
    assert float(np.abs(db).max()) > 0.5                                                 # (the field is there)


# -------------------------------------------------------------------------------------------------------------- query
_GOT = {}


def _queried(name):
    """query at the scene's points with D = 16 and with every other D of RS.CHANNELS (the leading columns): once."""
    if name not in _GOT:
        Q, f = RS.query_set(name), _field(name)
        pts = _t(Q["pts"])
        _GOT[name] = {D: f.query(pts, _t(Q["values"][:, :D])) for D in RS.CHANNELS}
    return _GOT[name]


@pytest.mark.parametrize("name", RS.QUERY)
def test_query_under_both_rules(name):
    Q = RS.query_set(name)
    got = _queried(name)[max(RS.CHANNELS)]
    O, (rd, rg, rv) = Q["oracle"], Q["restated"]
    gd, gg, gv, dom = (got[k].cpu().numpy() for k in ("density", "grad", "values", "dominant"))
    inm = Q["in_map"]
    for label, sl in Q["sets"]:
        # (in the map by the restatement's naming of the unit, which is the kernel's: the voxel floor(p / h) in fp32.  The face
        # points on the map's outer faces, or an ulp beyond, are not -- nor is a random point of `far_h13` that fp32, 3e-5 m
        # coarse out there, rounds onto the map's far face.  Those are dealt with below)
        idx = np.arange(len(inm))[sl][inm[sl]]
        assert len(idx) >= len(inm[sl]) - 2 or label == "face points"
        for what, g, ref, r32 in (("density", gd, O["density"], rd), ("grad", gg, O["grad"], rg), ("values16", gv, O["values"], rv)):
            e32, err = RS.rel(r32[idx], ref[idx]), RS.rel(g[idx], ref[idx])
            print(f"query {name} {label} {what}: err = {err:.3e}  e32 = {e32:.3e}  bound = {RS.bound(e32):.3e}")
            assert err <= RS.bound(e32), (name, label, what, err, e32, RS.bound(e32))
        e32_loc = RS.rel_local(rd[idx], O["density"][idx], Q["scale"][idx])
        err_loc = RS.rel_local(gd[idx], O["density"][idx], Q["scale"][idx])
        print(f"query {name} {label} density, local scale: err = {err_loc:.3e}  e32 = {e32_loc:.3e}  bound = {RS.bound(e32_loc):.3e}")
        assert err_loc <= RS.bound(e32_loc), (name, label, err_loc, e32_loc, RS.bound(e32_loc))
    # the face points: which of them get no density at all must agree with the restatement, point by point; outside the map
    # everything is exactly 0 / 0 / -1 / 0, whatever the oracle, which knows no bounds, has there
    sl = Q["sets"][2][1]
    assert np.array_equal(gd[sl] == 0, rd[sl] == 0), (name, int(((gd[sl] == 0) != (rd[sl] == 0)).sum()))
    assert np.array_equal(dom[sl] == -1, rd[sl] == 0)
    out = ~inm
    print(f"query {name}: {int(out.sum())} face points outside the map, {int((inm[sl] & (gd[sl] > 0)).sum())} inside with density")
    assert 12 <= out[sl].sum() and not gd[out].any() and (O["density"][out] > 0).any()
    zero = gd == 0
    assert np.array_equal(dom == -1, zero) and not gg[zero].any() and not gv[zero].any()
    if name == "far_h13":
        assert (Q["pts"][sl][:, 0] < 0).all()                                            # (negative coordinates on the faces)


@pytest.mark.parametrize("name", RS.QUERY)
def test_query_is_the_same_for_every_channel_count(name):
    """values is walked four channels at a time: density, grad and dominant do not depend on D, and column c is the same bits
    in every D that has it."""
    got = _queried(name)
    full = got[max(RS.CHANNELS)]
    assert float(full["values"].abs().max()) > 0
    for D in RS.CHANNELS:
        g = got[D]
        assert tuple(g["values"].shape) == (full["density"].shape[0], D)
        for key in ("density", "grad"):
            assert torch.equal(g[key].view(torch.int32), full[key].view(torch.int32)), (name, D, key)
        assert torch.equal(g["dominant"], full["dominant"]), (name, D)
        assert torch.equal(g["values"].view(torch.int32), full["values"][:, :D].contiguous().view(torch.int32)), (name, D)


@pytest.mark.parametrize("name", RS.QUERY)
def test_query_at_non_finite_points_is_exactly_zero(name):
    """NaN, +-inf and 1e30 in any coordinate give 0 / 0 / -1 / 0, and the finite rows between them are what they were."""
    Q, f = RS.query_set(name), _field(name)
    pts = Q["pts"][2048:2048 + 96].copy()
    vals = _t(Q["values"][:, :5])
    clean = f.query(_t(pts), vals)
    bad = [np.nan, np.inf, -np.inf, 1e30, -1e30]
    rows = np.arange(0, 90, 2)                                                           # every other row, 45 = 5 x 3 x 3 of them
    for i, row in enumerate(rows):
        pts[row, i % 3] = bad[(i // 3) % 5]
        if i >= 30:
            pts[row, (i + 1) % 3] = bad[(i // 3 + 1) % 5]                                # (two bad coordinates)
    got = f.query(_t(pts), vals)
    keep = np.ones(len(pts), bool)
    keep[rows] = False
    k, r = torch.from_numpy(keep).to(DEV), torch.from_numpy(rows).to(DEV)
    for key in ("density", "grad", "dominant", "values"):
        assert torch.equal(got[key][k].view(torch.int32), clean[key][k].view(torch.int32)), (name, key)
    assert float(clean["density"][k].max()) > 0
    for key in ("density", "grad", "values"):
        assert torch.equal(got[key][r].view(torch.int32), torch.zeros_like(got[key][r]).view(torch.int32)), (name, key)    # +0.0
    assert bool((got["dominant"][r] == -1).all())


# ------------------------------------------------------------------------------------------------- functional wrappers
def test_functional_wrappers_pass_cutoff_and_voxel_size_on():
    from collab_splats_amd import DensityField, gaussian_density, gaussian_density_grad
    sc = S.scene("bench_corner")
    pts = RS.query_set("bench_corner")["pts"][2048:4096]
    act = (_t(sc["means"]), _t(sc["quats"]), _t(sc["scales"]), _t(sc["opacities"]))
    p = _t(pts)
    d = gaussian_density(p, *act, voxel_size=0.013, cutoff=1.5)
    g = gaussian_density_grad(p, *act, voxel_size=0.013, cutoff=1.5)
    box = np.stack([pts.astype(np.float64).min(0), pts.astype(np.float64).max(0)])
    f = DensityField(*act, 0.013, cutoff=1.5, bounds=box)
    q = f.query(p)
    assert torch.equal(d.view(torch.int32), q["density"].view(torch.int32)) and float(d.max()) > 0
    assert torch.equal(g.view(torch.int32), q["grad"].view(torch.int32)) and g.shape == (2048, 3) and float(g.abs().max()) > 0
    # and they are not the default's: the cut-off reached the kernel
    d3 = gaussian_density(p, *act, voxel_size=0.013)
    assert not torch.equal(d3, d) and float(d3.max()) > float(d.max())


# -------------------------------------------------------------------------------------------------------- determinism
def test_two_builds_at_the_largest_cutoff_are_bitwise_equal():
    a, b = _build("bench_corner_r6"), _build("bench_corner_r6")
    ca, da, (oa, ia) = a.units()
    cb, db, (ob, ib) = b.units()
    assert np.array_equal(ca, cb) and np.array_equal(oa, ob) and np.array_equal(ia, ib) and np.array_equal(_bits(da), _bits(db))
    assert torch.equal(a._pool.view(torch.int32), b._pool.view(torch.int32)) and torch.equal(a._slot_map, b._slot_map)
    assert torch.equal(a._records.view(torch.int32), b._records.view(torch.int32)) and torch.equal(a._ranges, b._ranges)
