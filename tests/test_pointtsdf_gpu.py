"""GPU: point-cloud TSDF fusion with space carving (csrc/pointtsdf.hip) against the numpy restatement
(tests/pointtsdf_restatement.py): the allocated units and every integer plane equal, the meshes equal; the flush of the LDS
partial sums; order, splitting and chunking; the depth-map and model paths."""
import numpy as np
import pytest
import torch

import pointtsdf_scenes as PS
import tsdf_scenes as S
from pointtsdf_restatement import RestatedPointTSDF

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VS, TRUNC = 0.02, 0.06


def _t(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0 and b.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _same_units(a, b):
    names = ("coords", "sum_q", "count", "rgb_sum", "rgb_count")
    assert np.array_equal(a[0], b[0]), f"allocated units differ: {len(a[0])} vs {len(b[0])}"
    for name, x, y in zip(names[1:], a[1:], b[1:]):
        bad = np.argwhere(x != y)
        assert len(bad) == 0, f"{name} differs at {len(bad)} entries, first {bad[:3].tolist()}: {x[tuple(bad[0])]} vs {y[tuple(bad[0])]}"


def _check(vol, ref, min_weight=1):
    _same_units(vol.units(), ref.unit_arrays())
    v, f, c = (x.cpu().numpy() for x in vol.extract_mesh(min_weight))
    vr, fr, cr = ref.extract_mesh(min_weight)
    assert f.dtype == np.int32 and np.array_equal(f, fr)
    assert v.shape == vr.shape and _rel(v, vr) <= 1e-6 and _rel(c, cr) <= 1e-6
    return v, f


def _volume(carve=True, bounds=None, vs=VS, trunc=TRUNC):
    from collab_splats_amd import PointTSDFVolume
    return PointTSDFVolume(vs, trunc, carve, bounds=bounds, device=DEV), RestatedPointTSDF(vs, trunc, carve, bounds=bounds)


def _both(vol, ref, p, o, c=None):
    vol.integrate(_t(p), _t(o), None if c is None else _t(c))
    ref.integrate(p, o, c)


_SCAN = {}


def _scan():
    if not _SCAN:
        _SCAN.update(PS.sphere_scan())
    return _SCAN


def _cloud(views):
    """the views as one cloud with an origin per point"""
    p = np.concatenate([v[0] for v in views])
    o = np.concatenate([np.broadcast_to(v[1], v[0].shape) for v in views]).astype(np.float32)
    return p, o, np.concatenate([v[2] for v in views]).astype(np.float32)


# ------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("carve", [True, False])
def test_sphere_scan_equals_restatement(carve):
    """8 views of 48 x 36, one call per view with the view's origin: integers and mesh; the mesh lies on the sphere."""
    sc = _scan()
    vol, ref = _volume(carve)
    for p, o, c in sc["views"]:
        _both(vol, ref, p, o, c)
    v, f = _check(vol, ref)
    assert len(f) > 3000
    assert np.abs(np.linalg.norm(v - sc["centre"], axis=1) - sc["radius"]).max() <= VS
    assert vol.n_units == len(ref.units) and vol.n_pairs > 0


@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("offset", [0.0, -140.0])
def test_edge_rays_equal_restatement(offset, carve):
    """Rays along the axes, origins on voxel faces, voxel corners and unit corners (the unit corner at the world origin among
    them), exact diagonals, an origin per point; shifted by -140 voxels every unit coordinate is negative."""
    p, o = PS.edge_rays(VS, n=320, offset=offset, seed=2)
    if offset == 0.0:
        o[120] = 0.0                                                           # the unit corner (0, 0, 0) itself
    vol, ref = _volume(carve)
    _both(vol, ref, p, o, np.random.default_rng(0).random(p.shape).astype(np.float32))
    _check(vol, ref)
    coords = vol.units()[0]
    assert (coords.max() < 0) if offset else (coords.min() < 0 < coords.max())


def test_axis_rays_cross_three_units():
    """Rays along +-x, +-y, +-z from one origin, 56 voxels long: each crosses at least 3 unit boundaries."""
    o = (np.array([5.5, 3.5, 9.5]) * VS).astype(np.float32)
    p = np.stack([o + s * 56 * VS * np.eye(3)[a] for a in range(3) for s in (1, -1)]).astype(np.float32)
    vol, ref = _volume(True)
    _both(vol, ref, p, o)
    _same_units(vol.units(), ref.unit_arrays())
    coords = vol.units()[0]
    assert all(len(np.unique(coords[:, a])) >= 7 for a in range(3))


def test_points_outside_bounds_and_clipped_rays():
    """bounds cut the sphere in half: points outside them add nothing, rays are walked only inside the map."""
    sc = _scan()
    bounds = [[-1.0, -1.0, -1.0], [0.1, 1.0, 1.0]]
    vol, ref = _volume(True, bounds)
    for p, o, c in sc["views"][:4]:
        _both(vol, ref, p, o, c)
    _check(vol, ref)
    assert vol.units()[0][:, 0].max() == int(np.floor(0.1 / float(np.float32(VS) * np.float32(16))))
    far = (np.random.default_rng(1).uniform(2.0, 3.0, (50, 3))).astype(np.float32)   # every ray entirely outside the map
    before = vol.units()
    vol.integrate(_t(far), _t(np.float32([2.5, 2.5, 2.0])))
    _same_units(vol.units(), before)


def test_map_grows_with_a_second_call():
    sc = _scan()
    vol, ref = _volume(False)
    p, o, c = sc["views"][0]
    _both(vol, ref, p, o, c)
    dims = vol.dims.copy()
    shift = np.float32([-1.7, 0.9, -0.8])
    _both(vol, ref, p + shift, o + shift, c)
    assert np.any(vol.dims > dims)
    _check(vol, ref)


@pytest.mark.parametrize("units, far, band", [
    (((0, 0, 0), (256, 0, 0), (257, 0, 0)), (257, 0, 0), (257, 1 << 16)),
    (((40, 37, 38), (28, 40, 39), (40, 40, 40)), (40, 40, 40), ((1 << 16) + 1, (1 << 24) - 1))])
def test_lists_beyond_one_sort_pass(units, far, band):
    """The shared list driver (misplat_unit_lists) under point TSDF with map indices above one byte: 12 short rays without
    carving, four in each of three units, handed over unit by unit in turn, so the sort has to move every pair.  A map of 258
    entries takes two radix passes (and the identity third), with map indices 0, 256 and 257; one of 41^3 three, with map
    indices 65435 = 0xFF9B, 67227 = 0x1069B and 68920 on either side of 2^16.  The first two indices of each case share their
    low byte: after the first pass their pairs alternate, and only the higher passes part the two units' lists.  The scenes
    above never leave one pass.  A unit's rays run along +x through neighbouring voxel columns (2 x 2 in y, z), so the mesh is
    not empty.  In the second case a thirteenth ray of length 0 in unit (0, 0, 0) stretches the map to the origin and is then
    skipped: the restatement extracts densely over the box of the allocated units, which so stays 13 x 4 x 3 units while the
    map has 41^3 entries."""
    rng = np.random.default_rng(7)
    units = np.array(units, np.float64)
    yz = np.array([(0, j, k) for j in (0, 1) for k in (0, 1)], np.float64)
    # points in voxels 8 .. 9 of their unit: with sdf_trunc 3 voxels and the map's pad of 4 nothing leaves the unit
    p = (np.tile(units, (4, 1)) * 16 + 8.5 + np.repeat(yz, 3, 0) + rng.uniform(-0.2, 0.2, (12, 3))) * VS
    o = p - np.array([0.5, 0.0, 0.0])
    if units.min() > 0:
        p, o = np.concatenate([p, [[8.5 * VS] * 3]]), np.concatenate([o, [[8.5 * VS] * 3]])
    p, o = p.astype(np.float32), o.astype(np.float32)
    vol, ref = _volume(False)
    _both(vol, ref, p, o, rng.random(p.shape).astype(np.float32))
    assert np.array_equal(vol.lo, np.zeros(3)) and np.array_equal(vol.dims, np.array(far) + 1)
    assert band[0] <= int(np.prod(vol.dims)) <= band[1]
    assert vol.n_units == 3 and vol.n_pairs == 12           # one call: every unit is listed, so one holds >= 2 rays (all hold 4)
    m = (units[:, 0] + vol.dims[0] * (units[:, 1] + vol.dims[1] * units[:, 2])).astype(np.int64)
    assert m[0] % 256 == m[1] % 256 and m[0] // 256 != m[1] // 256
    assert np.array_equal(vol.units()[0], units[np.argsort(m)].astype(np.int64))
    assert len(_check(vol, ref)[1]) > 0


def test_empty_and_skipped_clouds():
    vol, ref = _volume(True)
    vol.integrate(torch.zeros((0, 3), device=DEV), torch.zeros(3, device=DEV))
    skipped = np.float32([[np.nan, 0, 0], [0.25, 0.5, 0.75], [np.inf, 1, 1], [1e7, 0, 0]])
    vol.integrate(_t(skipped), _t(np.float32([0.25, 0.5, 0.75])))
    assert vol.n_units == 0 and vol.units()[0].shape == (0, 3)
    v, f, c = vol.extract_mesh()
    assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == torch.int32 and c.shape == (0, 3)
    mixed = np.concatenate([skipped, PS.column_rays(VS, 5)[0]])
    origins = np.concatenate([np.tile(np.float32([0.25, 0.5, 0.75]), (4, 1)), PS.column_rays(VS, 5)[1]])
    _both(vol, ref, mixed, origins)
    _check(vol, ref, min_weight=5)


def test_min_weight_on_exact_counts():
    for repeat, expect in ((4, False), (5, True)):
        vol, ref = _volume(True)
        _both(vol, ref, *PS.column_rays(VS, repeat))
        _same_units(vol.units(), ref.unit_arrays())
        assert (vol.extract_mesh(min_weight=5)[1].shape[0] > 0) == expect
        _check(vol, ref, min_weight=repeat)


# ------------------------------------------------------------------------------------------------------ the LDS flush
def test_flush_boundary_of_the_lds_sums():
    """70 000 rays from one origin into one small patch: the origin's unit takes more than the 65 536 terms a voxel's 32-bit
    partial sum may hold, so its list is flushed in several pieces (of 8192 rays, by integer atomics); the origin's voxel counts
    exactly 70 000 and every integer equals the restatement's."""
    n = 70000
    p, o, c = PS.fan(VS, n)
    vol, ref = _volume(True)
    _both(vol, ref, p, o, c)
    coords, sum_q, count = vol.units()[:3]
    k = int(np.nonzero((coords == 0).all(1))[0][0])
    i = 2 | (4 << 4) | (7 << 8)
    assert count[k, i] == n and sum_q[k, i] == n * 16384
    _same_units(vol.units(), ref.unit_arrays())


# -------------------------------------------------------------------------------------------------- order and batching
def test_order_split_and_chunking_do_not_reach_the_result(monkeypatch):
    from collab_splats_amd import pointtsdf
    sc = _scan()
    p, o, c = _cloud(sc["views"][:3])
    n = len(p)

    def run(order, parts):
        vol, _ = _volume(True)
        for part in np.array_split(order, parts):
            vol.integrate(_t(p[part]), _t(o[part]), _t(c[part]))
        return vol

    base = run(np.arange(n), 1)
    want = base.units()
    mesh = [x.cpu().numpy() for x in base.extract_mesh(1)]
    perm = np.random.default_rng(3).permutation(n)
    for order, parts in ((perm, 1), (np.arange(n), 3), (perm, 37)):
        _same_units(run(order, parts).units(), want)
    monkeypatch.setattr(pointtsdf, "CHUNK_RAYS", 777)                           # several kernel chunks inside one call
    _same_units(run(np.arange(n), 1).units(), want)
    monkeypatch.undo()
    again = [x.cpu().numpy() for x in run(np.arange(n), 1).extract_mesh(1)]
    for x, y in zip(mesh, again):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "two runs differ"
    assert len(mesh[1]) > 500


# ---------------------------------------------------------------------------------------------- depth and model paths
@pytest.mark.parametrize("masked", [False, True])
def test_integrate_depth_equals_backproject_and_integrate(masked):
    from collab_splats_amd import PointTSDFVolume, backproject
    sc = _scan()
    d, c2w, intr, rgb = _t(sc["depths"]), _t(sc["c2w"]), _t(sc["intr"]), _t(sc["rgbs"])
    V, H, W = d.shape[:3]
    mask = None
    if masked:
        yy, xx = np.mgrid[:H, :W]
        mask = _t(np.repeat((((xx - 20) ** 2 + (yy - 15) ** 2) > 49)[None], V, 0))
    a = PointTSDFVolume(VS, TRUNC, device=DEV)
    a.integrate_depth(d, c2w, intr, rgbs=rgb, masks=mask)
    ok = d[..., 0] > 0
    if masked:
        ok &= mask
    at = torch.nonzero(ok.reshape(V, -1))
    f, pix = at[:, 0].int(), at[:, 1].int()
    pts, _, col = backproject(d, rgb, None, c2w, intr, f, pix)
    b = PointTSDFVolume(VS, TRUNC, device=DEV)
    b.integrate(pts, c2w[:, :, 3][f.long()], col)
    assert a.n_rays == b.n_rays == len(f) > 3000
    _same_units(a.units(), b.units())
    assert a.units()[3].sum() > 0                                               # colours arrived
    assert a.extract_mesh(1)[1].shape[0] > 1000      # (the maps were cast through pixel corners, lifted through centres: no sphere test)
    black = PointTSDFVolume(VS, TRUNC, device=DEV)
    black.integrate_depth(d, c2w, intr, masks=mask)                             # no rgbs: the same geometry, black
    _same_units(black.units()[:3], a.units()[:3])
    assert black.units()[3].sum() == 0


def test_model_tsdf_points_mesh_equals_manual_loop():
    from collab_splats_amd import PointTSDFVolume
    model = S.sphere_gaussians(20000).to(DEV)
    model.eval()
    W, H = 96, 72
    _, vms, _, _ = S.sphere_views(6, 8, 8)
    K = S.intrinsics(W, H, 60.0)
    cams = [S.pinhole_camera(M, K, W, H) for M in vms]
    vol = PointTSDFVolume(VS, TRUNC, True, device=DEV)
    for b in range(0, len(cams), 4):
        maps = model.render_views(cams[b:b + 4], batch_size=4)
        c2w, intr = model._camera_poses(cams[b:b + 4], DEV)
        vol.integrate_depth(maps["depth"], c2w, intr, rgbs=maps["rgb"])
    ref = [x.cpu().numpy() for x in vol.extract_mesh(2)]
    got = [x.cpu().numpy() for x in model.tsdf_points_mesh(cams, voxel_size=VS, sdf_trunc=TRUNC, min_weight=2, batch_size=4)]
    assert len(ref[1]) > 1000
    for x, y in zip(got, ref):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()
    v, f, c = model.tsdf_points_mesh(cams, voxel_size=VS, sdf_trunc=TRUNC, min_weight=2, batch_size=4, target_triangles=800)
    assert 0 < f.shape[0] <= 800 and c.shape == v.shape and int(f.max()) < v.shape[0]
    with pytest.raises(ValueError, match="target_triangles"):
        model.tsdf_points_mesh(cams, target_triangles=-1)
