"""CPU: every scene of tests/pointtsdf_regimes_scenes.py is in the regime it is there for, asserted on the numpy restatement
(tests/pointtsdf_restatement.py): what tests/test_pointtsdf_regimes_gpu.py rests on when it compares the kernels with it."""
import numpy as np
import pytest

import pointtsdf_regimes_scenes as RS
import pointtsdf_scenes as PS
from pointtsdf_restatement import RestatedPointTSDF, make_rays, u8

F = np.float32


def _fused(p, o, c, vs, trunc, carve, bounds=None):
    r = RestatedPointTSDF(vs, trunc, carve, bounds=bounds)
    r.integrate(p, o, c)
    return r


# ------------------------------------------------------------------------------------- 1: voxel size x truncation
def test_pair_count_counts_units_per_ray():
    """Three rays along +x of 30, 3 and 0 voxels from voxel (8, 8, 8): with carving 3 + 1 + 0 pairs (the walk runs 3 voxels
    past the point), without 1 + 1 + 0; a box over unit 1 alone keeps one pair."""
    vs = 0.02
    o = np.tile(F([8.5, 8.5, 8.5]) * F(vs), (3, 1))
    p = o + F(vs) * F([[30, 0, 0], [3, 0, 0], [0, 0, 0]])
    got = RS.pairs(p, o, vs, 0.06, True)
    assert got.tolist() == [[0, 0, 0, 0], [0, 1, 0, 0], [0, 2, 0, 0], [1, 0, 0, 0]]
    assert RS.pair_count(p, o, vs, 0.06, False) == 2
    assert RS.pair_count(p, o, vs, 0.06, True, bounds=[[0.4, 0.1, 0.1], [0.5, 0.2, 0.2]]) == 1


def test_thin_band_has_carving_updates_outside_it():
    """(0.02, 0.01): with carving some unit on a ray's path is updated (count > 0) and holds no band voxel at all (rgb_count
    0 everywhere), and thousands of voxels are updated outside the band."""
    vs, trunc = RS.THIN
    _, _, cnt, _, rc = _fused(*RS.bundle(vs), vs, trunc, True).unit_arrays()
    carved_only = (cnt.sum(1) > 0) & (rc.sum(1) == 0)
    outside = int(((cnt > 0) & (rc == 0)).sum())
    print(f"{len(cnt)} units, {int(carved_only.sum())} updated without a band voxel; {outside} voxels updated outside the band, "
          f"{int((rc > 0).sum())} inside")
    assert carved_only.sum() >= 1 and outside > 1000 and (rc > 0).sum() > 0


def test_wide_band_spans_three_units():
    """(0.02, 0.5): one ray's band voxels (|sdf| < trunc) lie in at least 3 units along an axis."""
    vs, trunc = RS.WIDE
    p, o, _ = RS.bundle(vs)
    g, sdf, ray = RestatedPointTSDF(vs, trunc, True).updates(p, o)
    band = np.abs(sdf) < F(trunc)
    most = max(len(np.unique(g[band & (ray == i), a] >> 4)) for i in range(len(p)) for a in range(3))
    print(f"a ray's band voxels span up to {most} units on an axis")
    assert most >= 3


@pytest.mark.parametrize("vs,trunc", RS.VOXEL_TRUNC)
def test_every_ray_of_the_bundle_takes_part(vs, trunc):
    p, o, _ = RS.bundle(vs)
    assert len(make_rays(p, o, vs, trunc, True)["index"]) == len(p) == 320


# --------------------------------------------------------------------------------- 2: a sphere at the workload's voxel
@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("shifted", [False, True])
def test_workload_sphere_mesh_lies_on_the_sphere(shifted, carve):
    """The restatement's mesh at voxel 0.01, at the world origin and translated by (37.3, -52.1, 18.7) m: every vertex within
    one voxel of the sphere (measured: 0.913 voxels both ways)."""
    sc, r = RS.scan(shifted), RS.restated_scan(shifted, carve)
    v, f, _ = r.extract_mesh(min_weight=1)
    worst = RS.off_sphere(v, sc) / RS.WORK[0]
    print(f"shifted {shifted} carving {carve}: {len(r.units)} units, {len(f)} triangles, worst distance {worst:.3f} voxels")
    assert len(f) > 10000 and worst <= 1.0
    if shifted:
        reach = max(np.abs(p).max() for p, _, _ in sc["views"]) / RS.WORK[0]
        assert 5000 < reach < 5300


# ------------------------------------------------------------------------------------------------------- 3: far out
@pytest.mark.parametrize("offset", RS.OFFSETS)
def test_far_bundles_keep_their_rays(offset):
    """At least 300 of the 320 rays take part at every offset; at -4e6 voxels every allocated unit lies beyond 2^17 units."""
    p, o, c = RS.bundle(RS.WORK[0], offset)
    kept = len(make_rays(p, o, *RS.WORK, True)["index"])
    r = _fused(p, o, c, *RS.WORK, True)
    coords = r.unit_arrays()[0]
    print(f"offset {offset}: {kept} of {len(p)} rays, {len(coords)} units, |unit| >= {np.abs(coords).min()}")
    assert kept >= 300
    if abs(offset) >= 4.0e6:
        assert np.abs(coords).min() > 1 << 17


# ------------------------------------------------------------------------------------------------------ 4: long rays
def test_long_rays_have_many_pairs():
    p, o = RS.long_rays()
    L = np.linalg.norm(p.astype(np.float64) - o, axis=1) / RS.WORK[0]
    assert 399 < L.min() and L.max() < 701 and np.abs(o).max() <= 5 * RS.WORK[0] * 1.001
    pr = RS.pairs(p, o, *RS.WORK, True)
    per_ray = np.bincount(pr[:, 0], minlength=len(p))
    units_off = len(_fused(p, o, None, *RS.WORK, False).units)
    print(f"{len(np.unique(pr[:, 1:], axis=0))} units with carving, {units_off} without; pairs per ray {per_ray.min()} .. "
          f"{per_ray.max()}")
    assert per_ray.max() >= 40 and units_off < 4 * len(p)
    # without carving the walk starts hundreds of voxels from the origin
    g, _, ray = RestatedPointTSDF(*RS.WORK, False).updates(p, o)
    assert np.abs(g - np.floor(o[ray] / F(RS.WORK[0]))).max(1).min() > 200


# ------------------------------------------------------------------------------------------------ 5: the map's padding
@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("offset", [0.0, RS.PAD_OFFSET])
def test_padding_rays_leave_the_box_of_their_points_and_origins(offset, carve):
    """At least 20 rays visit a unit that holds neither a point nor an origin of the call, and the extreme units of the
    bundle, in both senses of every axis, are such units: a map that covered only points and origins would clip them."""
    p, o, _ = RS.padding_rays(carve, offset)
    assert 190 <= len(p) <= 210 and len(make_rays(p, o, *RS.WORK, carve)["index"]) == len(p)
    held = RS.held_units(p, RS.WORK[0]) | RS.held_units(o, RS.WORK[0])
    pr = RS.pairs(p, o, *RS.WORK, carve)
    empty = np.array([tuple(u) not in held for u in pr[:, 1:].tolist()])
    rays = len(np.unique(pr[empty, 0]))
    units = pr[:, 1:]
    extreme = np.any((units == units.min(0)) | (units == units.max(0)), 1)
    print(f"offset {offset} carving {carve}: {len(np.unique(units, axis=0))} units visited, {len(held)} hold a point or an origin, "
          f"{rays} rays visit a unit that holds neither")
    assert rays >= 20
    assert np.all(units.max(0) - units.min(0) == 2) and empty[extreme].all()
    if offset:
        step = np.spacing(np.abs(p).min()) / RS.WORK[0]
        assert 0.125 <= step <= 0.25                                            # an fp32 step of a world coordinate, in voxels


@pytest.mark.parametrize("offset", [0.0, RS.PAD_OFFSET])
def test_origins_at_a_face_need_the_origins_padding(offset):
    """The rays with their origin at a face, alone: the points padded by sdf_trunc and a voxel stay inside the points' unit, so
    only the origins' voxel of padding takes the map beyond it.  Every origin lies within a quarter voxel of its face; 2^21
    voxels out some walks begin, at floorf(o / h) in fp32, in the unit beyond the face, which holds neither point nor origin."""
    p, o, second = RS.padding_rays(True, offset)
    p, o = p[second], o[second]
    vs = float(F(RS.WORK[0]))
    home = np.asarray(RS.PAD_UNIT) + int(offset) // 16
    assert RS.held_units(o, vs) == {tuple(home.tolist())}
    pad = (RS.WORK[1] + RS.WORK[0]) * 1.01                                      # (a hundredth more for the fp32 sums)
    assert RS.held_units(p.astype(np.float64) - pad, vs) == RS.held_units(p.astype(np.float64) + pad, vs) == {tuple(home.tolist())}
    faces = np.stack([home * 16 * vs, (home + 1) * 16 * vs])
    gap = np.abs(o.astype(np.float64)[:, None, :] - faces[None]).min((1, 2)) / vs
    pr = RS.pairs(p, o, *RS.WORK, True)
    beyond = len(np.unique(pr[(pr[:, 1:] != home).any(1), 0]))
    print(f"offset {offset}: {len(p)} rays, origins up to {gap.max():.3f} voxels from a face, {beyond} walks begin beyond it")
    assert len(p) == 102 and gap.max() <= 0.25 + (0.2 if offset else 1e-3)
    assert beyond >= (3 if offset else 0)


# -------------------------------------------------------------------------------------- 6: bounds through every face
@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("k", [0, 1])
def test_bounds_are_entered_through_every_face(k, carve):
    """From the restatement's walk and clip: at least 20 rays start inside the map, at least 20 have no voxel inside, and with
    carving at least 5 rays enter from outside through each of the map's six faces (their first voxel inside the map lies in
    the outermost voxel layer of that face).  Without carving a ray is its last 6 voxels and next to none of 640 happens to
    begin just outside a given face: there at least 20 rays have voxels on both sides of the map's boundary."""
    p, o, _ = RS.bounds_bundle(k)
    box = np.asarray(RS.bounds_box())
    assert box[0].min() > -20 * RS.BOUNDS_VS and box[1].max() < 20 * RS.BOUNDS_VS          # strictly inside the bundle
    assert np.all(np.abs(box / (16 * RS.BOUNDS_VS) - np.round(box / (16 * RS.BOUNDS_VS))) > 0.2)   # aligned to no unit
    started, never, crosses, first, (lo, hi) = RS.map_entries(p, o, RS.BOUNDS_VS, 0.06, carve, box)
    assert lo.tolist() == [-16, -16, -16] and hi.tolist() == [15, 15, 15]
    entered = ~started & ~never
    faces = [int((entered & (first[:, a] == (lo[a] if s == 0 else hi[a]))).sum()) for a in range(3) for s in (0, 1)]
    print(f"bundle {k} carving {carve}: entered through -x +x -y +y -z +z {faces}, started inside {int(started.sum())}, "
          f"never inside {int(never.sum())}, on both sides {int(crosses.sum())}")
    assert started.sum() >= 20 and never.sum() >= 20 and crosses.sum() >= 20
    assert not carve or min(faces) >= 5


# --------------------------------------------------------------------------------- 7: pieces of the accumulate kernel
@pytest.mark.parametrize("n", RS.FANS)
def test_fan_fills_whole_pieces(n):
    """Every ray of the fan is listed under the origin's unit, whose list is so n rays long, and the origin's voxel counts n."""
    p, o, c = PS.fan(RS.FAN_VS, n)
    pr = RS.pairs(p, o, RS.FAN_VS, RS.FAN_TRUNC, True)
    assert int((pr[:, 1:] == 0).all(1).sum()) == n
    coords, _, cnt, _, _ = _fused(p, o, c, RS.FAN_VS, RS.FAN_TRUNC, True).unit_arrays()
    k = int(np.nonzero((coords == 0).all(1))[0][0])
    print(f"{n} rays: {len(coords)} units, {len(pr)} pairs")
    assert cnt[k, RS.FAN_VOXEL] == n and n % RS.PIECE in (0, 1)


# ------------------------------------------------------------------------------------- 8: colours at the cast's edges
def test_edge_colours_under_the_restated_cast():
    """-0.5, 0, 0.5 / 255, 1 / 255, 0.999999, 1, 1.5, NaN, +inf, -inf as uint8(rgb * 255): 0 0 0 1 254 255 255 0 255 0, and every
    one of them reaches every channel of the 36 rays."""
    assert u8(np.asarray(RS.EDGE_COLOURS, np.float32)).tolist() == list(RS.EDGE_U8)
    c = RS.edge_colours(36)
    for k in range(3):
        assert len({repr(x) for x in c[:, k].tolist()}) == len(RS.EDGE_COLOURS)
    p, o = PS.column_rays(0.02, 1)
    rs = _fused(p, o, c, 0.02, 0.06, True).unit_arrays()[3]
    assert set(np.unique(rs).tolist()) == set(RS.EDGE_U8)                       # (a column's band voxels take one ray each)
