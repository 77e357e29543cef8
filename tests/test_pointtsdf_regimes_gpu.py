"""GPU: point-cloud TSDF fusion (csrc/pointtsdf.hip) off its one voxel size and at workload scale, on the scenes of
tests/pointtsdf_regimes_scenes.py, against the numpy restatement -- the plain walk of every ray, with no
map, no lists and no re-entry.  The comparison rule is test_pointtsdf_gpu.py's: the allocated unit coordinates equal; sum_q,
count, rgb_sum and rgb_count equal, integer for integer; where a mesh is compared the triangles equal, vertices and colours to
1e-6.  After a single ``integrate`` call ``n_pairs`` equals the distinct (ray, unit) pairs of the restatement's walk after its
clip: the first direct check of the list layer's count / emit sink under this path."""
import numpy as np
import pytest

import pointtsdf_regimes_scenes as RS
import pointtsdf_scenes as PS
from test_pointtsdf_gpu import _both, _check, _same_units, _t, _volume

pytestmark = pytest.mark.gpu


def _one_call(p, o, c, vs, trunc, carve, bounds=None, mesh=True):
    """One ``integrate`` call into a fresh volume: integers, pair count and, with ``mesh``, the mesh.  (vol, ref)"""
    vol, ref = _volume(carve, bounds, vs, trunc)
    _both(vol, ref, p, o, c)
    want = RS.pair_count(p, o, vs, trunc, carve, bounds)
    n_tri = len(_check(vol, ref)[1]) if mesh else None
    if not mesh:
        _same_units(vol.units(), ref.unit_arrays())
    print(f"{vol.n_units} units, {vol.n_pairs} pairs (restatement {want}), {int(ref.unit_arrays()[2].sum())} updates"
          + ("" if n_tri is None else f", {n_tri} triangles"))
    assert vol.n_units == len(ref.units) and vol.n_pairs == want > 0
    return vol, ref


# ------------------------------------------------------------------------------------- 1: voxel size x truncation
@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("vs,trunc", RS.VOXEL_TRUNC)
def test_voxel_sizes_and_truncations(vs, trunc, carve):
    """The edge-case bundle at the workload's (0.01, 0.03), a band thinner than a voxel (0.02, 0.01), one of 25 voxels, wider
    than a unit (0.02, 0.5), neither a round number (0.013, 0.0377), and (0.25, 0.75): the sdf arithmetic
    rintf((fminf(trunc, sdf) / trunc) * 16384) and the band test off the one pair of the other tests."""
    _one_call(*RS.bundle(vs), vs, trunc, carve)


# --------------------------------------------------------------------------------- 2: a sphere at the workload's voxel
@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("shifted", [False, True])
def test_workload_sphere(shifted, carve):
    """8 views of 48 x 36 of a sphere of radius 0.25 at voxel 0.01, a call per view; as it is and translated by (37.3, -52.1,
    18.7) m, up to 5210 voxels out: integers and mesh, the mesh within one voxel of the sphere."""
    sc = RS.scan(shifted)
    vol, _ = _volume(carve, None, *RS.WORK)
    for p, o, c in sc["views"]:
        vol.integrate(_t(p), _t(o), _t(c))
    ref = RS.restated_scan(shifted, carve)
    v, f = _check(vol, ref)
    worst = RS.off_sphere(v, sc) / RS.WORK[0]
    print(f"{vol.n_units} units, {vol.n_pairs} pairs, {len(f)} triangles, worst distance {worst:.3f} voxels")
    assert vol.n_units == len(ref.units) and len(f) > 10000 and worst <= 1.0


# ------------------------------------------------------------------------------------------------------- 3: far out
@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("offset", RS.OFFSETS)
def test_far_out(offset, carve):
    """The edge-case bundle 4051, 1e5 - 0.5, 2e6 and 4e6 voxels from the world origin at voxel 0.01 (the last at the 2^22 skip
    rule, where lattice coordinates keep half a voxel): integers and pair count."""
    _one_call(*RS.bundle(RS.WORK[0], offset), *RS.WORK, carve, mesh=False)


# ------------------------------------------------------------------------------------------------------ 4: long rays
@pytest.mark.parametrize("carve", [True, False])
def test_long_rays(carve):
    """16 rays of 400 to 700 voxels, an origin per point: with carving a ray is listed under 40 units and more; without, the
    walk starts at floorf(ol + s0 dl) hundreds of voxels from the origin."""
    p, o = RS.long_rays()
    _one_call(p, o, None, *RS.WORK, carve, mesh=False)


# ------------------------------------------------------------------------------------------------ 5: the map's padding
@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("offset", [0.0, RS.PAD_OFFSET])
def test_map_padding(offset, carve):
    """Rays that leave the box of their points and origins only within the fp32 padding of ``_box_units``; at offset 2^21
    voxels one fp32 step of a world coordinate is a fifth of a voxel.  The restatement has no map: a unit that the map clipped
    would be missing here."""
    p, o, second = RS.padding_rays(carve, offset)
    _one_call(p, o, None, *RS.WORK, carve, mesh=False)
    if carve:                                   # the rays with their origin at a face alone: only the origins' padding reaches out
        _one_call(p[second], o[second], None, *RS.WORK, carve, mesh=False)


# -------------------------------------------------------------------------------------- 6: bounds through every face
@pytest.mark.parametrize("carve", [True, False])
def test_bounds_through_every_face(carve):
    """640 rays and a bounds box strictly inside them that is aligned to no unit: rays enter the map through every face,
    start inside it and miss it.  A second bundle into the same volume."""
    box = RS.bounds_box()
    vol, ref = _one_call(*RS.bounds_bundle(0), RS.BOUNDS_VS, 0.06, carve, bounds=box)
    first = vol.n_pairs
    p, o, c = RS.bounds_bundle(1)
    _both(vol, ref, p, o, c)
    _check(vol, ref)
    assert vol.n_pairs - first == RS.pair_count(p, o, RS.BOUNDS_VS, 0.06, carve, box)
    coords = vol.units()[0]
    assert coords.min() == -1 and coords.max() == 0


# --------------------------------------------------------------------------------- 7: pieces of the accumulate kernel
@pytest.mark.parametrize("n", RS.FANS)
def test_piece_boundaries_of_the_accumulate_kernel(n):
    """The fan with 8192, 8193 and 16384 rays: the origin's unit list is exactly one full piece (flushed with plain loads and
    stores), a full piece and a piece of one ray, exactly two full pieces (both flushed with atomics).  With 8193 the fan
    goes in a second time: every flush adds to what is there."""
    p, o, c = PS.fan(RS.FAN_VS, n)
    vol, ref = _one_call(p, o, c, RS.FAN_VS, RS.FAN_TRUNC, True, mesh=False)
    times = 1
    if n == RS.PIECE + 1:
        _both(vol, ref, p, o, c)
        _same_units(vol.units(), ref.unit_arrays())
        times = 2
    coords, sum_q, count = vol.units()[:3]
    k = int(np.nonzero((coords == 0).all(1))[0][0])
    assert count[k, RS.FAN_VOXEL] == times * n and sum_q[k, RS.FAN_VOXEL] == times * n * 16384


def test_plain_flush_adds_to_what_is_there():
    """8192 rays twice into one volume: both calls flush the origin's unit with plain loads and stores."""
    p, o, c = PS.fan(RS.FAN_VS, RS.PIECE)
    vol, ref = _volume(True, None, RS.FAN_VS, RS.FAN_TRUNC)
    for _ in range(2):
        _both(vol, ref, p, o, c)
    _same_units(vol.units(), ref.unit_arrays())


# ------------------------------------------------------------------------------------- 8: colours at the cast's edges
def test_colours_at_the_casts_edges():
    """-0.5, 0, 0.5 / 255, 1 / 255, 0.999999, 1, 1.5, NaN, +inf, -inf in every channel: to_u8 truncates, clamps to 0 .. 255 and
    sends NaN to 0, as the restatement's u8."""
    p, o = PS.column_rays(0.02, 1)
    vol, ref = _one_call(p, o, RS.edge_colours(len(p)), 0.02, 0.06, True, mesh=False)
    assert set(np.unique(vol.units()[3]).tolist()) == set(RS.EDGE_U8)


# --------------------------------------------------------------------------------- 9: one origin or an origin per point
@pytest.mark.parametrize("carve", [True, False])
def test_one_origin_equals_an_origin_per_point(carve):
    """The bundle of (0.01, 0.03) from one shared origin, given as [3] and expanded to [P,3]: every plane identical."""
    p, _, c = RS.bundle(RS.WORK[0])
    o = (np.float32([1.3, -2.6, 0.7]) * np.float32(RS.WORK[0])).astype(np.float32)
    vol, ref = _one_call(p, o, c, *RS.WORK, carve, mesh=False)
    per_point, _ = _volume(carve, None, *RS.WORK)
    per_point.integrate(_t(p), _t(np.ascontiguousarray(np.broadcast_to(o, p.shape))), _t(c))
    _same_units(per_point.units(), vol.units())
    assert per_point.n_pairs == vol.n_pairs
