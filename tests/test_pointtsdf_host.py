"""CPU: the restatement of the point-cloud TSDF fusion (tests/pointtsdf_restatement.py, the oracle of csrc/pointtsdf.hip)
against things that share nothing with it: the visited voxels sandwiched by an fp64 segment-against-cube test, the mean tsdf
against vdbfusion's float running average in fp64, a scanned sphere's mesh against the sphere, carving against a floater,
min_weight against exact counts; and the argument validation of ``PointTSDFVolume``, which has no CPU path."""
import numpy as np
import pytest
import torch

import pointtsdf_scenes as PS
from pointtsdf_restatement import RestatedPointTSDF, make_rays, walk

F = np.float32
MARGIN = 1e-3                              # voxels: ten times the 1e-4 at which the walk was first found inside both bounds


# ------------------------------------------------------------------------------------------------------------ the walk
@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("vs,offset", [(0.01, 0.0), (0.03, 0.0), (0.01, 4096.0 - 45.0), (0.02, -(4096.0 - 45.0))])
def test_visited_voxels_sandwiched_by_fp64_slab_test(vs, offset, carve):
    """Every visited voxel's cube grown by 1e-3 voxel meets the fp64 segment, and every voxel whose cube shrunk by 1e-3 meets
    the segment (its ends trimmed by 1e-3) is visited.  Random rays, rays along the axes, origins on voxel faces, voxel corners
    and unit corners, points on corners, exact diagonals; coordinates up to 4096 voxels from the origin.  No ray, no voxel is
    excluded."""
    trunc = 3 * vs
    p, o = PS.edge_rays(vs, n=320, offset=offset, seed=int(offset) % 7)
    assert np.abs(p / F(vs)).max() < 4097 and (offset == 0 or np.abs(p / F(vs)).max() > 4000)
    R = make_rays(p, o, vs, trunc, carve)
    assert len(R["index"]) == len(p)                                            # (every ray takes part)
    ray, g = walk(R)
    vsd, trd = float(F(vs)), float(F(trunc))
    outside = missed = n_inner = 0
    for i in range(len(p)):
        O, P = o[i].astype(np.float64), p[i].astype(np.float64)
        L = np.linalg.norm(P - O)
        dl = (P - O) / L / vsd
        s0, s1 = (0.0 if carve else max(L - trd, 0.0)), L + trd
        seen = g[ray == i]
        grown = PS.segment_meets_cubes(O / vsd + s0 * dl, O / vsd + s1 * dl, seen - MARGIN, seen + 1 + MARGIN)
        outside += int((~grown).sum())
        a, b = O / vsd + (s0 + MARGIN * vsd) * dl, O / vsd + (s1 - MARGIN * vsd) * dl
        lo, hi = np.floor(np.minimum(a, b)).astype(np.int64) - 1, np.floor(np.maximum(a, b)).astype(np.int64) + 1
        cand = np.stack(np.meshgrid(*[np.arange(lo[k], hi[k] + 1) for k in range(3)], indexing="ij"), -1).reshape(-1, 3)
        inner = cand[PS.segment_meets_cubes(a, b, cand + MARGIN, cand + 1 - MARGIN)]
        n_inner += len(inner)
        have = {tuple(v) for v in seen.tolist()}
        missed += sum(tuple(v) not in have for v in inner.tolist())
        assert len(have) == len(seen)                                           # (no voxel twice)
    print(f"visited {len(g)}, must-visit {n_inner}, outside the grown cubes {outside}, missed {missed}")
    assert n_inner > 2000 and outside == 0 and missed == 0


def test_skipped_rays():
    """A non-finite point or origin, a point at its origin and a coordinate beyond 2^22 voxels take no part."""
    p = np.array([[0.1, 0.2, 0.3], [np.nan, 0, 0], [0.5, 0.5, 0.5], [np.inf, 0, 0], [0.2, 0.1, 0.0], [1e6, 0, 0]], np.float32)
    o = np.array([[0.0, 0.0, 0.0], [0, 0, 0], [0.5, 0.5, 0.5], [0, 0, 0], [0, np.nan, 0], [0, 0, 0]], np.float32)
    R = make_rays(p, o, 0.01, 0.03, True)
    assert R["index"].tolist() == [0]


# -------------------------------------------------------------------------------------------------------- the mean tsdf
@pytest.mark.parametrize("carve", [True, False])
def test_mean_tsdf_against_float_running_average(carve):
    """vdbfusion's update with its default constant weight, tsdf' = (tsdf w + t) / (w + 1), w' = w + 1, in fp64 in ray order,
    from fp64 distances: the fixed-point mean is within sdf_trunc 2^-15 (half a step of the quantisation) plus the fp32
    rounding of the sdf, 8 eps32 of the largest coordinate difference involved (three subtractions, three squares, two sums and
    a root, each half an ulp of a value no larger than that).  Voxels where fp64 cannot tell which side of a rule a ray falls
    on (sdf within 1e-5 sdf_trunc of -sdf_trunc, or |dot| below 1e-9) are left out and counted."""
    vs, trunc = 0.02, 0.06
    rng = np.random.default_rng(5)
    n = 600
    p = (rng.uniform(-0.1, 0.1, (n, 3)) + [0.3, 0.1, -0.2]).astype(np.float32)
    o = np.array([-0.6, 0.4, 0.5], np.float32)
    r = RestatedPointTSDF(vs, trunc, carve)
    g, sdf32, ray = r.updates(p, o)
    r.integrate(p, o)
    U, sq, cnt, _, _ = r.unit_arrays()
    vsd, trd = float(F(vs)), float(F(trunc))
    c =((g.astype(np.float32) + F(0.5)) * F(vs)).astype(np.float64)           # the centres the operation states, exactly
    P, O = p[ray].astype(np.float64), o.astype(np.float64)
    dot = ((c - O) * (P - c)).sum(1)
    sdf = np.where(dot >= 0, 1.0, -1.0) * np.linalg.norm(P - c, axis=1)
    shaky = (np.abs(sdf + trd) < 1e-5 * trd) | (np.abs(dot) < 1e-9)
    mean, w, bad = {}, {}, set()
    for k in np.argsort(ray, kind="stable"):
        key = tuple(g[k])
        if shaky[k]:
            bad.add(key)
        if sdf[k] > -trd:
            t = min(trd, sdf[k])
            mean[key] = (mean.get(key, 0.0) * w.get(key, 0.0) + t) / (w.get(key, 0.0) + 1.0)
            w[key] = w.get(key, 0.0) + 1.0
    index = {tuple(u): k for k, u in enumerate(U)}
    tol = trd * 2.0 ** -15 + 8 * float(np.finfo(np.float32).eps) * float(np.abs(P - c).max())
    worst, n_cmp = 0.0, 0
    for key, m in mean.items():
        if key in bad:
            continue
        k, i = index[tuple(np.asarray(key) >> 4)], (key[0] & 15) | ((key[1] & 15) << 4) | ((key[2] & 15) << 8)
        assert cnt[k, i] == w[key]
        worst = max(worst, abs(float(sq[k, i]) / float(cnt[k, i]) / 16384.0 * trd - m))
        n_cmp += 1
    print(f"compared {n_cmp} voxels, left out {len(bad)}, worst {worst:.3e}, bound {tol:.3e}")
    assert n_cmp > 1000 and len(bad) < 0.01 * n_cmp and worst <= tol


# ------------------------------------------------------------------------------------------------------------ the scenes
@pytest.fixture(scope="module")
def scan():
    return PS.sphere_scan()


def _fuse(scan, carve, floater=None, vs=0.02, trunc=0.06):
    r = RestatedPointTSDF(vs, trunc, carve)
    if floater is not None:
        r.integrate(*floater[:3])
    for pts, origin, col in scan["views"]:
        r.integrate(pts, origin, col)
    return r


def test_sphere_scan_mesh_lies_on_the_sphere(scan):
    """A sphere of radius 0.5 scanned by 8 views of 48 x 36 at voxel 0.02: the vertices lie within one voxel of it."""
    r = _fuse(scan, True)
    v, f, c = r.extract_mesh(min_weight=1)
    dist = np.abs(np.linalg.norm(v.astype(np.float64) - scan["centre"], axis=1) - scan["radius"])
    print(f"{len(v)} vertices, {len(f)} triangles, worst distance {dist.max():.4f} (voxel 0.02)")
    assert len(f) > 3000 and dist.max() <= 0.02
    tex = PS.S.texture(v.astype(np.float64))
    assert np.abs(c - tex).mean() < 0.05                                        # colours are the scanned texture's


def test_carving_removes_a_floater(scan):
    """An isolated clump of points scanned first: without carving it stays in the mesh; with carving the later views, which
    see through it onto the sphere, remove it (a voxel's mean turns positive once the rays through it outnumber the points
    behind which it lies: the clump is sparse and close to view 0's camera, where that view's rays are dense)."""
    floater = PS.clump(scan)
    near = lambda v: int((np.linalg.norm(v.astype(np.float64) - floater[3], axis=1) < 0.08).sum())   # noqa: E731
    kept = _fuse(scan, False, floater).extract_mesh(min_weight=1)[0]
    carved = _fuse(scan, True, floater).extract_mesh(min_weight=1)[0]
    print(f"vertices near the clump: {near(kept)} without carving, {near(carved)} with")
    assert near(kept) >= 3 and near(carved) == 0


def test_min_weight_counts():
    """A voxel with count 4 yields no cell at min_weight 5 and one with count 5 does."""
    vs = 0.02
    for repeat, expect in ((4, False), (5, True)):
        p, o = PS.column_rays(vs, repeat)
        r = RestatedPointTSDF(vs, 3 * vs, True)
        r.integrate(p, o)
        cnt = r.unit_arrays()[2]
        assert set(np.unique(cnt).tolist()) == {0, repeat}
        v, f, _ = r.extract_mesh(min_weight=5)
        assert (len(f) > 0) == expect
        assert len(r.extract_mesh(min_weight=repeat)[1]) > 0


def test_order_and_split_do_not_reach_the_integers(scan):
    pts, origin, col = scan["views"][0]
    a = RestatedPointTSDF(0.02, 0.06, True)
    a.integrate(pts, origin, col)
    b = RestatedPointTSDF(0.02, 0.06, True)
    perm = np.random.default_rng(0).permutation(len(pts))
    for part in np.array_split(perm, 5):
        b.integrate(pts[part], origin, col[part])
    for x, y in zip(a.unit_arrays(), b.unit_arrays()):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------------------ arguments
def test_no_cpu_fallback_and_argument_validation():
    from collab_splats_amd import MisplatError, PointTSDFVolume
    with pytest.raises(MisplatError, match="no CPU fallback"):
        PointTSDFVolume(0.01, 0.03, device="cpu")
    for bad in ((0.0, 0.03), (0.01, -1.0), (float("nan"), 0.03), (0.01, float("inf"))):
        with pytest.raises(ValueError, match="voxel_size and sdf_trunc"):
            PointTSDFVolume(*bad, device="cuda")
    with pytest.raises(ValueError, match="bounds"):
        PointTSDFVolume(0.01, 0.03, bounds=[[0, 0, 0], [1, -1, 1]], device="cuda")
    vol = PointTSDFVolume(0.01, 0.03, device="cuda")                            # (construction touches no device)
    z = torch.zeros
    with pytest.raises(ValueError, match=r"points must be .*\(4, 2\)"):
        vol.integrate(z(4, 2), z(3))
    with pytest.raises(ValueError, match=r"origin must be .*\(2, 3\)"):
        vol.integrate(z(4, 3), z(2, 3))
    with pytest.raises(ValueError, match=r"colors must be .*\(4, 4\)"):
        vol.integrate(z(4, 3), z(3), z(4, 4))
    with pytest.raises(MisplatError):                                           # CPU tensors: no fallback
        vol.integrate(z(4, 3), z(3))
    with pytest.raises(ValueError, match=r"depth must be .*\(2, 3\)"):
        vol.integrate_depth(z(2, 3), z(1, 3, 4), z(1, 4))
    with pytest.raises(ValueError, match=r"c2w must be .*\(2, 3, 4\)"):
        vol.integrate_depth(z(1, 4, 4), z(2, 3, 4), z(1, 4))
    with pytest.raises(ValueError, match="min_weight"):
        vol.extract_mesh(min_weight=2.5)
    assert vol.n_units == 0 and vol.units()[0].shape == (0, 3)
