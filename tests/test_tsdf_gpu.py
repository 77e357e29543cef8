"""GPU: TSDF fusion and marching cubes (csrc/tsdf.hip) against the fp32 restatement (tests/tsdf_restatement.py): allocated
units equal, voxel grids bit-identical, meshes equal; a 1080p sphere fused into a watertight, deterministic mesh; the
RaDe-GS model's batched extract_mesh equal to the reference's one-view-at-a-time loop.  Marching cubes alone on random
fields laid into the pool (all 256 configurations, unit seams, map borders, zeros, > 1024 units and > 1024 map blocks), held
against the restatement and against fp64 references that share nothing with it (tests/tsdf_fields.py); fusion from cameras
inside a room (off-centre, anisotropic, 65 views, far from the origin, tiny and odd images), depth and colour thresholds."""
import numpy as np
import pytest
import torch

import tsdf_fields as F_
import tsdf_scenes as S
from tsdf_restatement import RestatedTSDF

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _scene(name):
    if name == "sphere":
        d, vm, K, rgb = S.sphere_views(40, 96, 72)
        return dict(vs=0.02, trunc=0.06, dtrunc=3.0, d=d, vm=vm, K=K, rgb=rgb, mask=None, bounds=None)
    if name == "box":
        d, vm, K, rgb = S.box_views(40, 96, 72)
        return dict(vs=0.015, trunc=0.045, dtrunc=3.0, d=d, vm=vm, K=K, rgb=rgb, mask=None, bounds=None)
    if name == "plane":                     # masks cut discs out; depth_trunc cuts the far part of every view (holes)
        d, vm, K, rgb, mask = S.plane_views(40, 96, 72)
        return dict(vs=0.02, trunc=0.05, dtrunc=0.9, d=d, vm=vm, K=K, rgb=rgb, mask=mask, bounds=None)
    if name == "sphere_bounded":            # caller's bounds cut the sphere in half
        d, vm, K, rgb = S.sphere_views(40, 96, 72)
        return dict(vs=0.02, trunc=0.06, dtrunc=3.0, d=d, vm=vm, K=K, rgb=rgb, mask=None,
                    bounds=[[-1.0, -1.0, -1.0], [0.1, 1.0, 1.0]])
    raise KeyError(name)


def _fuse_gpu(sc, batch):
    from collab_splats_amd import TSDFVolume
    vol = TSDFVolume(sc["vs"], sc["trunc"], sc["dtrunc"], bounds=sc["bounds"], device=DEV)
    V = sc["d"].shape[0]
    for b in range(0, V, batch):
        sl = slice(b, b + batch)
        vol.integrate(_t(sc["d"][sl]), _t(sc["vm"][sl]), _t(sc["K"][sl]), _t(sc["rgb"][sl]),
                      None if sc["mask"] is None else _t(sc["mask"][sl]))
    return vol


def _fuse_ref(sc):
    r = RestatedTSDF(sc["vs"], sc["trunc"], sc["dtrunc"], bounds=sc["bounds"])
    r.integrate(sc["d"], sc["vm"], sc["K"], sc["rgb"], sc["mask"])
    return r


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0 and b.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _check_volume_and_mesh(vol, ref):
    cg, tg, wg, rg = vol.units()
    cr, tr, wr, rr = ref.unit_arrays()
    assert np.array_equal(cg, cr), f"allocated units differ: {len(cg)} vs {len(cr)}"
    for name, g, r in (("tsdf", tg, tr), ("w", wg, wr), ("rgb", rg, rr)):
        if not _same_bits(g, r):
            bad = np.argwhere(np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(r).view(np.uint32))
            raise AssertionError(f"{name} not bit-identical at {len(bad)} entries, first {bad[:3].tolist()}: "
                                 f"{g[tuple(bad[0])]} vs {r[tuple(bad[0])]}")
    v, f, c = (x.cpu().numpy() for x in vol.extract_mesh())
    vr, fr, cr_ = ref.extract_mesh()
    assert f.dtype == np.int32 and np.array_equal(f, fr)
    assert v.shape == vr.shape and _rel(v, vr) <= 1e-6 and _rel(c, cr_) <= 1e-6
    return v, f


_REF = {}                                   # restatement per scene (batching does not change it)


@pytest.mark.parametrize("batch", [1, 3, 64])
@pytest.mark.parametrize("name", ["sphere", "box", "plane", "sphere_bounded"])
def test_fusion_bit_identical_to_restatement(name, batch):
    sc = _scene(name)
    if name not in _REF:
        _REF[name] = _fuse_ref(sc)
    vol = _fuse_gpu(sc, batch)
    v, f = _check_volume_and_mesh(vol, _REF[name])
    assert len(f) > 100


def _closed(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    return bool(np.all(cnt == 2)), len(cnt)


def test_1080p_sphere_watertight_and_deterministic():
    from collab_splats_amd import TSDFVolume
    centre, radius, vs = (0.1, -0.05, 0.2), 0.3, 0.01
    d, vm, K, rgb = S.sphere_views(100, 1920, 1080, centre=centre, radius=radius)
    outs = []
    for _ in range(2):
        vol = TSDFVolume(vs, 0.03, 1.0, device=DEV)
        vol.integrate(_t(d), _t(vm), _t(K), _t(rgb))
        outs.append([x.cpu().numpy() for x in vol.extract_mesh()])
    (v, f, c), (v2, f2, c2) = outs
    assert _same_bits(v, v2) and np.array_equal(f, f2) and _same_bits(c, c2), "two runs differ"
    closed, n_edges = _closed(f)
    assert closed and len(v) - n_edges + len(f) == 2
    assert len(np.unique(f)) == len(v), "unreferenced vertices"
    assert len(np.unique(v, axis=0)) == len(v), "duplicate vertices"
    dist = np.abs(np.linalg.norm(v.astype(np.float64) - np.asarray(centre), axis=1) - radius)
    assert dist.max() <= vs
    assert np.all((c >= 0) & (c <= 1))


def test_all_zero_depth_gives_empty_mesh():
    from collab_splats_amd import TSDFVolume
    d, vm, K, rgb = S.sphere_views(4, 64, 48)
    vol = TSDFVolume(0.02, 0.06, 3.0, device=DEV)
    vol.integrate(_t(np.zeros_like(d)), _t(vm), _t(K), _t(rgb))
    v, f, c = vol.extract_mesh()
    assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3) and vol.n_units == 0
    v, f, c = TSDFVolume(0.02, 0.06, device=DEV).extract_mesh()                  # never integrated
    assert v.shape == (0, 3) and f.dtype == torch.int32


def test_unit_cap_raises():
    from collab_splats_amd import MisplatError, TSDFVolume
    d, vm, K, rgb = S.sphere_views(2, 64, 48)
    vol = TSDFVolume(0.002, 0.006, 3.0, device=DEV, max_units=1000)
    with pytest.raises(MisplatError, match="cap"):
        vol.integrate(_t(d), _t(vm), _t(K))


class _Box:
    """nerfstudio OrientedBox duck-type: R, T, S and within()."""

    def __init__(self, T, S_):
        self.R, self.T, self.S = torch.eye(3), torch.tensor(T), torch.tensor(S_)

    def within(self, pts):
        lo, hi = (self.T - self.S / 2).to(pts.device), (self.T + self.S / 2).to(pts.device)
        return ((pts >= lo) & (pts <= hi)).all(-1, keepdim=True)


@pytest.mark.parametrize("crop", [False, True])
def test_radegs_extract_mesh_equals_per_view_loop(crop):
    """mesh.py:1572-1630: one get_outputs_for_camera per view, each integrated alone, against the batched path."""
    from collab_splats_amd import TSDFVolume
    from collab_splats_amd.tsdf import camera_frame, obb_bounds
    model = S.sphere_gaussians(60000).to(DEV)
    model.eval()
    W, H = 160, 120
    _, vms, Ks, _ = S.sphere_views(10, 8, 8)
    K = S.intrinsics(W, H, 60.0)
    cams = [S.pinhole_camera(M, K, W, H) for M in vms]
    box = _Box([0.1, -0.05, 0.35], [1.0, 1.0, 0.4]) if crop else None
    vs, tr, dt = 0.01, 0.03, 1.0
    vol = TSDFVolume(vs, tr, dt, bounds=obb_bounds(box, tr), device=DEV)
    for cam in cams:
        out = model.get_outputs_for_camera(cam, obb_box=box)
        vm, Kc = camera_frame(cam)
        vol.integrate(out["median_depth"][None], vm[None].to(DEV), Kc[None].to(DEV), out["rgb"][None])
    v_ref, f_ref, c_ref = (x.cpu().numpy() for x in vol.extract_mesh())
    v, f, c = (x.cpu().numpy() for x in model.extract_mesh(cams, voxel_size=vs, sdf_trunc=tr, depth_trunc=dt, obb_box=box,
                                                           batch_size=4))
    assert len(f_ref) > 1000
    assert np.array_equal(f, f_ref) and _same_bits(v, v_ref) and _same_bits(c, c_ref)


# ---------------------------------------------------------------------------------------- marching cubes on injected fields
def _inject(field, vs, perm=None, lo=None, dims=None, spare=3):
    """A TSDFVolume holding ``field`` ({unit: [5,4096]}) as integrate() could have left it: the units of the field take the
    pool slots perm[k] (k: the unit's rank in map order; a permutation of 0..n-1), the map covers lo .. lo + dims - 1
    (default: the field's bounding box) and the pool has ``spare`` unused slots behind the n in use."""
    from collab_splats_amd import TSDFVolume
    U = np.array(sorted(field, key=lambda c: (c[2], c[1], c[0])), np.int64)
    n = len(U)
    lo = U.min(0) if lo is None else np.asarray(lo, np.int64)
    dims = U.max(0) - lo + 1 if dims is None else np.asarray(dims, np.int64)
    assert np.all(U >= lo) and np.all(U < lo + dims)
    perm = np.arange(n) if perm is None else np.asarray(perm, np.int64)
    assert np.array_equal(np.sort(perm), np.arange(n))
    m = (U[:, 0] - lo[0]) + dims[0] * ((U[:, 1] - lo[1]) + dims[1] * (U[:, 2] - lo[2]))
    slot_map = np.full(int(np.prod(dims)), -1, np.int32)
    slot_map[m] = perm
    pool = np.zeros((n + spare, 5, 4096), np.float32)
    pool[perm] = np.stack([field[tuple(u)] for u in U])
    vol = TSDFVolume(vs, 3 * vs, 3.0, device=DEV)
    vol.lo, vol.dims = lo.astype(np.int64), dims.astype(np.int64)
    vol._slot_map, vol._pool, vol.n_units = _t(slot_map), _t(pool), n
    return vol


def _mc_field(name):
    """(field, voxel size, closed, _inject keywords) of one injected field."""
    if name in ("block", "block_less_one"):           # 2 x 2 x 2 units from a negative coordinate: every configuration,
        field = F_.random_field(F_.block((-1, -2, 3), (2, 2, 2)), seed=11, p_neg=0.5, closed=True)     # cells across unit
        if name == "block_less_one":                  # faces, unit edges and the block's centre corner
            del field[(0, -2, 4)]                     # unallocated neighbours: an open surface
        return field, 0.013, name == "block", {}
    if name == "edge_and_corner":                     # units that meet along an edge ((0,0,0)-(1,1,0)) and at a corner
        return F_.random_field([(0, 0, 0), (1, 1, 0), (2, 2, 1)], seed=4, p_neg=0.5), 0.02, False, {}
    if name == "zeros":
        return F_.random_field(F_.block((0, 0, 0), (2, 1, 1)), seed=3, p_neg=0.4, w0=0.05, zeros=0.02), 0.02, False, {}
    if name == "positive":
        return F_.random_field([(1, 0, 0), (2, 0, 0)], seed=5, p_neg=0.0), 0.02, False, {}
    if name == "negative":
        return F_.random_field([(1, 0, 0), (2, 0, 0)], seed=6, p_neg=1.0), 0.02, False, {}
    if name == "map_corner_lo":                       # gx - 1 leaves the map; gx + 16 stays inside it, unallocated
        return F_.random_field([(3, -2, 7)], seed=7, p_neg=0.5), 0.02, False, dict(lo=(3, -2, 7), dims=(3, 2, 2))
    if name == "map_corner_hi":                       # gx + 16 leaves the map
        return F_.random_field([(5, -1, 8)], seed=8, p_neg=0.5), 0.02, False, dict(lo=(3, -2, 7), dims=(3, 2, 2))
    raise KeyError(name)


def _restated_mesh(field, vs):
    r = RestatedTSDF(vs, 3 * vs)
    r.units = {u: d.copy() for u, d in field.items()}
    return r.extract_mesh()


def _mesh(vol):
    return tuple(x.cpu().numpy() for x in vol.extract_mesh())


@pytest.mark.parametrize("name", ["block", "block_less_one", "edge_and_corner", "zeros", "positive", "negative",
                                  "map_corner_lo", "map_corner_hi"])
def test_marching_cubes_of_injected_field(name):
    """extract_mesh() on a field laid into the pool: equal to the restatement's mesh, on the fp64 vertex and colour rule, and
    (closed fields) closed, consistently oriented and winding once around exactly the negative voxels."""
    field, vs, closed, kw = _mc_field(name)
    cfg = F_.configurations(field)
    if name == "block":
        assert np.all(cfg > 0), f"configurations never taken: {np.flatnonzero(cfg == 0).tolist()}"
    if name == "zeros":
        plus, minus = F_.zeros_next_to_negatives(field)
        assert plus > 0 and minus > 0, "no +0.0 / -0.0 next to a negative voxel"
        assert any((d[1] == 0).any() for d in field.values())
    n = len(field)
    vol = _inject(field, vs, perm=np.random.default_rng(1).permutation(n), **kw)
    v, f, c = _mesh(vol)
    vr, fr, cr = _restated_mesh(field, vs)
    assert f.dtype == np.int32 and f.shape == fr.shape and np.array_equal(f, fr)
    assert v.shape == vr.shape and _rel(v, vr) <= 1e-6 and _rel(c, cr) <= 1e-6
    if name in ("positive", "negative"):
        assert cfg[0 if name == "positive" else 255] == cfg.sum() > 0
        assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3)
        return
    assert len(f) > 1000
    F_.check_vertices(field, vs, v, c)
    if closed:
        F_.check_directed_edges(f, len(v))
        F_.check_winding(field, vs, v, f, n=600, seed=5)


def test_slot_order_reaches_no_result():
    field, vs, _, _ = _mc_field("block")
    a = _mesh(_inject(field, vs, perm=np.arange(8)))
    b = _mesh(_inject(field, vs, perm=np.array([5, 2, 7, 0, 3, 6, 1, 4]), spare=9))
    assert len(a[1]) > 50000
    assert _same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and _same_bits(a[2], b[2])


def test_tsdf_and_poisson_front_ends_extract_the_same_mesh():
    """One closed 8-unit field through both callers of unitvolume.marching_cubes: TSDFVolume (the order found by
    misplat_tsdf_order under a random slot permutation) and poisson._extract (chi laid into the pool by misplat_poisson_mc_pool,
    order = the identity slot map).  Voxel size 1, origin 0, h 1 and iso 0.0 make both lattices the same: voxel g at g + 0.5
    (0 + v * 1.0 and chi - 0.0 are exact), so vertices and triangles are equal bit for bit; colours are not compared (the
    Poisson pool carries none)."""
    from collab_splats_amd import poisson
    field = F_.random_field(F_.block((0, 0, 0), (2, 2, 2)), p_neg=0.5, closed=True)
    for d in field.values():
        d[1] = 1.0
    v, f, _ = _mesh(_inject(field, 1.0, perm=np.random.default_rng(3).permutation(8), lo=(0, 0, 0)))
    chi = _t(F_.Dense(field).tsdf.transpose(2, 1, 0))                              # [z, y, x]
    assert chi.shape == (32, 32, 32)
    pv, pf, _, _ = poisson._extract(chi, 0.0, 5, np.zeros(3, np.float32), np.float32(1.0), torch.zeros_like(chi), None)
    assert len(f) > 1000
    assert pf.dtype == torch.int32 and np.array_equal(pf.cpu().numpy(), f)
    assert _same_bits(pv.cpu().numpy(), v)


def test_marching_cubes_over_more_than_1024_units():
    """A slab of 41 x 25 x 1 units: the per-unit vertex and triangle counts take a second trip of the one-workgroup scan.
    (Restating the slab takes 5 s and 2.6 GB of host memory, so the mesh is held against the independent references: the
    ordered fp64 vertex rule, which a wrong unit offset shifts, the directed-edge rule, which a wrong triangle offset or
    vertex base breaks, and the table's triangle total over the valid cells.)"""
    from collab_splats_amd import mc_tables as mc
    vs = 0.01
    field = F_.random_field(F_.block((-20, -12, 2), (41, 25, 1)), seed=2, p_neg=0.003, closed=True)
    assert len(field) == 1025
    vol = _inject(field, vs, perm=np.random.default_rng(3).permutation(1025))
    v, f, c = _mesh(vol)
    assert len(f) == F_.triangle_total(field, mc.tables()[0]) and len(f) > 50000
    F_.check_vertices(field, vs, v, c)
    F_.check_directed_edges(f, len(v))
    first_of_last = np.array([20 * 16, 12 * 16, 2 * 16]) * np.float32(vs)        # the 1025th unit's vertices are there
    assert np.all(v[-1] > first_of_last)


def test_order_beyond_1024_map_blocks():
    """misplat_tsdf_order over a map of 1028 blocks of 4096 entries: the scan of the block counts takes a second trip."""
    import ctypes as C
    from collab_splats_amd._lib import check, load, ptr, stream_ptr
    from collab_splats_amd.tsdf import Grid
    dims = (129, 128, 255)
    n_map = int(np.prod(dims))
    nb = (n_map + 4095) // 4096
    assert nb > 1024 and n_map > 4096 * 1024
    edge = 4096 * 1024
    rng = np.random.default_rng(0)
    idx = np.unique(np.concatenate([[0, 1, 15, 16, 4095, 4096, n_map - 1, n_map - 2, edge - 4096, edge - 17, edge - 1, edge,
                                     edge + 1, edge + 4095, edge + 4096, 4096 * (nb - 1), 4096 * (nb - 1) - 1],
                                    rng.integers(0, edge, 24), rng.integers(edge, n_map, 12)])).astype(np.int64)
    n = len(idx)
    assert (idx < edge).sum() > 20 and (idx >= edge).sum() > 10
    slot_map = np.full(n_map, -1, np.int32)
    slot_map[idx] = rng.permutation(n)
    grid = Grid(0.01, 0.03, 3.0)
    grid.lo[:] = [-60, -64, -100]
    grid.dims[:] = dims
    sm = _t(slot_map)
    scratch = torch.empty(2 * nb + 1, dtype=torch.int32, device=DEV)             # the sizes extract_mesh allocates
    order = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    check(load().misplat_tsdf_order(C.byref(grid), ptr(sm), ptr(scratch), ptr(order), stream_ptr()), "misplat_tsdf_order")
    assert np.array_equal(order.cpu().numpy().astype(np.int64), idx)
    assert int(scratch[2 * nb].item()) == n


# ------------------------------------------------------------------------------------------- fusion from inside a room
_K33 = (30.0, 22.0, 13.3, 12.1)                       # fx != fy, principal point off the centre of 33 x 21


def _room(name):
    p = dict(room65=dict(n=65, W=33, H=21, K=_K33, vs=0.02, trunc=0.06, dtrunc=0.7),
             room_far=dict(n=12, W=33, H=21, K=_K33, vs=0.02, trunc=0.06, dtrunc=0.7, offset=(300.0, -200.0, 150.0)),
             room5x3=dict(n=7, W=5, H=3, K=(4.5, 3.3, 2.2, 1.7), vs=0.03, trunc=0.09, dtrunc=0.7),
             room1x1=dict(n=9, W=1, H=1, K=(0.9, 0.8, 0.45, 0.55), vs=0.03, trunc=0.09, dtrunc=3.0),
             room97=dict(n=3, W=97, H=73, K=(88.0, 65.0, 39.1, 41.7), vs=0.02, trunc=0.06, dtrunc=0.7),
             room7=dict(n=7, W=33, H=21, K=_K33, vs=0.02, trunc=0.06, dtrunc=0.7))[name]
    d, vm, K, rgb = S.room_views(p["n"], p["W"], p["H"], p["K"], offset=p.get("offset", (0.0, 0.0, 0.0)))
    return dict(vs=p["vs"], trunc=p["trunc"], dtrunc=p["dtrunc"], d=d, vm=vm, K=K, rgb=rgb, mask=None, bounds=None)


def _assert_reach(sc, views):
    """The views meet voxels behind the camera, off all four image sides and in the first half pixel."""
    reach = S.projection_reach(RestatedTSDF(sc["vs"], sc["trunc"], sc["dtrunc"], bounds=sc["bounds"]), sc["d"], sc["vm"],
                               sc["K"], views)
    assert all(n > 0 for n in reach.values()), reach


@pytest.mark.parametrize("name,batch", [("room65", 65), ("room65", 1), ("room_far", 12), ("room5x3", 7), ("room1x1", 9),
                                        ("room97", 3)])
def test_room_fusion_bit_identical_to_restatement(name, batch):
    """Cameras inside the volume with fx != fy and an off-centre principal point: 65 views in one call (view 63 takes the top
    bit of the view word, view 64 a second batch) and in 65 calls; a scene 400 m from the origin; images smaller than the
    sample step; a width of 4 k + 1 with hundreds of samples per view."""
    sc = _room(name)
    if name not in _REF:
        _REF[name] = _fuse_ref(sc)
    V, H, W = sc["d"].shape[:3]
    _assert_reach(sc, sorted({0, V // 3, 2 * V // 3, V - 2, V - 1}))
    r = RestatedTSDF(sc["vs"], sc["trunc"], sc["dtrunc"])
    if name == "room65":
        assert V == 65 and len(r.touched_units(sc["d"][63, ..., 0], sc["vm"][63], sc["K"][63])) > 0, "bit 63 stays clear"
        assert len(r.touched_units(sc["d"][64, ..., 0], sc["vm"][64], sc["K"][64])) > 0
        assert (sc["d"] > np.float32(sc["dtrunc"])).sum() > 1000
    if name == "room_far":
        assert _REF[name].unit_arrays()[0].min(0)[0] > 900
    if name == "room97":
        assert W % 4 == 1 and ((W + 3) // 4) * ((H + 3) // 4) > 4 * 64
    if name in ("room5x3", "room1x1"):
        assert W < 8 and H < 4
    vol = _fuse_gpu(sc, batch)
    v, f = _check_volume_and_mesh(vol, _REF[name])
    assert len(f) > 1000 and vol.n_units > 15


_SPECIAL_SAMPLED = [(4, 4), (8, 4), (12, 4), (16, 8), (20, 8), (24, 12), (28, 12)]          # (u, v), both multiples of 4
_SPECIAL_UNSAMPLED = [(5, 5), (9, 6), (13, 7), (18, 9), (22, 10), (26, 13), (30, 14)]


def test_depth_specials_and_the_depth_threshold():
    """0, a negative depth, NaN, +inf and the float above depth_trunc are no data; depth_trunc itself and 1e-30 are data --
    at sampled pixels (allocation and integration) and at unsampled ones (integration alone)."""
    sc = _room("room7")
    dt = np.float32(sc["dtrunc"])
    values = [np.float32(0), np.float32(-0.5), np.float32(np.nan), np.float32(np.inf), dt, np.nextafter(dt, np.float32(np.inf)),
              np.float32(1e-30)]
    d = sc["d"].copy()
    for pos in (_SPECIAL_SAMPLED, _SPECIAL_UNSAMPLED):
        for (u, v), x in zip(pos, values):
            d[2, v, u, 0] = x
    assert all(u % 4 == 0 and v % 4 == 0 for u, v in _SPECIAL_SAMPLED)
    assert all(u % 4 != 0 and v % 4 != 0 for u, v in _SPECIAL_UNSAMPLED)
    sc["d"] = d
    ref = _fuse_ref(sc)
    for pos in (_SPECIAL_SAMPLED[4:5], _SPECIAL_UNSAMPLED[4:5]):                 # the threshold is under test: dropping the
        (u, v), = pos                                                            # pixel equal to depth_trunc changes the volume
        d0 = d.copy()
        assert d0[2, v, u, 0] == dt
        d0[2, v, u, 0] = 0
        other = _fuse_ref(dict(sc, d=d0))
        a, b = ref.unit_arrays(), other.unit_arrays()
        assert not (np.array_equal(a[0], b[0]) and _same_bits(a[2], b[2])), f"depth_trunc at pixel {(u, v)} reaches no voxel"
    _assert_reach(sc, range(7))
    _check_volume_and_mesh(_fuse_gpu(sc, 7), ref)
    _check_volume_and_mesh(_fuse_gpu(sc, 1), ref)


def test_colour_specials():
    """Colours at and outside [0, 1] and at the truncation's steps: uint8(rgb * 255), truncated, clamped."""
    sc = _room("room7")
    specials = np.array([0.0, 1.0, 0.999999, 1.5, -0.2] + [(k + 0.5) / 255 for k in (0, 1, 37, 127, 128, 253, 254)]
                        + [k / 255 for k in (1, 85, 254)], np.float32)
    rng = np.random.default_rng(4)
    rgb = sc["rgb"].copy()
    pick = rng.random(rgb.shape) < 0.5
    rgb[pick] = specials[rng.integers(0, len(specials), int(pick.sum()))]
    sc["rgb"] = rgb
    ref = _fuse_ref(sc)
    colours = ref.unit_arrays()[3]
    assert (colours == 255).any() and (colours == 0).any()
    _assert_reach(sc, range(7))
    _check_volume_and_mesh(_fuse_gpu(sc, 7), ref)


def test_calls_alternate_between_colour_and_none():
    sc = _room("room7")
    from collab_splats_amd import TSDFVolume
    vol = TSDFVolume(sc["vs"], sc["trunc"], sc["dtrunc"], device=DEV)
    ref = RestatedTSDF(sc["vs"], sc["trunc"], sc["dtrunc"])
    for k, b in enumerate(range(0, 7, 2)):
        sl = slice(b, b + 2)
        vol.integrate(_t(sc["d"][sl]), _t(sc["vm"][sl]), _t(sc["K"][sl]), None if k % 2 else _t(sc["rgb"][sl]))
        ref.integrate(sc["d"][sl], sc["vm"][sl], sc["K"][sl], None if k % 2 else sc["rgb"][sl])
    _assert_reach(sc, range(7))
    _check_volume_and_mesh(vol, ref)


@pytest.mark.parametrize("kind", ["outside", "cut"])
def test_room_under_bounds(kind):
    """Bounds that exclude every view leave no unit and an empty mesh; bounds through the room cut the volume."""
    sc = _room("room7")
    whole = len(_fuse_ref(sc).units)
    sc["bounds"] = [[5.0, 5.0, 5.0], [6.0, 6.0, 6.0]] if kind == "outside" else [[-1.0, -1.0, -1.0], [0.05, 1.0, 0.1]]
    ref = _fuse_ref(sc)
    vol = _fuse_gpu(sc, 3)
    v, f = _check_volume_and_mesh(vol, ref)
    if kind == "outside":
        assert vol.n_units == 0 and len(ref.units) == 0 and v.shape == (0, 3) and f.shape == (0, 3)
    else:
        _assert_reach(sc, range(7))
        assert 0 < vol.n_units < whole and len(f) > 300
