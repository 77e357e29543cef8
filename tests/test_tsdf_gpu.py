"""GPU: TSDF fusion and marching cubes (csrc/tsdf.hip) against the fp32 restatement (tests/tsdf_restatement.py): allocated
units equal, voxel grids bit-identical, meshes equal; a 1080p sphere fused into a watertight, deterministic mesh; the
RaDe-GS model's batched extract_mesh equal to the reference's one-view-at-a-time loop."""
import numpy as np
import pytest
import torch

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
