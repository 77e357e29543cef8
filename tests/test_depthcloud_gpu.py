"""GPU: oriented point clouds from depth and normal maps (csrc/depthcloud.hip, collab_splats_amd/depthcloud.py) against the
restatement (tests/depthcloud_restatement.py).  Edge images, candidate sets and sampled pixels are compared for equality; points,
normals and colours bit for bit (the kernels and the restatement write every fp32 expression in one order)."""
import os

import numpy as np
import pytest
import torch

import depthcloud_restatement as R
import depthcloud_scenes as Q
import tsdf_scenes as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depthcloud_goldens.npz")


def _t(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _np(x):
    return None if x is None else x.cpu().numpy()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


# ------------------------------------------------------------------------------------------------------------ edges
def _edges(depth, thr, r):
    import collab_splats_amd as m
    got = m.depth_edges(_t(depth), thr, r)
    assert got.dtype == torch.bool and got.is_cuda and tuple(got.shape) == depth.shape[:3]
    ref = R.depth_edges(depth.reshape(depth.shape[:3]), thr, r)
    assert np.array_equal(_np(got), ref), (depth.shape, thr, r)
    return ref


@pytest.mark.parametrize("W,H", [(16, 12), (64, 48), (65, 33), (121, 67), (200, 130)])
def test_edges_scene_every_radius(W, H):
    """Widths below one word, exactly one, one bit over, and two partial layouts of the last word; three views."""
    depth = np.stack([Q.edge_scene(H, W, seed=s) for s in (1, 2, 3)])
    for thr, r in [(0.004, 10), (0.004, 3), (0.01, 1), (0.01, 0), (0.004, 63)]:
        ref = _edges(depth, thr, r)
        assert ref.any()
    assert _edges(depth[:1, :, :, None], 0.01, 3).any()               # V = 1, [V,H,W,1] as render_views stacks it


@pytest.mark.parametrize("W,H", [(16, 12), (64, 12), (65, 40), (121, 67), (200, 130)])
def test_edges_single_pixels_at_word_and_image_borders(W, H):
    xs = sorted({x for x in (0, 63, 64, W - 1) if x < W})
    where = [(0, 0, x) for x in xs] + [(0, H - 1, x) for x in xs] + [(0, H // 2, x) for x in xs] + [(1, H - 1, W - 1), (1, 0, 0)]
    depth = Q.spikes(2, H, W, where)
    for r in (0, 1, 3, 10, 63):
        ref = _edges(depth, 0.01, r)
        if r == 0:
            assert sorted(zip(*np.nonzero(ref))) == sorted(where)
    if max(H, W) <= 64:
        assert ref.all()                                            # radius 63 covers the image from any pixel


def test_edges_equal_the_reference_goldens(gold):
    import collab_splats_amd as m
    for scene in range(3):
        depth = gold[f"edge{scene}_depth"]
        for j, (thr, dil) in enumerate(gold["edge_cases"]):
            ref = np.unpackbits(gold[f"edge{scene}_{j}"])[:depth.size].reshape(depth.shape).astype(bool)
            assert np.array_equal(_np(m.depth_edges(_t(depth[None]), float(thr), int(dil)))[0], ref)


def test_edges_radius_64_raises():
    import collab_splats_amd as m
    with pytest.raises(ValueError, match="dilation_itr"):
        m.depth_edges(_t(Q.spikes(1, 8, 8, [])), 0.01, 64)


# --------------------------------------------------------------------------------------------------------- sampling
def _sample(cand, S_, seed=0, frame_offset=0, keys=None):
    import collab_splats_amd as m
    f, p, c = m.sample_pixels(_t(cand), S_, seed=seed, frame_offset=frame_offset, keys=None if keys is None else _t(keys))
    assert f.dtype == p.dtype == c.dtype == torch.int32 and f.is_cuda and f.shape == p.shape
    rf, rp, rc = R.sample_pixels(cand, S_, seed, frame_offset, keys)
    assert np.array_equal(_np(c), rc) and np.array_equal(_np(f), rf) and np.array_equal(_np(p), rp), (cand.shape, S_)
    return rf, rp, rc


def _cands(V, H, W, seed, p=0.6):
    return np.random.default_rng(seed).random((V, H, W)) < p


def test_sample_above_at_and_below_the_candidate_count():
    cand = _cands(3, 67, 121, 0)                                    # four chunks of 2048 pixels a frame, the last partial
    cand[1] = False                                                 # no candidate, between two frames that have some
    n = int(cand[0].sum())
    for S_ in (1, 7, 1000, n - 1, n, n + 1, 10 ** 6):
        rf, rp, rc = _sample(cand, S_, seed=3)
        assert rc[1] == 0 and rc[0] == min(S_, n)
    with_mid = cand.copy()
    with_mid[1] = _cands(1, 67, 121, 9)[0]
    f2, p2, c2 = _sample(with_mid, 1000, seed=3)
    rf, rp, rc = R.sample_pixels(cand, 1000, seed=3)
    assert np.array_equal(p2[f2 != 1], rp) and c2[0] == rc[0] and c2[2] == rc[2]      # the others are unchanged


@pytest.mark.parametrize("W,H", [(16, 12), (64, 32), (200, 130)])
def test_sample_sizes_and_seeds(W, H):
    cand = _cands(2, H, W, 1)
    for seed, S_ in ((0, 5), (1, 100), (2 ** 32 - 1, H * W // 3)):
        _sample(cand, S_, seed=seed, frame_offset=7)


def test_sample_frame_of_more_than_1024_chunks():
    """1408 x 1500 pixels are 1032 chunks of 2048: the per-frame scan of the chunk counts takes a second round with a carry."""
    cand = _cands(2, 1500, 1408, 5, p=0.5)
    rf, rp, rc = _sample(cand, 6667, seed=1, frame_offset=30)
    assert rc.tolist() == [6667, 6667] and rp[6666] > 2048 * 1024


def test_sample_forced_keys_ties_and_pivot_remainder():
    cand = _cands(2, 40, 130, 2, p=0.8)
    zeros = np.zeros(cand.shape, np.int32)
    for S_ in (1, 77, 3000):
        _, rp, _ = _sample(cand, S_, keys=zeros)                     # all equal: the first S candidates in pixel order
        assert np.array_equal(rp[:S_], np.nonzero(cand[0].ravel())[0][:S_])
    two = (np.random.default_rng(3).random(cand.shape) < 0.5).astype(np.int32)
    n0 = int((cand[0] & (two[0] == 0)).sum())
    for S_ in (1, n0 - 1, n0, n0 + 1, n0 + 500):
        _sample(cand, S_, keys=two)                                 # the pivot is 0, then 1 with a remainder
    top = np.full(cand.shape, -1, np.int32)                         # 0xffffffff everywhere but a few: unsigned order
    top[0, 3, 5:9] = np.array([0x7fffffff, -2 ** 31, 5, -2], np.int32)
    cand[0, 3, 5:9] = True
    for S_ in (1, 2, 3, 4, 5):
        _sample(cand, S_, keys=top)


def test_sample_is_independent_of_batching():
    import collab_splats_amd as m
    cand = _cands(4, 48, 64, 4)
    f, p, c = (_np(x) for x in m.sample_pixels(_t(cand), 300, seed=11, frame_offset=0))
    for v in range(4):
        f1, p1, c1 = (_np(x) for x in m.sample_pixels(_t(cand[v:v + 1]), 300, seed=11, frame_offset=v))
        assert np.array_equal(p1, p[f == v]) and (f1 == 0).all() and c1[0] == c[v]
    again = [_np(x) for x in m.sample_pixels(_t(cand), 300, seed=11, frame_offset=0)]
    assert all(np.array_equal(a, b) for a, b in zip(again, (f, p, c)))


# --------------------------------------------------------------------------------------------------- back-projection
def test_backprojection_bitwise_on_the_golden_scenes(gold):
    import collab_splats_amd as m
    for scene in range(3):
        g = {k[len(f"bp{scene}_"):]: v for k, v in gold.items() if k.startswith(f"bp{scene}_")}
        idx = g["indices"]
        f = np.zeros(len(idx), np.int32)
        args = (g["depth"][None], g["rgb"][None], g["normals"][None], g["c2w"][None], g["intr"][None], f, idx)
        rp, rn, rc = R.backproject(*args)
        pts, nrm, col = m.backproject(*[_t(a) for a in args])
        assert _bits(_np(pts), rp) and _bits(_np(nrm), rn) and _bits(_np(col), rc)
        pts2, none, col2 = m.backproject(_t(args[0]), _t(args[1]), None, *[_t(a) for a in args[3:]])
        assert none is None and _bits(_np(pts2), rp) and _bits(_np(col2), rc)


def test_backprojection_batch_with_a_zero_normal():
    import collab_splats_amd as m
    V, H, W = 3, 33, 65
    depth, rgb, normals = Q.maps(V, H, W, seed=5)
    c2w, intr = Q.cameras(V)
    rng = np.random.default_rng(6)
    f = np.sort(rng.integers(0, V, 500)).astype(np.int32)
    p = rng.integers(0, H * W, 500).astype(np.int32)
    f[:3], p[:3] = [0, 1, 2], 0                                      # the pixels whose normal map holds 0.5: a zero vector
    rp, rn, rc = R.backproject(depth, rgb, normals, c2w, intr, f, p)
    pts, nrm, col = m.backproject(_t(depth[..., None]), _t(rgb), _t(normals), _t(c2w), _t(intr), _t(f).long(), _t(p).long())
    assert _bits(_np(pts), rp) and _bits(_np(nrm), rn) and _bits(_np(col), rc)
    assert (_np(nrm)[:3] == 0).all() and np.abs(np.linalg.norm(_np(nrm)[3:], axis=1) - 1).max() < 1e-6


# ------------------------------------------------------------------------------------------------ depth_normal_cloud
def test_cloud_candidate_rules():
    import collab_splats_amd as m
    V, H, W = 3, 48, 64
    depth = np.stack([Q.edge_scene(H, W, seed=s) for s in (4, 5, 6)])
    _, rgb, normals = Q.maps(V, H, W, seed=7)
    c2w, intr = Q.cameras(V)
    rng = np.random.default_rng(8)
    masks, valid = rng.random((V, H, W)) < 0.7, rng.random((V, H, W, 1)) < 0.8
    dev = [_t(x) for x in (depth, rgb, normals, c2w, intr)]
    everything = H * W + 1
    # without mask and edge filter: the reference's nonzero(ravel(depth))
    out = m.depth_normal_cloud(*dev, everything)
    cand = depth > 0
    assert (~cand).any()
    for v in range(V):
        assert np.array_equal(_np(out["pixel_ids"])[_np(out["frame_ids"]) == v], np.nonzero(depth[v].ravel())[0])
    assert _np(out["counts"]).tolist() == cand.reshape(V, -1).sum(1).tolist()
    # every rule at once: a masked, invalid, hole or edge pixel never appears
    out = m.depth_normal_cloud(*dev, everything, masks=_t(masks), valid=_t(valid), filter_edges=True, edge_threshold=0.004,
                               edge_dilation=3)
    want = R.candidates(depth, masks, valid, R.depth_edges(depth, 0.004, 3))
    assert 0 < want.sum() < (cand & masks).sum()
    got = np.zeros((V, H * W), bool)
    got[_np(out["frame_ids"]), _np(out["pixel_ids"])] = True
    assert np.array_equal(got.reshape(V, H, W), want)
    # sampled, against the chained restatement, bit for bit
    out = m.depth_normal_cloud(*dev, 200, seed=5, frame_offset=3, masks=_t(masks), valid=_t(valid), filter_edges=True,
                               edge_threshold=0.004, edge_dilation=3)
    f, p, c = R.sample_pixels(want, 200, seed=5, frame_offset=3)
    rp, rn, rc = R.backproject(depth, rgb, normals, c2w, intr, f, p)
    assert np.array_equal(_np(out["frame_ids"]), f) and np.array_equal(_np(out["pixel_ids"]), p) and np.array_equal(_np(out["counts"]), c)
    assert _bits(_np(out["points"]), rp) and _bits(_np(out["normals"]), rn) and _bits(_np(out["colors"]), rc)
    assert want.reshape(V, -1)[f, p].all()
    none = m.depth_normal_cloud(dev[0], dev[1], None, dev[3], dev[4], 200, seed=5, frame_offset=3)
    assert none["normals"] is None and none["points"].shape == (600, 3)


# ---------------------------------------------------------------------------------------------- Gaussian mask filter
def test_gaussian_mask_filter_against_the_reference_rule():
    """2000 Gaussians, 3 views, checkerboard masks; some placed at iu = 0 (kept by the strict rule), behind a camera and outside
    the frame.  Projections within 8 2^-24 (|u| + |v|) of a pixel boundary are generated away: the restatement and a kernel agree
    there anyway (same arithmetic), the direct loop is the reference's rule on those projections."""
    import collab_splats_amd as m
    rng = np.random.default_rng(9)
    H, W = 48, 64
    c2w, intr = Q.cameras(3)
    intr = intr.copy()
    intr[:, :2], intr[:, 2], intr[:, 3] = 50.0, W / 2 + 1.5, H / 2 - 0.75
    masks = ((np.indices((H, W)) // 4).sum(0) % 2 == 0)[None].repeat(3, 0)
    masks[1] = ~masks[1]

    def lift(v, u, w, z):                                            # world points that project to (u, w) at depth z in view v
        Rm, t = R._pose(c2w[v])
        cam = np.stack([(u - intr[v, 2]) * z / intr[v, 0], (w - intr[v, 3]) * z / intr[v, 1], z], 1)
        return cam @ Rm.T.astype(np.float64) + t

    parts = []
    for v in range(3):
        n = 600
        parts.append(lift(v, rng.uniform(-20, W + 20, n), rng.uniform(-20, H + 20, n), rng.uniform(1, 6, n)))   # in and around
        parts.append(lift(v, rng.uniform(0.6, 1.4, 30), rng.uniform(2, H - 2, 30), rng.uniform(1, 6, 30)))        # iu = 0
        parts.append(lift(v, rng.uniform(2, W - 2, 37), rng.uniform(2, H - 2, 37), -rng.uniform(1, 6, 37)))       # behind
    P = np.concatenate(parts)[:2000].astype(np.float32)
    assert len(P) == 2000
    near = np.zeros(len(P), bool)
    for v in range(3):
        u, w, z = R.project(P, c2w[v], intr[v])
        with np.errstate(invalid="ignore"):
            for a in (u.astype(np.float64) - 0.5, w.astype(np.float64) - 0.5):
                near |= np.abs(a - np.round(a)) <= 8 * 2.0 ** -24 * (np.abs(u) + np.abs(w))
    P = P[~near]
    assert len(P) > 1900
    want = np.ones(len(P), bool)
    hit_zero = behind = 0
    for v in range(3):
        u, w, z = R.project(P, c2w[v], intr[v])
        for i in range(len(P)):
            if not z[i] > 0:
                behind += 1
                continue
            iu, iv = int(np.floor(u[i] - np.float32(0.5))), int(np.floor(w[i] - np.float32(0.5)))
            hit_zero += iu == 0 and 0 < iv < H
            if iu > 0 and iu < W and iv > 0 and iv < H and not masks[v, iv, iu]:
                want[i] = False
    assert hit_zero >= 20 and behind >= 100 and 0.1 < want.mean() < 0.9
    assert np.array_equal(R.gaussian_mask_filter(P, c2w, intr, masks), want)
    keep = m.gaussian_mask_filter(_t(P), _t(c2w), _t(intr), _t(masks))
    assert keep.dtype == torch.bool and np.array_equal(_np(keep), want)
    keep = m.gaussian_mask_filter(_t(P), _t(c2w), _t(intr), _t(masks[..., None]).to(torch.uint8))
    assert np.array_equal(_np(keep), want)


# ------------------------------------------------------------------------------------------------------------ model
class _Box:
    def __init__(self, lo, hi):
        self.lo, self.hi = torch.tensor(lo), torch.tensor(hi)

    def within(self, pts):
        return ((pts >= self.lo.to(pts.device)) & (pts <= self.hi.to(pts.device))).all(-1, keepdim=True)


@pytest.fixture(scope="module")
def scene():
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene, view_matrix
    W, H = 64, 48
    sc = random_scene(3000, W, H, seed=21)
    model = radegs.RadegsModel(radegs.RadegsModelConfig(), sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"],
                               sc["sh"][:, 0], sc["sh"][:, 1:]).to(DEV)
    model.eval()
    model.step = 10 ** 6
    K = sc["Ks"][0].numpy().astype(np.float64)
    cams = [S.pinhole_camera(view_matrix(i)[0].numpy(), K, W, H) for i in range(4)]
    return model, cams, W, H


def _same(a, b):
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        elif a[k].dtype == torch.float32:
            assert _bits(_np(a[k]), _np(b[k])), k
        else:
            assert torch.equal(a[k], b[k]), k


def test_model_depth_normal_points(scene, tmp_path):
    from collab_splats_amd import write_ply
    model, cams, W, H = scene
    total = 1000
    spf = (total + 4) // 4
    out = model.depth_normal_points(cams, total_points=total, seed=3, batch_size=4)
    n = out["points"].shape[0]
    assert out["points"].shape == (n, 3) and out["normals"].shape == (n, 3) and out["colors"].shape == (n, 3)
    assert out["frame_ids"].shape == (n,) and out["pixel_ids"].shape == (n,) and out["counts"].shape == (4,)
    counts = _np(out["counts"])
    assert (counts <= spf).all() and counts.sum() == n and n > 0
    assert np.array_equal(np.bincount(_np(out["frame_ids"]), minlength=4), counts)
    _same(out, model.depth_normal_points(cams, total_points=total, seed=3, batch_size=4))       # two runs
    _same(out, model.depth_normal_points(cams, total_points=total, seed=3, batch_size=1))       # batching
    assert not torch.equal(out["pixel_ids"], model.depth_normal_points(cams, total_points=total, seed=4)["pixel_ids"])
    # every point of a frame reprojects into its own pixel of that frame
    pts, f, p = _np(out["points"]).astype(np.float64), _np(out["frame_ids"]), _np(out["pixel_ids"])
    for v, cam in enumerate(cams):
        c2w = cam.camera_to_worlds[0].double().numpy()
        Rm, t = c2w[:, :3] * np.array([1.0, -1.0, -1.0]), c2w[:, 3]
        c = (pts[f == v] - t) @ Rm
        assert (c[:, 2] > 0).all()
        u, w = c[:, 0] * cam.fx / c[:, 2] + cam.cx, c[:, 1] * cam.fy / c[:, 2] + cam.cy
        assert np.array_equal(np.floor(u).astype(np.int64) + W * np.floor(w).astype(np.int64), p[f == v])
    assert np.abs(np.linalg.norm(_np(out["normals"]).astype(np.float64), axis=1) - 1).max() < 1e-5
    # masks, opacity floor, edges and the crop narrow the cloud; a masked pixel never appears
    masks = torch.zeros(4, H, W, dtype=torch.bool)
    masks[:, :, : W // 2] = True
    half = model.depth_normal_points(cams, total_points=total, seed=3, masks=masks, min_accumulation=0.5, filter_edges=True,
                                     edge_threshold=0.004, edge_dilation=1)
    assert 0 < half["points"].shape[0] and (_np(half["pixel_ids"]) % W < W // 2).all()
    box = _Box([-1.0, -1.0, 0.0], [1.0, 1.0, 9.0])
    crop = model.depth_normal_points(cams, total_points=total, seed=3, obb_box=box)
    inside = _np(box.within(out["points"]).reshape(-1))
    assert 0 < inside.sum() < n and _bits(_np(crop["points"]), _np(out["points"])[inside])
    assert np.array_equal(_np(crop["counts"]), np.bincount(f[inside], minlength=4))
    clean = model.depth_normal_points(cams, total_points=total, seed=3, down_sample_voxel=0.5, outlier_removal=True)
    assert 0 < clean["points"].shape[0] < n and clean["normals"].shape == clean["points"].shape and clean["frame_ids"] is None
    # write_ply round-trips the cloud with normals
    path = str(tmp_path / "cloud_pcd.ply")
    write_ply(path, out["points"], torch.zeros(0, 3, dtype=torch.int32), out["colors"], out["normals"])
    raw = open(path, "rb").read()
    head, body = raw[:raw.index(b"end_header\n") + 11], raw[raw.index(b"end_header\n") + 11:]
    assert f"element vertex {n}\n".encode() in head and b"property float nx" in head and b"element face 0\n" in head
    rec = np.frombuffer(body, dtype=[("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)])
    assert len(rec) == n and _bits(rec["p"], _np(out["points"])) and _bits(rec["n"], _np(out["normals"]))
    assert np.array_equal(rec["c"], np.round(np.clip(_np(out["colors"]), 0, 1) * 255).astype(np.uint8))


def test_model_gaussian_points(scene):
    model, cams, W, H = scene
    n_all = model.means.shape[0]
    out = model.gaussian_points()
    assert out["points"].shape == (n_all, 3) and out["normals"].shape == (n_all, 3) and out["colors"].shape == (n_all, 3)
    assert torch.equal(out["indices"], torch.arange(n_all, device=DEV)) and _bits(_np(out["points"]), _np(model.means.detach()))
    assert _bits(_np(out["normals"]), _np(model.normals.detach()))
    col = _np(out["colors"])
    assert col.min() >= 0 and col.max() <= 1
    masks = torch.zeros(4, H, W, dtype=torch.bool)
    masks[:, :, : W // 2] = True
    from collab_splats_amd import gaussian_mask_filter
    c2w, intr = model._camera_poses(cams, DEV)
    keep = gaussian_mask_filter(model.means.detach(), c2w, intr, masks.to(DEV))
    ref = R.gaussian_mask_filter(_np(model.means.detach()), _np(c2w), _np(intr), masks.numpy())
    assert np.array_equal(_np(keep), ref) and 0 < ref.sum() < n_all
    a = model.gaussian_points(cameras=cams, masks=masks, min_opacity=0.5, mask_color=col[5].tolist())
    want = ref & (_np(torch.sigmoid(model.opacities.detach()).reshape(-1)) > 0.5) & (col != col[5]).all(1)
    assert np.array_equal(_np(a["indices"]), np.nonzero(want)[0]) and 0 < want.sum() < ref.sum()
    _same(a, model.gaussian_points(cameras=cams, masks=masks, min_opacity=0.5, mask_color=col[5].tolist()))
    assert not want[5] and 5 not in _np(model.gaussian_points(mask_color=col[5].tolist())["indices"]).tolist()
    box = _Box([-1.0, -1.0, 0.0], [1.0, 1.0, 9.0])
    b = model.gaussian_points(obb_box=box, down_sample_voxel=0.5, outlier_removal=True)
    assert 0 < b["points"].shape[0] < n_all and b["indices"] is None and b["normals"].shape == b["points"].shape
