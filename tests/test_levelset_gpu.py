"""GPU: the level-set search along rays (csrc/density.hip's density_raycast), the model's level-set clouds and meshes, and the
Laplacian smoothing (csrc/meshclean.hip) -- DESIGN.md section 26.

  1. raycast equals, bit for bit and with no exclusions, the search composed in torch fp32 from DensityField.query calls;
  2. raycast against the fp64 search on the fp64 oracle (tests/levelset_restatement.py) on the four long ray sets;
  3. determinism, and query / the pool are left as they were;
  4. RadegsModel.level_set_points / level_set_mesh;
  5. smooth_laplacian against its numpy restatement."""
import numpy as np
import pytest
import torch

import density_scenes as S
import levelset_restatement as LR
import levelset_scenes as LS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = torch.float32


def _t(x, dtype=F32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV).to(dtype)


_FIELDS = {}


def _field(name):
    if name not in _FIELDS:
        from collab_splats_amd import DensityField
        sc = S.scene(name)
        _FIELDS[name] = DensityField(_t(sc["means"]), _t(sc["quats"]), _t(sc["scales"]), _t(sc["opacities"]), sc["h"],
                                     cutoff=sc["cutoff"], min_opacity=sc["min_opacity"], bounds=sc["bounds"])
    return _FIELDS[name]


def _cast(field, rays, levels):
    return field.raycast(_t(rays["origins"]), _t(rays["dirs"]), _t(rays["t0"]), _t(rays["t1"]), levels)


def _div(a, b):
    """a / b in IEEE fp32, on the host in numpy: a device library may divide by a constant through its reciprocal, and the
    search's two divisions are part of what is compared bit for bit."""
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.float32(b)
    return torch.from_numpy(np.asarray(a.cpu().numpy() / b, np.float32)).to(DEV)


def _composed(field, rays, levels):
    """Section 26.1 in torch fp32 on the device, every density from field.query: (t [L,M] fp32, hit [L,M] bool).  Plain `*` then
    `+` throughout."""
    o, v, t0, t1 = (_t(rays[k]) for k in ("origins", "dirs", "t0", "t1"))
    M = o.shape[0]
    valid = torch.isfinite(o).all(1) & torch.isfinite(v).all(1) & torch.isfinite(t0) & torch.isfinite(t1) & (t1 > t0)
    j = torch.arange(64, dtype=F32, device=DEV)
    step = _div(t1 - t0, 63.0)
    tk = t0[:, None] + j[None, :] * step[:, None]
    D = field.query((o[:, None, :] + tk[:, :, None] * v[:, None, :]).reshape(-1, 3))["density"].reshape(M, 64)
    t_out = torch.zeros((len(levels), M), dtype=F32, device=DEV)
    hit_out = torch.zeros((len(levels), M), dtype=torch.bool, device=DEV)
    for li, level in enumerate(levels):
        lev = torch.tensor(level, dtype=F32, device=DEV)
        cross = (D[:, :-1] < lev) & (lev <= D[:, 1:]) & valid[:, None]
        rows = torch.nonzero(cross.any(1))[:, 0]
        if rows.numel() == 0:
            continue
        k = cross[rows].to(torch.int32).argmax(1)                         # (the first of equal maxima)
        a, b = tk[rows, k], tk[rows, k + 1]
        fstep = _div(b - a, 63.0)
        u = a[:, None] + j[None, :] * fstep[:, None]
        u[:, 0], u[:, 63] = a, b
        Fv = field.query((o[rows, None, :] + u[:, :, None] * v[rows, None, :]).reshape(-1, 3))["density"].reshape(-1, 64)
        Fv[:, 0], Fv[:, 63] = D[rows, k], D[rows, k + 1]
        fine = (Fv[:, :-1] < lev) & (lev <= Fv[:, 1:])
        assert bool(fine.any(1).all())                                     # F_0 < l <= F_63
        js = fine.to(torch.int32).argmax(1)
        r = torch.arange(rows.numel(), device=DEV)
        uj, un, Fj, Fn = u[r, js], u[r, js + 1], Fv[r, js], Fv[r, js + 1]
        t_out[li, rows] = uj + (un - uj) * _div(lev - Fj, Fn - Fj)
        hit_out[li, rows] = True
    return t_out, hit_out


def _assert_bitwise(field, rays, levels, label):
    got = _cast(field, rays, levels)
    t, hit = _composed(field, rays, levels)
    assert got["hit"].dtype == torch.bool and got["t"].dtype == F32 and tuple(got["t"].shape) == (len(levels), len(rays["t0"]))
    assert torch.equal(got["hit"], hit), (label, int((got["hit"] != hit).sum()))
    assert torch.equal(got["t"].view(torch.int32), t.view(torch.int32)), (label, float((got["t"] - t).abs().max()))
    assert bool((got["t"][~got["hit"]] == 0).all())
    return got


# ----------------------------------------------------------------------------------------- 1. bitwise against query
@pytest.mark.parametrize("levels", [(0.3,), LS.LEVELS], ids=["L1", "L3"])
@pytest.mark.parametrize("kind", ["long", "short"])
@pytest.mark.parametrize("name", sorted(LS.LONG))
def test_raycast_equals_the_composition_of_queries(name, kind, levels):
    rays = LS.long_set(name) if kind == "long" else LS.short_set(name)
    got = _assert_bitwise(_field(name), rays, levels, (name, kind))
    n = got["hit"].sum(1).tolist()
    print(name, kind, levels, "hits", n)
    assert all(0 < x for x in n) if kind == "long" else n[-2 if len(levels) == 3 else 0] > 0.9 * len(rays["t0"])


@pytest.mark.parametrize("name", ["batches_193", "clipped", "culled", "tiny", "bench_corner_r1.5", "bench_corner_r6"])
def test_raycast_equals_the_composition_on_the_small_scenes(name):
    """One list of 193 entries; a map of one unit with a Gaussian wider than it; culled Gaussians; a Gaussian smaller than a voxel;
    a cut-off of 1.5 and of 6 (density_regimes_scenes.py: two units at the bench's voxel size, 7 to 12 m from the origin).
    A fan from outside the scene's box through its middle (4 degrees wide for `tiny`, whose support is 0.018 across: the 35
    degree fan's rays all pass it by; 20 degrees for the two-unit maps, 0.32 x 0.16 x 0.16 m, aimed at the map's centre);
    the levels sit below the scene's own maximum."""
    f = _field(name)
    sc = S.scene(name)
    if name.startswith("bench_corner"):
        centre = ((f.lo + 0.5 * f.dims) * f.ulen).astype(np.float32)
    else:
        centre = sc["means"][np.isfinite(sc["means"]).all(1) & (np.abs(sc["means"]) < 1.5).all(1)].mean(0)
    fov = 4.0 if name == "tiny" else 20.0 if name.startswith("bench_corner") else 35.0
    o, v = LS.fan(centre - np.array([0.03, 0.05, 0.6], np.float32), centre, res=16, fov_deg=fov)
    rays = dict(origins=o, dirs=v, t0=np.full(256, 0.2, np.float32), t1=np.full(256, 1.0, np.float32))
    top = float(f._pool[:, 0].max())
    levels = (0.02 * top, 0.3 * top, 0.8 * top)
    got = _assert_bitwise(f, rays, levels, name)
    print(name, "max d", top, "hits", got["hit"].sum(1).tolist())
    assert int(got["hit"][0].sum()) > 0


def test_raycast_equals_the_composition_on_the_edge_rays():
    f = _field("random")
    for label, rays in LS.edge_rays().items():
        got = _assert_bitwise(f, rays, LS.LEVELS, label)
        if label in ("outside_the_map", "t1_below_t0", "t1_equals_t0", "nan_origin"):
            assert not bool(got["hit"].any()) and not bool(got["t"].any()), label
        if label.startswith("partial_workgroup") or label in ("unnormalised_dirs", "starting_inside"):
            assert bool(got["hit"].any()), label
    # |v| = 3.7: the same crossings as the unit directions, t in units of |v|
    unit = {k: a[:256] for k, a in LS.long_set("random").items()}
    g1, g37 = _cast(f, unit, LS.LEVELS), _cast(f, LS.edge_rays()["unnormalised_dirs"], LS.LEVELS)
    both = g1["hit"] & g37["hit"]
    assert int(both.sum()) > 100 and float(((g37["t"] * 3.7 - g1["t"])[both].abs() < 1e-3).float().mean()) > 0.98
    # L = 4 with a repeated level: rows 1 and 3 agree
    rays = LS.long_set("random")
    got = _assert_bitwise(f, rays, (0.1, 0.3, 0.5, 0.3), "L4")
    assert torch.equal(got["t"][1], got["t"][3]) and torch.equal(got["hit"][1], got["hit"][3])
    # units that no Gaussian reaches, inside the map; and a field with no unit at all
    fd = _field("tilted_disc")
    got = _assert_bitwise(fd, LS.unallocated_rays("tilted_disc"), LS.LEVELS, "unallocated")
    assert not bool(got["hit"].any())
    got = _assert_bitwise(_field("empty"), rays, LS.LEVELS, "empty")
    assert not bool(got["hit"].any()) and not bool(got["t"].any())
    got = f.raycast(torch.zeros((0, 3), device=DEV), torch.zeros((0, 3), device=DEV), torch.zeros(0, device=DEV),
                    torch.zeros(0, device=DEV), (0.3, 0.5))
    assert tuple(got["t"].shape) == (2, 0) and tuple(got["hit"].shape) == (2, 0)


# ------------------------------------------------------------------------------------------ 2. against the fp64 oracle
@pytest.mark.parametrize("name", sorted(LS.LONG))
def test_raycast_against_the_fp64_search(name):
    """A ray is left out for a level only if some coarse oracle sample lies within 1e-4 of the level (the project's standing
    bound: there fp32 may bracket elsewhere), at most 3 % per set and level.  On the rest: hit equals the oracle's; t lies in the
    oracle's coarse bracket (widened by 8 ulp of t1: the fp32 sample positions are the fp64 ones rounded); |d64(o + t v) - l| <=
    R64 + 1e-4 with R64 the residual of the fp64 search on the same rays; no fp64 fine sample more than one fine step in front
    of t reaches l + 1e-4."""
    rays, O = LS.long_set(name), LS.long_oracle(name)
    d64 = LR.oracle_density(S.oracle(name), S.restated(name))
    got = _cast(_field(name), rays, LS.LEVELS)
    t, hit = got["t"].cpu().numpy().astype(np.float64), got["hit"].cpu().numpy()
    o, v = rays["origins"].astype(np.float64), rays["dirs"].astype(np.float64)
    slack = 8 * 2.0 ** -23 * float(rays["t1"][0])
    for li, lev in enumerate(LS.LEVELS):
        out = (np.abs(O["D"] - lev) < 1e-4).any(1)
        assert out.mean() <= 0.03, (name, lev, out.mean())
        keep = ~out
        assert np.array_equal(hit[li][keep], O["hit"][li][keep]), (name, lev, int((hit[li] != O["hit"][li])[keep].sum()))
        sel = np.nonzero(keep & O["hit"][li])[0]
        k = O["k"][li][sel]
        lo, hi = O["tk"][sel, k], O["tk"][sel, k + 1]
        assert ((t[li][sel] >= lo - slack) & (t[li][sel] <= hi + slack)).all(), (name, lev)
        r64 = np.abs(d64(o[sel] + O["t"][li][sel][:, None] * v[sel]) - lev).max()
        res = np.abs(d64(o[sel] + t[li][sel][:, None] * v[sel]) - lev).max()
        fstep = (hi - lo) / 63.0
        front = O["u"][li][sel] < (t[li][sel] - fstep)[:, None]
        early = np.where(front, O["F"][li][sel], -np.inf).max()
        print(f"{name} level {lev}: left out {int(out.sum())}, hits {len(sel)}, residual {res:.3e}, R64 {r64:.3e}, "
              f"max |t - t64| {np.abs(t[li][sel] - O['t'][li][sel]).max():.3e}, largest sample in front {early:.6f}")
        assert res <= r64 + 1e-4, (name, lev, res, r64)
        assert early < lev + 1e-4, (name, lev, early)


# --------------------------------------------------------------------------------------------------- 3. determinism
def test_two_raycasts_are_bitwise_equal_and_leave_the_field_alone():
    f = _field("random")
    rays = LS.long_set("random")
    pts = _t(rays["origins"]) + 1.5 * _t(rays["dirs"])
    vals = torch.rand((f.n_gauss, 3), device=DEV)
    before = f.query(pts, vals)
    pool, ids, ranges, slots = f._pool.clone(), f._ids.clone(), f._ranges.clone(), f._slot_map.clone()
    a, b = _cast(f, rays, LS.LEVELS), _cast(f, rays, LS.LEVELS)
    assert torch.equal(a["t"].view(torch.int32), b["t"].view(torch.int32)) and torch.equal(a["hit"], b["hit"])
    after = f.query(pts, vals)
    for key in ("density", "grad", "dominant", "values"):
        assert torch.equal(before[key], after[key]), key
    assert torch.equal(f._pool.view(torch.int32), pool.view(torch.int32)) and torch.equal(f._ids, ids)
    assert torch.equal(f._ranges, ranges) and torch.equal(f._slot_map, slots)


def test_level_surface_points_is_raycast_then_query():
    from collab_splats_amd import level_surface_points
    f = _field("random")
    rays = LS.long_set("random")
    o, v, t0, t1 = (_t(rays[k]) for k in ("origins", "dirs", "t0", "t1"))
    vals = torch.rand((f.n_gauss, 4), device=DEV)
    out = level_surface_points(f, o, v, t0, t1, LS.LEVELS, values=vals)
    cast = f.raycast(o, v, t0, t1, LS.LEVELS)
    assert list(out) == list(LS.LEVELS)
    for li, lev in enumerate(LS.LEVELS):
        r = out[lev]
        ids = torch.nonzero(cast["hit"][li])[:, 0]
        assert r["ray_ids"].dtype == torch.int64 and torch.equal(r["ray_ids"], ids) and torch.equal(r["t"], cast["t"][li][ids])
        pts = o[ids] + cast["t"][li][ids][:, None] * v[ids]
        assert torch.equal(r["points"].view(torch.int32), pts.view(torch.int32))
        q = f.query(pts, vals)
        for key in ("density", "grad", "dominant", "values"):
            assert torch.equal(r[key], q[key]), key
        assert bool((r["density"] > 0).all()) and bool((r["dominant"] >= 0).all())      # (how close to the level: test 2)


# ------------------------------------------------------------------------------------------------------- 4. the model
class _Box:
    """Axis-aligned stand-in for nerfstudio's OrientedBox: R, T, S and within()."""

    def __init__(self, centre, size):
        self.R, self.T, self.S = torch.eye(3), torch.tensor(centre, dtype=F32), torch.tensor(size, dtype=F32)

    def within(self, pts):
        lo, hi = (self.T - self.S / 2).to(pts.device), (self.T + self.S / 2).to(pts.device)
        return ((pts >= lo) & (pts <= hi)).all(-1, keepdim=True)


_MODEL = {}
H = 0.04
ALL = 3 * 64 * 48                                                          # total_points that takes every candidate pixel


def _model():
    """600 Gaussians in |x| < 1.6, |y| < 1.2, 1 < z < 3 and three 64 x 48 cameras in front of them, looking along +z."""
    if not _MODEL:
        from collab_splats_amd import radegs
        from collab_splats_amd.synthetic import random_scene
        sc = random_scene(600, 64, 48, seed=3)
        sc["means"][:, :2] *= 0.2
        sc["means"][:, 2] = (sc["means"][:, 2] - 2.0) * 0.2 + 1.0
        sc["log_scales"] += 1.2
        model = radegs.RadegsModel(radegs.RadegsModelConfig(), sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"],
                                   sc["sh"][:, 0], sc["sh"][:, 1:]).to(DEV).eval()

        def cam(x, y, z):
            c2w = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0]))[:3].clone()          # OpenGL camera looking along world +z
            c2w[:, 3] = torch.tensor([x, y, z])
            return radegs.PinholeCamera.make(c2w, 50.0, 50.0, 64, 48)

        _MODEL.update(model=model, cams=[cam(0.0, 0.0, -1.0), cam(0.4, 0.1, -1.2), cam(-0.4, -0.2, -0.9)])
    return _MODEL["model"], _MODEL["cams"]


def _centres(cams):
    return torch.stack([c.camera_to_worlds.reshape(-1, 3, 4)[0, :, 3] for c in cams]).to(DEV).float()


def test_level_set_points_lie_on_the_levels():
    """The cloud's points against the fp64 oracle: the rays are rebuilt from the cloud's (frame, pixel) ids, the fp64 search on
    them gives R64, and both query's density and the oracle's at the points are within R64 + 1e-4 of the level."""
    from collab_splats_amd import backproject
    from density_restatement import Oracle
    model, cams = _model()
    cloud = model.level_set_points(cams, H, total_points=3000, outlier_removal=False)
    assert list(cloud) == [0.1, 0.3, 0.5]
    act = [x.cpu().numpy() for x in model._activated()]
    d64 = LR.oracle_density(Oracle(*act))
    field = model.density_field(H)
    maps = model.render_views(cams)
    c2w, intr = model._camera_poses(cams, DEV)
    for lev, c in cloud.items():
        n = c["points"].shape[0]
        assert n > 10 and c["frame_ids"].dtype == torch.int64 and int(c["frame_ids"].max()) <= 2
        assert c["normals"].shape == (n, 3) and c["colors"].shape == (n, 3) and c["pixel_ids"].shape == (n,)
        assert float(c["colors"].min()) >= 0 and float(c["colors"].max()) <= 1 + 1e-6
        P = backproject(maps["depth"], maps["rgb"], None, c2w, intr, c["frame_ids"], c["pixel_ids"])[0]
        o = c2w[c["frame_ids"], :, 3]
        t_c = torch.linalg.norm(P - o, dim=1)
        v = (P - o) / t_c[:, None]
        rays = [x.cpu().numpy() for x in (o, v, torch.clamp(t_c - 8 * H, min=0.0), t_c + 8 * H)]
        O = LR.search(d64, *rays, (lev,))
        hit = O["hit"][0]
        assert hit.mean() > 0.95                                           # (the fp64 search finds what the fp32 one found)
        p64 = rays[0][hit].astype(np.float64) + O["t"][0][hit][:, None] * rays[1][hit].astype(np.float64)
        r64 = np.abs(d64(p64) - lev).max()
        q = field.query(c["points"])["density"].cpu().numpy().astype(np.float64)
        got64 = d64(c["points"].cpu().numpy())
        print(f"level {lev}: {n} points, R64 {r64:.3e}, |query - l| {np.abs(q - lev).max():.3e}, |d64 - l| {np.abs(got64 - lev).max():.3e}")
        assert np.abs(q - lev).max() <= r64 + 1e-4 and np.abs(got64 - lev).max() <= r64 + 1e-4


@pytest.mark.parametrize("mode", ["analytical", "closest_gaussian", "average"])
def test_level_set_normals_and_batching(mode):
    model, cams = _model()
    a = model.level_set_points(cams, H, total_points=3000, return_normal=mode, batch_size=1)
    b = model.level_set_points(cams, H, total_points=3000, return_normal=mode, batch_size=4)
    centres = _centres(cams)
    for lev in a:
        for key in ("points", "normals", "colors", "frame_ids", "pixel_ids"):
            assert torch.equal(a[lev][key], b[lev][key]), (lev, key)
        n, p = a[lev]["normals"], a[lev]["points"]
        assert n.shape[0] > 10
        assert float((torch.linalg.norm(n, dim=1) - 1).abs().max()) < 1e-5
        v = torch.nn.functional.normalize(p - centres[a[lev]["frame_ids"]], dim=1)
        facing = (n * v).sum(1)
        print(mode, lev, n.shape[0], "max n.v", float(facing.max()))
        assert float(facing.max()) <= 1e-6


def test_masks_and_box_only_remove_points():
    model, cams = _model()
    full = model.level_set_points(cams, H, total_points=ALL, surface_levels=(0.3,), outlier_removal=False)[0.3]
    masks = torch.zeros((3, 48, 64), dtype=torch.bool, device=DEV)
    masks[:, :, :32] = True
    part = model.level_set_points(cams, H, total_points=ALL, surface_levels=(0.3,), outlier_removal=False, masks=masks)[0.3]
    key = lambda c: c["frame_ids"] * (64 * 48) + c["pixel_ids"].long()                  # noqa: E731
    kf, kp = key(full), key(part)
    assert 0 < kp.numel() < kf.numel() and bool((part["pixel_ids"] % 64 < 32).all())
    pos = torch.searchsorted(kf, kp)
    assert bool((kf[pos.clamp(max=kf.numel() - 1)] == kp).all())                        # (frame, pixel) ascending in both
    for k in ("points", "normals", "colors"):
        assert torch.equal(part[k], full[k][pos]), k
    box = _Box([0.0, 0.0, 2.0], [1.2, 1.2, 1.2])
    inside = model.level_set_points(cams, H, total_points=ALL, surface_levels=(0.3,), outlier_removal=False, obb_box=box)[0.3]
    assert 0 < inside["points"].shape[0] < full["points"].shape[0] and bool(box.within(inside["points"]).all())
    cleaned = model.level_set_points(cams, H, total_points=ALL, surface_levels=(0.3,), nb_neighbors=10, std_ratio=1.0)[0.3]
    assert 0 < cleaned["points"].shape[0] < full["points"].shape[0]


def test_level_set_mesh():
    model, cams = _model()
    v, t, c, d = model.level_set_mesh(cams, H, surface_level=0.3, poisson_depth=6, total_points=ALL)
    assert v.shape[0] > 0 and t.shape[0] > 0 and v.dtype == F32 and t.dtype == torch.int32
    assert int(t.min()) >= 0 and int(t.max()) < v.shape[0] and c.shape == v.shape and d.shape == (v.shape[0],)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(c).all())
    v0 = model.level_set_mesh(cams, H, surface_level=0.3, poisson_depth=6, total_points=ALL, smooth_iterations=0)[0]
    assert v0.shape == v.shape and not torch.equal(v0, v)


# --------------------------------------------------------------------------------------------------- 5. smoothing
@pytest.mark.parametrize("mesh", ["tetrahedron", "grid_patch", "bumpy_sphere"])
def test_smooth_laplacian_against_the_restatement(mesh):
    """One iteration: the kernel adds the same fp64 terms in the same order as the restatement and rounds once to fp32.  The fp64
    sums of n <= 17 terms (the largest vertex degree here) agree to about n 2^-52 relative (the square root and the divisions
    may round differently), far below half an fp32 ulp, so the two fp32 results differ by at most one ulp where a value falls
    on a rounding boundary: at most 2^-23 max |x|.  (A second iteration is compared from the first one's own output: a one-ulp
    difference in the positions changes the weights by more than an ulp.)"""
    from collab_splats_amd import smooth_laplacian
    v, t = getattr(LS, mesh)()
    rng = np.random.default_rng(2)
    a1, a2 = rng.uniform(0, 1, (len(v), 3)).astype(np.float32), rng.standard_normal((len(v), 5)).astype(np.float32)

    def close(got, ref):
        assert got.dtype == F32 and tuple(got.shape) == ref.shape
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref).max()
        assert err <= 2.0 ** -23 * np.abs(ref).max(), (mesh, err)

    got_v, (g1, g2) = smooth_laplacian(_t(v), _t(t, torch.int32), 1, 0.5, attributes=(_t(a1), _t(a2)))
    ref_v, (r1, r2) = LR.smooth_laplacian(v, t, 1, 0.5, [a1, a2])
    for got, ref in ((got_v, ref_v), (g1, r1), (g2, r2)):
        close(got, ref)
    for iterations in (1, 2, 3):                                           # two runs; the result lands in the outputs
        x = smooth_laplacian(_t(v), _t(t, torch.int32), iterations, 0.5, attributes=(_t(a1), _t(a2)))
        y = smooth_laplacian(_t(v), _t(t, torch.int32), iterations, 0.5, attributes=(_t(a1), _t(a2)))
        assert torch.equal(x[0].view(torch.int32), y[0].view(torch.int32)) and torch.equal(x[1][0], y[1][0])
        assert torch.equal(x[1][1], y[1][1]) and (iterations > 1 or torch.equal(x[0], got_v))
    # iterations = 2 is two calls with iterations = 1, bit for bit; the second step against the restatement from the first's output
    one = smooth_laplacian(_t(v), _t(t, torch.int32), 1, 0.5, attributes=(_t(a1),))
    two = smooth_laplacian(one[0], _t(t, torch.int32), 1, 0.5, attributes=one[1])
    both = smooth_laplacian(_t(v), _t(t, torch.int64), 2, 0.5, attributes=(_t(a1),))
    assert torch.equal(two[0].view(torch.int32), both[0].view(torch.int32)) and torch.equal(two[1][0], both[1][0])
    ref2_v, (ref2_a,) = LR.smooth_laplacian(one[0].cpu().numpy(), t, 1, 0.5, [one[1][0].cpu().numpy()])
    close(both[0], ref2_v)
    close(both[1][0], ref2_a)
    zero = smooth_laplacian(_t(v), _t(t, torch.int32), 0)
    assert torch.equal(zero[0], _t(v)) and zero[1] == ()
    if mesh == "grid_patch":
        assert torch.equal(got_v[9], _t(v)[9])                              # the vertex no triangle names
    if mesh == "tetrahedron":
        assert float(both[0].mean(0).abs().max()) < 1e-6
