"""CPU: the marching-cubes tables (generated, watertight, oriented), the fp32 TSDF restatement on analytic scenes (closed
sphere of the right volume; allocation equal to a brute-force enumeration of the rule), write_ply, and the TSDF API's
argument checks.  No GPU."""
import itertools
import os

import numpy as np
import pytest
import torch

import tsdf_fields as F_
import tsdf_scenes as S
from tsdf_restatement import RestatedTSDF
from collab_splats_amd import mc_tables as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_header_equals_generator_output():
    with open(os.path.join(ROOT, "collab_splats_amd", "csrc", "mc_tables.h")) as f:
        assert f.read() == mc.header_text()


def test_header_is_listed_as_a_build_dependency():
    from collab_splats_amd import build
    src = open(build.__file__).read()
    assert os.path.join(build.CSRC, "mc_tables.h") in build.headers() and '"tsdf.hip": ["-ffp-contract=off"]' in src

def _cases():
    ntri, tri, _ = mc.tables()
    for case in range(256):
        yield case, [tuple(int(e) for e in tri[case, 3 * k:3 * k + 3]) for k in range(int(ntri[case]))]


def _crossed(case):
    return {e for e, (c0, c1) in enumerate(mc.EDGES) if ((case >> c0) & 1) != ((case >> c1) & 1)}


def test_triangles_use_exactly_the_crossed_edges():
    for case, tris in _cases():
        used = {e for t in tris for e in t}
        assert used == _crossed(case), case
        assert all(len(set(t)) == 3 for t in tris), case
    assert dict(_cases())[0] == [] and dict(_cases())[255] == []


def _boundary(tris):
    """Triangle sides that appear once in the cell (the surface's boundary on the cube's faces)."""
    cnt = {}
    for t in tris:
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            k = (min(a, b), max(a, b))
            cnt[k] = cnt.get(k, 0) + 1
    return {k for k, n in cnt.items() if n % 2}


def test_face_segments_depend_only_on_the_face_signs():
    """Neighbouring cells see the same 4 signs on a shared face, so equal segments there make the surface watertight."""
    seen = {}
    for case, tris in _cases():
        bnd = _boundary(tris)
        on_face = set()
        for fi, (a, s, cyc, fe) in enumerate(mc.FACES):
            segs = frozenset(k for k in bnd if k[0] in fe and k[1] in fe)
            on_face |= segs
            key = (fi, tuple((case >> c) & 1 for c in cyc))
            assert seen.setdefault(key, segs) == segs, (case, fi)
        assert on_face == bnd, case                     # every boundary segment lies on a face
        for k in bnd:                                   # and on one face only
            assert sum(k[0] in fe and k[1] in fe for (_, _, _, fe) in mc.FACES) == 1
    # translate to the neighbour's frame: face (a, 1) of one cell is face (a, 0) of the next with the same corner signs
    for a in range(3):
        f0, f1 = 2 * a, 2 * a + 1
        _, _, cyc0, fe0 = mc.FACES[f0]
        _, _, cyc1, fe1 = mc.FACES[f1]
        shift = {e0: e1 for e0 in fe0 for e1 in fe1
                 if mc.EDGES[e1][0] == mc.EDGES[e0][0] | (1 << a) and e1 // 4 == e0 // 4}
        for signs in itertools.product((0, 1), repeat=4):
            s0 = {tuple(sorted((shift[x], shift[y]))) for x, y in seen[(f0, signs)]}
            assert s0 == set(seen[(f1, signs)]), (a, signs)


def test_triangles_face_the_positive_corners():
    for case, tris in _cases():
        for t in tris:
            P = [mc.edge_mid(e) for e in t]
            n = np.cross(P[1] - P[0], P[2] - P[0])
            dots = []
            for e in t:                                 # the normal against each crossed edge, negative -> positive end
                c0, c1 = mc.EDGES[e]
                pos, neg = (c0, c1) if not (case >> c0) & 1 else (c1, c0)
                dots.append(np.dot(n, mc.corner_pos(pos) - mc.corner_pos(neg)))
            assert min(dots) >= 0 and sum(dots) > 0, (case, t, dots)


def _sphere_mesh():
    centre, radius, vs = (0.1, -0.05, 0.2), 0.3, 0.02
    d, vm, K, rgb = S.sphere_views(24, 64, 64, centre=centre, radius=radius)
    r = RestatedTSDF(vs, 0.06, 3.0)
    r.integrate(d, vm, K, rgb)
    return r.extract_mesh(), centre, radius, vs


def test_restatement_sphere_is_closed_and_has_the_right_volume():
    (v, f, c), centre, radius, vs = _sphere_mesh()
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    edges, cnt = np.unique(e, axis=0, return_counts=True)
    assert len(f) > 1000 and np.all(cnt == 2)
    assert len(v) - len(edges) + len(f) == 2
    assert len(np.unique(f)) == len(v)
    dist = np.abs(np.linalg.norm(v.astype(np.float64) - np.asarray(centre), axis=1) - radius)
    assert dist.max() <= vs
    a, b, cc = (v[f[:, k]].astype(np.float64) for k in range(3))
    vol = np.einsum("ij,ij->i", a, np.cross(b, cc)).sum() / 6
    assert abs(vol / (4 / 3 * np.pi * radius ** 3) - 1) < 0.03
    assert np.all((c >= 0) & (c <= 1)) and c.std() > 0.05


def _restated(field, vs):
    r = RestatedTSDF(vs, 3 * vs)
    r.units = {u: d.copy() for u, d in field.items()}
    return r


def test_restated_random_block_against_independent_references():
    """A closed random field over 2 x 2 x 2 units takes all 256 configurations; the restatement's mesh of it has a vertex at
    the fp64 rule's place on every sign-changing lattice edge and nowhere else, is closed and consistently oriented, and
    winds once around every negative voxel centre and not at all around the others."""
    vs = 0.013
    field = F_.random_field(F_.block((-1, -2, 3), (2, 2, 2)), seed=11, p_neg=0.5, closed=True)
    cfg = F_.configurations(field)
    assert np.all(cfg > 0), f"configurations never taken: {np.flatnonzero(cfg == 0).tolist()}"
    ntri, _, _ = mc.tables()
    assert set(np.flatnonzero(ntri == 5)) <= set(np.flatnonzero(cfg)) and int((ntri == 5).sum()) == 32
    v, f, c = _restated(field, vs).extract_mesh()
    assert len(f) == F_.triangle_total(field, ntri) and len(f) > 50000
    F_.check_vertices(field, vs, v, c)
    F_.check_directed_edges(f, len(v))
    F_.check_winding(field, vs, v, f, n=600, seed=5)


def test_restated_open_fields_follow_the_vertex_rule():
    """Weight-0 voxels, exact zeros of both signs and unallocated neighbours: the vertices are still those of the rule."""
    vs = 0.02
    field = F_.random_field(F_.block((0, 0, 0), (2, 1, 1)), seed=3, p_neg=0.4, w0=0.05, zeros=0.02)
    plus, minus = F_.zeros_next_to_negatives(field)
    assert plus > 0 and minus > 0
    v, f, c = _restated(field, vs).extract_mesh()
    assert F_.check_vertices(field, vs, v, c) > 1000
    assert len(f) == F_.triangle_total(field, mc.tables()[0])
    assert len(np.unique(f)) == len(v)


def test_winding_number_of_a_tetrahedron():
    """The solid-angle sum itself: 1 inside an outward-facing tetrahedron, 0 outside, -1 inside the reversed one."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    q = np.array([[0.1, 0.2, 0.3], [0.6, 0.6, 0.6], [-0.1, 0.2, 0.2]])
    assert np.allclose(F_.winding_numbers(v, f, q), [1, 0, 0], atol=1e-12)
    assert np.allclose(F_.winding_numbers(v, f[:, ::-1], q), [-1, 0, 0], atol=1e-12)


def test_room_views_reach_what_they_are_for():
    """Cameras inside the volume: voxels behind every camera and off all four image sides, walls on every image border."""
    d, vm, K, rgb = S.room_views(7, 33, 21, (30.0, 22.0, 13.3, 12.1), offset=(300.0, -200.0, 150.0))
    assert d.shape == (7, 21, 33, 1) and rgb.shape == (7, 21, 33, 3) and vm.dtype == np.float32
    assert np.all(K[:, 0, 0] != K[:, 1, 1]) and np.all(K[:, 0, 2] != 33 / 2)
    for edge in (d[:, 0], d[:, -1], d[:, :, 0], d[:, :, -1]):
        assert (edge > 0).all()
    r = RestatedTSDF(0.02, 0.06, 0.7)
    reach = S.projection_reach(r, d, vm, K, range(7))
    assert all(n > 0 for n in reach.values()), reach
    assert r.touched_units(d[0, ..., 0], vm[0], K[0]).min(0)[0] > 900


@pytest.mark.parametrize("scene", ["sphere", "plane"])
def test_touched_units_equal_brute_force(scene):
    if scene == "sphere":
        d, vm, K, _ = S.sphere_views(6, 64, 48)
        masks, r = [None] * 6, RestatedTSDF(0.02, 0.06, 3.0)
    else:
        d, vm, K, _, masks = S.plane_views(6, 64, 48)
        r = RestatedTSDF(0.005, 0.04, 0.9)
    ul = float(r.ulen)
    for j in range(6):
        got = {tuple(u) for u in r.touched_units(d[j, ..., 0], vm[j], K[j], masks[j])}
        want = set()
        H, W = d.shape[1:3]
        M, Kj = vm[j].astype(np.float32), K[j].astype(np.float32)
        for v in range(0, H, 4):
            for u in range(0, W, 4):
                z = d[j, v, u, 0]
                if not (z > 0 and z <= r.dtrunc) or (masks[j] is not None and not masks[j][v, u]):
                    continue
                xc = ((np.float32(u) - Kj[0, 2]) * z) / Kj[0, 0]
                yc = ((np.float32(v) - Kj[1, 2]) * z) / Kj[1, 1]
                dx, dy, dz = xc - M[0, 3], yc - M[1, 3], z - M[2, 3]
                p = np.array([(M[0, a] * dx + M[1, a] * dy) + M[2, a] * dz for a in range(3)], np.float32)
                lo, hi = p - r.trunc, p + r.trunc
                base = np.floor(p / ul).astype(int)
                for o in itertools.product(range(-3, 4), repeat=3):      # every unit whose span meets the box
                    k = base + np.array(o)
                    if np.all(k * ul <= hi) and np.all((k + 1) * ul > lo):
                        want.add(tuple(int(x) for x in k))
        assert got == want and len(got) > 0, j


def test_write_ply_round_trips(tmp_path):
    from collab_splats_amd import write_ply
    rng = np.random.default_rng(0)
    v = rng.standard_normal((17, 3)).astype(np.float32)
    f = rng.integers(0, 17, (9, 3)).astype(np.int32)
    c = rng.random((17, 3)).astype(np.float32)
    p = str(tmp_path / "m.ply")
    write_ply(p, torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c))
    data = open(p, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int(next(x for x in lines if x.startswith("element vertex")).split()[-1])
    nf = int(next(x for x in lines if x.startswith("element face")).split()[-1])
    assert (nv, nf) == (17, 9)
    vt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    ft = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    assert len(body) == nv * vt.itemsize + nf * ft.itemsize
    vr = np.frombuffer(body[:nv * vt.itemsize], vt)
    fr = np.frombuffer(body[nv * vt.itemsize:], ft)
    assert np.array_equal(np.stack([vr["x"], vr["y"], vr["z"]], 1), v)
    assert np.array_equal(np.stack([vr["r"], vr["g"], vr["b"]], 1), np.round(c * 255).astype(np.uint8))
    assert np.all(fr["n"] == 3) and np.array_equal(fr["i"], f)


def test_api_rejects_cpu_tensors_and_bad_shapes():
    from collab_splats_amd import MisplatError, TSDFVolume
    with pytest.raises(MisplatError, match="no CPU fallback"):
        TSDFVolume(0.01, 0.03, device="cpu")
    with pytest.raises(ValueError):
        TSDFVolume(0.0, 0.03, device="cuda")
    vol = TSDFVolume(0.01, 0.03, 1.0, device="cuda")
    d, vm, K = torch.ones(2, 8, 8, 1), torch.eye(4).repeat(2, 1, 1), torch.eye(3).repeat(2, 1, 1)
    with pytest.raises(ValueError, match="viewmats"):
        vol.integrate(d, vm[:1], K)
    with pytest.raises(ValueError, match="depths"):
        vol.integrate(torch.ones(2, 8), vm, K)
    with pytest.raises(ValueError, match="rgbs"):
        vol.integrate(d, vm, K, rgbs=torch.ones(2, 8, 8, 4))
    with pytest.raises(ValueError, match="masks"):
        vol.integrate(d, vm, K, masks=torch.ones(2, 8, 9, dtype=torch.bool))
    with pytest.raises(MisplatError, match="no CPU fallback"):
        vol.integrate(d, vm, K)


def test_grid_struct_layout_matches_c(built_lib):
    import ctypes as C
    import subprocess
    import tempfile
    from collab_splats_amd.tsdf import Grid
    fields = [f[0] for f in Grid._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"misplat.h\"\nint main(){printf(\"%zu\\n\", sizeof(misplat_tsdf_grid));\n"
    src += "".join(f'printf("%zu\\n", offsetof(misplat_tsdf_grid, {f}));\n' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        vals = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert vals[0] == C.sizeof(Grid)
    assert vals[1:] == [getattr(Grid, f).offset for f in fields]
