"""CPU: what tests/meshsmooth_restatement.py (the oracle of tests/test_meshsmooth_gpu.py) computes on the scenes of
tests/meshsmooth_scenes.py -- the properties each scene was chosen for -- the arithmetic of the LDS cut-off of the
angle-and-area table, the mirrors of the constants, and the argument checks of the new options.  Without the feature every test
here fails: the package has no ``fair_vertices_curvature``, ``triangulate_holes`` no ``metric``."""
import os
import re

import numpy as np
import pytest
import torch

import meshfill_restatement as MF
import meshsmooth_restatement as R
import meshsmooth_scenes as S
import meshtri_restatement as MT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _the_feature_is_there():
    from collab_splats_amd import fair_vertices_curvature, meshfill  # noqa: F401
    assert "angle_area" in meshfill.METRICS and "curvature" in meshfill.FAIRINGS


def _patch(name, metric="angle_area"):
    V, T, att, size = S.triangulate_case(name)
    v, t, a, n_filled, info = S.triangulate_reference(name, metric)
    return V, T, t[len(T):], n_filled, info


# -------------------------------------------------------------------------------------------------------- constants
def _header(name):
    with open(os.path.join(ROOT, "include", "misplat.h")) as f:
        return int(re.search(rf"#define {name} (\d+)", f.read()).group(1))


def test_constants_mirror_the_header():
    from collab_splats_amd import meshfill
    for name, mirrors in (("MISPLAT_MESHTRI_ANGLE_LDS_LOOP", (meshfill.ANGLE_LDS_LOOP, R.ANGLE_LDS_LOOP, S.ANGLE_LDS_LOOP)),
                          ("MISPLAT_MESHTRI_ANGLE_STEPS", (meshfill.ANGLE_STEPS, R.ANGLE_STEPS)),
                          ("MISPLAT_MESHTRI_SMALL_LOOP", (meshfill.SMALL_LOOP, R.SMALL_LOOP, S.SMALL_LOOP)),
                          ("MISPLAT_MESHFILL_CG_VERTICES", (meshfill.CG_VERTICES, R.CG_VERTICES))):
        assert all(x == _header(name) for x in mirrors), name
    assert (_header("MISPLAT_MESHTRI_LDS_LOOP"), _header("MISPLAT_MESHTRI_MAX_LOOP"), _header("MISPLAT_MESHTRI_SMALL_LOOP")) == (176, 1024, 64)


def test_the_lds_cutoff_is_the_largest_loop_that_fits():
    """An entry is an fp64 area sum, a 16-bit badness and a 16-bit split; a polygon vertex its three fp32 coordinates, its int32
    index and its rim corner's three fp32 coordinates; a workgroup may declare 163840 bytes."""
    def bytes_of(n):
        return (8 + 2 + 2) * (n * (n - 1) // 2) + (12 + 4 + 12) * n
    n = _header("MISPLAT_MESHTRI_ANGLE_LDS_LOOP")
    assert bytes_of(n) <= 163840 < bytes_of(n + 1) and (n, bytes_of(n)) == (163, 163000)
    assert _header("MISPLAT_MESHTRI_SMALL_LOOP") < n < _header("MISPLAT_MESHTRI_LDS_LOOP")
    assert _header("MISPLAT_MESHTRI_ANGLE_STEPS") + 1 < 1 << 16              # the badness and "no candidate yet" fit 16 bits
    assert 1.0 - np.cos(np.radians(3.6)) > 2.0 / 1024 > 1.0 - np.cos(np.radians(3.5))      # bucket 1 starts at about 3.6 degrees


# ---------------------------------------------------------------------------------------------------- triangulation
@pytest.mark.parametrize("name", ["square_tie", "convex", "c_shape"])
def test_a_planar_hole_is_decided_by_the_area(name):
    V, T, faces, n_filled, info = _patch(name)
    _, _, faces_a, _, info_a = _patch(name, "area")
    assert n_filled == 1 and np.array_equal(faces, faces_a) and info["badness"].tolist() == [0]
    assert np.array_equal(info["area"].view(np.int64), info_a["area"].view(np.int64))
    assert (S.face_normals(V, T)[:, 2] > 0).all() and (S.face_normals(V, faces)[:, 2] > 0).all()
    if name != "square_tie":
        P = S.convex_polygon() if name == "convex" else S.c_polygon()
        assert info["area"].tolist() == [S.polygon_area(P)]


def test_the_ridge_quad_separates_the_metrics():
    V, T, faces, _, info = _patch("ridge_quad")
    _, _, faces_a, _, info_a = _patch("ridge_quad", "area")
    assert faces_a.tolist() == [[0, 1, 3], [1, 2, 3]] and faces.tolist() == [[0, 1, 2], [0, 2, 3]]
    assert info_a["area"][0] < info["area"][0]                      # the area alone prefers the other diagonal
    assert info["badness"].tolist() == [72] == [R.triangulation_badness(V, T, faces)]
    assert R.triangulation_badness(V, T, faces_a) == 149
    # the buckets of the docstring's angles: 45 degrees, 45 - atan(1/4), acos(16/17)
    assert [int(np.floor((1 - np.cos(a)) * 512)) for a in (np.pi / 4, np.pi / 4 - np.arctan(0.25), np.arccos(16 / 17))] == [149, 72, 30]


@pytest.mark.parametrize("name", ["triangle", "ridge_quad", "pentagon", "collinear", "three_loops", "small_cutoff", "lds_cutoff"])
def test_every_apex_once_and_no_new_vertex(name):
    V, T, faces, n_filled, info = _patch(name)
    v, t = S.triangulate_reference(name)[:2]
    assert len(v) == len(V) and info["n_fans"] == 0 and info["fallback"].tolist() == [0] * n_filled
    loop, edges, _, perimeter = R.MC.mesh_holes(V, T)
    size = S.triangulate_case(name)[3]
    at = 0
    for l in np.flatnonzero(perimeter < size):
        code, q = MT.loop_polygon(edges[loop == l].astype(np.int64))
        mine = faces[at:at + len(q) - 2]
        at += len(q) - 2
        assert np.array_equal(mine[:, 1], q[1:-1])                  # apex k = 1 .. n - 2, each once, in order
        assert np.isin(mine, q).all()
    assert at == len(faces)
    # the Euler characteristic rises by one per closed loop (a face more than edges, no vertex)
    def euler(tri):
        return len(np.unique(tri)) - S.edge_counts(tri)[0] + len(tri)
    assert euler(t) == euler(T) + n_filled
    assert info["badness"].tolist() == [R.triangulation_badness(V, T, faces)] if n_filled == 1 else True


def test_a_zero_area_candidate_has_no_crease():
    V, T, faces, _, info = _patch("collinear")
    Q = V[:5]
    assert MT.area(Q, 1, 2, 3) == 0 and int(R.crease(R.face_normal(Q[1], Q[2], Q[3]), np.array([0.0, 0.0, 1.0]))) == 0
    assert info["badness"].tolist() == [0] and not any(sorted(f) == [1, 2, 3] for f in faces.tolist())
    assert info["area"].tolist() == [3.0]


def test_the_fallbacks_keep_their_codes_and_fans():
    V, T, faces, n_filled, info = _patch("fallbacks")
    ref = MT.triangulate_holes(V, T, S.triangulate_case("fallbacks")[3], S.triangulate_case("fallbacks")[2])
    assert info["fallback"].tolist() == [MT.NOT_SIMPLE, MT.TOO_SHORT, MT.TOO_LONG, MT.TOO_LONG] and len(info["badness"]) == 0
    assert np.array_equal(S.triangulate_reference("fallbacks")[1], ref[1])


# ---------------------------------------------------------------------------------------------------------- fairing
SOLVED = ["one_vertex", "planar_fan", "sphere_cap", "block_1023", "block_1024", "block_1025", "two_patches", "shared_rim"]


def test_a_planar_fan_keeps_the_bits_of_its_z():
    V, T, free, _ = S.fair_case("planar_fan")
    out, info = S.fair_reference("planar_fan")
    assert np.array_equal(out[:, 2].view(np.int32), V[:, 2].view(np.int32)) and not np.array_equal(out[free, :2], V[free, :2])
    assert np.array_equal(out[~free].view(np.int32), V[~free].view(np.int32))


def test_the_thin_plate_cap_is_closer_to_the_sphere_than_the_membrane():
    V, T, free, _ = S.fair_case("sphere_cap")
    out, info = S.fair_reference("sphere_cap")
    membrane = MF.fair(V, T, free, np.float32(1e-3 * S.mean_edge_length(V, T)), 10000, ())[0]
    plate, lid = S.radial_error(out, free), S.radial_error(membrane, free)
    print(f"sphere cap: {int(free.sum())} free, flat {S.radial_error(V, free):.4g}, membrane {lid:.4g}, thin plate {plate:.4g}")
    assert plate < 0.25 * lid


@pytest.mark.parametrize("name", SOLVED)
def test_cg_reaches_the_direct_solve(name):
    """Within 1e-3 mean edge lengths of numpy.linalg.solve on the dense system, converged, and in fewer iterations than the
    bound (the patch's free count).  A patch of one or two unknowns is the exception to the last: CG needs as many iterations as
    it has unknowns, which is the bound itself, so there the count is only held to the bound."""
    V, T, free, _ = S.fair_case(name)
    out, info = S.fair_reference(name)
    solved = info["code"] == 0
    assert info["converged"][solved].all() and not info["converged"][~solved].any()
    _, patches = R.curvature_patches(T, free)
    for (Fp, _), it, code in zip(patches, info["iterations"], info["code"]):
        assert (it < len(Fp) or it == len(Fp) <= 2) if code == 0 else it == 0
    direct = R.direct_curvature(V, T, free)
    far = np.linalg.norm(out.astype(np.float64) - direct, axis=1).max() / S.mean_edge_length(V, T)
    print(f"{name}: iterations {info['iterations'].tolist()}, {far:.3g} mean edge lengths from the direct solve")
    assert far < 1e-3


def test_patches_codes_and_the_cap():
    _, info = S.fair_reference("two_patches")
    assert info["code"].tolist() == [0, 0, 0, 1] and info["iterations"].tolist()[2:] == [1, 0]
    V, T, free, _ = S.fair_case("shared_rim")
    _, patches = R.curvature_patches(T, free)
    assert len(patches) == 1 and patches[0][0].tolist() == [6, 18] and 12 in patches[0][1].tolist()
    assert S.fair_reference("closed")[1]["code"].tolist() == [2]
    out, info = S.fair_reference("too_large")
    assert info["code"].tolist() == [3] and int(S.fair_case("too_large")[2].sum()) == 257 * 257 > R.CG_VERTICES
    assert np.array_equal(out.view(np.int32), S.fair_case("too_large")[0].view(np.int32))
    info = S.fair_reference("capped")[1]
    assert info["iterations"].tolist() == [3] and info["converged"].tolist() == [False] and info["residual"][0] > 1e-6


def test_the_stop_is_translation_invariant():
    """The stop is relative to the start's residual, which a translation of the whole mesh leaves alone: far from the origin
    the solve still converges below its own bound and lands on the same surface.  The translated input is rounded to fp32 at a
    magnitude of 64 (half an ulp is 3.8e-6 a coordinate), so the two results agree to that order, not to the bit: within 1e-3
    mean edge lengths (1.5e-4 here), the bar of the direct solve."""
    V, T, free, _ = S.fair_case("sphere_cap")
    shift = np.float32([64, -32, 16])
    a, b = R.fair_curvature(V, T, free), R.fair_curvature(V + shift, T, free)
    assert b[1]["converged"].all() and int(b[1]["iterations"][0]) < int(free.sum())
    far = np.abs((b[0].astype(np.float64) - shift) - a[0]).max() / S.mean_edge_length(V, T)
    assert far < 1e-3


def test_the_dot_product_order():
    x = np.random.default_rng(0).standard_normal(3000)
    assert abs(R.block_dot(x, x) - float(x @ x)) < 1e-9 and R.block_dot(x[:0], x[:0]) == 0.0
    assert R.block_dot(np.array([1e16, 1.0, -1e16]), np.ones(3)) == 1.0         # three threads, then the tree: (1e16 + -1e16) + 1


# --------------------------------------------------------------------------------------------------------- the fill
def test_the_smooth_fill_on_the_restatement():
    V, T, att, size, max_len = S.fill_case("cut_sphere")
    v, t, a, n_filled, info = S.fill_reference("cut_sphere", **S.SMOOTH)
    m = S.fill_reference("cut_sphere", triangulation="min_area", metric="angle_area", flip=True)
    new = np.arange(len(v)) >= len(V)
    assert n_filled == 1 and info["n_fans"] == 0 and len(S.boundary_edges(t)) == 0
    assert info["curvature_code"].tolist() == [0] and info["curvature_converged"].tolist() == [True]
    assert np.array_equal(v[:len(V)].view(np.int32), V.view(np.int32)) and np.array_equal(t[:len(T)], T)
    assert np.array_equal(t, m[1]) and np.array_equal(a[0].view(np.int32), m[2][0].view(np.int32))
    assert S.radial_error(v, new) < S.radial_error(m[0], new)
    print(f"cut sphere: membrane {S.radial_error(m[0], new):.4g}, curvature {S.radial_error(v, new):.4g}")


# -------------------------------------------------------------------------------------------------------- arguments
def _mesh():
    return torch.tensor([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=torch.float32), torch.tensor([[0, 1, 2], [0, 2, 3]])


@pytest.mark.parametrize("kw", [dict(rtol=-1.0), dict(rtol="tight"), dict(rtol=float("inf")), dict(max_iterations=-1),
                                dict(max_iterations=2.5), dict(free=torch.ones(3, dtype=torch.bool)), dict(free=torch.ones(4))])
def test_curvature_arguments(kw):
    from collab_splats_amd import fair_vertices_curvature
    v, t = _mesh()
    args = dict(free=torch.ones(4, dtype=torch.bool))
    args.update(kw)
    with pytest.raises(ValueError, match="fair_vertices_curvature"):
        fair_vertices_curvature(v, t, **args)


def test_option_arguments_and_cpu_tensors():
    from collab_splats_amd import MisplatError, fair_vertices_curvature, fill_holes_nicely, triangulate_holes
    v, t = _mesh()
    with pytest.raises(ValueError, match="metric must be"):
        triangulate_holes(v, t, metric="dihedral")
    with pytest.raises(ValueError, match="metric must be"):
        fill_holes_nicely(v, t, triangulation="min_area", metric="dihedral")
    with pytest.raises(ValueError, match="needs triangulation='min_area'"):
        fill_holes_nicely(v, t, metric="angle_area")
    with pytest.raises(ValueError, match="fairing must be"):
        fill_holes_nicely(v, t, fairing="willmore")
    with pytest.raises(MisplatError, match="no CPU fallback"):
        triangulate_holes(v, t, metric="angle_area")
    with pytest.raises(MisplatError, match="no CPU fallback"):
        fair_vertices_curvature(v, t, torch.ones(4, dtype=torch.bool))
    with pytest.raises(MisplatError, match="no CPU fallback"):
        fill_holes_nicely(v, t, triangulation="min_area", metric="angle_area", fairing="curvature")


def test_finish_mesh_knows_smooth():
    import tsdf_scenes
    v, t = _mesh()
    model = tsdf_scenes.sphere_gaussians(16)
    with pytest.raises(ValueError, match="'min_area' or 'smooth'"):
        model.finish_mesh(v, t, torch.zeros(4, 3), fill="smoothest")
