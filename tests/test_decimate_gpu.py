"""GPU: quadric-error simplification (csrc/decimate.hip) against tests/decimate_restatement.py.  Every case compares with the
restatement for equality: position bits, triangles, vertex_map, attribute bits, rounds.  What is asserted about a result beyond
that (closedness, outline, area, loops) was first checked on the restatement's output, on the CPU."""
import numpy as np
import pytest
import torch

import decimate_restatement as R
import decimate_scenes as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_REF = {}


def _ref(key, V, T, target, attributes=(), max_rounds=256):
    if key not in _REF:
        _REF[key] = R.simplify(V, T, target, attributes, max_rounds)
    return _REF[key]


def _run(V, T, target, attributes=(), max_rounds=256, dtype=torch.int64):
    from collab_splats_amd import simplify_quadric_decimation
    v, t, a, vm, r = simplify_quadric_decimation(torch.from_numpy(np.ascontiguousarray(V)).to(DEV),
                                                 torch.from_numpy(np.ascontiguousarray(T)).to(DEV).to(dtype), target,
                                                 tuple(torch.from_numpy(x).to(DEV) for x in attributes), max_rounds)
    assert v.dtype == torch.float32 and t.dtype == dtype and vm.dtype == torch.int64 and isinstance(r, int)
    return v, t, a, vm, r


def _same(got, ref):
    v, t, a, vm, r = got
    rv, rt, ra, rvm, rr = ref
    assert r == rr
    assert tuple(t.shape) == rt.shape and np.array_equal(t.cpu().numpy().astype(np.int64), rt.astype(np.int64))
    assert tuple(v.shape) == rv.shape and np.array_equal(v.cpu().numpy().view(np.int32), rv.view(np.int32))
    assert np.array_equal(vm.cpu().numpy(), rvm)
    assert len(a) == len(ra)
    for x, rx in zip(a, ra):
        assert tuple(x.shape) == rx.shape and np.array_equal(x.cpu().numpy().view(np.int32), rx.view(np.int32))


def _check(key, V, T, target, **kw):
    got = _run(V, T, target, **kw)
    _same(got, _ref(key, V, T, target, **kw))
    return got


def _stats(v, t):
    from collab_splats_amd import mesh_components, mesh_edge_stats
    st = mesh_edge_stats(v, t)
    return st, int(mesh_components(v, t)[1].shape[0])


@pytest.mark.parametrize("level,target", [(3, 320), (2, 80)])
def test_icosphere_stays_a_closed_sphere(level, target):
    V, T = S.icosphere(level)
    v, t, _, vm, _ = _check(("ico", level), V, T, target)
    n = t.shape[0]
    assert target - 2 < n <= target
    st, comps = _stats(v, t)
    assert st["n_boundary"] == 0 and st["n_nonmanifold"] == 0 and comps == 1
    assert v.shape[0] - st["n_edges"] + n == 2
    assert int(vm.min()) >= 0 and int(vm.max()) == v.shape[0] - 1


def test_sheet_keeps_its_plane_outline_and_area():
    V, T = S.sheet(32)
    v, t, _, _, _ = _check("sheet32", V, T, 200)
    assert 198 < t.shape[0] <= 200
    assert bool((v[:, 2] == 0).all())
    for corner in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)):
        assert bool((v == torch.tensor(corner, dtype=torch.float32, device=DEV)).all(1).any()), corner
    assert abs(S.total_area(v.cpu().numpy(), t.cpu().numpy()) - 1.0) <= 1e-6
    assert _stats(v, t)[0]["n_nonmanifold"] == 0


def test_holes_survive():
    from collab_splats_amd import mesh_holes
    V, T = S.sheet(64, S.THREE_HOLES)
    before = int(mesh_holes(torch.from_numpy(V).to(DEV), torch.from_numpy(T).to(DEV))[2].shape[0])
    v, t, _, _, _ = _check("holes", V, T, 1000)
    assert 998 < t.shape[0] <= 1000
    assert before == 4 and int(mesh_holes(v, t)[2].shape[0]) == before


def test_no_triangle_and_one_triangle():
    V = np.eye(3, dtype=np.float32)
    v, t, _, vm, r = _check("T0", V, np.zeros((0, 3), np.int64), 0)
    assert v.shape == (0, 3) and t.shape == (0, 3) and r == 0 and vm.tolist() == [-1, -1, -1]
    v, t, _, vm, r = _check("T1", V, np.array([[0, 1, 2]]), 0)
    assert t.shape == (0, 3) and r == 1
    v, t, _, vm, r = _check("T1keep", V, np.array([[0, 1, 2]]), 1)
    assert t.tolist() == [[0, 1, 2]] and r == 0


def test_257_triangles_and_a_repeated_corner():
    V, T = S.sheet(16)
    T = T[:257].copy()
    T[100] = [5, 5, 9]                                              # dropped first
    v, t, _, _, _ = _check("T257", V, T, 100)
    assert 98 < t.shape[0] <= 100


def test_target_at_or_above_the_count_is_the_identity_up_to_compaction():
    V, T = S.sheet(8, [(2, 5, 2, 5)])                               # grid vertices inside the hole are unreferenced
    for target in (len(T), len(T) + 7):
        v, t, _, vm, r = _check(("id", target), V, T, target)
        used = np.zeros(len(V), bool)
        used[T.reshape(-1)] = True
        assert r == 0 and np.array_equal(v.cpu().numpy(), V[used]) and t.shape[0] == len(T)
        assert np.array_equal(V[used][t.cpu().numpy()], V[T])
        assert np.array_equal(vm.cpu().numpy() >= 0, used) and bool((vm[torch.from_numpy(~used).to(DEV)] == -1).all())


def test_target_zero_stops_by_itself():
    V, T = S.icosphere(1)
    v, t, _, _, r = _check("ico1->0", V, T, 0)
    assert t.shape[0] >= 4 and r < 256
    st, comps = _stats(v, t)
    assert st["n_boundary"] == 0 and st["n_nonmanifold"] == 0 and comps == 1


def test_max_rounds_bounds_the_loop():
    V, T = S.icosphere(2)
    v, t, _, _, r = _check("ico2 3 rounds", V, T, 80, max_rounds=3)
    assert r == 3 and t.shape[0] > 80


def test_hub_of_valence_300():
    V, T = S.fan(300)
    v, t, _, _, _ = _check("fan", V, T, 100)
    assert 98 < t.shape[0] <= 100


def test_four_face_edge_is_never_collapsed():
    V, T = S.tetra_pair(2)
    v, t, _, _, _ = _check("tetra2", V, T, 0)
    assert _stats(v, t)[0]["n_nonmanifold"] == 1                    # the shared edge is still there, with its four faces


def test_unreferenced_vertices_map_to_minus_one():
    V, T = S.icosphere(1)
    V = np.concatenate([np.full((3, 3), 9.0, np.float32), V, np.full((2, 3), -9.0, np.float32)])
    v, t, _, vm, _ = _check("loose", V, T + 3, 40)
    assert vm[:3].tolist() == [-1] * 3 and vm[-2:].tolist() == [-1] * 2 and float(v.abs().max()) < 2


def test_two_components_both_survive_closed():
    V, T = S.merge(S.icosphere(2), S.icosphere(1, 0.3, (3.0, 0.0, 0.0)))
    v, t, _, _, _ = _check("merge", V, T, 120)
    st, comps = _stats(v, t)
    assert comps == 2 and st["n_boundary"] == 0 and st["n_nonmanifold"] == 0
    assert 118 < t.shape[0] <= 120


def test_attributes_dtypes_and_determinism():
    V, T = S.icosphere(2)
    att = (S.colour_ramp(V), np.full((len(V), 2), 0.7, np.float32))
    got = _check("attrs", V, T, 80, attributes=att)
    assert bool((got[2][1] == 0.7).all()) and got[2][0].shape == got[0].shape
    again = _run(V, T, 80, attributes=att)
    small = _run(V, T, 80, attributes=att, dtype=torch.int32)
    for other in (again, small):
        assert other[4] == got[4] and torch.equal(other[0].view(torch.int32), got[0].view(torch.int32))
        assert torch.equal(other[1].long(), got[1]) and torch.equal(other[3], got[3])
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(other[2], got[2]))


def test_model_mesh_with_target_triangles():
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    sc = random_scene(600, 64, 48, seed=3)                                  # the scene of test_density_gpu.py::test_model_surface
    sc["means"][:, :2] *= 0.2
    sc["means"][:, 2] = (sc["means"][:, 2] - 2.0) * 0.2 + 1.0
    sc["log_scales"] += 1.2
    model = radegs.RadegsModel(radegs.RadegsModelConfig(), sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"],
                               sc["sh"][:, 0], sc["sh"][:, 1:]).to(DEV).eval()
    raw = model.marching_cubes_mesh(voxel_size=0.04)
    same = model.marching_cubes_mesh(voxel_size=0.04, target_triangles=None)
    assert all(x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(raw, same))
    # half the faces: the level set of this scene is 287 small closed blobs (3 384 faces), and a closed component stops at its
    # last four faces (the tetrahedron, where every collapse would fold two faces onto each other): 1 148, above a fifth
    n = raw[1].shape[0] // 2
    v, t, c = model.marching_cubes_mesh(voxel_size=0.04, target_triangles=n)
    assert 0 < t.shape[0] <= n and t.dtype == raw[1].dtype and int(t.min()) >= 0 and int(t.max()) < v.shape[0]
    assert c.shape == v.shape and float(c.min()) >= 0 and float(c.max()) <= 1 and bool(torch.isfinite(v).all())
    with pytest.raises(ValueError, match="target_triangles"):
        model.marching_cubes_mesh(voxel_size=0.04, target_triangles=-1)
