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
    _same(got, _ref(key, V, T, target, **{k: x for k, x in kw.items() if k != "dtype"}))
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


def _model():
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    sc = random_scene(600, 64, 48, seed=3)                                  # the scene of test_density_gpu.py::test_model_surface
    sc["means"][:, :2] *= 0.2
    sc["means"][:, 2] = (sc["means"][:, 2] - 2.0) * 0.2 + 1.0
    sc["log_scales"] += 1.2
    return radegs.RadegsModel(radegs.RadegsModelConfig(), sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"],
                              sc["sh"][:, 0], sc["sh"][:, 1:]).to(DEV).eval()


def test_model_mesh_with_target_triangles():
    model = _model()
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


# ------------------------------------------------------------------------- irregular, defective and workload-sized scenes
# S.CASES; what each reaches in the restatement (three-pass tables, both target branches, every refusal, a landing sort over
# two radix tiles) is asserted in test_decimate_host.py::test_restatement_on_the_irregular_scenes.
def _case(name, dtype=torch.int64):
    V, T, att, target, max_rounds = S.case(name)
    _REF[("case", name)] = S.reference(name)[0]
    return _check(("case", name), V, T, target, attributes=att, max_rounds=max_rounds, dtype=dtype)


@pytest.mark.parametrize("name", S.SMALL)
def test_irregular_and_defective_scenes(name):
    _case(name)                                                     # (positions compare as bits: defects' NaN rows too)


@pytest.mark.parametrize("name", ["high_behind", "high_scattered", "jitter272 3 rounds"])
def test_three_pass_tables_from_int32_triangles(name):
    _case(name, torch.int32)


def test_three_rounds_at_a_workload_size():
    got = _case("jitter272 3 rounds")
    assert got[4] == 3


def test_landing_sort_over_two_tiles_twice():
    got = _case("jitter272 landing")
    again = _run(*S.case("jitter272 landing")[:2], S.case("jitter272 landing")[3])
    assert again[4] == got[4] == 1 and torch.equal(again[0].view(torch.int32), got[0].view(torch.int32))
    assert torch.equal(again[1], got[1]) and torch.equal(again[3], got[3])


# ------------------------------------------------------------------------------------------ marching-cubes meshes, whole
def _against_the_restatement(v, t, c, target):
    from collab_splats_amd import simplify_quadric_decimation
    ref = R.simplify(v.cpu().numpy(), t.cpu().numpy(), target, (c.cpu().numpy(),))
    got = simplify_quadric_decimation(v, t, target, attributes=(c,))
    assert got[1].dtype == t.dtype
    _same(got, ref)
    return got, ref


def test_model_mesh_equals_the_restatement():
    """The marching-cubes mesh of test_model_mesh_with_target_triangles (287 closed blobs, slivers where the level set grazes
    a lattice point) to half its faces, the colours as the attribute: the exporter's call, and the plain call on its raw mesh."""
    model = _model()
    v, t, c = model.marching_cubes_mesh(voxel_size=0.04)
    n = t.shape[0] // 2
    got, ref = _against_the_restatement(v, t, c, n)
    mv, mt, mc = model.marching_cubes_mesh(voxel_size=0.04, target_triangles=n)
    assert mt.dtype == t.dtype and np.array_equal(mt.cpu().numpy(), ref[1])
    assert np.array_equal(mv.cpu().numpy().view(np.int32), ref[0].view(np.int32))
    assert np.array_equal(mc.cpu().numpy().view(np.int32), ref[2][0].view(np.int32))


def test_open_level_set_mesh_equals_the_restatement():
    """density_scenes.clipped at 0.5: the bounds cut through the wide Gaussian's level set, and marching cubes emits no cell
    beyond them, so the mesh ends in boundary loops."""
    import density_scenes as DS
    from collab_splats_amd import DensityField
    sc = DS.scene("clipped")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)      # noqa: E731
    f = DensityField(dev(sc["means"]), dev(sc["quats"]), dev(sc["scales"]), dev(sc["opacities"]), sc["h"], bounds=sc["bounds"])
    vals = np.random.default_rng(3).uniform(0, 1, (f.n_gauss, 3)).astype(np.float32)
    v, t, c = f.extract_mesh(0.5, values=dev(vals))
    _, boundary, nonmanifold = S.edge_counts(t.cpu().numpy())
    print("clipped at 0.5:", tuple(v.shape), tuple(t.shape), "boundary edges", boundary, "non-manifold", nonmanifold)
    assert t.shape[0] > 200 and boundary > 0
    _against_the_restatement(v, t, c, t.shape[0] // 2)


# ------------------------------------------------------------------------------------------------------- entry points
def _entry_state(dead=()):
    import ctypes as C
    from collab_splats_amd._lib import load
    V, T = S.icosphere(1)
    st = dict(lib=load(), M=len(V), T=len(T), pos=torch.from_numpy(V).to(DEV),
              tri=torch.from_numpy(T).to(DEV).to(torch.int32).contiguous(), alive=torch.ones(len(T), dtype=torch.int32, device=DEV),
              quadrics=torch.zeros((len(V), 10), dtype=torch.float64, device=DEV),
              into=torch.full((len(V),), -1, dtype=torch.int32, device=DEV),
              counts=torch.full((3,), -7, dtype=torch.int32, device=DEV))
    for f in dead:
        st["alive"][f] = 0
    st["bytes"] = int(st["lib"].misplat_decimate_workspace(C.c_int64(st["M"]), C.c_int64(st["T"])))
    assert st["bytes"] > 0
    st["ws"] = torch.full((st["bytes"] + 4096,), 0xA5, dtype=torch.uint8, device=DEV)      # the last 4 KiB: a guard
    return st


def _round(st, n_alive, ws_bytes=None, null=None, first=1):
    import ctypes as C
    from collab_splats_amd._lib import ptr, stream_ptr
    p = {k: (C.c_void_p(0) if k == null else ptr(st[k])) for k in ("pos", "tri", "alive", "quadrics", "ws", "counts")}
    return st["lib"].misplat_decimate_round(p["pos"], C.c_int64(st["M"]), p["tri"], C.c_int64(st["T"]), p["alive"], C.c_int64(n_alive),
                                            p["quadrics"], first, p["ws"], C.c_int64(st["bytes"] if ws_bytes is None else ws_bytes),
                                            p["counts"], stream_ptr())


def _apply(st, n_alive, n_selected, channels=0, att=None, ws_bytes=None):
    import ctypes as C
    from collab_splats_amd._lib import ptr, stream_ptr
    return st["lib"].misplat_decimate_apply(ptr(st["pos"]), C.c_int64(st["M"]), ptr(st["tri"]), C.c_int64(st["T"]), ptr(st["alive"]),
                                            C.c_int64(n_alive), ptr(att), channels, ptr(st["quadrics"]), ptr(st["into"]),
                                            C.c_int64(n_selected), C.c_int64(-1), ptr(st["ws"]),
                                            C.c_int64(st["bytes"] if ws_bytes is None else ws_bytes), stream_ptr())


def _snapshot(st):
    torch.cuda.synchronize()
    return {k: st[k].clone() for k in ("pos", "tri", "alive", "quadrics", "into", "counts", "ws")}


def _unchanged(st, before, keys):
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(st[k].view(torch.uint8), before[k].view(torch.uint8)), k


def test_entry_points_refuse_what_the_header_excludes():
    """MISPLAT_EINVAL (-1) and MISPLAT_EWORKSPACE (-3) before any launch: no tensor of the state and no byte of the workspace
    changes."""
    import ctypes as C
    st = _entry_state()
    lib, M, T = st["lib"], st["M"], st["T"]
    limit = ((1 << 31) - 4096 + 5) // 6                             # the smallest T with 6 T >= 2^31 - 4096
    assert 6 * limit >= (1 << 31) - 4096 > 6 * (limit - 1)
    assert lib.misplat_decimate_workspace(C.c_int64(M), C.c_int64(0)) == -1
    assert lib.misplat_decimate_workspace(C.c_int64(3), C.c_int64(limit)) == -1
    assert lib.misplat_decimate_workspace(C.c_int64(3), C.c_int64(limit - 1)) > 0
    before = _snapshot(st)
    everything = tuple(before)
    for null in ("pos", "tri", "alive", "quadrics", "ws", "counts"):
        assert _round(st, T, null=null) == -1, null
    assert _round(st, T + 1) == -1 and _round(st, 0) == -1
    assert _round(st, T, ws_bytes=st["bytes"] - 1) == -3
    att = torch.zeros((M, 4097), dtype=torch.float32, device=DEV)
    assert _apply(st, T, 0) == -1 and _apply(st, T, T + 1) == -1
    assert _apply(st, T, 1, channels=4097, att=att) == -1
    assert _apply(st, T, 1, channels=3, att=None) == -1              # channels without attributes
    assert _apply(st, T, 1, ws_bytes=st["bytes"] - 1) == -3
    _unchanged(st, before, everything)


@pytest.mark.parametrize("off", [-1, 0, 1])
def test_round_with_a_wrong_live_count(off):
    """decimate.hip: "a wrong n_alive reads face 0, never beyond the list".  Every access of live_list_kernel, emit_kernel and
    what follows them is bounded by the n passed in (the list is zeroed first and only positions below n are written), so a count
    one too small leaves the last live face out and one too large lists face 0 twice: counts[0] still reports the true
    count (what the wrapper checks), the mesh is untouched, nothing is written past the declared workspace."""
    st = _entry_state(dead=(17,))
    true = st["T"] - 1
    before = _snapshot(st)
    assert _round(st, true + off) == 0
    _unchanged(st, before, ("pos", "tri", "alive", "into"))
    counts = st["counts"].tolist()
    assert counts[0] == true and 0 < counts[1] <= counts[2] <= 2 * counts[1]
    assert bool((st["ws"][st["bytes"]:] == 0xA5).all())
    if off == 0:                                                    # the consistent call: the restatement's first round
        V, T = S.icosphere(1)
        rounds = []
        R.simplify(V, np.delete(T, 17, 0), 0, max_rounds=1, on_round=lambda *a: rounds.append(S.round_account(*a)))
        assert counts[1:] == [rounds[0]["selected"], rounds[0]["selected_faces"]]
