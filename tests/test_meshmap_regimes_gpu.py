"""GPU: the kNN vertex map (csrc/meshmap.hip) off the one regime of tests/test_meshmap_gpu.py, against the restatement
(tests/meshmap_restatement.py) on the scenes of tests/meshmap_regimes_scenes.py, whose stated properties
tests/test_meshmap_regimes_host.py holds on the CPU.  Neighbour indices, distance bits and validity are compared bit for bit
everywhere.  Values: bit for bit with the ordered fp32 restatement where no exp is involved (k = 1, sigma = 0: the chunk
boundaries), bit for bit between calls that must agree (channels, views, non-finite rows), and otherwise within the
per-vertex bar of the fp64 aggregation.

The per-vertex bar (meshmap_regimes_scenes.vertex_bound), with u = 2^-24 and every term from the restatement alone.

Weights.  The fp64 reference has x = (dj^2 - d0^2) c, c = 1 / (2 sigma^2), e = exp(-x), w = e / sum_j e.  The kernel has
fl(dj dj) = dj^2 (1 + d1), fl(d0 d0) = d0^2 (1 + d2), their difference (1 + d3), c rounded to fp32 (1 + d4; the fp64 sum
behind sigma runs in another order than numpy's, which moves c by less than 2^-40 and is counted as a fifth u on x), the
product (1 + d5), all |d| <= u: its argument is off by at most u (dj^2 + d0^2) c + 4 u x = u (s + 4 x), so its exponential
by the factor exp(u (s + 4 x)).  expf is documented at 1 ulp on the device; numpy's fp32 exp, which the fp32 yardstick
uses, documents under 3; EXP_ULPS = 3 ulp = 6 u covers both.  So e_j is off relatively by at most
ee_j = exp(u (s_j + 4 x_j)) (1 + 6 u) - 1, and by nothing where dj = d0 (both sides have e = 1, j = 0 among them).  The
row sum of k positive terms in j order adds (1 + u)^(k-1), each term carrying its own error: relatively
eta = sum_j w_j ((1 + ee_j) (1 + u)^(k-1) - 1).  The division adds u: w_j is off relatively by at most
eps_j = (1 + ee_j) (1 + u) / (1 - eta) - 1.  eps_v is the largest eps over the contributions that reach v.  (A weight that
underflows in fp32 would have relative error 1: the bound refuses a scene with x >= 80, and no scene here has one.)

A weighted mean under perturbed weights.  out' = sum w (1 + eps) f / sum w (1 + eps) and out = sum w f / sum w differ by
sum w eps (f - out) / sum w (1 + eps), because sum w (f - out) = 0: at most eps_v / (1 - eps_v) times
B_v = sum w |f - out| / sum w, the weighted mean deviation.  B_v <= A_v + |out| <= 2 A_v with A_v = sum w |f| / sum w: the
plain product eps_v A_v would not be a bound (the denominator moves too), eps_v B_v is, and it is 0 for a vertex with one
contribution, whose value is f whatever the weight.

Sums.  A list of L contributions is summed from 0 in chunks of kChunk and the C = ceil(L / kChunk) chunk sums from 0 in chunk
order: n = min(L, kChunk) - 1 + C - 1 roundings on the path of any term, one more in the numerator for the product w f.
With g_num = (1 + u)^(n+1) - 1 and g_den = (1 + u)^n - 1 the computed quotient is within
(g_num A' + g_den |out'|) / (1 - g_den) of out', where A' <= A_v (1 + eps_v) / (1 - eps_v).  The final division rounds once:
a factor (1 + u) on the error so far and u |out|, for which the bar has 2^-23 |ref64|.  Together

    bound_v = [eps_v/(1-eps_v) B_v + (g_num A_v + g_den (|ref64| + eps_v/(1-eps_v) B_v)) (1+eps_v)/((1-eps_v)(1-g_den))] (1+u)
              + 2^-23 |ref64|

which to first order is (gamma_v + eps_v) A_v + 2^-23 |ref64| with gamma_v = (2 n + 1) u and B_v in the place of its ceiling
2 A_v.  Products and sums are assumed not to underflow (the smallest magnitudes here are 1e-3 times weights above e^-80).

The unit step.  n = o / (|o| + 1e-8) moves by at most 2 |delta| / (|o| + 1e-8) when o moves by delta (the numerator by
|delta|, the denominator by at most |delta|), |delta| the 2-norm of the three bounds above; the fp32 step itself rounds
three squares and two sums (3 u on the squared norm, 1.5 u after the root), the root, the sum with 1e-8 and the division:
4 u on a component of at most 1, and float32(1e-8) for 1e-8 moves the quotient by |float32(1e-8) - 1e-8| / (|o| + 1e-8).

tests/test_meshmap_regimes_host.py holds the fp32 yardstick (aggregate_ordered) to this bar at every covered vertex of
every scene below that uses it, and the bar to the old tensor-wide one (1e-5 max|F|) on the unit-magnitude blobs."""
import numpy as np
import pytest
import torch

import meshmap_regimes_scenes as S
import meshmap_restatement as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(x, dtype=np.float32):
    return torch.as_tensor(np.array(x, dtype, order="C")).to(DEV)                # (a copy: the scenes are read-only)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _knn_gpu(V, P, k, tr):
    from collab_splats_amd.meshmap import _knn
    idx, d, valid = _knn(_t(V), _t(P), k=k, sdf_trunc=tr)
    return idx.cpu().numpy().astype(np.int64), d.cpu().numpy(), valid.cpu().numpy()


def _check_knn(name, k, trunc=None):
    """The device's neighbours of a scene against the brute force: validity, indices and distance bits."""
    s = S.scene(name)
    tr = s["trunc"] if trunc is None else trunc
    idx, d, valid = _knn_gpu(s["V"], s["P"], k, tr)
    with np.errstate(invalid="ignore"):
        ri, rd, _, rv = S.restated_knn(name, k, trunc)
    assert np.array_equal(valid, rv)
    assert np.array_equal(idx[valid], ri[rv])
    assert np.array_equal(d[valid].view(np.uint32), rd[rv].view(np.uint32))
    assert np.all(idx[~valid] == -1) and np.all(d[~valid] == np.inf)
    return valid


def _map(s, k, values="F", normals=False, trunc=None):
    import collab_splats_amd as m
    fn = m.normals2vertex if normals else m.features2vertex
    return fn(_t(s["V"]), _t(s["P"]), _t(s[values]), k=k, sdf_trunc=s["trunc"] if trunc is None else trunc)


def _check_bar(name, k, values="F", normals=False):
    """The neighbours bit for bit, then the map within the per-vertex bar of the fp64 aggregation of those neighbours."""
    assert (name, k, values, normals) in S.BAR_CASES                  # (the host test holds the yardstick to the same bar)
    _check_knn(name, k)
    out = _map(S.scene(name), k, values, normals).cpu().numpy()
    ref, bound, covered, ordered = S.bar(name, k, values, normals)
    assert out.shape == ref.shape and out.dtype == np.float32
    err = np.abs(out.astype(np.float64) - ref)
    ratio = err[covered] / bound[covered]
    print(f"meshmap bar: {name} k={k} {values}: max err / bound = {ratio.max():.3f} over {covered.sum()} vertices "
          f"(the fp32 yardstick: {(np.abs(ordered.astype(np.float64) - ref)[covered] / bound[covered]).max():.3f})")
    assert np.all(err[covered] <= bound[covered])
    assert np.all(out[~covered] == 0)
    if normals:                                  # |o| / (|o| + 1e-8): short of 1 by 1e-5 where the magnitudes are 1e-3
        length = np.linalg.norm(ref[covered], axis=1)
        assert np.all(length > 1 - 2e-5) and np.all(length <= 1)
        assert np.all(np.abs(np.linalg.norm(out[covered].astype(np.float64), axis=1) - length) <= 1e-6)
    return out


# ------------------------------------------------------------------------------------------------- 1. every k class
@pytest.mark.parametrize("k", S.K_CLASSES)
@pytest.mark.parametrize("name", ["uniform", "duplicated", "sparse_grid"])
def test_every_list_size_class(name, k):
    """k = 4, 8 and 16 leave no pinned front slot in knn_kernel<4 / 8 / 16>, k = 1, 5 and 9 leave the most."""
    valid = _check_knn(name, k)
    assert valid.mean() > 0.3


# ---------------------------------------------------------------------------------- 2. far from the origin, 3. the limit
@pytest.mark.parametrize("k", [5, 16])
def test_far_from_the_origin(k):
    """|x| up to 2500 at sdf_trunc = 0.03: the rounding margin of the box and of the stop test is most of a cell."""
    _check_bar("far", k)


def test_margin_grows_with_the_coordinates():
    """At x = 2500 the cell of a vertex and the face the stop test measures to disagree by a float: each point's true second
    neighbour is indexed one cell past the box, nearer than the face by less than a decoy inside it (the host test holds that a
    stop test with the margin of the origin would take the decoy)."""
    assert _check_knn("margin_traps", 2).all()


@pytest.mark.parametrize("k", [5, 16])
def test_at_the_coordinate_limit(k):
    s = S.scene("limit")
    valid = _check_knn("limit", k)
    kinds = s["kinds"]
    assert valid[kinds == 0].mean() > 0.9 and 0.05 < valid[kinds == 1].mean() < 0.95 and not valid[kinds >= 2].any()


def test_vertices_beyond_the_limit_or_not_finite_are_refused():
    import collab_splats_amd as m
    s = S.scene("limit")
    P, F = _t(s["P"][:50]), torch.zeros((50, 2), device=DEV)
    assert m.features2vertex(_t(s["V"]), P, F, sdf_trunc=s["trunc"]).shape == (len(s["V"]), 2)       # the last coordinate passes
    past = np.nextafter(s["top"], np.float32(np.inf))
    for axis, value in ((0, past), (1, -past), (2, np.float32(1e6)), (0, np.nan), (1, np.inf), (2, -np.inf)):
        V = s["V"].copy()
        V[len(V) // 2, axis] = value
        with pytest.raises(ValueError, match="within 2\\^18 sdf_trunc"):
            m.features2vertex(_t(V), P, F, sdf_trunc=s["trunc"])
        with pytest.raises(ValueError, match="within 2\\^18 sdf_trunc"):
            m.normals2vertex(_t(V), P, torch.zeros((50, 3), device=DEV), sdf_trunc=s["trunc"])


# ------------------------------------------------------------------------------------------------ 4. the inclusive rule
@pytest.mark.parametrize("k", [1, 5])
def test_validity_is_inclusive_at_equality(k):
    """d = 2^-5 exactly: valid at sdf_trunc = 2^-5 and one float above, invalid one float below."""
    s = S.scene("inclusive")
    for tr, at_valid in S.inclusive_truncs():
        valid = _check_knn("inclusive", k, tr)
        assert valid.sum() == s["n_on"] + (s["n_at"] if at_valid else 0)
        assert np.all(valid[s["kinds"] == 0] == at_valid) and valid[s["kinds"] == 1].all() and not valid[s["kinds"] == 2].any()


# --------------------------------------------------------------------------------------------- 5. truncation extremes
def test_truncation_far_larger_than_the_scene():
    """sdf_trunc = 50 over an extent of 0.4: every vertex in one or two cells, every row valid."""
    assert _check_knn("trunc_large", 5).all()
    _check_bar("trunc_large", 5)


def test_truncation_far_smaller_than_the_scene():
    """sdf_trunc = 1e-4 over an extent of 0.4: almost every row invalid (the sort key M), the valid rows' other neighbours
    hundreds of cells away."""
    assert 0.02 < _check_knn("trunc_small", 5).mean() < 0.30
    _check_bar("trunc_small", 5)


# --------------------------------------------------------------------------------------- 6. chunk boundaries, bit for bit
@pytest.mark.parametrize("name", ["chunks_k1", "chunks_sigma0"])
def test_chunk_boundaries_bitwise(name):
    """Lists of 1, 511 .. 513, 1023 .. 1025 and 2049 contributions, interleaved in point order, with weights that involve no
    exp (k = 1: w = 1; sigma = 0: w = 1 / 3): the output is the ordered fp32 restatement's bit for bit, which holds the sort's
    stability, the chunk counts, the owner table and the tail of the last chunk at once."""
    s = S.scene(name)
    k = s["k"]
    _check_knn(name, k)
    idx, d, _, valid = S.restated_knn(name, k)
    counts = np.bincount(idx[valid].reshape(-1), minlength=len(s["V"]))
    assert sorted(set(counts)) == sorted(S.chunk_lengths())
    out = _map(s, k).cpu().numpy()
    ref = R.aggregate_ordered(len(s["V"]), idx, d, valid, s["F"], chunk=S.chunk())
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    assert not np.array_equal(ref, R.aggregate_ordered(len(s["V"]), idx, d, valid, s["F"], chunk=S.chunk() + 1))
    import collab_splats_amd as m
    nrm = m.normals2vertex(_t(s["V"]), _t(s["P"]), _t(s["F"][:, :3]), k=k, sdf_trunc=s["trunc"]).cpu().numpy()
    ref = R.aggregate_ordered(len(s["V"]), idx, d, valid, s["F"][:, :3], normalise=True, chunk=S.chunk())
    assert np.array_equal(nrm.view(np.uint32), ref.view(np.uint32))


# ---------------------------------------------------------------------------------------------------- 7. channel counts
def test_one_channel():
    _check_bar("d1", 5)


def test_the_channel_cap():
    import collab_splats_amd as m
    from collab_splats_amd.meshmap import map_to_vertices
    s = S.scene("d4096")
    assert s["F"].shape == (300, 4096) and s["V"].shape == (257, 3)
    _check_bar("d4096", 5)
    wide = torch.zeros((300, 4097), device=DEV)
    with pytest.raises(ValueError, match="beyond the library's limits"):
        m.features2vertex(_t(s["V"]), _t(s["P"]), wide, sdf_trunc=s["trunc"])
    with pytest.raises(ValueError, match="beyond the library's limits"):
        map_to_vertices(_t(s["V"]), _t(s["P"]), wide, sdf_trunc=s["trunc"], n_unit=3)


def test_unit_step_moves_the_first_three_channels_only():
    import collab_splats_amd as m
    from collab_splats_amd.meshmap import map_to_vertices
    s = S.scene("d7")
    V, P, F = _t(s["V"]), _t(s["P"]), _t(s["F"])
    both = map_to_vertices(V, P, F, k=5, sdf_trunc=s["trunc"], n_unit=3)
    feat = m.features2vertex(V, P, F, k=5, sdf_trunc=s["trunc"])
    nrm = m.normals2vertex(V, P, F[:, :3], k=5, sdf_trunc=s["trunc"])
    assert both.shape == (len(s["V"]), 7)
    assert torch.equal(_bits(both[:, 3:]), _bits(feat[:, 3:])) and torch.equal(_bits(both[:, :3]), _bits(nrm))
    assert not torch.equal(both[:, :3], feat[:, :3]) and bool((feat[:, 3:] != 0).any())


def test_each_channel_equals_a_call_with_it_alone():
    import collab_splats_amd as m
    s = S.scene("d13")
    V, P, F = _t(s["V"]), _t(s["P"]), _t(s["F"])
    wide = m.features2vertex(V, P, F, k=5, sdf_trunc=s["trunc"])
    for c in (0, 6, 12):
        one = m.features2vertex(V, P, F[:, c:c + 1], k=5, sdf_trunc=s["trunc"])
        assert one.shape == (len(s["V"]), 1) and torch.equal(_bits(one[:, 0]), _bits(wide[:, c]))


def test_strided_fp64_and_fp16_views():
    """Any view is the fp32 contiguous run of the same converted values, bit for bit."""
    import collab_splats_amd as m
    s = S.scene("d7")
    rng = np.random.default_rng(70)
    for normals in (False, True):
        fn = m.normals2vertex if normals else m.features2vertex
        F = s["F"][:, :3] if normals else s["F"]
        V64 = _t(s["V"].astype(np.float64) + 1e-9 * rng.standard_normal(s["V"].shape), np.float64)
        P64 = _t(s["P"].astype(np.float64) + 1e-9 * rng.standard_normal(s["P"].shape), np.float64)
        F64 = _t(F.astype(np.float64) * (1 + 1e-9), np.float64)
        for V, P, Fv in ((V64, P64, F64), (V64.half(), P64.half(), F64.half())):
            plain = fn(V.float().contiguous(), P.float().contiguous(), Fv.float().contiguous(), k=5, sdf_trunc=s["trunc"])
            assert bool((plain != 0).any())
            assert torch.equal(_bits(fn(V, P, Fv, k=5, sdf_trunc=s["trunc"])), _bits(plain))
            Vs = torch.zeros((len(V), 6), dtype=V.dtype, device=DEV)
            Vs[:, ::2] = V
            Fs = torch.zeros((len(P), 2 * Fv.shape[1] + 1), dtype=Fv.dtype, device=DEV)
            Fs[:, 1::2] = Fv
            Vs, Ps, Fs = Vs[:, ::2], P.t().contiguous().t(), Fs[:, 1::2]
            assert not Vs.is_contiguous() and not Ps.is_contiguous() and not Fs.is_contiguous()
            assert torch.equal(_bits(fn(Vs, Ps, Fs, k=5, sdf_trunc=s["trunc"])), _bits(plain))


# ------------------------------------------------------------------------------------------------ 8. non-finite points
def test_non_finite_points_are_invalid_and_touch_nothing_else():
    import collab_splats_amd as m
    s = S.scene("nonfinite")
    keep, tr = s["keep"], s["trunc"]
    valid = _check_knn("nonfinite", 5)
    assert not valid[~keep].any()
    idx, d, valid = _knn_gpu(s["V"], s["P"], 5, tr)
    assert np.all(idx[~keep] == -1) and np.all(d[~keep] == np.inf)
    ci, cd, cv = _knn_gpu(s["V"], s["P_clean"], 5, tr)
    assert np.array_equal(idx[keep], ci) and np.array_equal(d[keep].view(np.uint32), cd.view(np.uint32))
    assert np.array_equal(valid[keep], cv) and cv.mean() > 0.8
    for fn in (m.features2vertex, m.normals2vertex):
        out = fn(_t(s["V"]), _t(s["P"]), _t(s["F"]), k=5, sdf_trunc=tr)                   # (the rows' values are NaN too)
        clean = fn(_t(s["V"]), _t(s["P_clean"]), _t(s["F_clean"]), k=5, sdf_trunc=tr)
        assert bool(torch.isfinite(out).all()) and bool((out != 0).any())
        assert torch.equal(_bits(out), _bits(clean))


# ------------------------------------------------------------------------------------- 9. the bar on a mixed-scale scene
@pytest.mark.parametrize("k", [5, 16])
@pytest.mark.parametrize("normals", [False, True])
def test_mixed_scales_per_vertex(normals, k):
    """Magnitudes 1e-3 .. 1e3 by blob and rows at d / sigma above 10 beside rows at d / sigma below 0.1: every vertex is held
    to its own bar, the ones reached by the far rows alone included."""
    _check_bar("mixed", k, "N3" if normals else "F", normals)
