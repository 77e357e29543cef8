"""CPU: the numpy restatement of the screened Poisson reconstruction (tests/poisson_restatement.py) alone meets the conditions the
GPU tests hold csrc/poisson.hip to, and the host side of collab_splats_amd/poisson.py validates its arguments.

Bounds: the figures of the fp64 prototype the feature was specified with.  Where this restatement
reproduces a figure, the figure is the bound, rounded up in its second digit (the fp32 solve moves a crossing by ~1e-4 h); where it
does not (another seed), the bound is 3 x the restatement's own value, recorded next to it."""
import functools
import math

import numpy as np
import pytest
import torch

import poisson_restatement as R
import poisson_scenes as S


@functools.lru_cache(maxsize=None)
def recon(name):
    p, n, c, depth = S.scene(name)
    return R.reconstruct(p, n, c, depth)


def _radial_error(out, v=None):
    v = out["vertices"] if v is None else v
    return np.abs(np.linalg.norm(v.astype(np.float64) - S.CENTRE, axis=1) - S.RADIUS) / float(out["h"])


# ---------------------------------------------------------------------------------------------------------------- system
def test_operator_is_symmetric_positive_and_rhs_sums_to_zero():
    out = recon("sphere5")
    G, D = out["G"], out["D"].astype(np.float64)
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal((G, G, G)), rng.standard_normal((G, G, G))
    Ax, Ay = R.apply_A(D, x), R.apply_A(D, y)
    assert abs(np.vdot(x, Ay) - np.vdot(Ax, y)) <= 1e-12 * abs(np.vdot(x, Ay))
    assert np.vdot(x, Ax) > 0 and np.vdot(y, Ay) > 0
    screened = out["D"] > R.neighbours(G)                                          # (a weight below 6 eps32 Wbar rounds away)
    assert (out["D"] >= R.neighbours(G)).all() and not (screened & (out["Wq"] == 0)).any()
    assert screened.sum() > 0.99 * (out["Wq"] > 0).sum()
    # the constant vector: A 1 = the screening term alone (the Neumann Laplacian annihilates it)
    assert np.allclose(R.apply_A(D, np.ones((G, G, G))), D - R.neighbours(G).astype(np.float64), atol=1e-12)
    # sum b: the central differences telescope, so on the integer grids sum_i dV_a(i) is exactly (V_a on the upper border cells) -
    # (V_a on the lower ones).  At scale 1.1 the extreme samples sit 1.45 cells inside the cube and put a little weight there, so
    # sum b is small, not 0; with a wider margin (scale 1.25: 3.2 cells) the border cells are empty and sum b = 0 exactly.  A is
    # positive definite through the screening term, so the solve needs no compatibility condition on b.
    def telescoped(Vq):
        total = sum(int((R._shift(Vq[a], a, 1) - R._shift(Vq[a], a, -1)).sum()) for a in range(3))
        border = sum(int(np.take(Vq[a], -1, axis=2 - a).sum()) - int(np.take(Vq[a], 0, axis=2 - a).sum()) for a in range(3))
        return total, border

    total, border = telescoped(out["Vq"])
    assert total == border
    b = out["b"].astype(np.float64)
    assert abs(b.sum() + 0.5 * border * 2.0 ** -30) <= 4 * np.finfo(np.float32).eps * np.abs(b).sum()
    assert abs(b.sum()) <= 1e-3 * np.abs(b).sum()
    p, n, c, depth = S.scene("sphere5")
    o, h, G = R.grid(p, depth, 1.25)
    Wq, Vq, _ = R.splat(p, n, None, o, h, G)
    assert telescoped(Vq) == (0, 0)
    b = R.system(Wq, Vq)[1].astype(np.float64)
    assert abs(b.sum()) <= 4 * np.finfo(np.float32).eps * np.abs(b).sum()


def test_splat_weights_are_a_partition_of_unity_in_fixed_point():
    for name, (p, n, c, scale) in S.splat_edge_cases().items():
        o, h, G = R.grid(p, 5, scale)
        Wq, Vq, Cq = R.splat(p, n, c, o, h, G)
        assert abs(int(Wq.sum()) - len(p) * 2 ** 30) <= 8 * len(p), name          # 8 roundings of at most half a unit each
        assert (Cq is None) == (c is None)
        if name == "cell_centres":                                                 # f = 0: one cell takes the whole point
            assert o.tolist() == [0.0, 0.0, 0.0] and float(h) == 2.0 ** -4
            assert int(Wq.sum()) == len(p) * 2 ** 30 and (Wq % 2 ** 30 == 0).all()
            idx = np.floor(p[2:] / h).astype(np.int64)
            want = np.zeros((G, G, G), np.int64)
            np.add.at(want, (idx[:, 2], idx[:, 1], idx[:, 0]), 2 ** 30)
            want[0, 0, 0] += 2 ** 30                                               # the anchors, clamped into the corner cells
            want[G - 1, G - 1, G - 1] += 2 ** 30
            assert np.array_equal(Wq, want)
        if name == "zero_normal":
            assert np.isfinite(R.system(Wq, Vq)[1]).all()


# ----------------------------------------------------------------------------------------------------------------- solve
@pytest.mark.parametrize("name", ["sphere5", "sphere6", "cap5"])
def test_fp32_cg_against_fp64_solve(name):
    """Prototype: 76 / 139 / 112 iterations, true residual 9.4e-6, max|chi32 - chi64| / max|chi64| = 1.1e-4 / 1.4e-4 / 7.2e-5.
    This restatement: 76 / 139 / 112, 9.35e-6 / 9.32e-6 / 9.36e-6, 1.10e-4 / 1.62e-4 / 7.17e-5."""
    out = recon(name)
    G = out["G"]
    assert out["converged"] and out["iterations"] <= 8 * G and out["residual"] <= 1e-5
    true32 = R.true_residual(out["b"], out["D"], out["chi"])
    x64, it64, res64, conv64 = R.cg(out["b"], out["D"], 1e-12, 50 * G, np.float64)
    assert conv64 and R.true_residual(out["b"], out["D"], x64) <= 1e-11
    err = np.abs(out["chi"] - x64).max() / np.abs(x64).max()
    print(name, "iterations", out["iterations"], "true residual", true32, "chi error", err, "fp64 iterations", it64)
    assert true32 <= 2e-5                     # the recurrence stops at 1e-5; fp32 lets the true residual drift from it by less than that
    assert err <= 3 * 1.4e-4                  # 3 x the prototype's largest


def test_iteration_cap_does_not_raise():
    out = recon("sphere5")
    x, it, resid, conv = R.cg(out["b"], out["D"], 1e-5, 10)
    assert it == 10 and not conv and 1e-5 < resid < 1.0 and np.isfinite(x).all()
    x0, it0, resid0, conv0 = R.cg(out["b"], out["D"], 1e-5, 0)
    assert it0 == 0 and not conv0 and resid0 == 1.0 and not x0.any()
    z = np.zeros_like(out["b"])
    assert R.cg(z, out["D"], 1e-5)[1:] == (0, 0.0, True)                          # b = 0: chi = 0, no 0 / 0


# ------------------------------------------------------------------------------------------------- the device's order
U64 = 2.0 ** -53                              # the unit roundoff of fp64


def _gamma(d):
    return d * U64 / (1.0 - d * U64)


def _bits64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _same_run(a, b):
    return all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a[:4], b[:4])) and _bits64(a[4], b[4]) \
        and a[5:] == b[5:]


@pytest.mark.parametrize("n", [1024, 4096, 32 * 1024, 1025 * 1024, 2304 * 1024])
def test_exact_sums_are_within_the_path_bound_of_fsum(n):
    """Bound: every addition returns (a + b)(1 + e) with |e| <= u = 2^-53.  A summand that passes through d additions on its way to
    the root carries the product of d such factors, so |computed - exact| <= ((1 + u)^d - 1) sum |v_i| <= gamma_d sum |v_i| with
    gamma_d = d u / (1 - d u) (Higham, Accuracy and Stability, section 4.2: any order of summation).  d is the longest path of the
    two-level sum (``sum_path_length``): the lane's 3 additions (4 in the mean, which starts from 0.0), 6 + 3 of the workgroup's
    tree, the thread's trips through the partials, 6 + 15 of the second tree: 34 for one trip, 36 for three.  math.fsum is the
    exact sum rounded once; the mean adds that rounding, the division's and the reference's own division: gamma_(d + 3)."""
    rng = np.random.default_rng(n)
    v = rng.standard_normal(n) * np.exp(rng.uniform(-6.0, 6.0, n))
    got = R.second_level(R.block_partials(v))
    d = R.sum_path_length(n)
    assert d == 3 + 9 + (n // 1024 + 1023) // 1024 + 21
    assert abs(got - math.fsum(v)) <= _gamma(d) * math.fsum(np.abs(v))
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    prod = a.astype(np.float64) * b.astype(np.float64)                             # exact: 24 + 24 bits
    assert abs(R.dot_exact(a, b) - math.fsum(prod)) <= _gamma(d) * math.fsum(np.abs(prod))
    for m in (n, n - 1023, n + 1):                                                 # the mean's ragged last block
        if m < 1:
            continue
        for wide in (False, True):
            x = S.mean_values(m, wide)
            want = math.fsum(x.astype(np.float64)) / m
            dm = R.sum_path_length(m, lane_adds=4) + 3
            assert abs(R.mean_exact(x) - want) <= _gamma(dm) * math.fsum(np.abs(x.astype(np.float64))) / m


def test_exact_sums_are_not_numpys_order():
    """On a cancelling input the order shows: the device's tree and numpy's pairwise sum round differently."""
    rng = np.random.default_rng(3)
    v = rng.standard_normal(32 * 1024) * 1e6
    v[1::2] = -v[::2] + rng.standard_normal(16 * 1024)                             # pairs that cancel to O(1)
    got, ref = R.second_level(R.block_partials(v)), float(np.sum(v))
    exact = math.fsum(v)
    bound = _gamma(R.sum_path_length(len(v))) * math.fsum(np.abs(v))
    assert abs(got - exact) <= bound and abs(ref - exact) <= bound
    assert got != ref
    x = S.mean_values((1 << 20) + 1, wide=True)
    assert R.mean_exact(x) != float(np.sum(x.astype(np.float64)) / len(x))
    x = S.mean_values((1 << 20) + 1)                                               # one exponent: every order is exact
    assert R.mean_exact(x) == float(np.sum(x.astype(np.float64)) / len(x)) == math.fsum(x.astype(np.float64)) / len(x)
    a = rng.standard_normal((32, 32, 32)).astype(np.float32)
    assert R.dot_exact(a, a) != float(np.vdot(a.astype(np.float64), a.astype(np.float64)))


def test_tree_primitives_on_hand_values():
    """Powers of two that only one order sums without loss: the wave tree pairs lane i with lane i + 32 first."""
    w = np.zeros(64)
    w[0], w[32], w[1] = 1.0, -1.0, 2.0 ** -60                                      # (w0 + w32) + ... keeps the small term
    assert R._wave_tree(w) == 2.0 ** -60
    assert float(np.cumsum(w[[0, 1, 32]])[-1]) == 0.0                              # the ascending order would lose it
    v = np.zeros(256)
    v[0], v[64], v[128], v[192] = 1.0, 2.0 ** -53, 2.0 ** -53, -1.0                # waves in ascending order: both halves are lost
    assert R._block_tree(v, 4) == 0.0
    lane = np.array([1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -52])                     # ((a0 + a1) + a2) + a3
    assert R._lane4(lane) == 1.0 + 2.0 ** -52 and math.fsum(lane) == 1.0 + 2.0 ** -51
    part = np.zeros(2048)
    part[5], part[1029], part[6] = 1.0, -1.0, 2.0 ** -60                           # thread 5 adds partials 5 and 1029 before the tree
    assert R.second_level(part) == 2.0 ** -60
    assert R.mean_exact(np.array([3.0], np.float32)) == 3.0 and R.mean_exact(np.array([1, 2, 4], np.float32)) == 7.0 / 3.0


@pytest.mark.parametrize("name", ["sphere5", "sparse5"])
def test_exact_order_cg_converges_like_the_numpy_order_cg(name):
    """The two differ only in the order of their sums: the same bars as the GPU's chi is held to against ``cg`` (3 x its true
    residual, 4 x its distance from the fp64 solution)."""
    out = recon(name)
    b, D, G = out["b"], out["D"], out["G"]
    x, r, z, p, st, it, done = R.cg_exact(b, D, 1e-5)
    info = R.exact_info(st)
    assert done == 1 and info["converged"] and 0 < it <= 8 * G and info["residual"] <= 1e-5 and info["iterations"] == it
    x64 = R.cg(b, D, 1e-12, 50 * G, np.float64)[0]
    true32, err32 = R.true_residual(b, D, out["chi"]), np.abs(out["chi"] - x64).max() / np.abs(x64).max()
    true_x, err_x = R.true_residual(b, D, x), np.abs(x - x64).max() / np.abs(x64).max()
    print(name, "iterations", it, "(", out["iterations"], ") true residual", true_x, "(", true32, ") chi error", err_x, "(", err32, ")")
    assert true_x <= 3 * true32 and err_x <= 4 * err32


@pytest.mark.parametrize("name, k, total", [("dense4", 1, 3), ("dense4", 5, 17), ("sphere5", 16, 17), ("sphere5", 7, None)])
def test_exact_order_cg_continues_where_it_stopped(name, k, total):
    if name == "dense4":
        b, D = S.dense_random_system(4)
    else:
        b, D = recon(name)["b"], recon(name)["D"]
    whole = R.cg_exact(b, D, 1e-5, None, total)
    part = R.cg_exact(b, D, 1e-5, None, k)
    assert part[5] == k and part[6] == 0
    rest = R.cg_exact(b, D, 1e-5, None, None if total is None else total - k, start=part)
    assert _same_run(rest, whole) and whole[5] == (total if total is not None else whole[5])
    again = R.cg_exact(b, D, 1e-5, None, 16, start=whole) if total is None else None   # after the stop: a no-op
    assert again is None or (_same_run(again, whole) and whole[6] == 1)


def test_exact_order_cg_stop_rules():
    b, D = S.dense_random_system(4)
    assert (D > R.neighbours(16)).all() and (D < R.neighbours(16) + 2).all() and (b != 0).all()
    run = R.cg_exact(b, D, 1e-5, 10)
    assert run[5:] == (10, 2) and run[4][R.S_ITERS] == 10.0 and not R.exact_info(run[4])["converged"]
    nine = R.cg_exact(b, D, 1e-5, 10, 9)
    assert nine[6] == 0 and np.array_equal(nine[3], run[3])                        # the cap's iteration leaves p alone, as the
    assert not np.array_equal(R.cg_exact(b, D, 1e-5, None, 10)[3], run[3])         # direction kernel's guard does; an uncapped one moves it
    assert _same_run(R.cg_exact(b, D, 1e-5, 10, 1, start=nine), run)
    none = R.cg_exact(b, D, 1e-5, 0)
    assert none[5:] == (0, 2) and not none[0].any() and np.array_equal(none[1], b) and none[4][R.S_RR] == none[4][R.S_BB]
    zero = R.cg_exact(np.zeros_like(b), D, 1e-5)
    assert zero[5:] == (0, 1) and not zero[0].any() and R.exact_info(zero[4]) == {"iterations": 0, "residual": 0.0, "converged": True}
    loose = R.cg_exact(b, D, 1e-1)
    assert loose[6] == 1 and loose[4][R.S_RR] <= 1e-2 * loose[4][R.S_BB] and 0 < loose[5] < R.cg_exact(b, D, 1e-5)[5]
    first = R.cg_exact(b, D, 1e-5, None, 1)[4]                                      # alpha and beta are floats held in doubles
    assert first[R.S_ALPHA] == float(np.float32(first[R.S_ALPHA])) and first[R.S_BETA] == float(np.float32(first[R.S_BETA]))
    assert first[R.S_ALPHA] != 0 and first[R.S_BETA] != 0 and first[R.S_PAP] > 0


# -------------------------------------------------------------------------------------------------------------- geometry
# scene -> bound on max | |v - centre| - R | / h.  Prototype: 0.06, 0.085, 0.18 (sparse); this restatement: 0.0603, 0.0727, 0.301
# (another seed for the 2 000 points: 3 x 0.301).
GEOMETRY = {"sphere5": 0.065, "sphere6": 0.085, "sparse5": 0.91}


@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_sphere_geometry(name):
    out = recon(name)
    v, t = out["vertices"], out["triangles"]
    err = _radial_error(out)
    vol = R.signed_volume(v, t) / (4.0 / 3.0 * np.pi * S.RADIUS ** 3)
    print(name, "vertices", len(v), "triangles", len(t), "max error / h", err.max(), "volume ratio", vol)
    assert err.max() <= GEOMETRY[name]
    assert R.euler(v, t) == 2
    assert abs(vol - 1.0) <= 0.006            # outward (positive) and within the prototype's 0.6 %
    assert (out["density"] >= 0).all() and out["colors"].min() >= 0 and out["colors"].max() <= 1.0 + 1e-6


def test_sphere_with_positional_noise():
    """Prototype: 0.13 h at 0.01 noise; this restatement: 0.126 h."""
    p, n, c = S.sphere(20000, seed=0, noise=0.01)
    out = R.reconstruct(p, n, c, 5)
    err = _radial_error(out)
    print("noise 0.01: max error / h", err.max())
    assert err.max() <= 0.13 and R.euler(out["vertices"], out["triangles"]) == 2


def test_open_cap_is_closed_by_a_sheet_that_the_density_trim_removes():
    """Prototype: 22 % of the crossings at density 0, errors up to 4.5 h; above 0.25 x the median positive density 0.124 h."""
    out = recon("cap5")
    v, t, d = out["vertices"], out["triangles"], out["density"]
    err = _radial_error(out)
    med = float(np.median(d[d > 0]))
    print("cap: density 0 at", (d == 0).mean(), "max error / h", err.max(), "kept", err[d >= 0.25 * med].max())
    assert 0.15 <= (d == 0).mean() <= 0.30 and err.max() > 2.0
    tv, tt, td, index = R.trim(v, t, d, 0.0, 0.25 * med)
    assert _radial_error(out, tv).max() <= 0.13
    assert tt.min() == 0 and tt.max() == len(tv) - 1 and len(np.unique(tt)) == len(tv)
    assert np.array_equal(tv, v[index]) and (np.diff(index) > 0).all()


# ------------------------------------------------------------------------------------------------------------------ trim
def _hand_mesh():
    """A strip of four triangles over six vertices, density rising along it, plus one unreferenced vertex."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 2, 0], [1, 2, 0], [5, 5, 5]], np.float32)
    t = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4], [3, 5, 4]], np.int32)
    d = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 9.0], np.float32)
    return v, t, d


def test_trim_on_a_hand_built_mesh():
    v, t, d = _hand_mesh()
    tv, tt, td, index = R.trim(v, t, d, 0.0, 0.15)                                 # vertex 0 goes, and with it triangle 0
    assert index.tolist() == [1, 2, 3, 4, 5] and tt.tolist() == [[0, 2, 1], [1, 2, 3], [2, 4, 3]]
    assert np.array_equal(tv, v[index]) and np.array_equal(td, d[index])
    tv, tt, td, index = R.trim(v, t, d, 0.5, None)                                 # the median: 0.4; vertices 0, 1, 2 go
    assert np.quantile(d.astype(np.float64), 0.5) == d[3] and index.tolist() == [3, 4, 5] and tt.tolist() == [[0, 2, 1]]
    tv, tt, td, index = R.trim(v[:6], t, d[:6], 0.0, None)                         # the identity
    assert np.array_equal(tv, v[:6]) and np.array_equal(tt, t) and index.tolist() == list(range(6))


def test_module_trim_matches_the_restatement_on_the_host_side():
    """poisson_trim's quantile is numpy's linear rule, two elements read from the sorted tensor."""
    from collab_splats_amd import poisson
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 10, 101, 1000):
        d = rng.random(n).astype(np.float32)
        d[: n // 3] = d[0]                                                         # ties
        s = torch.sort(torch.from_numpy(d).double()).values
        for q in (0.0, 0.01, 0.07, 0.25, 0.5, 0.77, 0.99, 1.0):
            assert poisson._quantile(s, q) == float(np.quantile(d.astype(np.float64), q)), (n, q)


# ------------------------------------------------------------------------------------------------------------ validation
def test_degenerate_and_non_finite_extent():
    one = np.array([[0.5, 0.25, 1.0]], np.float32)
    for bad in (one, np.repeat(one, 5, 0)):
        with pytest.raises(ValueError, match="degenerate"):
            R.grid(bad, 5)
    with pytest.raises(ValueError, match="finite"):
        R.grid(np.array([[0, 0, 0], [1, np.nan, 0]], np.float32), 5)
    o, h, G = R.grid(np.array([[0, 0, 0], [1, 0, 0]], np.float32), 4)             # flat in two axes is fine: the cube is the longest
    assert G == 16 and float(h) == float(np.float32(1.1) / np.float32(16))


def test_host_side_validation():
    import collab_splats_amd as m
    p = torch.rand(10, 3)
    for depth in (3, 10, 5.0, True):
        with pytest.raises(ValueError, match="depth"):
            m.poisson_grid(p, depth=depth)
    with pytest.raises(ValueError, match="points"):
        m.poisson_grid(torch.rand(10, 2), depth=5)
    with pytest.raises(m.MisplatError):                                            # no CPU fallback
        m.poisson_grid(p, depth=5)
    with pytest.raises(m.MisplatError):
        m.poisson_reconstruct(p, p, depth=5)
    with pytest.raises(ValueError, match="normals"):
        m.poisson_reconstruct(p, p[:5], depth=5)
    with pytest.raises(TypeError, match="int64"):
        m.poisson_solve(torch.zeros(16, 16, 16), torch.zeros(3, 16, 16, 16))
    with pytest.raises(ValueError, match="G = 2\\^depth"):
        m.poisson_solve(torch.zeros(8, 8, 8, dtype=torch.int64), torch.zeros(3, 8, 8, 8, dtype=torch.int64))
    v, t, d = (torch.from_numpy(x) for x in _hand_mesh())
    with pytest.raises(ValueError, match="quantile"):
        m.poisson_trim(v, t, d, quantile=1.5)
    with pytest.raises(ValueError, match="density"):
        m.poisson_trim(v, t, d[:3])
    with pytest.raises(ValueError, match="triangle indices"):
        m.poisson_trim(v[:3], t, d[:3])
