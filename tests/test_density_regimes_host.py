"""CPU: the conditions tests/test_density_regimes_gpu.py rests on, checked on the yardsticks (tests/density_restatement.py) for
every scene of tests/density_regimes_scenes.py:

  * the fp32 restatement leaves room under the cap of both rules: 8 e32 < 1e-4 tensor-wide and by the local scale;
  * the restatement's lists are conservative (test_density_host.py's check, on these names);
  * every allocated unit's list is longer than two LDS batches;
  * the voxels left out of the bitwise comparison of skipping against not skipping are at most 0.2 % of a scene;
  * the scenes are what they say: the map, the thin Gaussians, the opacity-0 Gaussians of `mo0`, the pairs `mo.5` removes,
    the plates of `far_h13_edges` that only the sub-brick test's slack keeps."""
import numpy as np
import pytest

import density_regimes_scenes as RS
import density_scenes as S
import test_density_host as TH
from density_restatement import Restated


@pytest.mark.parametrize("name", RS.NAMES)
def test_restatement_leaves_room_under_both_rules(name):
    d = S.oracle_map(name)[0]
    f = S.restated_map(name)
    e32 = RS.rel(f, d)
    e32_loc = RS.rel_local(f, d, RS.scale_map(name))
    print(f"{name}: e32 = {e32:.3e}  e32_loc = {e32_loc:.3e}  (x 8: {8 * e32:.2e}, {8 * e32_loc:.2e})  max d = {d.max():.3f}")
    assert 8 * e32 < 1e-4 and 8 * e32_loc < 1e-4


@pytest.mark.parametrize("name", RS.NAMES)
def test_lists_are_conservative(name):
    TH.test_lists_are_conservative(name)


@pytest.mark.parametrize("name", RS.NAMES)
def test_scene_is_its_map_with_lists_of_several_batches(name):
    lo, dims, n, h, cutoff, _, mo, _ = RS.SCENES["far_h13" if name == RS.EDGES else name]
    n += len(RS.edge_cases()) if name == RS.EDGES else 0
    R, sc = S.restated(name), S.scene(name)
    assert tuple(R.lo) == tuple(lo) and tuple(R.dims) == tuple(dims) and len(R.lists) == 2 and sc["means"].shape == (n, 3)
    assert float(R.r) == cutoff and sc["cutoff"] == cutoff and sc["min_opacity"] == mo and sc["h"] == h
    lens = [len(v) for v in R.lists.values()]
    print(f"{name}: lists of {lens}, thinnest Gaussian {sc['scales'].min() / h:.4f} voxels, largest |A| {np.abs(R.A[R.ok]).max():.0f}")
    assert min(lens) > 2 * S.BATCH
    assert sc["scales"].min() < 0.00045 and sc["scales"].max() > 0.035                  # 0.0004 .. 0.04, as the workload's


@pytest.mark.parametrize("name", RS.NAMES + ("random",))
def test_the_cutoff_shells_hold_few_voxels(name):
    share = float(RS.shell_map(name).mean())
    print(f"{name}: {share:.2e} of the voxels have a listed Gaussian within {RS.SHELL} r^2 of its cut-off")
    assert share <= RS.SHELL_SHARE


def test_what_the_scenes_are_there_for():
    sc, R = S.scene("bench_corner"), S.restated("bench_corner")
    assert sc["scales"].min() / sc["h"] < 0.05                                          # 1 / 25 of a voxel
    assert S.scene("coarse")["scales"].min() / S.scene("coarse")["h"] < 0.01            # 1 / 125
    assert np.exp(-0.5 * 1.5 ** 2) > 0.3 and np.exp(-0.5 * 36.0) < 2e-8                 # ecut at r = 1.5 and at r = 6
    far = S.restated("far_h13")
    assert far.lo[0] < 0 and np.abs(far.lo * float(far.L)).min() > 250.0                # hundreds of metres out
    assert tuple(S.restated("far_h13_z").dims) == (1, 1, 2)
    # mo0: the opacity-0 Gaussians take part (records, lists) and add nothing
    sc0, R0 = S.scene("bench_corner_mo0"), S.restated("bench_corner_mo0")
    zero = np.nonzero(sc0["opacities"] == 0)[0]
    assert len(zero) == RS.N_ZERO and R0.ok[zero].all() and R0.ok.all()
    listed = set(g for lst in R0.lists.values() for g in lst)
    assert len(listed & set(zero.tolist())) >= 3
    other = sc0["opacities"] != 0
    assert np.array_equal(sc0["opacities"][other], sc["opacities"][other]) and np.array_equal(sc0["means"], sc["means"])
    assert R0.lists == R.lists                                   # (they keep the places they have with their drawn opacities)
    # mo.5: at least a fifth of the pairs its Gaussians have at the default min_opacity go
    Rd0 = Restated(sc0["means"], sc0["quats"], sc0["scales"], sc0["opacities"], sc0["h"], bounds=sc0["bounds"])
    assert not Rd0.ok[zero].any() and Rd0.n_pairs < R0.n_pairs   # (the default min_opacity would drop them)
    sc5, R5 = S.scene("bench_corner_mo.5"), S.restated("bench_corner_mo.5")
    Rd = Restated(sc5["means"], sc5["quats"], sc5["scales"], sc5["opacities"], sc5["h"], bounds=sc5["bounds"])
    print(f"pairs: min_opacity 0 {R0.n_pairs} against {Rd0.n_pairs}; min_opacity 0.5 {R5.n_pairs} against {Rd.n_pairs}")
    assert R5.n_pairs <= 0.8 * Rd.n_pairs and (sc5["opacities"][R5.ok] >= 0.5).all() and not R5.ok.all()


def test_the_brick_edge_plates_need_the_slack():
    """Every plate of `far_h13_edges` reaches one voxel, with a term well clear of its cut-off; the accumulate kernel's
    sub-brick test, restated in its fp32 operations, keeps the plate for that voxel's wave with the 2^-20 slack and would pass
    over it without."""
    R, O = S.restated(RS.EDGES), S.oracle(RS.EDGES)
    cases = RS.edge_cases()
    assert len(cases) >= 6 and len(set(c[3] for c in cases)) == 2 and len(set(c[4] for c in cases)) == 4    # both units, every wave
    c, _ = R.map_voxel_centres()
    for g, axis, side, m, wave, voxel in cases:
        col = int(np.nonzero(O.ids == g)[0][0])
        k, t, _, _ = O.terms(c[m])
        mm = float((t[voxel, col] ** 2).sum())
        assert (k[:, col] > 0).sum() == 1 and k[voxel, col] > 0.05 * O.o[col] * O.ecut and g in R.lists[m]
        assert 1e-2 * O.r2 < O.r2 - mm < 2e-2 * O.r2
        lx, ly = voxel & 15, (voxel >> 4) & 15
        assert wave == (lx >> 3) + 2 * (ly >> 3)
        assert not RS.brick_test_skips(R, g, m, wave) and RS.brick_test_skips(R, g, m, wave, slack=False), (g, axis, side)


def test_scale_is_the_sum_of_the_terms_sizes():
    """Oracle.scale by hand on two Gaussians: inside both, inside one, just outside a cut-off (counted), far outside (0)."""
    from density_restatement import Oracle
    means = np.array([[0, 0, 0], [0.3, 0, 0]], np.float32)
    quats = np.tile(np.array([[1, 0, 0, 0]], np.float32), (2, 1))
    s = np.float64(np.float32(0.1))
    O = Oracle(means, quats, np.full((2, 3), 0.1, np.float32), np.array([0.5, 0.25], np.float32), cutoff=2.0)
    x = np.array([0.15, 0.05, 0.2 * (1 + 2e-4), 0.7])
    got = O.scale(np.stack([x, 0 * x, 0 * x], 1))
    m0, m1 = (x / s) ** 2, ((x - np.float64(np.float32(0.3))) / s) ** 2
    ecut = np.exp(-2.0)
    t0, t1 = 0.5 * (np.exp(-m0 / 2) * (1 + m0 / 2) + ecut), 0.25 * (np.exp(-m1 / 2) * (1 + m1 / 2) + ecut)
    assert np.allclose(got, [t0[0] + t1[0], t0[1], t0[2] + t1[2], 0.0], rtol=1e-12, atol=0)
    assert m0[2] > 4.0 and O.evaluate(np.array([[x[2], 0, 0]]))["density"][0] == O.terms(np.array([[x[2], 0, 0]]))[0][0, 1]
