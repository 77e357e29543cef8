"""CPU: the holed grid of tests/meshadj_scenes.py reaches, at each of its three sizes, the regime it was built for, asserted on
the restatements: tests/test_meshadj_gpu.py compares the device with the same references."""
import numpy as np
import pytest

import meshadj_scenes as S
import meshclean_restatement as MC


@pytest.mark.parametrize("M,passes", zip(S.SIZES, (1, 2, 3)))
def test_the_grid_sits_at_one_two_and_three_key_bytes(M, passes):
    V, T, att = S.holed_grid(M)
    assert len(V) == M == len(att) and att.shape[1] == 2 and len(T) == 130 and T.min() == M - S.N_GRID and T.max() == M - 1
    assert S.radix_passes(M - 1) == passes
    used = np.unique(T)
    assert len(used) == S.N_GRID - 9                                # the 3 x 3 block is gone
    loop, edges, n_edges, _ = MC.mesh_holes(V, T)
    assert sorted(n_edges.tolist()) == [16, 36]                     # the hole and the outline
    assert len(np.unique(V[used], axis=0)) == len(used)


@pytest.mark.parametrize("M", S.SIZES)
def test_decimation_runs_two_rounds_and_cuts_the_last(M):
    """The apply call of a round names what the round call sorted (every round); the last round's selection removes more faces
    than are needed, so the landing sort orders it and a prefix is applied."""
    V, T, att = S.holed_grid(M)
    (v, t, a, vm, r), rounds = S.decimate_reference(M)
    assert r == len(rounds) >= 2 and len(t) <= len(T) // 2 < len(t) + 2
    assert all(x["applied"] == x["selected"] > 0 for x in rounds[:-1])
    assert 0 < rounds[-1]["applied"] < rounds[-1]["selected"]
    assert all(x["M"] == M for x in rounds) and [x["faces"] for x in rounds][0] == len(T)
    assert (vm[:M - S.N_GRID] == -1).all() and len(a) == 1 and a[0].shape == (len(v), 2)
