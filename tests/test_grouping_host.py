"""CPU: the grouping restatement (tests/grouping_restatement.py) against the goldens recorded from the reference's own code
(tests/golden/make_grouping_goldens.py) and against a brute-force per-mask, per-patch form; and the argument checks of
collab_splats_amd.grouping, which raise before the GPU is touched.  Everything compared is an integer: equality throughout."""
import numpy as np
import pytest
import torch

import grouping_restatement as R
import grouping_scenes as Q


@pytest.fixture(scope="module")
def gold():
    return Q.load_goldens()


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------- goldens
def test_projection_equals_the_reference(gold):
    W, H, _ = (int(x) for x in gold["A_size"])
    flat, valid = R.project(gold["A_radii"], gold["A_means2d"], W, H)
    assert np.array_equal(flat, gold["A_flat"]) and np.array_equal(valid, gold["A_valid"])
    halves = gold["A_means2d"][::7]
    assert np.all(halves - np.floor(halves) == 0.5) and (gold["A_means2d"] < 0).any() and (gold["A_means2d"][:, 0] > W).any()


def test_front_sets_equal_the_reference(gold):
    W, H, P = (int(x) for x in gold["A_size"])
    flat, valid = R.project(gold["A_radii"], gold["A_means2d"], W, H)
    assert list(R.mask_ids(gold["A_mask"])) == [3, 7, 8, 200, 4097, 65535]                  # ids with gaps
    for j, fp in enumerate(gold["A_fps"]):
        ids, mask_of, sets = R.front_sets(flat, valid, gold["A_depths"], gold["A_mask"], float(fp), P)
        _same(sets, Q.unpack(gold[f"A_ids{j}"], gold[f"A_off{j}"]))
        assert all(np.array_equal(np.nonzero(mask_of == i)[0], s) for i, s in enumerate(sets))


def test_cell_of_100_with_0_29_keeps_28(gold):
    W, H, P = (int(x) for x in gold["B_size"])
    flat, valid = R.project(gold["B_radii"], gold["B_means2d"], W, H)
    assert int((valid & (flat == 11 + 6 * W)).sum()) == 100
    sets = R.front_sets(flat, valid, gold["B_depths"], gold["B_mask"], 0.29, P)[2]
    _same(sets, Q.unpack(gold["B_ids"], gold["B_off"]))
    assert sum(int((s < 100).sum()) for s in sets) == 28 and int(R.front_count(0.29, 100)) == 28


@pytest.mark.parametrize("tag", ["C", "D"])
def test_sequences_equal_the_reference(gold, tag):
    views, (W, H, P, N) = Q.golden_sequence(gold, tag)
    bank = R.Bank(0.1)
    for radii, means, depths, mask, labels, sets, members in views:
        flat, valid = R.project(radii, means, W, H)
        mine = R.front_sets(flat, valid, depths, mask, 0.5, P)[2]
        _same(mine, sets)
        assert np.array_equal(bank.associate(mine), labels)
        _same(bank.bank, members)
    if tag == "C":
        assert np.array_equal(views[2][4], views[0][4])                                  # the repeated view re-matches its labels
    else:
        assert views[1][4].tolist() == [0, 0, 0, 1, 2] and len(views[1][5][0]) == 9 and len(views[1][5][3]) == 0


def test_threshold_is_compared_in_fp32():
    bank = R.Bank(0.1)
    bank.update(np.array([0]), [np.arange(20)])
    assert bank.assign([np.arange(19, 28)]).tolist() == [0]           # inter 1, n 9: float32(1 / 10.00000001) is not < float32(0.1)
    assert 1 / (9 + 1 + 1e-8) < 0.1                                   # (a double comparison would open a new label)


# ------------------------------------------------------------------------------------------------------ brute force
@pytest.mark.parametrize("W,H,P,N,fp,distinct", [(45, 70, 32, 1500, 0.5, True), (20, 12, 32, 600, 0.2, True), (65, 33, 7, 1200, 1.0, True),
                                                 (33, 21, 5, 900, 0.29, False), (16, 16, 1, 300, 1e-6, False)])
def test_cells_equal_the_per_mask_per_patch_loop(W, H, P, N, fp, distinct):
    radii, means, depths = Q.random_view(N + P, N, W, H, distinct)
    mask = Q.blocks_mask(N, W, H, [2, 3, 9, 300], 7, 5)
    flat, valid = R.project(radii, means, W, H)
    _same(R.front_sets(flat, valid, depths, mask, fp, P)[2], R.front_sets_brute(flat, valid, depths, mask, fp, P))


# -------------------------------------------------------------------------------------------------- argument checks
def _meta(n=8, w=16, h=12):
    return {"radii": torch.full((1, n, 2), 3, dtype=torch.int32), "means2d": torch.ones(1, n, 2), "depths": torch.ones(1, n),
            "width": w, "height": h}


def test_argument_checks_raise_before_the_gpu_is_touched():
    import collab_splats_amd as m
    from collab_splats_amd import grouping as G
    mask = np.ones((12, 16), np.int32)
    for kw in ({"num_patches": 0}, {"num_patches": 129}, {"num_patches": 2.0}, {"front_percentage": 0.0},
               {"front_percentage": 1.5}, {"front_percentage": float("nan")}, {"front_percentage": "x"}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            m.front_gaussians(_meta(), mask, **kw)
    with pytest.raises(ValueError, match="mask ids"):
        m.front_gaussians(_meta(), np.full((12, 16), 65536, np.int32))
    with pytest.raises(ValueError, match="mask ids"):
        m.front_gaussians(_meta(), torch.full((12, 16), -1, dtype=torch.int64))
    with pytest.raises(ValueError, match="integer mask ids"):
        m.front_gaussians(_meta(), np.ones((12, 16), np.float32))
    with pytest.raises(ValueError, match="integer mask ids"):
        m.front_gaussians(_meta(), np.ones((1, 12, 16), np.int32))
    with pytest.raises(ValueError, match="rendered at"):
        m.front_gaussians(_meta(), np.ones((16, 12), np.int32))
    with pytest.raises(ValueError, match="lacks"):
        m.front_gaussians({"radii": torch.ones(1, 8, 2)}, mask)
    with pytest.raises(ValueError, match="meta must hold"):
        m.front_gaussians(dict(_meta(), means2d=torch.ones(1, 7, 2)), mask)
    with pytest.raises(ValueError, match="width height"):
        m.project_gaussians(dict(_meta(), width=1 << 16, height=1 << 15))
    with pytest.raises(ValueError, match="one length"):
        m.front_gaussians({"proj_flattened": torch.zeros(8, dtype=torch.int64), "proj_depths": torch.ones(7),
                           "valid_mask": torch.ones(8, dtype=torch.bool)}, mask)
    with pytest.raises(ValueError, match="num_gaussians"):
        m.MemoryBank(8.0)
    with pytest.raises(ValueError, match="Gaussians"):
        m.MemoryBank(0)
    with pytest.raises(ValueError, match="Gaussians"):
        m.MemoryBank(1 << 31)
    with pytest.raises(ValueError, match="iou_threshold"):
        m.MemoryBank(8, "x")
    bank = m.MemoryBank(8)
    front = G.FrontGaussians(torch.full((9,), -1, dtype=torch.int32), torch.ones(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="bank holds 8"):
        bank.assign(front)
    with pytest.raises(ValueError, match="front_gaussians' result"):
        bank.assign({"mask_of": None})
    front = G.FrontGaussians(torch.full((8,), -1, dtype=torch.int32), torch.ones(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="labels must be an integer tensor"):
        bank.update(torch.zeros(2, dtype=torch.int64), front)
    with pytest.raises(ValueError, match="label must be in"):
        bank.members(0)
    bank.total_masks = (1 << 26) + 1                                  # M L beyond the overlap table
    with pytest.raises(ValueError, match="2\\^26"):
        bank.assign(front)
    with pytest.raises(ValueError, match="labels must be an integer tensor"):
        m.convert_matched_mask(torch.zeros(2), mask)
    with pytest.raises(ValueError, match="mask ids"):
        m.convert_matched_mask(torch.zeros(1, dtype=torch.int64), np.full((12, 16), 70000, np.int64))


def test_valid_arguments_on_the_host_fail_loudly_instead_of_falling_back():
    import collab_splats_amd as m
    with pytest.raises(m.MisplatError):
        m.front_gaussians(_meta(), np.ones((12, 16), np.int32))
    with pytest.raises(m.MisplatError):
        m.project_gaussians(_meta())
