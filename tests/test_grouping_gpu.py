"""GPU: Gaussian grouping (csrc/grouping.hip, collab_splats_amd/grouping.py) against the restatement
(tests/grouping_restatement.py) and the goldens recorded from the reference.  Everything compared is an integer: equality
throughout, no tolerances."""
import numpy as np
import pytest
import torch

import grouping_restatement as R
import grouping_scenes as Q
import tsdf_scenes as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _np(x):
    return x.detach().cpu().numpy()


@pytest.fixture(scope="module")
def gold():
    return Q.load_goldens()


def _meta(radii, means, depths, W, H):
    return {"radii": _t(radii)[None], "means2d": _t(means)[None], "depths": _t(depths)[None], "width": W, "height": H}


def _check_front(front, ref):
    ids, mask_of, sets = ref
    assert front.mask_of.dtype == front.counts.dtype == front.mask_ids.dtype == torch.int32 and front.mask_of.is_cuda
    assert np.array_equal(_np(front.mask_ids), ids)
    assert np.array_equal(_np(front.mask_of), mask_of)
    assert np.array_equal(_np(front.counts), [len(s) for s in sets])
    got = front.sets()
    assert len(got) == len(sets) and all(g.dtype == torch.int64 and np.array_equal(_np(g), s) for g, s in zip(got, sets))


def _front(radii, means, depths, mask, fp=0.5, P=32):
    import collab_splats_amd as m
    H, W = mask.shape
    front = m.front_gaussians(_meta(radii, means, depths, W, H), _t(mask), fp, P)
    flat, valid = R.project(radii, means, W, H)
    ref = R.front_sets(flat, valid, depths, mask, fp, P)
    _check_front(front, ref)
    return front, ref


# ------------------------------------------------------------------------------------------------------- projection
def test_project_gaussians_equals_the_reference(gold):
    import collab_splats_amd as m
    W, H, _ = (int(x) for x in gold["A_size"])
    means = gold["A_means2d"].copy()
    means[:4] = [[np.nan, 3.0], [np.inf, -np.inf], [2.5, 3.5], [-0.5, 0.5]]               # 2.5 -> 2, 3.5 -> 4, -0.5 -> 0, 0.5 -> 0
    pr = m.project_gaussians(_meta(gold["A_radii"], means, gold["A_depths"], W, H))
    flat, valid = R.project(gold["A_radii"], means, W, H)
    assert pr["proj_flattened"].dtype == torch.int64 and pr["valid_mask"].dtype == torch.bool and pr["proj_depths"].is_cuda
    assert np.array_equal(_np(pr["proj_flattened"]), flat) and np.array_equal(_np(pr["valid_mask"]), valid)
    assert np.array_equal(_np(pr["proj_flattened"][4:]), gold["A_flat"][4:]) and np.array_equal(_np(pr["valid_mask"]), gold["A_valid"])
    assert flat[:4].tolist() == [3 * W, W - 1, 2 + 4 * W, 0]
    assert np.array_equal(_np(pr["gaussian_ids"]), np.nonzero(valid)[0]) and np.array_equal(_np(pr["proj_depths"]), gold["A_depths"])
    # the result serves front_gaussians like the meta itself
    front = m.front_gaussians(pr, _t(gold["A_mask"]), 0.5, 32)
    _check_front(front, R.front_sets(flat, valid, gold["A_depths"], gold["A_mask"], 0.5, 32))


# -------------------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("N", [1, 63, 64, 65, 4095, 4096, 4097, 8193])
def test_front_at_wave_and_radix_tile_boundaries(N):
    """45 x 70 with 32 patches; N around one wave and around the sort's 4096-item tile, more than one tile at 8193."""
    W, H = 70, 45
    radii, means, depths = Q.random_view(N, N, W, H)
    mask = Q.blocks_mask(3, W, H, [3, 7, 8, 200, 4097], 9, 7)
    _front(radii, means, depths, mask)
    _front(radii, means, depths, mask, 0.2)


@pytest.mark.parametrize("ids,P,passes", [([3, 7, 8], 4, 1), ([3, 7, 8, 200, 4097], 128, 3)])
def test_front_cell_count_at_the_sort_pass_counts(ids, P, passes):
    """The second sort's keys are the cells 0 .. M P P (M P P: no cell), 8 bits a pass: 48 cells take one pass, 81 920 three
    (one-pixel patches, most of the 128 x 128 empty).  Two and four passes: the cases above and test_front_mask_ids_up_to_65535."""
    W, H, N = 70, 45, 3000
    radii, means, depths = Q.random_view(len(ids), N, W, H)
    mask = Q.blocks_mask(4, W, H, ids, 9, 7)
    none = len(ids) * P * P
    assert (none < 256, 65536 < none < 1 << 24) == (passes == 1, passes == 3)
    for fp in (0.5, 0.2):
        front, (got_ids, mask_of, _) = _front(radii, means, depths, mask, fp, P)
        assert got_ids.tolist() == ids and set(np.unique(mask_of)) == set(range(-1, len(ids)))


@pytest.mark.parametrize("W,H,P", [(70, 45, 32), (12, 20, 32), (33, 65, 7)])
def test_front_image_sizes_and_fractions(W, H, P):
    """45 x 70 with P = 32; 20 x 12 with P = 32 (one-pixel patches, most of the 32 x 32 empty); 65 x 33 with P = 7."""
    N = 3000
    radii, means, depths = Q.random_view(W, N, W, H)
    mask = Q.blocks_mask(H, W, H, [1, 2, 5, 6, 40], 5, 4)
    for fp in (0.5, 0.2, 0.29, 1.0, 1e-6):
        front, (ids, mask_of, sets) = _front(radii, means, depths, mask, fp, P)
        if fp == 1.0:                                                # everything valid on a mask pixel
            flat, valid = R.project(radii, means, W, H)
            assert np.array_equal(mask_of >= 0, valid & (mask.reshape(-1)[flat] > 0))
    front_t, _ = _front(radii, means, depths, mask.T.copy(), 0.5, P)                      # and the transposed image


def test_front_equals_the_reference_goldens(gold):
    import collab_splats_amd as m
    W, H, P = (int(x) for x in gold["A_size"])
    meta = _meta(gold["A_radii"], gold["A_means2d"], gold["A_depths"], W, H)
    for j, fp in enumerate(gold["A_fps"]):
        front = m.front_gaussians(meta, gold["A_mask"], float(fp), P)                     # a host image is uploaded
        want = Q.unpack(gold[f"A_ids{j}"], gold[f"A_off{j}"])
        assert [_np(s).tolist() for s in front.sets()] == [s.tolist() for s in want]
    W, H, P = (int(x) for x in gold["B_size"])
    front = m.front_gaussians(_meta(gold["B_radii"], gold["B_means2d"], gold["B_depths"], W, H), _t(gold["B_mask"]), 0.29, P)
    assert [_np(s).tolist() for s in front.sets()] == [s.tolist() for s in Q.unpack(gold["B_ids"], gold["B_off"])]
    assert int((front.mask_of[:100] >= 0).sum()) == 28                                   # the cell of 100: int(0.29 * 100) = 28


def test_front_edge_cases():
    W, H, N = 40, 30, 2000
    radii, means, depths = Q.random_view(5, N, W, H)
    mask = Q.blocks_mask(5, W, H, [1, 2, 3], 8, 6)
    # all Gaussians invalid
    front, _ = _front(np.ones_like(radii), means, depths, mask)
    assert int((front.mask_of >= 0).sum()) == 0 and front.num_masks == 3 and int(front.counts.sum()) == 0
    # an all-zero mask: M = 0
    front, _ = _front(radii, means, depths, np.zeros((H, W), np.int32))
    assert front.num_masks == 0 and front.sets() == [] and int((front.mask_of >= 0).sum()) == 0
    # one mask covering the whole image
    front, (_, _, sets) = _front(radii, means, depths, np.full((H, W), 9, np.int32))
    assert front.num_masks == 1 and len(sets[0]) > 0
    # all Gaussians in one cell: one mask, one patch
    big = radii.copy()
    big[:] = 2
    for fp in (0.5, 0.29, 1.0, 1e-6):
        front, (_, _, sets) = _front(big, means, depths, np.full((H, W), 9, np.int32), fp, 1)
        assert len(sets[0]) == max(int(fp * N), 1)
    # cells of size 1: distinct pixels, one-pixel patches -> every Gaussian is selected whatever the fraction
    n1 = W * H
    pix = np.random.default_rng(0).permutation(n1)
    m1 = np.stack([pix % W, pix // W], axis=1).astype(np.float32)
    front, (_, mask_of, _) = _front(np.full((n1, 2), 2, np.int32), m1, np.ones(n1, np.float32), np.full((H, W), 1, np.int32), 1e-6, 40)
    assert (mask_of == 0).all()
    # equal depths: ties go by id
    r, mm, d = Q.random_view(6, N, W, H, distinct_depths=False)
    for fp in (0.5, 0.2):
        _front(r, mm, d, mask, fp, 4)
    front, (_, mask_of, _) = _front(big, np.full((N, 2), 7.0, np.float32), np.full(N, 2.0, np.float32), np.full((H, W), 1, np.int32), 0.25, 8)
    assert np.array_equal(np.nonzero(mask_of == 0)[0], np.arange(N // 4))
    # negative, zero and infinite depths keep the order of the fp32 values
    d2 = depths.copy()
    d2[:6] = [-1.0, 0.0, np.inf, -np.inf, 1e-30, -1e-30]
    _front(big, means, d2, mask, 0.3, 3)


def test_front_mask_ids_up_to_65535():
    W, H, N = 64, 48, 4000
    radii, means, depths = Q.random_view(7, N, W, H)
    mask = Q.blocks_mask(7, W, H, [1, 255, 256, 32768, 65534, 65535], 8, 8)
    front, (ids, _, _) = _front(radii, means, depths, mask, 0.5, 32)
    assert ids[-1] == 65535 and ids[0] == 1
    front64 = __import__("collab_splats_amd").front_gaussians(_meta(radii, means, depths, W, H), _t(mask, torch.int64), 0.5, 32)
    assert torch.equal(front64.mask_of, front.mask_of)
    # many masks: one per pixel
    many = (np.arange(W * H, dtype=np.int32) + 1).reshape(H, W)
    _front(radii, means, depths, many, 0.5, 128)


def test_front_two_runs_are_bitwise_equal():
    W, H, N = 70, 45, 8193
    radii, means, depths = Q.random_view(8, N, W, H, distinct_depths=False)
    mask = Q.blocks_mask(8, W, H, [3, 4, 5, 6], 9, 7)
    a, _ = _front(radii, means, depths, mask, 0.5, 32)
    b, _ = _front(radii, means, depths, mask, 0.5, 32)
    assert torch.equal(a.mask_of, b.mask_of) and torch.equal(a.counts, b.counts) and torch.equal(a.mask_ids, b.mask_ids)


# ------------------------------------------------------------------------------------------------------------- bank
def _check_bank(bank, ref):
    assert bank.total_masks == ref.total_masks
    assert np.array_equal(_np(bank.sizes()), [len(b) for b in ref.bank])
    for label, b in enumerate(ref.bank):
        got = bank.members(label)
        assert got.dtype == torch.int64 and np.array_equal(_np(got), b), label


@pytest.mark.parametrize("tag", ["C", "D"])
def test_bank_replays_the_golden_sequences(gold, tag):
    import collab_splats_amd as m
    views, (W, H, P, N) = Q.golden_sequence(gold, tag)
    bank, again, ref = m.MemoryBank(N, 0.1), m.MemoryBank(N, 0.1), R.Bank(0.1)
    for radii, means, depths, mask, labels, sets, members in views:
        front = m.front_gaussians(_meta(radii, means, depths, W, H), _t(mask), 0.5, P)
        assert [_np(s).tolist() for s in front.sets()] == [s.tolist() for s in sets]
        got = bank.assign(front)
        assert got.dtype == torch.int64 and np.array_equal(_np(got), labels)
        assert np.array_equal(_np(bank.assign(front)), labels)                          # assign leaves the bank alone
        bank.update(got, front)
        assert torch.equal(again.associate(front), got)                                 # two runs are bitwise equal
        ref.update(labels, sets)
        for label, b in enumerate(members):
            assert np.array_equal(_np(bank.members(label)), b)
        _check_bank(bank, ref)
        assert torch.equal(again._off, bank._off) and torch.equal(again._lab, bank._lab)
        want = R.convert_matched_mask(labels, mask)
        img = m.convert_matched_mask(got, _t(mask))
        assert img.dtype == torch.int32 and np.array_equal(_np(img), want)
    if tag == "D":                                                   # inter 1, n 9; two masks, one label; an empty set
        assert _np(got).tolist() == [0, 0, 0, 1, 2] and _np(bank.sizes()).tolist() == [28, 0, 3]


def _sets_front(sets, N):
    """a FrontGaussians with the given disjoint sets"""
    from collab_splats_amd.grouping import FrontGaussians
    mask_of = np.full(N, -1, np.int32)
    for i, s in enumerate(sets):
        mask_of[s] = i
    return FrontGaussians(_t(mask_of), _t(np.arange(1, len(sets) + 1, dtype=np.int32)), _t(np.array([len(s) for s in sets], np.int32)))


@pytest.mark.parametrize("N", [300, 4097])
def test_bank_gaussians_with_many_labels_and_forced_labels(N):
    """update with labels of the caller's choice: every view puts its sets under new labels, so a Gaussian collects one label
    per view (lists grow at the front, in the middle and at the end); then assignments against that bank."""
    import collab_splats_amd as m
    rng = np.random.default_rng(N)
    bank, ref = m.MemoryBank(N, 0.1), R.Bank(0.1)
    for view in range(12):
        perm = rng.permutation(N)
        cuts = np.sort(rng.choice(np.arange(1, N), 3, replace=False))
        sets = [np.sort(s) for s in np.split(perm[: N - N // 5], cuts[cuts < N - N // 5])]
        M = len(sets)
        # a descending numbering of new labels, or old labels picked at random: insertions anywhere in the lists
        labels = (ref.total_masks + np.arange(M)[::-1]) if view % 3 != 2 else rng.integers(0, ref.total_masks, M)
        front = _sets_front(sets, N)
        bank.update(_t(labels.astype(np.int64)), front)
        ref.update(labels, sets)
        _check_bank(bank, ref)
    assert int((bank._off[1:] - bank._off[:-1]).max()) >= 8
    for view in range(3):
        perm = rng.permutation(N)
        sets = [np.sort(s) for s in np.array_split(perm[: N // 2], 5)] + [np.zeros(0, np.int64)]
        front = _sets_front(sets, N)
        assert np.array_equal(_np(bank.assign(front)), ref.assign(sets))
        assert np.array_equal(_np(bank.associate(front)), ref.associate(sets))
        _check_bank(bank, ref)
    with pytest.raises(ValueError, match="labels must be in"):
        bank.update(_t(np.full(len(sets), bank.total_masks + len(sets), np.int64)), front)
    _check_bank(bank, ref)                                           # a refused update changes nothing


def test_bank_thresholds_ties_and_more_labels_than_threads():
    """More labels than the assignment's 256 threads; equal q under several labels (the lowest wins, from any thread's stride);
    q exactly at, just under and over the threshold."""
    import collab_splats_amd as m
    N, L = 3000, 700
    bank, ref = m.MemoryBank(N, 0.1), R.Bank(0.1)
    sets0 = [np.array([i]) for i in range(L)]                        # label i = {i}
    bank.update(_t(np.arange(L, dtype=np.int64)), _sets_front(sets0, N))
    ref.update(np.arange(L), sets0)
    sets = [np.array([600, 300, 44, 1000, 1001]),                    # three labels with inter 1: the lowest, 44
            np.r_[699, 1100:1108],                                   # inter 1, n 9: q = float32(0.1), matches 699
            np.r_[257, 1200:1209],                                   # inter 1, n 10: below the threshold: new
            np.r_[5, 1300:1303],                                     # well above
            np.arange(2000, 2004)]                                   # no overlap: new
    front = _sets_front([np.sort(s) for s in sets], N)
    got = _np(bank.assign(front))
    assert got.tolist() == [44, 699, L, 5, L + 1] and np.array_equal(got, ref.assign([np.sort(s) for s in sets]))
    for thr, want in ((0.5, [L, L + 1, L + 2, L + 3, L + 4]), (0.0, [44, 699, 257, 5, 0]), (1.0 / 6.0, [44, L, L + 1, 5, L + 2])):
        b2, r2 = m.MemoryBank(N, thr), R.Bank(thr)
        b2.update(_t(np.arange(L, dtype=np.int64)), _sets_front(sets0, N))
        r2.update(np.arange(L), sets0)
        got = _np(b2.assign(front))
        assert np.array_equal(got, r2.assign([np.sort(s) for s in sets])) and got.tolist() == want, thr


# ------------------------------------------------------------------------------------------------------------ model
def test_model_associate_masks_equals_the_restatement_on_model_info():
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene, view_matrix
    W, H, N = 64, 48, 2000
    sc = random_scene(N, W, H, seed=33)
    model = radegs.RadegsModel(radegs.RadegsModelConfig(), sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"],
                               sc["sh"][:, 0], sc["sh"][:, 1:]).to(DEV)
    model.eval()
    model.step = 10 ** 6
    K = sc["Ks"][0].numpy().astype(np.float64)
    cams = [S.pinhole_camera(view_matrix(i)[0].numpy(), K, W, H) for i in range(3)]
    masks = []
    for v in range(3):                                               # rectangular masks, ids with a gap, some background
        mk = np.zeros((H, W), np.int32)
        mk[4:30, 3 + 5 * v:28 + 5 * v] = 1
        mk[10:44, 34:60] = 2 + v
        mk[34:46, 2:30] = 7
        masks.append(mk)
    bank, labels, matched = model.associate_masks(cams, [_t(mk) for mk in masks])
    ref = R.Bank(0.1)
    for v in range(3):
        model.get_outputs(cams[v])
        info = model.info
        assert int(info["width"]) == W and int(info["height"]) == H
        flat, valid = R.project(_np(info["radii"][0]), _np(info["means2d"][0]), W, H)
        sets = R.front_sets(flat, valid, _np(info["depths"][0]), masks[v], 0.5, 32)[2]
        assert sum(len(s) for s in sets) > 100
        want = ref.associate(sets)
        assert np.array_equal(_np(labels[v]), want)
        assert np.array_equal(_np(matched[v]), R.convert_matched_mask(want, masks[v]))
    _check_bank(bank, ref)
    assert bank.total_masks >= 3 and not model.training
    # a second call carries the bank on: the first view again re-matches its own labels
    bank2, labels2, _ = model.associate_masks(cams[:1], [masks[0]], bank=bank)
    assert bank2 is bank and np.array_equal(_np(labels2[0]), ref.associate(R.front_sets(*_model_view(model, cams[0], W, H), masks[0], 0.5, 32)[2]))
    _check_bank(bank, ref)


def _model_view(model, cam, W, H):
    model.get_outputs(cam)
    info = model.info
    flat, valid = R.project(_np(info["radii"][0]), _np(info["means2d"][0]), W, H)
    return flat, valid, _np(info["depths"][0])
