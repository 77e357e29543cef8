"""Inputs shared by the grouping tests (tests/test_grouping_host.py, tests/test_grouping_gpu.py): random views, block mask
images and the readers of tests/golden/grouping_goldens.npz."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grouping_goldens.npz")


def load_goldens():
    return dict(np.load(GOLD))


def unpack(ids, off):
    return [ids[off[i]:off[i + 1]].astype(np.int64) for i in range(len(off) - 1)]


def golden_sequence(gold, tag):
    """[(radii, means2d, depths, mask, labels, sets, bank)] per view of a golden sequence, and (W, H, P, N)."""
    W, H, P, N = (int(x) for x in gold[f"{tag}_size"])
    views = []
    for v, (gi, mi) in enumerate(gold[f"{tag}_views"]):
        views.append((gold[f"{tag}_radii{gi}"], gold[f"{tag}_means2d{gi}"], gold[f"{tag}_depths{gi}"], gold[f"{tag}_mask{mi}"],
                      gold[f"{tag}{v}_labels"].astype(np.int64), unpack(gold[f"{tag}{v}_ids"], gold[f"{tag}{v}_off"]),
                      unpack(gold[f"{tag}{v}_bank_ids"], gold[f"{tag}{v}_bank_off"])))
    return views, (W, H, P, N)


def random_view(seed, N, W, H, distinct_depths=True):
    """radii int32 [N,2] (some invalid), means2d fp32 [N,2] (some off screen, every 7th at an exact half), depths fp32 [N]"""
    rng = np.random.default_rng(seed)
    means = np.stack([rng.uniform(-6, W + 6, N), rng.uniform(-6, H + 6, N)], axis=1).astype(np.float32)
    means[::7] = np.floor(means[::7]) + 0.5
    radii = rng.integers(0, 5, (N, 2)).astype(np.int32)
    if distinct_depths:
        depths = rng.permutation(N).astype(np.float32) * 0.01 + 1.0
    else:
        depths = rng.integers(1, 6, N).astype(np.float32)             # many ties
    return radii, means, depths


def blocks_mask(seed, W, H, ids, bw, bh):
    """rectangular blocks of the given mask ids and background"""
    rng = np.random.default_rng(seed)
    grid = rng.choice(np.concatenate([[0], np.asarray(ids)]), size=(-(-H // bh), -(-W // bw)))
    return np.kron(grid, np.ones((bh, bw), np.int64))[:H, :W].astype(np.int32)
