"""Generates tests/golden/grouping_goldens.npz by RUNNING THE REFERENCE's own code in the build container, as
make_depthcloud_goldens.py does: only the input and output arrays are committed, nothing of the reference's text.

The reference's files cannot be imported here (nerfstudio, cv2, SAM): they are parsed, and only ``project_gaussians``
(utils/utils.py), ``create_patch_mask`` and ``mask_id_to_binary_mask`` (utils/segmentation.py) and the methods
``process_mask_gaussians``, ``select_front_gaussians``, ``_assign_labels`` and ``_update_memory_bank`` of grouping.py's class are
executed, with their decorators stripped (``torch.compile(max-autotune)`` is not exercised).

``torch.topk`` leaves equal depths open: the generator asserts that no cell of any scene has equal depths at its k-th boundary,
so the reference's sets are unambiguous.

    python tests/golden/make_grouping_goldens.py
"""
import ast
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import grouping_restatement as R  # noqa: E402

REF = "/root/reference/collab_splats"
OUT = os.path.join(HERE, "grouping_goldens.npz")


def _functions(path, names, inside_class=False):
    tree = ast.parse(open(path).read())
    body = tree.body
    if inside_class:
        body = [n for c in tree.body if isinstance(c, ast.ClassDef) for n in c.body]
    found = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in found) == sorted(names), [n.name for n in found]
    for n in found:
        n.decorator_list = []
    return ast.fix_missing_locations(ast.Module(body=found, type_ignores=[]))


def load_reference():
    ns = {"torch": torch, "np": np, "math": math, "Dict": dict, "tqdm": lambda it, **kw: it}
    for path, names, inside in (
            (os.path.join(REF, "utils", "utils.py"), ["project_gaussians"], False),
            (os.path.join(REF, "utils", "segmentation.py"), ["create_patch_mask", "mask_id_to_binary_mask"], False),
            (os.path.join(REF, "utils", "grouping.py"), ["process_mask_gaussians", "select_front_gaussians", "_assign_labels",
                                                          "_update_memory_bank"], True)):
        exec(compile(_functions(path, names, inside), path, "exec"), ns)
    return ns


class Grouper:
    """The state the reference's methods touch, around the executed functions."""

    def __init__(self, ns, iou_threshold=0.1):
        self.ns = ns
        self.params = types.SimpleNamespace(debug=False, iou_threshold=iou_threshold)
        self.memory_bank = []
        self.total_masks = 0
        self.process_mask_gaussians = ns["process_mask_gaussians"]

    def select(self, meta, composite, P, fp=None):
        patch = self.ns["create_patch_mask"](np.zeros(composite.shape + (3,)), num_patches=P)
        kw = {} if fp is None else {"front_percentage": fp}
        sets = self.ns["select_front_gaussians"](self, meta=meta, composite_mask=composite, patch_mask=patch, **kw)
        return [torch.sort(s)[0].numpy().astype(np.int64) for s in sets]

    def assign(self, sets):
        return self.ns["_assign_labels"](self, [torch.from_numpy(s) for s in sets]).numpy()

    def update(self, labels, sets):
        self.ns["_update_memory_bank"](self, torch.from_numpy(labels), [torch.from_numpy(s) for s in sets])


def meta_of(radii, means2d, depths, W, H):
    return {"radii": torch.from_numpy(radii)[None], "means2d": torch.from_numpy(means2d)[None],
            "depths": torch.from_numpy(depths)[None], "width": W, "height": H}


def pack(sets):
    """sorted id lists as (concatenated ids int32, offsets int32)."""
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    return (np.concatenate(sets) if sets else np.zeros(0)).astype(np.int32), off


def assert_unambiguous(flat, valid, depths, composite, fp, P):
    """no cell has equal depths at its k-th boundary"""
    H, W = composite.shape
    ids = R.mask_ids(composite)
    pix = composite.reshape(-1)[flat]
    g = np.nonzero(valid & (pix > 0))[0]
    py, px = R.patch_of(flat[g], W, H, P)
    cell = (np.searchsorted(ids, pix[g]) * P + py) * P + px
    for c in np.unique(cell):
        d = np.sort(depths[g[cell == c]])
        k = int(R.front_count(fp, len(d)))
        assert k >= len(d) or d[k - 1] != d[k], (c, k)


def random_view(rng, N, W, H, halves=True):
    means = np.stack([rng.uniform(-6, W + 6, N), rng.uniform(-6, H + 6, N)], axis=1).astype(np.float32)    # some off screen
    if halves:
        means[::7] = np.floor(means[::7]) + 0.5                                                              # exact halves
    radii = rng.integers(0, 5, (N, 2)).astype(np.int32)                                                      # (0,1),(1,1).. invalid
    depths = rng.permutation(N).astype(np.float32) * 0.01 + 1.0                                              # all distinct
    return radii, means, depths


def blocks_mask(rng, W, H, ids, bw, bh):
    """rectangular blocks of mask ids (with gaps) and background"""
    grid = rng.choice(np.concatenate([[0], ids]), size=(-(-H // bh), -(-W // bw)))
    return np.kron(grid, np.ones((bh, bw), np.int64))[:H, :W].astype(np.int32)


def check(got, want, what):
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        assert np.array_equal(a, b), what


def main():
    ns = load_reference()
    out = {}
    # ---- A: selection on 45 x 70, ids with gaps, halves, off-screen means, three fractions
    rng = np.random.default_rng(0)
    W, H, N, P = 70, 45, 2000, 32
    radii, means, depths = random_view(rng, N, W, H)
    comp = blocks_mask(rng, W, H, np.array([3, 7, 8, 200, 4097, 65535]), 9, 7)
    flat, valid = R.project(radii, means, W, H)
    pr = ns["project_gaussians"](meta_of(radii, means, depths, W, H))
    assert np.array_equal(pr["proj_flattened"].numpy(), flat) and np.array_equal(pr["valid_mask"].numpy(), valid)
    out.update(A_radii=radii, A_means2d=means, A_depths=depths, A_mask=comp, A_size=np.array([W, H, P]), A_flat=flat.astype(np.int32),
               A_valid=valid, A_fps=np.array([0.5, 0.2, 1.0]))
    for j, fp in enumerate([0.5, 0.2, 1.0]):
        assert_unambiguous(flat, valid, depths, comp, fp, P)
        sets = Grouper(ns).select(meta_of(radii, means, depths, W, H), comp, P, fp)
        check(R.front_sets(flat, valid, depths, comp, fp, P)[2], sets, ("A", fp))
        out[f"A_ids{j}"], out[f"A_off{j}"] = pack(sets)
    # ---- B: one-pixel patches (20 x 12, P = 32); a cell of exactly 100 valid Gaussians with 0.29 -> k = 28
    rng = np.random.default_rng(1)
    W, H, N, P = 20, 12, 400, 32
    radii, means, depths = random_view(rng, N, W, H, halves=False)
    comp = blocks_mask(rng, W, H, np.array([1, 2, 5]), 5, 4)
    comp[6, 11] = 5
    means[:100] = [11.2, 5.8]                                                                               # pixel (11, 6)
    radii[:100] = 3
    flat, valid = R.project(radii, means, W, H)
    others = (flat == 11 + 6 * W) & valid
    others[:100] = False
    radii[others] = 0                                                                                       # exactly 100 there
    flat, valid = R.project(radii, means, W, H)
    assert int((valid & (flat == 11 + 6 * W)).sum()) == 100
    assert_unambiguous(flat, valid, depths, comp, 0.29, P)
    sets = Grouper(ns).select(meta_of(radii, means, depths, W, H), comp, P, 0.29)
    check(R.front_sets(flat, valid, depths, comp, 0.29, P)[2], sets, "B")
    assert sum(int((s < 100).sum()) for s in sets) == 28
    out.update(B_radii=radii, B_means2d=means, B_depths=depths, B_mask=comp, B_size=np.array([W, H, P]))
    out["B_ids"], out["B_off"] = pack(sets)
    # ---- C: four views, the first and the second seen again (old labels are re-matched), the default fraction
    rng = np.random.default_rng(2)
    W, H, N, P = 65, 33, 900, 7
    v0 = random_view(rng, N, W, H)
    v1 = random_view(rng, N, W, H)
    v1 = (v1[0], (0.5 * v0[1] + 0.5 * v1[1]).astype(np.float32), v1[2])
    m0 = blocks_mask(rng, W, H, np.array([1, 2, 3, 4, 9]), 13, 11)
    m1 = blocks_mask(rng, W, H, np.array([2, 4, 6, 8, 10, 12]), 8, 17)
    out["C_size"] = np.array([W, H, P, N])
    _sequence(ns, out, "C", [v0, v1], [m0, m1], [(0, 0), (1, 1), (0, 0), (1, 0)], W, H, P)
    # ---- D: the threshold case inter = 1, n = 9 (matches: fp32 comparison), an empty mask set, two masks taking one label
    W, H, N, P = 20, 12, 40, 32                                      # one-pixel patches: every valid Gaussian is selected
    def view(pixels, valid_ids):
        means = np.array([[p % W, p // W] for p in pixels], np.float32)
        radii = np.zeros((N, 2), np.int32)
        radii[valid_ids] = 2
        return radii, means, (np.arange(N, dtype=np.float32) + 1.0)
    pixels = np.arange(N) * 3 % (W * H)                                                                     # distinct pixels
    compD0 = np.zeros((H, W), np.int32)
    compD0.reshape(-1)[pixels[:20]] = 1                              # view 0: Gaussians 0..19 valid; mask 1 = 0..19
    compD1 = np.zeros((H, W), np.int32)
    compD1.reshape(-1)[pixels[[19, 20, 21, 22, 23, 24, 25, 26, 27]]] = 4     # mask 4: 9 Gaussians, one (19) in label 0
    compD1.reshape(-1)[pixels[[0, 1, 2]]] = 6                        # mask 6: inside label 0
    compD1.reshape(-1)[pixels[[3, 4]]] = 9                           # mask 9: inside label 0 too: two masks, one label
    compD1.reshape(-1)[pixels[[30, 31]]] = 11                        # mask 11: only invalid Gaussians: an empty set
    compD1.reshape(-1)[pixels[[32, 33, 34]]] = 12                    # mask 12: new Gaussians: a new label
    out["D_size"] = np.array([W, H, P, N])
    labels = _sequence(ns, out, "D", [view(pixels, np.arange(20)), view(pixels, np.r_[0:5, 19:28, 32:35])], [compD0, compD1],
                       [(0, 0), (1, 1)], W, H, P)
    assert labels[1].tolist() == [0, 0, 0, 1, 2], labels[1]
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(out), "arrays,", os.path.getsize(OUT), "bytes")


def _sequence(ns, out, tag, gauss, masks, views, W, H, P):
    """views: (index into gauss, index into masks) per view; the inputs are stored once"""
    ref, mine, all_labels = Grouper(ns), R.Bank(0.1), []
    out[f"{tag}_views"] = np.array(views)
    for i, (radii, means, depths) in enumerate(gauss):
        out.update({f"{tag}_radii{i}": radii, f"{tag}_means2d{i}": means, f"{tag}_depths{i}": depths})
    for i, comp in enumerate(masks):
        out[f"{tag}_mask{i}"] = comp
    for v, (gi, mi) in enumerate(views):
        (radii, means, depths), comp = gauss[gi], masks[mi]
        flat, valid = R.project(radii, means, W, H)
        assert_unambiguous(flat, valid, depths, comp, 0.5, P)
        sets = ref.select(meta_of(radii, means, depths, W, H), comp, P)
        check(R.front_sets(flat, valid, depths, comp, 0.5, P)[2], sets, (tag, v))
        labels = ref.assign(sets)
        assert np.array_equal(mine.assign(sets), labels), (tag, v)
        ref.update(labels, sets)
        mine.update(labels, sets)
        assert ref.total_masks == mine.total_masks == len(ref.memory_bank)
        bank = [np.unique(b.numpy()).astype(np.int64) for b in ref.memory_bank]
        check(mine.bank, bank, (tag, v, "bank"))
        out[f"{tag}{v}_labels"] = labels.astype(np.int32)
        out[f"{tag}{v}_ids"], out[f"{tag}{v}_off"] = pack(sets)
        out[f"{tag}{v}_bank_ids"], out[f"{tag}{v}_bank_off"] = pack(bank)
        all_labels.append(labels)
    return all_labels


if __name__ == "__main__":
    main()
