"""numpy restatement of the Gaga-style Gaussian grouping (collab_splats/utils/grouping.py ``select_front_gaussians`` /
``process_mask_gaussians`` / ``_assign_labels`` / ``_update_memory_bank`` and utils/utils.py ``project_gaussians``): the oracle of
csrc/grouping.hip.  Test infrastructure only; the product never imports it.

A pixel belongs to at most one mask and exactly one patch, so a Gaussian belongs to at most one (mask, patch) cell per view: the
reference's loop over masks and patches is a segmented "front fraction by depth" over cells.  ``front_sets`` is that form,
``front_sets_brute`` the reference's loop structure; tests/test_grouping_host.py holds them equal.

Stated choices where the reference leaves something open: inside a cell equal depths fall by lower Gaussian id (``torch.topk``
leaves ties open); depths are ordered by ``depth_key`` (a total order of the fp32 bit patterns: -0 below +0, NaNs at the ends);
a NaN mean lands on pixel 0.
"""
import numpy as np


def depth_key(d):
    """uint32 keys whose unsigned order is the order of the fp32 values."""
    b = np.ascontiguousarray(d, np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def project(radii, means2d, W, H):
    """utils.py:13-40 for one camera: (flat int64 [N], valid bool [N]).  radii [N,2], means2d [N,2]."""
    valid = (np.asarray(radii) > 1).any(axis=1)
    r = np.rint(np.asarray(means2d, np.float32))                   # half to even, as torch.round
    r = np.where(np.isnan(r), np.float32(0), r)
    x = np.clip(r[:, 0], 0, W - 1).astype(np.int64)
    y = np.clip(r[:, 1], 0, H - 1).astype(np.int64)
    return x + y * W, valid


def mask_ids(composite):
    u = np.unique(np.asarray(composite))
    return u[u > 0].astype(np.int64)


def patch_of(flat, W, H, P):
    pw, ph = -(-W // P), -(-H // P)
    return np.minimum((flat // W) // ph, P - 1), np.minimum((flat % W) // pw, P - 1)


def front_count(fp, n):
    """max(int(fp * n), 1): a double product, truncated (0.29 * 100 -> 28)."""
    return np.maximum((np.float64(fp) * np.asarray(n, np.float64)).astype(np.int64), 1)


def front_sets(flat, valid, depths, composite, fp=0.5, P=32):
    """(mask_ids [M], mask_of int32 [N] (-1: not selected), sets: M sorted int64 arrays)."""
    composite = np.asarray(composite)
    H, W = composite.shape
    ids = mask_ids(composite)
    N = len(flat)
    mask_of = np.full(N, -1, np.int32)
    pix = composite.reshape(-1)[flat].astype(np.int64)
    g = np.nonzero(np.asarray(valid) & (pix > 0))[0]
    if len(g):
        m = np.searchsorted(ids, pix[g])
        py, px = patch_of(np.asarray(flat)[g], W, H, P)
        cell = (m * P + py) * P + px
        order = np.lexsort((g, depth_key(np.asarray(depths)[g]), cell))
        cs, gs, ms = cell[order], g[order], m[order]
        start = np.searchsorted(cs, cs, side="left")
        n = np.searchsorted(cs, cs, side="right") - start
        keep = (np.arange(len(cs)) - start) < front_count(fp, n)
        mask_of[gs[keep]] = ms[keep]
    return ids, mask_of, [np.nonzero(mask_of == i)[0].astype(np.int64) for i in range(len(ids))]


def front_sets_brute(flat, valid, depths, composite, fp=0.5, P=32):
    """The reference's structure: per mask, per non-empty patch, gather, filter, take the front k.  M sorted int64 arrays."""
    composite = np.asarray(composite)
    H, W = composite.shape
    flat, valid, key = np.asarray(flat), np.asarray(valid), depth_key(depths)
    py, px = patch_of(np.arange(H * W), W, H, P)
    out = []
    for i in mask_ids(composite):
        binary = composite.reshape(-1) == i
        picked = []
        for a in range(P):
            for b in range(P):
                patch = binary & (py == a) & (px == b)
                if not patch.any():
                    continue
                gs = np.nonzero(patch[flat])[0]
                gs = gs[valid[gs]]
                if len(gs) == 0:
                    continue
                k = max(int(fp * len(gs)), 1)
                if k < len(gs):
                    gs = gs[np.argsort(key[gs], kind="stable")[:k]]
                picked.append(gs)
        out.append(np.sort(np.concatenate(picked)).astype(np.int64) if picked else np.zeros(0, np.int64))
    return out


class Bank:
    """grouping.py:284-351: the memory bank of Gaussian sets per label."""

    def __init__(self, iou_threshold=0.1):
        self.threshold = np.float32(iou_threshold)
        self.bank = []

    @property
    def total_masks(self):
        return len(self.bank)

    def assign(self, sets):
        M, L = len(sets), len(self.bank)
        if L == 0:
            return np.arange(M, dtype=np.int64)
        labels = np.zeros(M, np.int64)
        total = L
        for i, s in enumerate(sets):
            inter = np.array([len(np.intersect1d(b, s)) for b in self.bank], np.int64)
            q = (inter / (len(s) + inter + 1e-8)).astype(np.float32)          # the quotient in double, stored as fp32
            sel = int(np.argmax(q))                                            # the lowest label among equals
            if q[sel] < self.threshold:
                sel = total
                total += 1
            labels[i] = sel
        return labels

    def update(self, labels, sets):
        for label, s in zip(np.asarray(labels).tolist(), sets):
            while label >= len(self.bank):
                self.bank.append(np.zeros(0, np.int64))
            self.bank[label] = np.union1d(self.bank[label], s).astype(np.int64)

    def associate(self, sets):
        labels = self.assign(sets)
        self.update(labels, sets)
        return labels


def convert_matched_mask(labels, composite):
    """int32 image: a pixel of the mask of rank i gets labels[i] + 1, background 0."""
    composite = np.asarray(composite)
    ids = mask_ids(composite)
    assert len(ids) == len(labels)
    table = np.zeros(int(ids.max()) + 1 if len(ids) else 1, np.int64)
    table[ids] = np.asarray(labels, np.int64) + 1
    return table[composite.astype(np.int64)].astype(np.int32)
