"""Gaga-style Gaussian grouping on the MI355X (csrc/grouping.hip): per view, the front Gaussians of every
segmentation mask; across views, a memory bank of Gaussian sets per label.

The reference does this on the host (collab_splats/utils/grouping.py ``select_front_gaussians`` / ``process_mask_gaussians`` /
``_assign_labels`` / ``_update_memory_bank`` with utils/utils.py ``project_gaussians``): per mask a loop over up to 32 x 32
patches, each gathering an [H W] boolean through all N projected pixels, and one ``torch.unique(torch.cat(...))`` per (mask,
label) pair.  A pixel belongs to at most one mask and exactly one patch, so a Gaussian belongs to at most one (mask, patch) cell per
view: here the selection is one O(N) pass and two stable radix sorts, and the bank is a sorted label list per Gaussian.  Everything
works on device tensors; there is no CPU fallback.

What differs from the reference on purpose: equal depths inside a cell fall by lower Gaussian id (``torch.topk`` leaves ties
open); ``convert_matched_mask`` maps a mask id to ``label + 1`` by the id's rank among the ids present and returns int32 (the
reference asserts ids 1..M without gaps and wraps labels at uint8); ``RadegsModel.associate_masks`` processes every view (the
reference's loop ends with a stray ``break`` after the first frame).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from ._lib import load, ptr, require_gpu, run

MAX_PATCHES = 128
MAX_MASK_ID = 65535
MAX_PAIRS = 1 << 26                     # masks x labels of one assignment
_PROJ_KEYS = ("proj_flattened", "proj_depths", "valid_mask", "gaussian_ids")


# ---------------------------------------------------------------------------------------------------------- helpers
def _count(name: str, n: int) -> int:
    if not 1 <= n < 1 << 31:
        raise ValueError(f"{name}: the number of Gaussians must be in 1..2^31-1, got {n}")
    return n


def _meta_arrays(name: str, meta: Dict) -> Tuple[Tensor, Tensor, Tensor, int, int]:
    """camera 0 of the rasterizer's meta: radii [N,2], means2d [N,2], depths [N], width, height."""
    for k in ("radii", "means2d", "depths", "width", "height"):
        if k not in meta:
            raise ValueError(f"{name}: meta lacks {k!r} (the rasterizer's meta dict is expected)")
    radii, means2d, depths = meta["radii"], meta["means2d"], meta["depths"]
    if not all(isinstance(t, Tensor) for t in (radii, means2d, depths)):
        raise ValueError(f"{name}: meta's radii, means2d and depths must be tensors")
    if radii.dim() == 3:
        radii = radii[0]
    if means2d.dim() == 3:
        means2d = means2d[0]
    if depths.dim() == 2:
        depths = depths[0]
    n = int(depths.shape[0]) if depths.dim() == 1 else -1
    if n < 0 or tuple(radii.shape) != (n, 2) or tuple(means2d.shape) != (n, 2):
        raise ValueError(f"{name}: meta must hold radii [(C,)N,2], means2d [(C,)N,2] and depths [(C,)N], got "
                         f"{tuple(meta['radii'].shape)}, {tuple(meta['means2d'].shape)}, {tuple(meta['depths'].shape)}")
    w, h = int(meta["width"]), int(meta["height"])
    if w < 1 or h < 1 or w * h >= 1 << 31:
        raise ValueError(f"{name}: width height must be in 1..2^31-1, got {w} x {h}")
    _count(name, n)
    return radii, means2d, depths, w, h


def _project(radii: Tensor, means2d: Tensor, depths: Tensor, w: int, h: int) -> Tuple[Tensor, Tensor, Tensor]:
    """(flat int32 [N], valid uint8 [N], depths fp32 [N]) on the device."""
    require_gpu(radii, means2d, depths)
    n = int(depths.shape[0])
    if radii.dtype != torch.int32:                                   # (the rasterizer's are int32; anything else: by its own > 1)
        radii = (radii > 1).to(torch.int32) * 2
    radii = radii.detach().contiguous()
    means2d = means2d.detach().to(torch.float32).contiguous()
    flat = torch.empty(n, dtype=torch.int32, device=depths.device)
    valid = torch.empty(n, dtype=torch.uint8, device=depths.device)
    run("misplat_grouping_project", ptr(radii), ptr(means2d), n, w, h, ptr(flat), ptr(valid))
    return flat, valid, depths.detach().to(torch.float32).contiguous()


def project_gaussians(meta: Dict) -> Dict[str, Tensor]:
    """The reference's ``project_gaussians`` (utils.py:13-40) for camera 0 of the rasterizer's ``meta``, left on the device:
    ``proj_flattened`` int64 [N] (x + y W of the mean rounded half to even and clamped to the image: an off-screen Gaussian lands
    on a border pixel), ``proj_depths`` [N], ``valid_mask`` bool [N] (any radius > 1) and ``gaussian_ids`` int64 (the valid
    ones)."""
    radii, means2d, depths, w, h = _meta_arrays("project_gaussians", meta)
    flat, valid, depths = _project(radii, means2d, depths, w, h)
    valid = valid.view(torch.bool)
    return {"proj_flattened": flat.to(torch.int64), "proj_depths": depths, "valid_mask": valid,
            "gaussian_ids": valid.nonzero(as_tuple=False).squeeze(-1)}


def _mask_image(name: str, composite_mask) -> Tuple[Union[Tensor, np.ndarray], int, int]:
    """The [H,W] image of mask ids, its ids checked to be 0..65535 (on the host for a host image, by one read otherwise)."""
    m = composite_mask
    if isinstance(m, np.ndarray):
        if m.ndim != 2 or m.dtype.kind not in "biu":
            raise ValueError(f"{name}: composite_mask must be an [H,W] image of integer mask ids, got {m.dtype} {m.shape}")
    elif isinstance(m, Tensor):
        if m.dim() != 2 or m.dtype.is_floating_point or m.dtype.is_complex:
            raise ValueError(f"{name}: composite_mask must be an [H,W] image of integer mask ids, got {m.dtype} {tuple(m.shape)}")
    else:
        raise ValueError(f"{name}: composite_mask must be a tensor or an array, got {type(m).__name__}")
    h, w = (int(x) for x in m.shape)
    if h < 1 or w < 1 or h * w >= 1 << 31:
        raise ValueError(f"{name}: composite_mask must hold 1..2^31-1 pixels, got {h} x {w}")
    if not (isinstance(m, Tensor) and m.dtype in (torch.uint8, torch.bool)) and not (isinstance(m, np.ndarray) and m.dtype.kind == "b"):
        lo, hi = (int(m.min()), int(m.max()))
        if lo < 0 or hi > MAX_MASK_ID:
            raise ValueError(f"{name}: mask ids must be in 0..{MAX_MASK_ID}, got {lo}..{hi}")
    return m, w, h


def _mask_device(m, device) -> Tensor:
    if isinstance(m, np.ndarray):
        m = torch.from_numpy(np.ascontiguousarray(m).astype(np.int32))
    return m.detach().to(device=device, dtype=torch.int32).contiguous()


def _workspace(n: int, device) -> Tensor:
    b = int(load().misplat_grouping_workspace(n))
    if b < 0:
        raise ValueError(f"grouping: {n} Gaussians are beyond the library's limits (< 2^31)")
    return torch.empty(b, dtype=torch.uint8, device=device)


def _mask_ids(mask: Tensor, ws: Tensor) -> Tensor:
    """The ascending positive ids of the image (one host read: their number); leaves the id -> rank table in ws."""
    ids = torch.empty(MAX_MASK_ID, dtype=torch.int32, device=mask.device)
    n = torch.empty(1, dtype=torch.int32, device=mask.device)
    run("misplat_grouping_mask_ids", ptr(mask), mask.numel(), ptr(ws), ws.numel(), ptr(ids), ptr(n))
    return ids[:int(n.item())]


# ------------------------------------------------------------------------------------------------------- front sets
class FrontGaussians:
    """One view's selection: ``mask_ids`` int32 [M] (the positive ids of the mask image, ascending; a mask's index is its rank
    here), ``mask_of`` int32 [N] (the index of the mask a Gaussian was selected for, -1 for the others: a Gaussian is in at most
    one set) and ``counts`` int32 [M] (the set sizes)."""

    def __init__(self, mask_of: Tensor, mask_ids: Tensor, counts: Tensor):
        self.mask_of, self.mask_ids, self.counts = mask_of, mask_ids, counts

    @property
    def num_masks(self) -> int:
        return int(self.mask_ids.shape[0])

    @property
    def num_gaussians(self) -> int:
        return int(self.mask_of.shape[0])

    def sets(self) -> List[Tensor]:
        """Per mask the sorted ids (int64) of its Gaussians; a set has no order in the reference."""
        sel = (self.mask_of >= 0).nonzero(as_tuple=False).squeeze(-1)
        order = torch.sort(self.mask_of[sel], stable=True)[1]
        return list(torch.split(sel[order], self.counts.tolist()))


def front_gaussians(meta_or_proj: Dict, composite_mask, front_percentage: float = 0.5, num_patches: int = 32) -> FrontGaussians:
    """The reference's ``select_front_gaussians`` for one view.  ``meta_or_proj``: the rasterizer's ``meta`` (camera 0) or what
    ``project_gaussians`` returned; ``composite_mask`` [H,W]: integer mask ids 0..65535, 0 the background, gaps allowed.

    A valid Gaussian on a pixel of mask m belongs to the cell (m, patch of the pixel), the image being cut into ``num_patches`` x
    ``num_patches`` patches of ceil(W / P) x ceil(H / P) pixels.  A cell of n Gaussians keeps max(int(front_percentage n), 1) of
    them (a double product, truncated), the nearest by depth, equal depths by lower id; a mask's set is the union over its cells.
    The reference's ``associate()`` always uses the default 0.5 (``GroupingParams.front_percentage`` is never passed)."""
    name = "front_gaussians"
    if not isinstance(num_patches, int) or isinstance(num_patches, bool) or not 1 <= num_patches <= MAX_PATCHES:
        raise ValueError(f"{name}: num_patches must be an integer in 1..{MAX_PATCHES}, got {num_patches!r}")
    try:
        fp = float(front_percentage)
    except (TypeError, ValueError):
        fp = float("nan")
    if not 0.0 < fp <= 1.0:
        raise ValueError(f"{name}: front_percentage must be in (0, 1], got {front_percentage!r}")
    if not isinstance(meta_or_proj, dict) and not hasattr(meta_or_proj, "keys"):
        raise ValueError(f"{name}: the rasterizer's meta or project_gaussians' result is expected, got {type(meta_or_proj).__name__}")
    is_proj = all(k in meta_or_proj for k in _PROJ_KEYS[:3])
    if is_proj:
        flat, depths, valid = (meta_or_proj[k] for k in _PROJ_KEYS[:3])
        n = int(flat.shape[0]) if isinstance(flat, Tensor) and flat.dim() == 1 else -1
        if n < 0 or not all(isinstance(t, Tensor) and tuple(t.shape) == (n,) for t in (depths, valid)):
            raise ValueError(f"{name}: proj_flattened, proj_depths and valid_mask must be tensors of one length [N]")
        _count(name, n)
        mask, w, h = _mask_image(name, composite_mask)
        require_gpu(flat, depths, valid)
        flat = flat.to(torch.int32).contiguous()
        valid = (valid if valid.dtype == torch.bool else valid != 0).contiguous().view(torch.uint8)
        depths = depths.detach().to(torch.float32).contiguous()
    else:
        radii, means2d, depths, w, h = _meta_arrays(name, meta_or_proj)
        n = int(depths.shape[0])
        mask, mw, mh = _mask_image(name, composite_mask)
        if (mw, mh) != (w, h):
            raise ValueError(f"{name}: composite_mask is {mh} x {mw} but the view was rendered at {h} x {w}")
        flat, valid, depths = _project(radii, means2d, depths, w, h)
    dev = depths.device
    mask = _mask_device(mask, dev)
    require_gpu(mask)
    ws = _workspace(n, dev)
    ids = _mask_ids(mask, ws)
    m = int(ids.shape[0])
    mask_of = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(m, dtype=torch.int32, device=dev)
    run("misplat_grouping_front", ptr(flat), ptr(valid), ptr(depths), n, ptr(mask), w, h, num_patches, m, fp, ptr(ws),
        ws.numel(), ptr(mask_of), ptr(counts))
    return FrontGaussians(mask_of, ids, counts)


def convert_matched_mask(labels: Tensor, composite_mask) -> Tensor:
    """int32 [H,W]: every pixel of the mask of rank i (among the positive ids present, ascending) becomes ``labels[i] + 1``, the
    background stays 0.  Unlike the reference's version the ids may have gaps and nothing wraps at 255."""
    name = "convert_matched_mask"
    if not isinstance(labels, Tensor) or labels.dim() != 1 or labels.dtype.is_floating_point:
        raise ValueError(f"{name}: labels must be an integer tensor [M]")
    mask, w, h = _mask_image(name, composite_mask)
    require_gpu(labels)
    mask = _mask_device(mask, labels.device)
    ws = _workspace(1, labels.device)
    m = int(_mask_ids(mask, ws).shape[0])
    if m != int(labels.shape[0]):
        raise ValueError(f"{name}: {int(labels.shape[0])} labels for an image of {m} masks")
    out = torch.zeros(h, w, dtype=torch.int32, device=labels.device)
    if m > 0:
        labels = labels.to(torch.int64).contiguous()
        run("misplat_grouping_relabel", ptr(mask), h * w, ptr(ws), ws.numel(), ptr(labels), ptr(out))
    return out


# ------------------------------------------------------------------------------------------------------------- bank
class MemoryBank:
    """The reference's memory bank (grouping.py:284-351): per label the set of Gaussians seen under it, kept on the device as
    the ascending list of labels of every Gaussian (a Gaussian may carry several).

    ``assign`` compares every mask's set with every label's set as the bank stood before the view: inter = |bank[l] & set|, q =
    float32(inter / (n + inter + 1e-8)); the mask takes the lowest label of maximal q, or, when q < float32(iou_threshold), the
    next new label (numbered in mask order; an empty set opens an empty label).  Two masks of one view may take one label.  The
    first view (an empty bank) gets arange(M).  ``update`` merges every set into its label.  ``update`` reads one small vector
    back (the new number of pairs and the label range); ``assign`` reads nothing."""

    def __init__(self, num_gaussians: int, iou_threshold: float = 0.1):
        if not isinstance(num_gaussians, int) or isinstance(num_gaussians, bool):
            raise ValueError(f"MemoryBank: num_gaussians must be an integer, got {num_gaussians!r}")
        self.num_gaussians = _count("MemoryBank", num_gaussians)
        try:
            t = float(iou_threshold)
        except (TypeError, ValueError):
            t = float("nan")
        if t != t:
            raise ValueError(f"MemoryBank: iou_threshold must be a number, got {iou_threshold!r}")
        self.iou_threshold = t
        self.total_masks = 0
        self._pairs = 0
        self._off: Optional[Tensor] = None                           # int32 [N + 1]
        self._lab: Optional[Tensor] = None                           # int32 [max(pairs, 1)]
        self._sizes: Optional[Tensor] = None                         # int32 [total_masks]
        self._ws: Optional[Tensor] = None

    def _check_front(self, name: str, front: FrontGaussians) -> None:
        if not isinstance(front, FrontGaussians):
            raise ValueError(f"{name}: front_gaussians' result is expected, got {type(front).__name__}")
        if front.num_gaussians != self.num_gaussians:
            raise ValueError(f"{name}: the view selects among {front.num_gaussians} Gaussians, the bank holds {self.num_gaussians}")
        if front.num_masks * self.total_masks > MAX_PAIRS:
            raise ValueError(f"{name}: {front.num_masks} masks x {self.total_masks} labels are beyond the library's limits "
                             f"(<= 2^26 pairs)")

    def _state(self, device) -> None:
        if self._off is None:
            self._off = torch.zeros(self.num_gaussians + 1, dtype=torch.int32, device=device)
            self._lab = torch.zeros(1, dtype=torch.int32, device=device)     # (never empty: an empty tensor has no pointer)
            self._sizes = torch.zeros(0, dtype=torch.int32, device=device)
            self._ws = _workspace(self.num_gaussians, device)

    def assign(self, front: FrontGaussians) -> Tensor:
        """labels int64 [M] for the view's masks; the bank is not changed."""
        self._check_front("MemoryBank.assign", front)
        require_gpu(front.mask_of)
        dev = front.mask_of.device
        self._state(dev)
        m, l = front.num_masks, self.total_masks
        labels = torch.empty(m, dtype=torch.int64, device=dev)
        if m == 0:
            return labels
        count = None
        if l > 0:
            count = torch.empty(m * l, dtype=torch.int32, device=dev)
            run("misplat_grouping_overlap", ptr(front.mask_of), self.num_gaussians, ptr(self._off), ptr(self._lab), m, l,
                ptr(count))
        n_new = torch.empty(1, dtype=torch.int32, device=dev)
        run("misplat_grouping_assign", ptr(count), ptr(front.counts), m, l, self.iou_threshold, ptr(labels), ptr(n_new))
        return labels

    def update(self, labels: Tensor, front: FrontGaussians) -> None:
        """bank[labels[i]] |= set i, for every mask of the view.  Labels may be old ones or new ones up to total_masks + M - 1."""
        name = "MemoryBank.update"
        self._check_front(name, front)
        m, n = front.num_masks, self.num_gaussians
        if not isinstance(labels, Tensor) or tuple(labels.shape) != (m,) or labels.dtype.is_floating_point:
            raise ValueError(f"{name}: labels must be an integer tensor [M] with M = {m}")
        if m == 0:
            return
        if self._pairs + n >= 1 << 31:
            raise ValueError(f"{name}: the bank would exceed 2^31 (Gaussian, label) pairs")
        require_gpu(labels, front.mask_of)
        dev = front.mask_of.device
        self._state(dev)
        labels = labels.to(torch.int64).contiguous()
        new_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
        run("misplat_grouping_merge_count", ptr(front.mask_of), n, ptr(labels), m, ptr(self._off), ptr(self._lab),
            ptr(self._ws), self._ws.numel(), ptr(new_off))
        lo, hi = torch.aminmax(labels)
        pairs, lo, hi = torch.stack((new_off[n].to(torch.int64), lo, hi)).tolist()      # the call's host read
        if lo < 0 or hi >= self.total_masks + m:
            raise ValueError(f"{name}: labels must be in 0..{self.total_masks + m - 1} (old labels, or new ones numbered from "
                             f"total_masks), got {lo}..{hi}")
        total = max(self.total_masks, hi + 1)
        sizes = torch.zeros(total, dtype=torch.int32, device=dev)
        sizes[:self.total_masks] = self._sizes
        new_lab = torch.empty(pairs, dtype=torch.int32, device=dev) if pairs > 0 else torch.zeros(1, dtype=torch.int32, device=dev)
        run("misplat_grouping_merge_copy", ptr(front.mask_of), n, ptr(labels), m, ptr(self._off), ptr(self._lab), ptr(new_off),
            pairs, ptr(new_lab), ptr(sizes), total)
        self._off, self._lab, self._sizes, self._pairs, self.total_masks = new_off, new_lab, sizes, pairs, total

    def associate(self, front: FrontGaussians) -> Tensor:
        """``assign`` then ``update``; returns the labels."""
        labels = self.assign(front)
        self.update(labels, front)
        return labels

    def sizes(self) -> Tensor:
        """int64 [total_masks]: the number of Gaussians under every label."""
        if self._sizes is None:
            return torch.zeros(0, dtype=torch.int64)
        return self._sizes.to(torch.int64)

    def members(self, label: int) -> Tensor:
        """int64: the sorted ids of the Gaussians under ``label``."""
        if not isinstance(label, int) or isinstance(label, bool) or not 0 <= label < self.total_masks:
            raise ValueError(f"MemoryBank.members: label must be in 0..{self.total_masks - 1}, got {label!r}")
        flags = torch.empty(self.num_gaussians, dtype=torch.uint8, device=self._off.device)
        run("misplat_grouping_members", ptr(self._off), ptr(self._lab), self.num_gaussians, label, ptr(flags))
        return flags.view(torch.bool).nonzero(as_tuple=False).squeeze(-1)
