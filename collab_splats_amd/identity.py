"""Identity training for Gaussian grouping (plumbing around csrc/identity.hip; no kernels and no arithmetic here).

The step after ``RadegsModel.associate_masks``: every Gaussian carries an identity vector, the vectors are rendered as
pass-through channels, a 1 x 1 convolution classifies every pixel onto the bank's labels and is trained with cross-entropy
against the ``matched`` images, plus a KL term that keeps the classes of neighbouring Gaussians alike.  This is the recipe of
Gaussian Grouping (Ye et al., ECCV 2024) and Gaga (Lyu et al., 2024).  The reference only sketches it
(collab_splats/utils/grouping.py:110-136, ``GroupingClassifier.setup_train``: ``torch.nn.Parameter(n, dim)``
is not valid, ``in_proj`` is never used, no training loop exists), so everything here is restated from the published method
and parity with the reference is unpinned.  ``in_proj`` stays out for that reason.  DESIGN.md section 33.

``identity_loss`` and ``identity_3d_loss`` are one autograd node each over fused kernels that never form a [K, P] tensor;
``identity_labels`` is one launch.  Reachable as ``ops.identity_loss`` / ``ops.identity_labels`` / ``ops.identity_3d_loss``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple, Union

import torch
from torch import Tensor, nn

from . import _lib
from ._lib import ptr, require_gpu, run
from .featureloss import _features_view

MAX_DIM = 32
MAX_CLASSES = 4096
MAX_NEIGHBOURS = 16


class IdentityField(nn.Module):
    """The trainable state of identity training: ``identities`` [N, identity_dim] (zeros by default) and ``classifier``, a
    1 x 1 convolution identity_dim -> num_classes with the reference's parameter shape [K, D, 1, 1] (grouping.py:125).  The
    parameters are contiguous fp32 tensors: ``FusedAdam`` takes them as they are."""

    def __init__(self, num_gaussians: int, num_classes: int, identity_dim: int = 16, identities: Optional[Tensor] = None):
        super().__init__()
        _check_sizes(identity_dim, num_classes, "IdentityField")
        if int(num_gaussians) < 1:
            raise ValueError(f"IdentityField: at least one Gaussian, got {num_gaussians}")
        if identities is None:
            identities = torch.zeros(int(num_gaussians), int(identity_dim), dtype=torch.float32)
        elif tuple(identities.shape) != (int(num_gaussians), int(identity_dim)) or identities.dtype != torch.float32:
            raise ValueError(f"IdentityField: identities must be float32 [{num_gaussians}, {identity_dim}], got "
                             f"{identities.dtype} {tuple(identities.shape)}")
        self.identities = nn.Parameter(identities.detach().clone().contiguous())
        self.classifier = nn.Conv2d(int(identity_dim), int(num_classes), kernel_size=1)

    @property
    def identity_dim(self) -> int:
        return self.classifier.in_channels

    @property
    def num_classes(self) -> int:
        return self.classifier.out_channels

    def flat(self) -> Tuple[Tensor, Tensor]:
        """(weight [K, D], bias [K]): views of the convolution's parameters (gradients flow)."""
        c = self.classifier
        return c.weight.view(c.out_channels, c.in_channels), c.bias

    def loss_2d(self, rendered: Tensor, target: Tensor, validate: bool = True) -> Tensor:
        return identity_loss(rendered, self, target, validate)

    def loss_3d(self, neighbours: "IdentityNeighbours") -> Tensor:
        return identity_3d_loss(self.identities, self, neighbours)

    @torch.no_grad()
    def pixel_labels(self, rendered: Tensor, return_confidence: bool = False):
        return identity_labels(rendered, self, return_confidence)

    @torch.no_grad()
    def gaussian_labels(self, return_confidence: bool = False):
        """[N] int32 class + 1 of every Gaussian's own identity vector."""
        n = int(self.identities.shape[0])
        out = identity_labels(self.identities.detach().view(n, 1, -1), self, return_confidence)
        return (out[0].view(n), out[1].view(n)) if return_confidence else out.view(n)


Classifier = Union[IdentityField, Tuple[Tensor, Tensor]]


class IdentityNeighbours:
    """The pairs of the 3-D loss: ``sample`` [M] int64 rows and ``table`` [M, k] int32 (k in 1..16) neighbour rows; an entry
    that is -1 or its own sample is skipped.  The reverse table -- for every row the slots (2 * pair + side; side 0 the sample,
    1 the entry) that name it, a CSR in ascending slot order -- is built once here with a stable sort: the backward GATHERS a
    row's gradient through it, in that fixed order."""

    def __init__(self, sample: Tensor, table: Tensor, num_rows: int):
        if sample.dim() != 1 or sample.dtype != torch.int64 or sample.shape[0] < 1:
            raise ValueError(f"IdentityNeighbours: sample must be a non-empty int64 [M], got {sample.dtype} {tuple(sample.shape)}")
        if table.dim() != 2 or table.dtype != torch.int32 or table.shape[0] != sample.shape[0]:
            raise ValueError(f"IdentityNeighbours: table must be int32 [M, k] with M = {sample.shape[0]}, got {table.dtype} "
                             f"{tuple(table.shape)}")
        if not 1 <= int(table.shape[1]) <= MAX_NEIGHBOURS:
            raise ValueError(f"IdentityNeighbours: k must be 1..{MAX_NEIGHBOURS}, got {table.shape[1]}")
        if int(num_rows) < 1 or int(sample.shape[0]) * int(table.shape[1]) > 2 ** 27:
            raise ValueError(f"IdentityNeighbours: num_rows must be >= 1 and M k <= 2^27, got {num_rows} and {tuple(table.shape)}")
        require_gpu(sample, table)
        self.sample, self.table, self.num_rows = sample.contiguous(), table.contiguous(), int(num_rows)
        n = self.num_rows
        s = self.sample[:, None].expand_as(self.table)
        t = self.table.to(torch.int64)
        ok = (s >= 0) & (s < n) & (t >= 0) & (t < n) & (t != s)
        rows = torch.stack((torch.where(ok, s, n), torch.where(ok, t, n)), dim=-1).reshape(-1)     # [2 M k], slot order
        order = torch.sort(rows, stable=True)[1]
        self.rev_slots = order.to(torch.int32).contiguous()
        counts = torch.bincount(rows, minlength=n + 1)[:n]
        self.rev_offsets = torch.cat((counts.new_zeros(1), torch.cumsum(counts, 0))).contiguous()   # [n + 1] int64


def identity_neighbours(means: Tensor, num_samples: int = 1000, k: int = 5, radius: float = 1.0, seed: int = 0) -> IdentityNeighbours:
    """``num_samples`` rows drawn without replacement by a generator seeded with ``seed``, and for each its k + 1 nearest
    Gaussians from the existing exact kNN (``meshmap._knn(means, means[sample], k + 1, radius)``): the sample itself is among
    them and is dropped by the table's own rule, which leaves the ``k`` nearest others.  The kNN marks a row invalid (-1) only
    when its NEAREST hit is beyond ``radius``, which the self hit never is, so entries further away than ``radius`` are set to
    -1 here from the distances the kNN returns: a sample with no other Gaussian within ``radius`` takes no part."""
    from .meshmap import _knn
    if means.dim() != 2 or means.shape[1] != 3:
        raise ValueError(f"identity_neighbours: means must be [N, 3], got {tuple(means.shape)}")
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_NEIGHBOURS - 1:
        raise ValueError(f"identity_neighbours: k must be an integer in 1..{MAX_NEIGHBOURS - 1}, got {k!r}")
    if not isinstance(num_samples, int) or isinstance(num_samples, bool) or num_samples < 1:
        raise ValueError(f"identity_neighbours: num_samples must be a positive integer, got {num_samples!r}")
    require_gpu(means)
    n = int(means.shape[0])
    if n < k + 1:
        raise ValueError(f"identity_neighbours: {n} Gaussians but k + 1 = {k + 1} neighbours asked for")
    g = torch.Generator().manual_seed(int(seed))
    sample = torch.randperm(n, generator=g)[:min(num_samples, n)].to(means.device)
    means = means.detach()
    idx, dist, _ = _knn(means, means[sample], k + 1, float(radius))
    return IdentityNeighbours(sample, idx.masked_fill(dist > float(radius), -1), n)


def _check_sizes(dim: int, classes: int, what: str) -> None:
    if not 1 <= int(dim) <= MAX_DIM:
        raise ValueError(f"{what}: the identity width must be 1..{MAX_DIM}, got {dim}")
    if not 1 <= int(classes) <= MAX_CLASSES:
        raise ValueError(f"{what}: the number of classes must be 1..{MAX_CLASSES}, got {classes}")


def _flat(classifier: Classifier, dim: int, what: str) -> Tuple[Tensor, Tensor]:
    if isinstance(classifier, IdentityField):
        w, b = classifier.flat()
    elif isinstance(classifier, (tuple, list)) and len(classifier) == 2:
        w, b = classifier
    else:
        raise ValueError(f"{what}: classifier must be an IdentityField or (weight [K, D], bias [K])")
    if w.dim() != 2 or b.dim() != 1 or b.shape[0] != w.shape[0]:
        raise ValueError(f"{what}: weight must be [K, D] and bias [K], got {tuple(w.shape)} and {tuple(b.shape)}")
    _check_sizes(w.shape[1], w.shape[0], what)
    if int(w.shape[1]) != int(dim):
        raise ValueError(f"{what}: vectors of width {dim} against a classifier of width {w.shape[1]}")
    if w.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError(f"{what}: classifier parameters must be float32, got {w.dtype} and {b.dtype}")
    return w, b


def _scratch(lib, rows: int, dim: int, classes: int, mode: int, dev, what: str) -> Tensor:
    n = int(lib.misplat_identity_scratch_floats(rows, dim, classes, mode))
    if n < 0:
        raise ValueError(f"{what}: sizes outside the kernels' limits ({rows} rows, width {dim}, {classes} classes)")
    return torch.empty(n, device=dev, dtype=torch.float32)


class _IdentityLoss(torch.autograd.Function):
    """The 2-D identity loss as ONE autograd node: two launches forward, three backward; the scratch holds one log-sum-exp per
    pixel and the weight gradient's partial sums per row split, never a [K, P] tensor."""

    @staticmethod
    def forward(ctx, features, stride, validate, weight, bias, target):
        lib = _lib.load()
        H, W, D = (int(v) for v in features.shape)
        K = int(weight.shape[0])
        dev = features.device
        weight, bias = weight.contiguous(), bias.contiguous()
        scratch = _scratch(lib, H * W, D, K, 0, dev, "identity_loss")
        counts = torch.empty(2, device=dev, dtype=torch.int32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        run("misplat_identity_loss_fwd", H, W, D, stride, C.c_void_p(features.data_ptr()), K, ptr(weight), ptr(bias),
            ptr(target), ptr(scratch), ptr(counts), ptr(loss))
        if validate:
            n_bad = int(counts.tolist()[1])                                   # the call's one host read
            if n_bad:
                raise ValueError(f"identity_loss: {n_bad} target pixels lie outside 0..{K}")
        ctx.save_for_backward(features, weight, bias, target, scratch, counts)
        ctx.meta = (H, W, D, K, int(stride))
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 6
        H, W, D, K, stride = ctx.meta
        features, weight, bias, target, scratch, counts = ctx.saved_tensors
        dev = weight.device
        g = g.to(torch.float32).contiguous()
        v_features = torch.empty(H, W, D, device=dev, dtype=torch.float32)
        v_w, v_b = torch.empty_like(weight), torch.empty_like(bias)
        run("misplat_identity_loss_bwd", H, W, D, stride, C.c_void_p(features.data_ptr()), K, ptr(weight), ptr(bias),
            ptr(target), ptr(scratch), ptr(counts), ptr(g), ptr(v_features), ptr(v_w), ptr(v_b))
        return v_features, None, None, v_w, v_b, None


def identity_loss(features: Tensor, classifier: Classifier, target: Tensor, validate: bool = True) -> Tensor:
    """Cross-entropy of the per-pixel classification of a rendered identity image, as a device scalar with gradients to
    ``features``, ``weight`` and ``bias``:

        z = W x + b,   ce = logsumexp(z) - z[t - 1],   loss = sum over labelled pixels of ce / max(n_labelled, 1)

    ``features`` [H, W, D] float32 on the GPU, D in 1..32 (a channel slice of a wider image is read in place); ``classifier`` an
    ``IdentityField`` or ``(weight [K, D], bias [K])``, K in 1..4096; ``target`` [H, W] int32 as
    ``grouping.convert_matched_mask`` returns it: 0 unlabelled, t in 1..K class t - 1.  This is
    ``F.cross_entropy(logits, target - 1, ignore_index=-1)`` except that an image without a labelled pixel gives exactly 0 and
    exact-zero gradients (torch: NaN).  ``validate=True`` reads (n_labelled, n_out_of_range) back once and raises ``ValueError``
    for a target outside 0..K; ``validate=False`` makes no host read and counts such pixels as unlabelled."""
    what = "identity_loss"
    feats, stride = _features_view(features, what)
    w, b = _flat(classifier, feats.shape[2], what)
    if target.dim() != 2 or tuple(target.shape) != tuple(feats.shape[:2]):
        raise ValueError(f"{what}: target must be [H, W] = {tuple(feats.shape[:2])}, got {tuple(target.shape)}")
    if target.dtype != torch.int32:
        raise ValueError(f"{what}: target must be int32, got {target.dtype}")
    require_gpu(feats, w, b, target)
    return _IdentityLoss.apply(feats, stride, bool(validate), w, b, target.contiguous())


@torch.no_grad()
def identity_labels(features: Tensor, classifier: Classifier, return_confidence: bool = False):
    """[H, W] int32: the argmax class + 1 of every pixel (ties: the smallest class index), the value range of
    ``convert_matched_mask``; with ``return_confidence`` also the fp32 largest softmax probability.  One fused launch, no
    logits tensor.  Rows work too: ``features`` [N, 1, D]."""
    what = "identity_labels"
    feats, stride = _features_view(features, what)
    w, b = _flat(classifier, feats.shape[2], what)
    require_gpu(feats, w, b)
    H, W, D = (int(v) for v in feats.shape)
    w, b = w.detach().contiguous(), b.detach().contiguous()
    labels = torch.empty(H, W, device=feats.device, dtype=torch.int32)
    conf = torch.empty(H, W, device=feats.device, dtype=torch.float32) if return_confidence else None
    run("misplat_identity_labels", H * W, D, stride, C.c_void_p(feats.data_ptr()), int(w.shape[0]), ptr(w), ptr(b), ptr(labels),
        ptr(conf))
    return (labels, conf) if return_confidence else labels


class _Identity3DLoss(torch.autograd.Function):
    """The 3-D consistency loss as ONE autograd node: two launches forward, four backward.  The identities' gradient is a dense
    [N, D] gathered through the reverse table (no ``index_add_``, no atomics)."""

    @staticmethod
    def forward(ctx, identities, weight, bias, nb):
        lib = _lib.load()
        N, D = (int(v) for v in identities.shape)
        K = int(weight.shape[0])
        M, k = (int(v) for v in nb.table.shape)
        dev = identities.device
        identities, weight, bias = identities.contiguous(), weight.contiguous(), bias.contiguous()
        scratch = _scratch(lib, M * k, D, K, 1, dev, "identity_3d_loss")
        counts = torch.empty(2, device=dev, dtype=torch.int32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        run("misplat_identity_3d_fwd", N, D, ptr(identities), K, ptr(weight), ptr(bias), M, k, ptr(nb.sample), ptr(nb.table),
            ptr(scratch), ptr(counts), ptr(loss))
        ctx.save_for_backward(identities, weight, bias, scratch, counts)
        ctx.nb = nb
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        identities, weight, bias, scratch, counts = ctx.saved_tensors
        nb = ctx.nb
        N, D = (int(v) for v in identities.shape)
        M, k = (int(v) for v in nb.table.shape)
        g = g.to(torch.float32).contiguous()
        v_e, v_w, v_b = torch.empty_like(identities), torch.empty_like(weight), torch.empty_like(bias)
        run("misplat_identity_3d_bwd", N, D, ptr(identities), int(weight.shape[0]), ptr(weight), ptr(bias), M, k,
            ptr(nb.sample), ptr(nb.table), ptr(nb.rev_offsets), ptr(nb.rev_slots), ptr(scratch), ptr(counts), ptr(g), ptr(v_e),
            ptr(v_w), ptr(v_b))
        return v_e, v_w, v_b, None


def identity_3d_loss(identities: Tensor, classifier: Classifier, neighbours: IdentityNeighbours) -> Tensor:
    """The 3-D regularisation of Gaussian Grouping as a device scalar with gradients to ``identities`` [N, D], ``weight`` and
    ``bias``: with p_j = softmax(W e_j + b) and exact log-softmax (no ``+ 1e-10``),

        loss = sum_j sum_{i valid} KL(p_sample_j || p_table_ji) / max(n_valid_pairs, 1)

    over the entries of ``neighbours.table`` that are neither -1 nor their own sample; no valid pair gives exactly 0."""
    what = "identity_3d_loss"
    if not isinstance(neighbours, IdentityNeighbours):
        raise ValueError(f"{what}: neighbours must be an IdentityNeighbours")
    if identities.dim() != 2:
        raise ValueError(f"{what}: identities must be [N, D], got {tuple(identities.shape)}")
    if identities.dtype != torch.float32:
        raise ValueError(f"{what}: identities must be float32, got {identities.dtype}")
    w, b = _flat(classifier, identities.shape[1], what)
    if int(identities.shape[0]) != neighbours.num_rows:
        raise ValueError(f"{what}: {identities.shape[0]} identity rows but the neighbours were built over {neighbours.num_rows}")
    require_gpu(identities, w, b, neighbours.sample)
    return _Identity3DLoss.apply(identities, w, b, neighbours)
