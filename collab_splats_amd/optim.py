"""Fused multi-tensor Adam (HIP) for the Gaussian parameter groups -- SURVEY.md section 8(f) rank 3.

The reference trains with one ``torch.optim.Adam`` per parameter group (nerfstudio ``AdamOptimizerConfig``,
``/root/reference/collab_splats/configs/rade_gs_method.py:44-71``: lr per group, ``eps=1e-15``).  ``FusedAdam``
keeps that interface (``param_groups``, ``state[p]["exp_avg"|"exp_avg_sq"|"step"]``, so the densification
strategy's optimizer-state surgery works unchanged) and ``step_all`` updates every group of every optimizer in
ONE kernel launch (``misplat_adam_step``) instead of ~6 x 5 elementwise kernels.

``SelectiveAdam`` is the same optimizer stepped under a row mask (the Gaussians visible in the step's views,
``visibility_from_radii``): ``selective_step_all`` lists the flagged rows on the device and ``misplat_adam_step_rows`` steps
those rows only -- DESIGN.md section 37.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Tuple

import torch

from . import _lib
from ._lib import run

MAX_TENSORS = 8                                  # MISPLAT_ADAM_MAX_TENSORS


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` semantics (no weight decay, no amsgrad, maximize=False), fp32 CUDA parameters."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps))

    def _entries(self) -> List[tuple]:
        out = []
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.dtype != torch.float32 or not p.is_cuda:
                    raise _lib.MisplatError("FusedAdam: parameters must be float32 tensors on the GPU (no CPU fallback)")
                if p.grad.is_sparse:
                    raise _lib.MisplatError("FusedAdam: sparse gradients are not supported")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                out.append((p, st, float(group["lr"]), float(b1), float(b2), float(group["eps"])))
        return out

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        _launch(self._entries())
        return loss


@torch.no_grad()
def step_all(optimizers: Iterable[FusedAdam] | Dict[str, FusedAdam]) -> None:
    """One fused launch (per distinct (betas, eps)) over all parameters of several ``FusedAdam`` instances."""
    if isinstance(optimizers, dict):
        optimizers = optimizers.values()
    entries: List[tuple] = []
    for opt in optimizers:
        if not isinstance(opt, FusedAdam):
            raise TypeError("step_all() takes FusedAdam optimizers")
        entries += opt._entries()
    _launch(entries)


def _launch(entries: List[tuple]) -> None:
    if not entries:
        return
    by_hyper: Dict[tuple, List[tuple]] = {}
    for e in entries:
        by_hyper.setdefault(e[3:], []).append(e)
    for (b1, b2, eps), es in by_hyper.items():
        for i in range(0, len(es), MAX_TENSORS):
            chunk = es[i:i + MAX_TENSORS]
            n = len(chunk)
            ps, gs, ms, vs, numel, lrs, steps = [], [], [], [], [], [], []
            keep = []                                    # contiguous gradient copies must outlive the launch
            for p, st, lr, _, _, _ in chunk:
                if not p.is_contiguous() or not st["exp_avg"].is_contiguous() or not st["exp_avg_sq"].is_contiguous():
                    raise _lib.MisplatError("FusedAdam: parameters and their moments must be contiguous")
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                if g.dtype != torch.float32 or g.shape != p.shape:
                    raise _lib.MisplatError("FusedAdam: gradient must be float32 with the parameter's shape")
                keep.append(g)
                ps.append(p.data_ptr()); gs.append(g.data_ptr())
                ms.append(st["exp_avg"].data_ptr()); vs.append(st["exp_avg_sq"].data_ptr())
                numel.append(p.numel()); lrs.append(lr); steps.append(int(st["step"].item()) + 1)
            vp = C.c_void_p * n
            run("misplat_adam_step", n, vp(*ps), vp(*gs), vp(*ms), vp(*vs), (C.c_int64 * n)(*numel), (C.c_float * n)(*lrs),
                (C.c_int64 * n)(*steps), b1, b2, eps)
            for _, st, _, _, _, _ in chunk:              # a refused launch has stepped nothing: the counts stay too
                st["step"] += 1
            del keep


# ---- row-selective Adam: only the Gaussians visible in the step's views are stepped ----------------------------------------

class SelectiveAdam(FusedAdam):
    """A ``FusedAdam`` (same hyper-parameters, same ``state`` layout, so the densification strategies edit it unchanged) whose
    ``step`` takes a row mask: ``visibility`` is a bool or uint8 GPU tensor ``[N]`` and every parameter that has a gradient
    has ``shape[0] == N``.  Rows with flag 1 get the bits ``FusedAdam`` gives them; rows with flag 0 keep the parameter,
    ``exp_avg`` and ``exp_avg_sq`` bit for bit.  ``state["step"]`` advances by one for every parameter that has a gradient,
    whatever the mask, and the bias correction uses that count (the convention of ``torch.optim.SparseAdam``).  gsplat
    users know the idea as ``SelectiveAdam`` / ``visible_adam``; parity with its kernel is unpinned.
    Data-parallel replicas must pass the same mask to stay identical."""

    @torch.no_grad()
    def step(self, visibility, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        _launch_rows(self._entries(), visibility)
        return loss


@torch.no_grad()
def selective_step_all(optimizers: Iterable[SelectiveAdam] | Dict[str, SelectiveAdam], visibility: torch.Tensor) -> None:
    """Step all parameters of several ``SelectiveAdam`` instances under one row mask: the id list is built once, then one row
    launch per distinct (betas, eps) and per chunk of 8 tensors."""
    if isinstance(optimizers, dict):
        optimizers = optimizers.values()
    entries: List[tuple] = []
    for opt in optimizers:
        if not isinstance(opt, SelectiveAdam):
            raise TypeError("selective_step_all() takes SelectiveAdam optimizers")
        entries += opt._entries()
    _launch_rows(entries, visibility)


@torch.no_grad()
def visibility_from_radii(radii: torch.Tensor) -> torch.Tensor:
    """uint8 ``[N]`` from the projection's ``info["radii"]`` (int32 ``[C, N, 2]``): 1 where both radii are positive for some
    camera, i.e. ``(radii > 0).all(-1).any(0)``."""
    if not isinstance(radii, torch.Tensor) or not radii.is_cuda:
        raise _lib.MisplatError("visibility_from_radii: radii must be a tensor on the GPU (no CPU fallback)")
    if radii.dtype != torch.int32 or radii.dim() != 3 or radii.shape[0] < 1 or radii.shape[2] != 2:
        raise _lib.MisplatError("visibility_from_radii: radii must be int32 [C, N, 2] with C >= 1")
    radii = radii.contiguous()
    n = radii.shape[1]
    flags = torch.empty(n, device=radii.device, dtype=torch.uint8)
    with torch.cuda.device(radii.device):
        run("misplat_visible_rows", _lib.ptr(radii), radii.shape[0], n, _lib.ptr(flags))
    return flags


_row_ws: Dict[torch.device, dict] = {}                   # the row list's work arrays, one set per device, kept from step to step


def _row_list(visibility: torch.Tensor):
    """(ids, count): the ascending ids of the flagged rows in an int32 list of capacity N and their number, which stays on the
    device.  Four small launches over work arrays that live from step to step (as ``parallel.GradientBuckets._ws``)."""
    n, dev = visibility.numel(), visibility.device
    nbytes = (n + 7) // 8
    n_blocks = (nbytes + 255) // 256
    ws = _row_ws.get(dev)
    if ws is None or ws["n"] != n:
        ws = _row_ws[dev] = dict(n=n, flags=torch.empty(n, device=dev, dtype=torch.uint8),
                                 bits=torch.empty(nbytes, device=dev, dtype=torch.uint8),
                                 counts=torch.empty(n_blocks, device=dev, dtype=torch.int32),
                                 offs=torch.empty(n_blocks, device=dev, dtype=torch.int64),
                                 total=torch.empty(1, device=dev, dtype=torch.int64),
                                 ids=torch.empty(n, device=dev, dtype=torch.int32))
    flags = visibility
    if not flags.is_contiguous() or flags.data_ptr() % 8:   # (misplat_touched_bits reads 8 flags at a time)
        flags = ws["flags"].copy_(visibility)
    run("misplat_touched_bits", C.c_void_p(flags.data_ptr()), n, _lib.ptr(ws["bits"]))
    run("misplat_union_count", _lib.ptr(ws["bits"]), 1, nbytes, _lib.ptr(ws["counts"]))
    run("misplat_union_scan", _lib.ptr(ws["counts"]), n_blocks, _lib.ptr(ws["offs"]), _lib.ptr(ws["total"]))
    run("misplat_union_ids", _lib.ptr(ws["bits"]), 1, nbytes, _lib.ptr(ws["offs"]), _lib.ptr(ws["ids"]), n)
    return ws["ids"], ws["total"]


def _launch_rows(entries: List[tuple], visibility) -> None:
    # everything is checked before anything is launched: a refused step moves neither a row nor a step count
    if not isinstance(visibility, torch.Tensor) or not visibility.is_cuda:
        raise _lib.MisplatError("SelectiveAdam: visibility must be a tensor on the GPU (no CPU fallback)")
    if visibility.dtype not in (torch.bool, torch.uint8) or visibility.dim() != 1:
        raise _lib.MisplatError("SelectiveAdam: visibility must be a bool or uint8 tensor [N]")
    if not entries:
        return
    n = visibility.numel()
    grads = []
    for p, st, _, _, _, _ in entries:
        if p.dim() < 1 or p.shape[0] != n:
            raise _lib.MisplatError(f"SelectiveAdam: a parameter of shape {tuple(p.shape)} under a mask of {n} rows")
        if p.device != visibility.device:
            raise _lib.MisplatError("SelectiveAdam: parameters and visibility must be on the same device")
        if not p.is_contiguous() or not st["exp_avg"].is_contiguous() or not st["exp_avg_sq"].is_contiguous():
            raise _lib.MisplatError("SelectiveAdam: parameters and their moments must be contiguous")
        if st["exp_avg"].shape != p.shape or st["exp_avg_sq"].shape != p.shape:
            raise _lib.MisplatError("SelectiveAdam: the moments must have the parameter's shape")
        if p.grad.dtype != torch.float32 or p.grad.shape != p.shape:
            raise _lib.MisplatError("SelectiveAdam: gradient must be float32 with the parameter's shape")
        grads.append(p.grad if p.grad.is_contiguous() else p.grad.contiguous())   # (the copies outlive the launches)
    by_hyper: Dict[tuple, List[tuple]] = {}
    for e, g in zip(entries, grads):
        if e[0].numel():
            by_hyper.setdefault(e[3:], []).append(e + (g,))
        else:                                            # (a tensor of no elements has nothing to step but its count)
            e[1]["step"] += 1
    with torch.cuda.device(visibility.device):
        if by_hyper:
            ids, count = _row_list(visibility)
        for (b1, b2, eps), es in by_hyper.items():
            for i in range(0, len(es), MAX_TENSORS):
                chunk = es[i:i + MAX_TENSORS]
                k = len(chunk)
                vp = C.c_void_p * k
                run("misplat_adam_step_rows", k, vp(*[e[0].data_ptr() for e in chunk]), vp(*[e[6].data_ptr() for e in chunk]),
                    vp(*[e[1]["exp_avg"].data_ptr() for e in chunk]), vp(*[e[1]["exp_avg_sq"].data_ptr() for e in chunk]),
                    (C.c_int32 * k)(*[e[0].numel() // n for e in chunk]), n, (C.c_float * k)(*[e[2] for e in chunk]),
                    (C.c_int64 * k)(*[int(e[1]["step"].item()) + 1 for e in chunk]), b1, b2, eps, _lib.ptr(ids), n,
                    _lib.ptr(count))
                for e in chunk:                          # (whatever the mask holds: the count is the step's, not the row's)
                    e[1]["step"] += 1
