"""MCMC densification (csrc/mcmc.hip): the fixed-budget alternative to ``DefaultStrategy``.

"3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al. 2024): every ``refine_every`` steps the dead Gaussians
(opacity <= ``min_opacity``) are *relocated* onto alive ones sampled by opacity, the model *grows* by 5 % up to ``cap_max``, and
on every step the means receive noise shaped by each Gaussian's covariance and gated by its opacity.  gsplat's ``MCMCStrategy``
and ``relocation`` are absent from this machine: the operations are restated from the published method, with gsplat's
parameter names and defaults **[UNVERIFIED-UPSTREAM]**; parity with gsplat's code is unpinned.

The three kernels draw from the counter-based generator of csrc/hashmix.h, keyed by ``(seed, step)``: two replicas driven by
the same seed stay bit-identical, which torch's global RNG (``torch.randn``, ``torch.multinomial``) does not give under
view-sharded data parallelism -- and the sampler has no 2^24 limit on the number of rows.  There is no CPU fallback.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Dict, Optional, Tuple

import torch
from torch import Tensor

from ._lib import MisplatError, load, ptr, require_gpu, run
from .strategy import _update_param_with_optimizer

N_MAX = 51                      # MISPLAT_MCMC_N_MAX: the largest ratio of the relocation
_NOTHING = 1                    # MISPLAT_MCMC_NOTHING
_ADD_STREAM = 0x5851F42D        # sample_add's draws of a step use seed + this: not the draws of the step's relocation


class NothingToSample(MisplatError):
    """Every weight handed to ``sample_by_opacity`` is zero."""


def binomial_table(n_max: int = N_MAX, device=None) -> Tensor:
    """[n_max, n_max] float64, ``[i, k] = C(i, k)`` (0 for k > i): exact, C(50, 25) < 2^53."""
    t = torch.zeros(n_max, n_max, dtype=torch.float64)
    for i in range(n_max):
        for k in range(i + 1):
            t[i, k] = float(math.comb(i, k))
    return t if device is None else t.to(device)


def sample_by_opacity(opacities: Tensor, m: int, seed: int, step: int, min_opacity: Optional[float] = None) -> Tuple[Tensor, Tensor]:
    """``m`` draws with replacement from the rows of ``opacities`` ([N] float32, ACTIVATED, on the GPU), row i with probability
    proportional to ``floor(o_i 2^24)`` -- zero for ``o_i <= min_opacity`` when that is given.  Returns ``(idx [m] int64,
    counts [N] int32)``: the rows drawn and how often each was.  Exact integer work (int64 prefix sums, 64 random bits a draw,
    binary search): the same ``(seed, step)`` gives the same draws anywhere.  Raises ``NothingToSample`` when every weight is 0
    (one 4-byte host read)."""
    require_gpu(opacities)
    opacities = opacities.detach().reshape(-1)
    if opacities.dtype != torch.float32:
        raise MisplatError(f"sample_by_opacity: opacities must be float32, got {opacities.dtype}")
    opacities = opacities.contiguous()
    n, m = int(opacities.shape[0]), int(m)
    if n < 1 or m < 1:
        raise ValueError(f"sample_by_opacity: needs N >= 1 rows and m >= 1 draws, got N = {n}, m = {m}")
    lib = load()
    nbytes = int(lib.misplat_mcmc_sample_workspace_bytes(n))
    if nbytes < 0:
        raise MisplatError(f"sample_by_opacity: N = {n} out of range")
    dev = opacities.device
    work = torch.empty(nbytes // 8 + 1, device=dev, dtype=torch.int64)
    idx = torch.empty(m, device=dev, dtype=torch.int64)
    counts = torch.empty(n, device=dev, dtype=torch.int32)
    status = torch.empty(1, device=dev, dtype=torch.int32)
    run("misplat_mcmc_sample", n, ptr(opacities), min_opacity is not None, 0.0 if min_opacity is None else min_opacity, m, seed,
        step, ptr(work), work.numel() * 8, ptr(idx), ptr(counts), ptr(status))
    if int(status.item()) == _NOTHING:
        raise NothingToSample("sample_by_opacity: every weight is zero, nothing to sample")
    return idx, counts


def compute_relocation(opacities: Tensor, scales: Tensor, ratios: Tensor, binoms: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """The paper's Eq. 9: the opacity and scale of each of ``ratios`` copies that together look like one Gaussian of
    (``opacities`` [M], ``scales`` [M, 3]), both ACTIVATED.  ``ratios`` [M] integers, clamped to 1 .. ``binoms.shape[0]``
    (51 by default).  Returns ``(new_opacities [M], new_scales [M, 3])`` float32; the double sum runs in fp64."""
    require_gpu(opacities, scales, ratios)
    m = int(opacities.numel())
    if m < 1 or tuple(scales.shape) != (m, 3) or int(ratios.numel()) != m:
        raise ValueError(f"compute_relocation: opacities [M >= 1], scales [M, 3], ratios [M]; got {tuple(opacities.shape)}, "
                         f"{tuple(scales.shape)}, {tuple(ratios.shape)}")
    dev = opacities.device
    if binoms is None:
        binoms = binomial_table(N_MAX, dev)
    if binoms.dim() != 2 or binoms.shape[0] != binoms.shape[1]:
        raise ValueError(f"compute_relocation: binoms must be [n_max, n_max], got {tuple(binoms.shape)}")
    binoms = binoms.to(device=dev, dtype=torch.float64).contiguous()
    o = opacities.detach().reshape(-1).to(torch.float32).contiguous()
    s = scales.detach().to(torch.float32).contiguous()
    r = ratios.detach().reshape(-1).to(torch.int32).contiguous()
    new_o, new_s = torch.empty_like(o), torch.empty_like(s)
    run("misplat_mcmc_relocation", m, ptr(o), ptr(s), ptr(r), ptr(binoms), binoms.shape[0], ptr(new_o), ptr(new_s))
    return new_o.reshape(opacities.shape), new_s


@torch.no_grad()
def inject_noise_to_position(params, optimizers, state: Dict[str, Any], scaler: float, seed: int, step: int) -> None:
    """``means += Sigma (z g scaler)`` in place, one launch: ``Sigma`` each Gaussian's covariance, ``z`` standard normals of
    ``(seed, step, i)``, ``g`` the gate that switches the noise off for opaque Gaussians (``misplat_mcmc_noise``)."""
    means, opac, scales, quats = (params[k].data for k in ("means", "opacities", "scales", "quats"))
    require_gpu(means, opac, scales, quats)
    n = int(means.shape[0])
    if n == 0:
        return
    for name, t, shape in (("means", means, (n, 3)), ("scales", scales, (n, 3)), ("quats", quats, (n, 4))):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise MisplatError(f"inject_noise_to_position: {name} must be a contiguous float32 {shape}, got "
                               f"{tuple(t.shape)} {t.dtype}")
    if opac.numel() != n or opac.dtype != torch.float32 or not opac.is_contiguous():
        raise MisplatError(f"inject_noise_to_position: opacities must hold {n} contiguous float32 logits")
    run("misplat_mcmc_noise", n, ptr(means), ptr(opac), ptr(scales), ptr(quats), scaler, seed, step)


def _relocated_values(params, idx: Tensor, counts: Tensor, min_opacity: float, binoms) -> Tuple[Tensor, Tensor]:
    """(opacity logits, log scales) of the rows ``idx`` after each has been split into ``counts + 1`` copies."""
    opac = torch.sigmoid(params["opacities"].data.reshape(-1)[idx])
    new_o, new_s = compute_relocation(opac, torch.exp(params["scales"].data[idx]), counts[idx] + 1, binoms)
    new_o = torch.clamp(new_o, min=min_opacity, max=1.0 - torch.finfo(torch.float32).eps)
    return torch.logit(new_o), torch.log(new_s)


@torch.no_grad()
def relocate(params, optimizers, state: Dict[str, Any], mask: Tensor, min_opacity: float, seed: int, step: int) -> int:
    """The rows of ``mask`` (dead) take the parameters of rows sampled, by opacity, from the others; every sampled row and its
    copies get the relocated opacity and scale, and the sampled rows' Adam moments are zeroed.  Returns the number relocated
    (0, and nothing launched, when no row or every row is dead)."""
    dead = torch.where(mask)[0]
    n, n_dead = int(mask.shape[0]), int(dead.shape[0])
    if n_dead == 0 or n_dead == n:
        return 0
    weights = torch.sigmoid(params["opacities"].data.reshape(-1)).masked_fill_(mask, 0.0)
    try:
        idx, counts = sample_by_opacity(weights, n_dead, seed, step, min_opacity)
    except NothingToSample:
        return 0
    new_logit, new_log_scale = _relocated_values(params, idx, counts, min_opacity, state.get("binoms"))

    def param_fn(name: str, p: Tensor) -> Tensor:
        # duplicates in idx name the same source row and hence the same count: they all store the same value, so plain
        # indexed stores are deterministic
        if name == "opacities":
            p[idx] = new_logit.reshape((-1,) + tuple(p.shape[1:]))
        elif name == "scales":
            p[idx] = new_log_scale
        p[dead] = p[idx]
        return p

    def optimizer_fn(key: str, v: Tensor) -> Tensor:
        v[idx] = 0
        return v

    _update_param_with_optimizer(param_fn, optimizer_fn, params, optimizers)
    return n_dead


@torch.no_grad()
def sample_add(params, optimizers, state: Dict[str, Any], n: int, min_opacity: float, seed: int, step: int) -> int:
    """``n`` new rows: copies of rows sampled by opacity from all rows, source and copies with the relocated opacity and scale,
    appended with zero Adam moments.  Returns the number added."""
    n = int(n)
    if n <= 0 or int(params["means"].shape[0]) == 0:
        return 0
    try:
        idx, counts = sample_by_opacity(torch.sigmoid(params["opacities"].data.reshape(-1)), n, seed, step)
    except NothingToSample:
        return 0
    new_logit, new_log_scale = _relocated_values(params, idx, counts, min_opacity, state.get("binoms"))

    def param_fn(name: str, p: Tensor) -> Tensor:
        if name == "opacities":
            p[idx] = new_logit.reshape((-1,) + tuple(p.shape[1:]))      # (duplicates store the same value, as in relocate)
        elif name == "scales":
            p[idx] = new_log_scale
        return torch.cat([p, p[idx]])

    def optimizer_fn(key: str, v: Tensor) -> Tensor:
        return torch.cat([v, torch.zeros((n, *v.shape[1:]), device=v.device, dtype=v.dtype)])

    _update_param_with_optimizer(param_fn, optimizer_fn, params, optimizers)
    return n


@dataclass
class RelocationStrategy:
    """The MCMC controller; gsplat's ``MCMCStrategy`` parameter names and defaults [UNVERIFIED-UPSTREAM].  ``seed`` keys the
    counter-based generator: every rank that runs the same steps with the same seed draws the same samples and noise."""
    cap_max: int = 1_000_000
    noise_lr: float = 5e5
    refine_start_iter: int = 500
    refine_stop_iter: int = 25_000
    refine_every: int = 100
    min_opacity: float = 0.005
    verbose: bool = False
    seed: int = 0

    def initialize_state(self) -> Dict[str, Any]:
        return {"binoms": binomial_table(N_MAX)}

    def check_sanity(self, params, optimizers) -> None:
        for key in ("means", "scales", "quats", "opacities"):
            assert key in params, f"{key} is required in params but missing."
        for key in optimizers:
            assert key in params, f"optimizer {key} has no parameter"

    def step_pre_backward(self, params, optimizers, state: Dict[str, Any], step: int, info: Dict[str, Any]) -> None:
        """Nothing to retain: this controller reads no gradient."""

    def step_post_backward(self, params, optimizers, state: Dict[str, Any], step: int, info: Dict[str, Any],
                           lr: float) -> Tuple[int, int]:
        """Returns (n_relocated, n_added) of this call.  ``lr``: the means group's current learning rate."""
        dev = params["means"].device
        if state["binoms"].device != dev:
            state["binoms"] = state["binoms"].to(dev)
        n_relocated = n_added = 0
        if self.refine_start_iter < step < self.refine_stop_iter and step % self.refine_every == 0:
            n_relocated = self._relocate_gs(params, optimizers, state, step)
            n_added = self._add_new_gs(params, optimizers, state, step)
            if self.verbose:
                print(f"Step {step}: {n_relocated} relocated, {n_added} added; now {len(params['means'])} Gaussians")
        inject_noise_to_position(params, optimizers, state, scaler=lr * self.noise_lr, seed=self.seed, step=step)
        return n_relocated, n_added

    @torch.no_grad()
    def _relocate_gs(self, params, optimizers, state: Dict[str, Any], step: int) -> int:
        dead = torch.sigmoid(params["opacities"].data.reshape(-1)) <= self.min_opacity
        return relocate(params, optimizers, state, dead, self.min_opacity, self.seed, step)

    @torch.no_grad()
    def _add_new_gs(self, params, optimizers, state: Dict[str, Any], step: int) -> int:
        n = int(params["means"].shape[0])
        n_new = max(0, min(int(self.cap_max), int(1.05 * n)) - n)
        return sample_add(params, optimizers, state, n_new, self.min_opacity, int(self.seed) + _ADD_STREAM, step)
