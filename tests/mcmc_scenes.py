"""Scenes of the MCMC densification tests (tests/test_mcmc_host.py, tests/test_mcmc_gpu.py): inputs and, computed once and
shared, their restatements (tests/mcmc_restatement.py).  Everything is numpy; nothing here touches the GPU."""
import ctypes as C
import functools
import os
import re

import numpy as np

import mcmc_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "collab_splats_amd", "csrc")
MIN_OPACITY = 0.005


def _constant(header: str, name: str) -> int:
    text = open(os.path.join(CSRC, header)).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))


def scan_block() -> int:
    """Rows one workgroup scans (wgprims.h): the span of the sampler's first scan level."""
    return _constant("wgprims.h", "kScanBlock")


def stream_span() -> int:
    """Rows the noise kernel's capped grid covers in one trip: more need the grid-stride loop."""
    return _constant("mcmc.hip", "kThreads") * _constant("mcmc.hip", "kMaxBlocks")


def scan_level(n: int) -> int:
    """1: one workgroup's block; 2: several blocks, their totals in one trip of the carry scan; 3: the totals need a second
    trip (more than ``scan_block()`` blocks)."""
    b = scan_block()
    return 1 if n <= b else (2 if n <= b * b else 3)


# ---------------------------------------------------------------------------------------------------------------- sample
def sample_sizes():
    b = scan_block()
    return [1, 63, 64, 65, b - 1, b, b + 1, b * b + 1]


SAMPLE_DRAWS = [1, 65, 3000]


@functools.lru_cache(maxsize=None)
def sample_opacities(n: int) -> np.ndarray:
    """Activated opacities with exact zeros and rows at or below MIN_OPACITY: a dead prefix, a dead suffix and interior dead
    runs (where n has room for them); the rest uniform in (MIN_OPACITY, 1], a few exactly 1."""
    rng = np.random.default_rng(1000 + n)
    o = rng.uniform(0.01, 1.0, n).astype(np.float32)
    if n >= 63:
        low = rng.uniform(0.0, MIN_OPACITY, n).astype(np.float32)
        run = max(n // 16, 3)
        for a in (0, n - run, n // 3, (2 * n) // 3):                       # prefix, suffix, two interior runs
            o[a:a + run] = low[a:a + run]
        o[n // 2] = np.float32(MIN_OPACITY)                               # exactly the threshold: dead (<=)
        o[rng.integers(0, n, max(n // 20, 2))] = 0.0                      # exact zeros, scattered
        o[n // 5] = 0.0
        o[n // 4] = 1.0
    return o


@functools.lru_cache(maxsize=None)
def sample_restated(n: int, m: int, seed: int, step: int, thresholded: bool):
    return R.sample(sample_opacities(n), m, seed, step, MIN_OPACITY if thresholded else None)


# ------------------------------------------------------------------------------------------------------------ relocation
RELOC_OPACITIES = [0.005, 0.1, 0.5, 0.9, 0.99]
RELOC_NEAR_ONE = 1.0 - 2.0 ** -20
RELOC_RATIOS = [1, 2, 3, 7, 51, 200]
_DECADES = [1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3]                          # six decades


@functools.lru_cache(maxsize=None)
def relocation_scene(name: str):
    """``grid``: every (o, n) of RELOC_OPACITIES x RELOC_RATIOS; ``near_one``: o = 1 - 2^-20 with every n -- the rows that need
    the fp64 sum.  Each (o, n) comes with anisotropic scales from six decades, rotated through the axes."""
    opac = RELOC_OPACITIES if name == "grid" else [RELOC_NEAR_ONE]
    rng = np.random.default_rng(7 if name == "grid" else 8)
    o, n, s = [], [], []
    for oi in opac:
        for ni in RELOC_RATIOS:
            for r in range(len(_DECADES)):
                o.append(oi)
                n.append(ni)
                s.append([_DECADES[r] * rng.uniform(1, 9), _DECADES[(r + 2) % 7] * rng.uniform(1, 9),
                          _DECADES[(r + 4) % 7] * rng.uniform(1, 9)])
    return np.array(o, np.float32), np.array(s, np.float32), np.array(n, np.int32)


@functools.lru_cache(maxsize=None)
def relocation_restated(name: str, fp32: bool):
    return R.relocation(*relocation_scene(name), dtype=np.float32 if fp32 else np.float64)


# ----------------------------------------------------------------------------------------------------------------- noise
def noise_sizes():
    return [1, 64, 65, 257, stream_span() + 77]


NOISE_SCALER = 80.0                                                        # lr 1.6e-4 x noise_lr 5e5


@functools.lru_cache(maxsize=None)
def noise_scene(n: int):
    """(opacity logits [n, 1], log scales [n, 3], quats [n, 4]): logits around the gate's threshold and far from it, +-30 among
    them; scales over six decades; quaternions of lengths 1e-2 .. 1e2."""
    rng = np.random.default_rng(2000 + n)
    logits = (rng.normal(-5.3, 1.5, n)).astype(np.float32)                 # sigmoid(-5.3) = 0.005: the gate's half point
    logits[::7] = rng.normal(0.0, 3.0, len(logits[::7])).astype(np.float32)
    if n >= 64:
        logits[3], logits[11], logits[40], logits[41] = 30.0, -30.0, 30.0, -30.0
    log_scales = rng.uniform(np.log(1e-3), np.log(1e3), (n, 3)).astype(np.float32)
    quats = (rng.normal(size=(n, 4)) * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)
    return logits.reshape(n, 1), log_scales, quats


@functools.lru_cache(maxsize=None)
def noise_restated(n: int, seed: int, step: int, fp32: bool):
    return R.noise_displacement(*noise_scene(n), NOISE_SCALER, seed, step, np.float32 if fp32 else np.float64)


# -------------------------------------------------------------------------------------------------------------- strategy
@functools.lru_cache(maxsize=None)
def toy_model(n: int = 300, seed: int = 5):
    """Parameters of a toy model: about a third of the rows dead, their opacities far below MIN_OPACITY (sigmoid(-8) = 3e-4)
    and the others far above (at least sigmoid(-2) = 0.12), so no activation's last bit decides who is dead."""
    rng = np.random.default_rng(seed)
    dead = rng.uniform(size=n) < 1.0 / 3.0
    logits = np.where(dead, -8.0, rng.uniform(-2.0, 3.0, n)).astype(np.float32)
    return {"means": rng.normal(size=(n, 3)).astype(np.float32),
            "scales": rng.uniform(np.log(0.01), np.log(0.3), (n, 3)).astype(np.float32),
            "quats": rng.normal(size=(n, 4)).astype(np.float32),
            "opacities": logits.reshape(n, 1),
            "features_dc": rng.normal(size=(n, 1, 3)).astype(np.float32)}, dead


# ----------------------------------------------------------------------------------------------------------------- C ABI
def abi_bad_calls(lib):
    """(label, status) of calls that must be refused before anything is launched: the pointers are made up and never read."""
    p, null = C.c_void_p(0x1000), C.c_void_p(0)
    i64, i32, f32, u32 = C.c_int64, C.c_int32, C.c_float, C.c_uint32
    out = []

    def noise(n=8, means=p, opac=p, scales=p, quats=p):
        return lib.misplat_mcmc_noise(i64(n), means, opac, scales, quats, f32(1.0), u32(0), u32(0), null)

    def sample(n=8, m=4, opac=p, work=p, idx=p, status=p, nbytes=1 << 20):
        return lib.misplat_mcmc_sample(i64(n), opac, i32(0), f32(0.0), i64(m), u32(0), u32(0), work, i64(nbytes), idx, p, status, null)

    def reloc(m=8, n_max=51, opac=p, scales=p, ratios=p, binoms=p, new_o=p, new_s=p):
        return lib.misplat_mcmc_relocation(i64(m), opac, scales, ratios, binoms, i32(n_max), new_o, new_s, null)

    out += [("noise n < 0", noise(n=-1)), ("noise n = 0", noise(n=0))]
    out += [(f"noise null {k}", noise(**{k: null})) for k in ("means", "opac", "scales", "quats")]
    out += [("sample n < 0", sample(n=-1)), ("sample m < 0", sample(m=-1)), ("sample m = 0", sample(m=0)),
            ("sample workspace too small", sample(nbytes=8))]
    out += [(f"sample null {k}", sample(**{k: null})) for k in ("opac", "work", "idx", "status")]
    out += [("relocation m < 0", reloc(m=-1)), ("relocation n_max = 52", reloc(n_max=52)), ("relocation n_max = 0", reloc(n_max=0))]
    out += [(f"relocation null {k}", reloc(**{k: null})) for k in ("opac", "scales", "ratios", "binoms", "new_o", "new_s")]
    out.append(("workspace n < 0", int(lib.misplat_mcmc_sample_workspace_bytes(i64(-1)))))
    return out
