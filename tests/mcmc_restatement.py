"""numpy restatement of csrc/mcmc.hip: the hash schedule and the sampler in uint32 / uint64 / int64
(exact: the device must equal them bit for bit), the noise step and the relocation in fp64, with an fp32 variant of the float
parts that runs the same operations in the same order in ``np.float32`` (what the tolerance of the GPU tests is built on)."""
import math

import numpy as np

N_MAX = 51
NOISE_STREAM, SAMPLE_STREAM = 1, 2
ADD_STREAM = 0x5851F42D

_U = np.uint32


def mix32(seed, i, draw):
    """csrc/hashmix.h, elementwise over uint32 arrays."""
    with np.errstate(over="ignore"):
        seed, i, draw = (np.asarray(v).astype(_U) for v in (seed, i, draw))
        x = seed * _U(0x9E3779B1) + i * _U(0x85EBCA77) + draw * _U(0xC2B2AE3D) + _U(0x27D4EB2F)
        x ^= x >> _U(16); x = x * _U(0x85EBCA6B); x ^= x >> _U(13); x = x * _U(0xC2B2AE35); x ^= x >> _U(16)
        x = x + i
        x ^= x >> _U(15); x = x * _U(0x2C1B3C6D); x ^= x >> _U(12); x = x * _U(0x297A2D39); x ^= x >> _U(15)
    return x


def _key(seed: int, step: int, stream: int):
    return mix32(_U(seed & 0xFFFFFFFF), _U(step & 0xFFFFFFFF), _U(stream))


# ----------------------------------------------------------------------------------------------------------------- noise
def noise_words(seed: int, step: int, n: int) -> np.ndarray:
    """[n, 4] uint32: the four words of every Gaussian."""
    key = _key(seed, step, NOISE_STREAM)
    i = np.arange(n, dtype=np.uint32)
    return np.stack([mix32(key, i, _U(k)) for k in range(4)], axis=1)


def normals(words: np.ndarray, dtype=np.float64) -> np.ndarray:
    """[n, 3] standard normals by Box-Muller: uniforms ((w >> 8) + 1) 2^-24 in (0, 1] under the log, (w >> 8) 2^-24 in [0, 1) for
    the angle."""
    f = dtype
    u0 = ((words[:, 0] >> 8).astype(np.int64) + 1).astype(f) * f(2.0 ** -24)
    u1 = ((words[:, 2] >> 8).astype(np.int64) + 1).astype(f) * f(2.0 ** -24)
    a0 = f(2.0) * ((words[:, 1] >> 8).astype(f) * f(2.0 ** -24))
    a1 = f(2.0) * ((words[:, 3] >> 8).astype(f) * f(2.0 ** -24))
    r0 = np.sqrt(f(-2.0) * np.log(u0))
    r1 = np.sqrt(f(-2.0) * np.log(u1))
    pi = f(np.pi)
    return np.stack([r0 * np.cos(pi * a0), r0 * np.sin(pi * a0), r1 * np.cos(pi * a1)], axis=1).astype(f)


def gate(opacity_logits: np.ndarray, dtype=np.float64) -> np.ndarray:
    f = dtype
    with np.errstate(over="ignore"):
        o = f(1.0) / (f(1.0) + np.exp(-opacity_logits.astype(f)))
        return (f(1.0) / (f(1.0) + np.exp(f(-100.0) * ((f(1.0) - o) - f(0.995))))).astype(f)


def noise_displacement(opacity_logits, log_scales, quats, scaler: float, seed: int, step: int, dtype=np.float64) -> np.ndarray:
    """d [n, 3] = R diag(s^2) R^T (z g scaler), the kernel's operation order, in ``dtype``."""
    f = dtype
    n = log_scales.shape[0]
    z = normals(noise_words(seed, step, n), f)
    g = gate(np.asarray(opacity_logits).reshape(-1), f)
    s = np.exp(log_scales.astype(f))
    q = quats.astype(f)
    q = q * (f(1.0) / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]))[:, None]
    w, x, y, zz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = f(1.0), f(2.0)
    R = [[one - two * (y * y + zz * zz), two * (x * y - w * zz), two * (x * zz + w * y)],
         [two * (x * y + w * zz), one - two * (x * x + zz * zz), two * (y * zz - w * x)],
         [two * (x * zz - w * y), two * (y * zz + w * x), one - two * (x * x + y * y)]]
    t = g * f(scaler)
    v = [z[:, k] * t for k in range(3)]
    a = [(s[:, k] * s[:, k]) * ((R[0][k] * v[0] + R[1][k] * v[1]) + R[2][k] * v[2]) for k in range(3)]
    d = [(R[k][0] * a[0] + R[k][1] * a[1]) + R[k][2] * a[2] for k in range(3)]
    return np.stack(d, axis=1).astype(f)


# ---------------------------------------------------------------------------------------------------------------- sample
def weights(opacities: np.ndarray, min_opacity=None) -> np.ndarray:
    """int64 [n]: floor(min(o, 1) 2^24) in fp32 (exact), 0 for o <= 0, NaN and o <= min_opacity."""
    o = np.asarray(opacities, np.float32).reshape(-1)
    q = (np.minimum(np.nan_to_num(o, nan=0.0), np.float32(1.0)) * np.float32(16777216.0)).astype(np.int64)
    dead = ~(o > 0)
    if min_opacity is not None:
        dead |= o <= np.float32(min_opacity)
    q[dead] = 0
    return q


def sample(opacities: np.ndarray, m: int, seed: int, step: int, min_opacity=None):
    """(idx [m] int64, counts [n] int32), or None when every weight is zero."""
    q = weights(opacities, min_opacity)
    incl = np.cumsum(q, dtype=np.int64)
    total = int(incl[-1])
    if total == 0:
        return None
    key = _key(seed, step, SAMPLE_STREAM)
    j = np.arange(m, dtype=np.uint32)
    u = (mix32(key, j, _U(0)).astype(np.uint64) << np.uint64(32)) | mix32(key, j, _U(1)).astype(np.uint64)
    r = np.array([(int(v) * total) >> 64 for v in u], dtype=np.int64)
    idx = np.searchsorted(incl, r, side="right").astype(np.int64)          # the first i with incl[i] > r
    return idx, np.bincount(idx, minlength=q.shape[0]).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ relocation
def binomial_table(n_max: int = N_MAX) -> np.ndarray:
    t = np.zeros((n_max, n_max), np.float64)
    for i in range(n_max):
        for k in range(i + 1):
            t[i, k] = float(math.comb(i, k))
    return t


def relocation(opacities, scales, ratios, dtype=np.float64, n_max: int = N_MAX):
    """(o' [m], s' [m, 3]) in ``dtype``: o' = -expm1(log1p(-o) / n); D summed over i = 1..n, k = 0..i-1 in that order with the
    running power p <- p o'; s' = (o / D) s."""
    f = dtype
    o = np.asarray(opacities, np.float32).reshape(-1).astype(f)
    s = np.asarray(scales, np.float32).astype(f)
    n = np.clip(np.asarray(ratios).reshape(-1).astype(np.int64), 1, n_max)
    with np.errstate(divide="ignore"):
        op = (-np.expm1(np.log1p(-o) / n.astype(f))).astype(f)
    binoms = binomial_table(n_max)
    coef = np.array([[(-1.0) ** k for k in range(n_max)]]) * (binoms.astype(f) / np.sqrt(np.arange(1, n_max + 1, dtype=f))[None, :])
    coef = coef.astype(f)
    D = np.zeros_like(o)
    for i in range(1, int(n.max()) + 1):
        live = n >= i
        p = op.copy()
        for k in range(i):
            D = np.where(live, D + coef[i - 1, k] * p, D).astype(f)
            p = (p * op).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = np.where(o > 0, o / D, f(1.0)).astype(f)
    return op, (fac[:, None] * s).astype(f)


# ------------------------------------------------------------------------------------------------------------ the rule
def rel_err(got, oracle) -> float:
    """DESIGN.md section 21.4's metric: max |got - oracle| / max |oracle|."""
    got, oracle = np.asarray(got, np.float64), np.asarray(oracle, np.float64)
    return float(np.abs(got - oracle).max() / max(np.abs(oracle).max(), 1e-300))


def bound_from(fp32_err: float) -> float:
    """8 x the fp32 restatement's error on the same scene, floored at 2^-23 and capped at 1e-4 (section 21.4)."""
    return min(max(8.0 * fp32_err, 2.0 ** -23), 1e-4)
