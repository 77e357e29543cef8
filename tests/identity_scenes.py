"""Seeded scenes of the identity tests.  Every value is drawn in float32, so the fp64 oracle, the fp32 yardstick and the GPU see
the same numbers.  After the draw, every pixel whose top-two logit margin (fp64) is below ``MARGIN`` times the scene's largest
|logit| is drawn again until none is left: the argmax of ``identity_labels`` can then be asked for at EVERY pixel
(tests/test_identity_host.py asserts the margin on the CPU).  ``tie`` is the one scene with an exact tie.

The kernels walk the classes in units of 16 (csrc/identity.hip ``kUnit``), hold the row in 16 or 32 registers (exactly full, or
guarded), and split the weight gradient's rows over ``PS = min(tiles of 256 rows, clamp(512 / class units, 8, 64))`` workgroups
per class unit; ``LAUNCH`` names the regime each scene is there for and the host test asserts it from the formula."""
import functools

import torch

import identity_restatement as R

MARGIN = 1e-3

# name: (H, W), D, K, share of unlabelled pixels, seed
SCENES = {
    "d1": ((7, 9), 1, 5, 0.3, 3001),
    "d16_k16": ((33, 67), 16, 16, 0.3, 3002),            # the full 16-register path; K = one class unit exactly; W % 64 != 0
    "k17": ((20, 30), 16, 17, 0.3, 3003),                # a second class unit of one class
    "d32": ((19, 21), 32, 40, 0.3, 3004),                # the full 32-register path, a ragged third unit
    "d13": ((10, 10), 13, 33, 0.5, 3005),                # guarded, 16 registers
    "d20": ((10, 12), 20, 3, 0.2, 3006),                 # guarded, 32 registers
    "k1": ((9, 11), 16, 1, 0.3, 3007),
    "k2": ((9, 11), 5, 2, 0.3, 3008),
    "one_pixel": ((1, 1), 16, 7, 0.0, 3009),
    "unlabelled": ((12, 13), 16, 6, 1.0, 3010),          # no labelled pixel at all
    "k15": ((6, 50), 16, 15, 0.3, 3011),                 # one class short of a unit
}
# the launch regimes of the weight gradient; the last column of LAUNCH: (tiles, PS)
LAUNCH_SCENES = {
    "splits_2": ((16, 20), 16, 20, 0.3, 3021),           # 2 tiles, the second ragged; PS = tiles
    "cap_64": ((130, 127), 16, 3, 0.6, 3022),            # 65 tiles over the cap of 64: split 0 walks two tiles
    "cap_mid": ((84, 80), 32, 300, 0.3, 3023),           # 19 class units: cap 26, 27 tiles
    "cap_8": ((42, 50), 2, 1040, 0.3, 3024),             # 65 class units: the cap's floor of 8, 9 tiles (K beyond the other scenes': the
                                                         # floor is reached by no smaller K)
}
LAUNCH = {"splits_2": (2, 2), "cap_64": (65, 64), "cap_mid": (27, 26), "cap_8": (9, 8)}
ALL_SCENES = {**SCENES, **LAUNCH_SCENES}
MISSING_CLASS = 5                                        # 1-based target value no pixel of "d16_k16" carries

# 3-D scenes: N rows, D, K, M samples, k, seed
SCENES_3D = {
    "k1": (50, 16, 6, 10, 1, 3101),
    "k16": (300, 16, 20, 40, 16, 3102),                  # -1 entries and self entries among the 16
    "m1": (30, 13, 17, 1, 5, 3103),
    "shared": (12, 32, 17, 4, 3, 3104),                  # row 0 is a sample and the neighbour of the three other samples
    "d1": (40, 1, 2, 7, 4, 3105),
    "big": (5000, 16, 256, 1000, 6, 3106),               # 12 000 rows of the weight gradient: 47 tiles over the cap of 32
}


def plan(rows: int, K: int):
    """(tiles, PS) as csrc/identity.hip ``make_plan`` derives them."""
    tiles = (rows + 255) // 256
    units = (K + 15) // 16
    cap = min(max(512 // units, 8), 64)
    return tiles, min(tiles, cap)


@functools.lru_cache(maxsize=None)
def make(name: str):
    if name == "tie":
        return _tie()
    (H, W), D, K, unl, seed = ALL_SCENES[name]
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)                 # noqa: E731
    features = rn(H, W, D)
    weight, bias = 2.0 * rn(K, D) / D ** 0.5, 0.3 * rn(K)
    for _ in range(200):
        _, _, margin, top = R.labels(features.double(), weight.double(), bias.double())
        low = margin < 2.0 * MARGIN * top
        if not bool(low.any()):
            break
        features[low] = rn(int(low.sum()), D)
    target = torch.randint(1, K + 1, (H, W), generator=g).to(torch.int32)
    target[torch.rand(H, W, generator=g) < unl] = 0
    if name == "d16_k16":
        target[target == MISSING_CLASS] = MISSING_CLASS + 1
    return {"name": name, "features": features, "weight": weight, "bias": bias, "target": target}


def _tie():
    """Classes 3 and 7 share a row and a bias and win everywhere: an exact tie in any arithmetic; the answer is class 3."""
    g = torch.Generator().manual_seed(3050)
    weight, bias = torch.randn(9, 4, generator=g), torch.zeros(9)
    weight[7] = weight[3]
    features = (4.0 + torch.rand(6, 11, 1, generator=g)) * weight[3] / float(weight[3] @ weight[3])
    target = torch.randint(0, 10, (6, 11), generator=g).to(torch.int32)
    return {"name": "tie", "features": features.contiguous(), "weight": weight, "bias": bias, "target": target}


@functools.lru_cache(maxsize=None)
def make_3d(name: str):
    N, D, K, M, k, seed = SCENES_3D[name]
    g = torch.Generator().manual_seed(seed)
    identities = torch.randn(N, D, generator=g)
    weight, bias = 1.5 * torch.randn(K, D, generator=g) / D ** 0.5, 0.3 * torch.randn(K, generator=g)
    sample = torch.randperm(N, generator=g)[:M]
    table = torch.randint(0, N, (M, k), generator=g).to(torch.int32)
    if name == "k16":
        table[torch.rand(M, k, generator=g) < 0.2] = -1
        table[::3, 5] = sample[::3].to(torch.int32)                                    # self entries
        table[7] = -1                                                                  # a sample without any neighbour
    if name == "shared":
        sample = torch.tensor([0, 5, 7, 9])
        table = torch.tensor([[5, 7, 3], [0, 2, 7], [0, 5, -1], [4, 0, 0]], dtype=torch.int32)
    return {"name": name, "identities": identities, "weight": weight, "bias": bias, "sample": sample, "table": table}


def _run(sc, dtype):
    return R.loss_2d(sc["features"].to(dtype), sc["weight"].to(dtype), sc["bias"].to(dtype), sc["target"])


def _run_3d(sc, dtype):
    return R.loss_3d(sc["identities"].to(dtype), sc["weight"].to(dtype), sc["bias"].to(dtype), sc["sample"], sc["table"])


@functools.lru_cache(maxsize=None)
def oracle(name: str):
    """The fp64 restatement of a scene: computed once, shared by the tests, never written to."""
    return _run(make(name), torch.float64)


@functools.lru_cache(maxsize=None)
def yardstick(name: str):
    return _run(make(name), torch.float32)


@functools.lru_cache(maxsize=None)
def oracle_3d(name: str):
    return _run_3d(make_3d(name), torch.float64)


@functools.lru_cache(maxsize=None)
def yardstick_3d(name: str):
    return _run_3d(make_3d(name), torch.float32)


@functools.lru_cache(maxsize=None)
def oracle_labels(name: str, dtype=torch.float64):
    sc = make(name)
    return R.labels(sc["features"].to(dtype), sc["weight"].to(dtype), sc["bias"].to(dtype))


def rel_err(a: torch.Tensor, ref: torch.Tensor) -> float:
    """max |a - ref| / max |ref| over the whole tensor (0 where both are all zero; inf where only the reference is)."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    diff, top = float((a - ref).abs().max()), float(ref.abs().max())
    if not (diff == diff):
        return float("inf")
    if top == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / top
