"""Seeded scenes of the text-query tests.  Every value is drawn in float32 (so the fp64 oracle, the fp32 yardstick and the GPU
see the same numbers).  The decoder is at unit scale -- w ~ N(0, 1) / sqrt(fan_in), biases 0.1 N(0, 1) -- and the embeddings
have unit-norm rows, the positives first.  The shapes are the smallest at which the kernels can still go wrong."""
import functools

import torch
import torch.nn.functional as F

import textquery_restatement as R

# name: (render H, W), L, Hd, C, Q, n_pos, work (h, w), out (H, W)
SCENES = {
    "shrink": ((24, 40), 13, 64, 96, 5, 2, (16, 24), (24, 40)),      # shrinking resize, the final upsample, several of each kind
    "enlarge": ((9, 7), 13, 64, 768, 2, 1, (24, 40), (9, 7)),        # enlarging resize, wide C in the fold, the smallest Q
    "generic": ((12, 20), 5, 80, 33, 8, 3, (12, 20), (12, 20)),      # Hd != 64, odd C, identity resize, no upsample
    "ragged": ((5, 3), 1, 1, 1, 64, 63, (7, 11), (5, 3)),            # every limit's edge, a pixel count that fills no wave
    "saturated": ((8, 8), 13, 64, 16, 3, 1, (8, 8), (8, 8)),         # logits more than 200 apart: exact 0 / 1, no NaN
}
METHODS = ("standard", "pairwise")
ROWS_SCENE = "shrink"                                   # the row form runs on this scene's decoder and queries
ROW_COUNTS = (1, 63, 64, 1000)
SATURATED_BIAS = 40.0


@functools.lru_cache(maxsize=None)
def make(name: str):
    (H, W), L, Hd, C, Q, n_pos, work, out = SCENES[name]
    g = torch.Generator().manual_seed(2300 + sorted(SCENES).index(name))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)                 # noqa: E731
    features = rn(H, W, L)
    w_hidden, b_hidden = rn(Hd, L) / L ** 0.5, 0.1 * rn(Hd)
    w_out, b_out = rn(C, Hd) / Hd ** 0.5, 0.1 * rn(C)
    embeddings = F.normalize(rn(Q, C), dim=1)
    if name == "saturated":
        # embedding 0 (the positive one) lies along b_out, the others are orthogonal to it, and |b_out| = 40: c = (40, 0, 0)
        # up to rounding against products A hid of a few units, so the logits are some 600 apart at T = 0.05
        d = F.normalize(b_out, dim=0)
        rest = embeddings[1:] - (embeddings[1:] @ d)[:, None] * d
        embeddings = torch.cat([d[None], F.normalize(rest, dim=1)])
        b_out = SATURATED_BIAS * d
    return {"name": name, "features": features, "w_hidden": w_hidden, "b_hidden": b_hidden, "w_out": w_out, "b_out": b_out,
            "embeddings": embeddings, "n_pos": n_pos, "work": work, "out": out}


@functools.lru_cache(maxsize=None)
def saturated_negative():
    """``saturated`` with the aligned embedding among the negatives: every similarity is exactly 0."""
    sc = dict(make("saturated"))
    sc["embeddings"] = sc["embeddings"][[1, 0, 2]].contiguous()
    return sc


@functools.lru_cache(maxsize=None)
def row_latents():
    """[1000, 13]: the rows of the row-form tests; a test with N rows takes the first N."""
    return torch.randn(max(ROW_COUNTS), SCENES[ROWS_SCENE][1], generator=torch.Generator().manual_seed(2399), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def oracle(name: str, method: str, at_work: bool = False):
    """The fp64 restatement of a scene ([H_out, W_out, 1]; ``at_work``: before the final resize): computed once, shared by the
    tests, never written to."""
    return R.similarity_map(make(name), torch.float64, method, out_hw=None if at_work else "scene")


@functools.lru_cache(maxsize=None)
def yardstick(name: str, method: str, at_work: bool = False):
    """The fp32 restatement of the same scene."""
    return R.similarity_map(make(name), torch.float32, method, out_hw=None if at_work else "scene")


@functools.lru_cache(maxsize=None)
def row_oracle(method: str, dtype=torch.float64):
    """[1000]: the restatement on every row of ``row_latents`` (a row's value does not depend on the other rows)."""
    return R.row_similarity(make(ROWS_SCENE), row_latents(), dtype, method)


def abs_err(a: torch.Tensor, ref: torch.Tensor) -> float:
    """max |a - ref| over the whole tensor (the similarity lies in 0..1, so the measure is absolute); NaN counts as inf."""
    d = float((a.detach().double().cpu() - ref.detach().double().cpu()).abs().max())
    return d if d == d else float("inf")
