"""Restatement of the text-query similarity map, in the reference's own order of operations, in torch on the CPU at a chosen
dtype.  The fp64 run is the oracle of the GPU tests; the fp32 run is their yardstick for rounding.  Nothing here is folded: the
decoded features [C, h, w] exist, as they do in the reference.

    1. x = F.interpolate(features -> work_hw, bilinear, align_corners=False)     rade_features_model.py:159-171
    2. p = branch(relu(hidden_conv(x)))                                          utils/features.py:454-455 (1 x 1 convolutions)
    3. raw = einsum("chw,nc->nhw", p, E)                                         utils/features.py:269
    4. "standard" / "pairwise": softmax, stack, softmax, min, NaN -> 0 in its order   utils/features.py:272-325
    5. F.interpolate(similarity -> image size)                                   rade_features_model.py:525-535
       (the reference keeps the map only when the sizes differ; this project always sets it: DESIGN.md section 23)

``folded``: the algorithm of csrc/textquery.hip (A = E w_out, c = E b_out, the closed form of "pairwise") in the same dtype,
used by the host tests to show that the fold changes nothing beyond rounding.
"""
import torch
import torch.nn.functional as F


def decode_main(features, w_hidden, b_hidden, w_out, b_out, work_hw):
    """features [H, W, L] -> the main branch [C, h, w] (steps 1 and 2)."""
    x = F.interpolate(features.permute(2, 0, 1).unsqueeze(0), size=tuple(work_hw), mode="bilinear", align_corners=False)
    h = F.relu(F.conv2d(x, w_hidden[:, :, None, None], b_hidden))
    return F.conv2d(h, w_out[:, :, None, None], b_out).squeeze(0)


def decode_rows(latents, w_hidden, b_hidden, w_out, b_out):
    """latents [N, L] -> [N, C]: ``per_gaussian_forward`` (utils/features.py:470-476)."""
    return F.linear(F.relu(F.linear(latents, w_hidden, b_hidden)), w_out, b_out)


def compute_similarity(decoded, embeddings, n_pos, softmax_temp=0.05, method="standard"):
    """The similarity of utils/features.py:268-325 in its order of operations, the encoded queries passed in: ``decoded``
    [C, h, w], ``embeddings`` [Q, C] -> [h, w, 1].  The products of every pixel with every query (one einsum, :269); a softmax
    over the Q queries at the temperature (:275).  "standard": the positive queries' probabilities summed (:281).  "pairwise"
    (:284-318): the mean of the positive products, repeated once per negative, stacked over the negatives; a softmax over
    those 2 n_neg rows; the smallest of the repeats' probabilities; NaN -> 0."""
    _, h, w = decoded.shape
    raw = torch.einsum("chw,nc->nhw", decoded, embeddings).reshape(embeddings.shape[0], h * w)          # [Q, pixels]
    if method == "standard":
        sim = torch.softmax(raw / softmax_temp, dim=0)[:n_pos].sum(dim=0)
    elif method == "pairwise":
        neg = raw[n_pos:]
        mean_pos = raw[:n_pos].mean(dim=0, keepdim=True)
        stacked = torch.cat([mean_pos.expand(neg.shape[0], -1), neg], dim=0)                              # [2 n_neg, pixels]
        sim = torch.softmax(stacked / softmax_temp, dim=0)[:neg.shape[0]].min(dim=0).values
        sim = torch.nan_to_num(sim, nan=0.0)
    else:
        raise ValueError(method)
    return sim.reshape(h, w, 1)


def resize_map(sim, out_hw):
    """[h, w, 1] -> [H, W, 1]: the bilinear resize of the heat map (step 5, rade_features_model.py:525-535); equal sizes: the
    map itself."""
    if tuple(sim.shape[:2]) == tuple(out_hw):
        return sim
    return F.interpolate(sim[None, None, :, :, 0], size=tuple(out_hw), mode="bilinear", align_corners=False)[0, 0, :, :, None]


def similarity_map(scene, dtype, method, softmax_temp=0.05, out_hw="scene"):
    """A scene of tests/textquery_scenes.py through steps 1-5: [H_out, W_out, 1].  ``out_hw=None``: the map at ``work``."""
    t = {k: scene[k].to(dtype) for k in ("features", "w_hidden", "b_hidden", "w_out", "b_out", "embeddings")}
    p = decode_main(t["features"], t["w_hidden"], t["b_hidden"], t["w_out"], t["b_out"], scene["work"])
    sim = compute_similarity(p, t["embeddings"], scene["n_pos"], softmax_temp, method)
    out_hw = scene["out"] if out_hw == "scene" else out_hw
    return sim if out_hw is None else resize_map(sim, out_hw)


def row_similarity(scene, latents, dtype, method, softmax_temp=0.05):
    """[N]: the rows decoded (``decode_rows``) and queried as a [C, N, 1] image."""
    t = {k: scene[k].to(dtype) for k in ("w_hidden", "b_hidden", "w_out", "b_out", "embeddings")}
    p = decode_rows(latents.to(dtype), t["w_hidden"], t["b_hidden"], t["w_out"], t["b_out"])
    return compute_similarity(p.t().reshape(p.shape[1], -1, 1), t["embeddings"], scene["n_pos"], softmax_temp, method).reshape(-1)


# ------------------------------------------------------------------------------------------ the kernels' algorithm
def fold(embeddings, w_out, b_out):
    """A = E w_out [Q, Hd], c = E b_out [Q]."""
    return embeddings @ w_out, embeddings @ b_out


def pairwise_closed_form(z, n_pos):
    """z [..., Q] logits (already divided by T) -> exp(p) / (n_neg exp(p) + sum_j exp(n_j)), the maximum subtracted first."""
    p = z[..., :n_pos].mean(-1, keepdim=True)
    neg = z[..., n_pos:]
    top = torch.maximum(p, neg.max(-1, keepdim=True).values)
    e = torch.exp(p - top)
    r = (e / (neg.shape[-1] * e + torch.exp(neg - top).sum(-1, keepdim=True)))[..., 0]
    return torch.nan_to_num(r, nan=0.0)


def folded(scene, dtype, method, softmax_temp=0.05, out_hw="scene", latents=None):
    """The folded algorithm on a scene (or, with ``latents`` [N, L], on rows): x, hid, z = (A hid + c) / T, the reduction."""
    t = {k: scene[k].to(dtype) for k in ("features", "w_hidden", "b_hidden", "w_out", "b_out", "embeddings")}
    A, c = fold(t["embeddings"], t["w_out"], t["b_out"])
    if latents is None:
        x = F.interpolate(t["features"].permute(2, 0, 1).unsqueeze(0), size=tuple(scene["work"]), mode="bilinear",
                          align_corners=False)[0].permute(1, 2, 0)                                   # [h, w, L]
    else:
        x = latents.to(dtype)
    hid = torch.relu(x @ t["w_hidden"].t() + t["b_hidden"])
    z = (hid @ A.t() + c) / softmax_temp
    if method == "standard":
        sim = torch.nan_to_num(torch.softmax(z, -1)[..., :scene["n_pos"]].sum(-1), nan=0.0)
    else:
        sim = pairwise_closed_form(z, scene["n_pos"])
    if latents is not None:
        return sim
    out_hw = scene["out"] if out_hw == "scene" else out_hw
    return sim[..., None] if out_hw is None else resize_map(sim[..., None], out_hw)
