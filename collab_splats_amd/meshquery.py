"""Queries on the mesh's vertex features: text similarity and radius-graph clustering.

``query_similarity`` restates the reference's ``compute_similarity`` behind ``Splatter.query_mesh``
(collab_splats/wrapper/splatter.py:502-567, collab_splats/utils/features.py:237-325): an optional decoder MLP on the vertex
features, their products with the text embeddings, and a softmax at a temperature.  It is dense GEMM plus a row softmax,
which torch already runs well on the device: plain torch on whatever device the inputs are on, no HIP.

``mesh_clustering`` / ``cluster_labels`` restate the reference's ``mesh_clustering`` (collab_splats/utils/mesh.py:523-576):
threshold the similarity, join selected vertices closer than ``spatial_radius``, keep the connected components of more than
``min_cluster_size`` vertices.  The reference searches an Open3D KD-tree in a Python loop and writes a dense adjacency
matrix; this build runs a union-find over the implicit radius graph on the device (csrc/cluster.hip) with O(M) memory.
There is no CPU fallback for the clustering.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from ._lib import MisplatError, load, ptr, require_gpu, run
from .meshmap import COORD_CELLS, _prep


# ------------------------------------------------------------------------------------------------------ similarity
def query_similarity(features: Tensor, text_embeddings: Tensor, n_positive: int, method: str = "pairwise",
                     softmax_temp: float = 0.05, decoder: Optional[Sequence[Tensor]] = None) -> Tensor:
    """Similarity of every vertex to the positive text queries, [M] fp32 in 0..1.

    ``features`` [M,C_in]; ``text_embeddings`` [Q,C], unit-norm rows, the first ``n_positive`` positive and the others
    negative (at least one of each); ``decoder`` None or (w_hidden [Hd,C_in], b_hidden [Hd], w_out [C,Hd], b_out [C]): the
    features first go through relu(x w_hidden^T + b_hidden) w_out^T + b_out.  With raw = features text_embeddings^T:
    "standard" is softmax(raw / T, dim 1)[:, :n_positive].sum(1); "pairwise" is the reference's: p = the mean positive
    product, one softmax over n_neg copies of p and the n_neg negatives, the minimum over the copies' (equal)
    probabilities, exp(p/T) / (n_neg exp(p/T) + sum_j exp(n_j/T)), NaN -> 0."""
    if method not in ("standard", "pairwise"):
        raise ValueError(f"query_similarity: unknown method {method!r}: choose 'standard' or 'pairwise'")
    if features.dim() != 2:
        raise ValueError(f"query_similarity: features must be [M,C], got {tuple(features.shape)}")
    if text_embeddings.dim() != 2:
        raise ValueError(f"query_similarity: text_embeddings must be [Q,C], got {tuple(text_embeddings.shape)}")
    Q = text_embeddings.shape[0]
    if not isinstance(n_positive, int) or isinstance(n_positive, bool) or not 1 <= n_positive <= Q - 1:
        raise ValueError(f"query_similarity: n_positive must be an integer in 1..Q-1 = {Q - 1} (at least one positive and "
                         f"one negative embedding), got {n_positive!r}")
    if not (softmax_temp > 0 and math.isfinite(softmax_temp)):
        raise ValueError(f"query_similarity: softmax_temp must be positive and finite, got {softmax_temp!r}")
    x = features.detach().to(torch.float32)
    emb = text_embeddings.detach().to(device=x.device, dtype=torch.float32)
    if decoder is not None:
        if len(decoder) != 4:
            raise ValueError("query_similarity: decoder must be (w_hidden, b_hidden, w_out, b_out)")
        w_h, b_h, w_o, b_o = (t.detach().to(device=x.device, dtype=torch.float32) for t in decoder)
        if (w_h.dim() != 2 or w_h.shape[1] != x.shape[1] or b_h.shape != (w_h.shape[0],) or w_o.dim() != 2
                or w_o.shape[1] != w_h.shape[0] or b_o.shape != (w_o.shape[0],)):
            raise ValueError(f"query_similarity: decoder shapes {[tuple(t.shape) for t in decoder]} do not fit features of "
                             f"width {x.shape[1]}")
        x = F.linear(F.relu(F.linear(x, w_h, b_h)), w_o, b_o)
    if x.shape[1] != emb.shape[1]:
        raise ValueError(f"query_similarity: features of width {x.shape[1]} against text embeddings of width {emb.shape[1]}")
    z = F.linear(x, emb) / softmax_temp                                      # [M,Q] logits
    if method == "standard":
        return torch.softmax(z, dim=1)[:, :n_positive].sum(1)
    zp = z[:, :n_positive].mean(1, keepdim=True)                             # (mean of the products) / T
    zn = z[:, n_positive:]
    top = torch.maximum(zp, zn.max(1, keepdim=True).values)
    e = torch.exp(zp - top)
    sim = (e / ((Q - n_positive) * e + torch.exp(zn - top).sum(1, keepdim=True)))[:, 0]
    return torch.where(torch.isnan(sim), torch.zeros_like(sim), sim)


def similarity_colors(similarity: Tensor) -> Tensor:
    """[M,3] fp32 vertex colours of a query (what ``write_ply(..., colors=...)`` takes): the similarity divided by its
    maximum (if that is positive) in the red channel, zeros elsewhere."""
    s = similarity.detach().to(torch.float32).reshape(-1)
    out = torch.zeros((s.shape[0], 3), dtype=torch.float32, device=s.device)
    if s.shape[0] == 0:
        return out
    top = s.max()
    out[:, 0] = torch.where(top > 0, s / top, s)
    return out


# ------------------------------------------------------------------------------------------------------ clustering
def _check(name: str, vertices: Tensor, per_vertex: Tensor, what: str, radius, min_cluster_size) -> None:
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{name}: vertices must be [M,3], got {tuple(vertices.shape)}")
    M = vertices.shape[0]
    if tuple(per_vertex.shape) not in ((M,), (M, 1)):
        raise ValueError(f"{name}: {what} must be [M] or [M,1] with M = {M}, got {tuple(per_vertex.shape)}")
    r = float(radius)
    if not (r > 0 and math.isfinite(r)):
        raise ValueError(f"{name}: the radius must be positive and finite, got {radius!r}")
    r32 = torch.tensor(r, dtype=torch.float32)
    if not (bool(torch.isfinite(r32)) and bool(torch.isfinite(1.0 / r32)) and float(r32) > 0):
        raise ValueError(f"{name}: the radius must be positive and finite in fp32 (and so must 1 / radius), got {radius!r}")
    if not isinstance(min_cluster_size, int) or isinstance(min_cluster_size, bool) or not 0 <= min_cluster_size < 2 ** 31:
        raise ValueError(f"{name}: min_cluster_size must be an integer >= 0, got {min_cluster_size!r}")
    if M > 0:
        v = vertices.detach().to(torch.float32)
        bad = (~torch.isfinite(v)).any() | ((v.abs() * (1.0 / r)) >= COORD_CELLS).any()
        if bool(bad):                                           # host read 1 of 2
            raise ValueError(f"{name}: vertices must be finite and within 2^18 radius of the origin on every axis")
    require_gpu(vertices, per_vertex)


def _cluster(vertices: Tensor, mask: Tensor, radius: float, min_cluster_size: int) -> Tuple[Tensor, Tensor, int]:
    """(labels [M] int32, sizes [M] int32 of which the first n are set, n) for prepared inputs."""
    M = vertices.shape[0]
    dev = vertices.device
    labels = torch.full((M,), -1, dtype=torch.int32, device=dev)
    sizes = torch.empty(M, dtype=torch.int32, device=dev)
    if M == 0:
        return labels, sizes, 0
    n = int(load().misplat_cluster_workspace(M))
    if n < 0:
        raise ValueError(f"meshquery: {M} vertices are beyond the library's limits")
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    run("misplat_cluster_radius", ptr(vertices), M, ptr(mask), radius, min_cluster_size, ptr(ws), ws.numel(), ptr(labels),
        ptr(sizes), ptr(count))
    return labels, sizes, int(count.item())                     # host read 2 of 2


def cluster_labels(vertices: Tensor, mask: Tensor, radius: float, min_cluster_size: int = 10) -> Tuple[Tensor, Tensor]:
    """Connected components of the radius graph over the vertices whose ``mask`` is set.

    Selected vertices i != j are joined iff d2 < r2 with d2 = ((dx dx + dy dy) + dz dz) and r2 = r r in fp32, r =
    float32(radius).  Components of more than ``min_cluster_size`` vertices are kept and numbered 0, 1, ... in ascending
    order of their smallest vertex index.  Returns (labels [M] int32: the cluster of each vertex, -1 if it is not selected
    or its component was dropped; sizes [n_clusters] int32), both on the device.  Two runs are bitwise equal."""
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"cluster_labels: mask must be bool or uint8, got {mask.dtype}")
    _check("cluster_labels", vertices, mask, "mask", radius, min_cluster_size)
    v = _prep(vertices)
    m = (mask.detach().reshape(-1) != 0).to(torch.uint8).contiguous()
    labels, sizes, n = _cluster(v, m, float(radius), min_cluster_size)
    return labels, sizes[:n]


def mesh_clustering(vertices: Tensor, similarity_values: Tensor, similarity_threshold: float = 0.8,
                    spatial_radius: float = 0.03, min_cluster_size: int = 10) -> List[Tensor]:
    """The reference's ``mesh_clustering`` on the device: the vertices with ``similarity_values > similarity_threshold`` (both
    as fp32), joined within ``spatial_radius`` (``cluster_labels``), as one int64 tensor of ascending vertex indices per
    kept cluster, the clusters in ascending order of their smallest vertex.  No vertex selected: []."""
    _check("mesh_clustering", vertices, similarity_values, "similarity_values", spatial_radius, min_cluster_size)
    thr = float(similarity_threshold)
    if math.isnan(thr):
        raise ValueError("mesh_clustering: similarity_threshold is NaN")
    v = _prep(vertices)
    sim = _prep(similarity_values).reshape(-1)
    mask = (sim > torch.tensor(thr, dtype=torch.float32, device=sim.device)).to(torch.uint8)
    labels, sizes, n = _cluster(v, mask, float(spatial_radius), min_cluster_size)
    if n == 0:
        return []
    counts = sizes[:n].tolist()                 # the split points of a Python list live on the host: n integers
    order = torch.sort(labels, stable=True).indices                      # by cluster, ascending vertex index inside each
    return list(torch.split(order[labels.shape[0] - sum(counts):], counts))


__all__ = ["query_similarity", "similarity_colors", "cluster_labels", "mesh_clustering", "MisplatError"]
