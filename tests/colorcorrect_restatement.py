"""The colour correction of csrc/colorcorrect.hip restated on the CPU (numpy, fp64), literally after DESIGN.md section 35:

    x starts as pred (float32).  Per iteration: the 10 monomials a = (r^2, rg, rb, g^2, gb, b^2, r, g, b, 1) of every pixel of x
    in fp64; per output channel c the mask  unclipped(pred_c) & unclipped(x_c) & unclipped(gt_c)  with
    unclipped(z) = eps <= z <= 1 - eps  compared in float32 (eps and 1 - eps rounded to float32 first);  G_c = A_m^T A_m  and
    r_c = A_m^T gt_c  over the masked rows;  w_c = G_c^+ r_c  from ``numpy.linalg.eigh`` with the eigenvalues
    <= 2^-46 lambda_max dropped (G_c = 0: w_c = 0);  x'_c = clip(((a0 w0 + a1 w1) + a2 w2) + ..., 0, 1)  for every pixel,
    rounded once to float32.

One view at a time ([H, W, 3] or [P, 3]); the batch is the caller's loop.  ``solver`` swaps the solve (the host test's
independent oracle is the published formulation: ``lstsq`` on the masked design matrix); ``order`` permutes the pixels before
the sums (what a different summation order moves).  ``apply_chain`` is the apply alone, driven by given warps: with the
device's warps it reproduces the device's image bit for bit."""
from __future__ import annotations

import numpy as np

NUM_ITERS = 5
EPS = 0.5 / 255
CUT = 2.0 ** -46


def thresholds(eps: float = EPS):
    """(lo, hi) as float32: eps and 1 - eps, the subtraction in float32 as the library does it."""
    lo = np.float32(eps)
    return lo, np.float32(1.0) - lo


def unclipped(z: np.ndarray, eps: float = EPS) -> np.ndarray:
    lo, hi = thresholds(eps)
    assert z.dtype == np.float32
    return (z >= lo) & (z <= hi)


def monomials(x: np.ndarray) -> np.ndarray:
    """[P, 3] float32 -> [P, 10] float64 (products of float32 values are exact in fp64)."""
    assert x.dtype == np.float32
    r, g, b = (x[:, k].astype(np.float64) for k in range(3))
    return np.stack([r * r, r * g, r * b, g * g, g * b, b * b, r, g, b, np.ones_like(r)], axis=1)


def apply_warp(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    """[P, 3] float32, [10, 3] float64 -> [P, 3] float32: the sum in ascending k, every product and sum rounded on its own."""
    a = monomials(x)
    out = np.empty_like(x)
    for c in range(3):
        s = a[:, 0] * w[0, c]
        for k in range(1, 10):
            s = s + a[:, k] * w[k, c]
        out[:, c] = np.clip(s, 0.0, 1.0).astype(np.float32)
    return out


def solve_eigh(A: np.ndarray, y: np.ndarray):
    """(w, lambda / lambda_max descending or None): minimum-norm least squares of the masked rows through the normal equations."""
    G, r = A.T @ A, A.T @ y
    lam, vec = np.linalg.eigh(G)
    top = lam.max() if lam.size else 0.0
    if not top > 0.0:
        return np.zeros(10), None
    keep = lam > CUT * top
    w = vec[:, keep] @ ((vec[:, keep].T @ r) / lam[keep])
    return w, np.sort(lam / top)[::-1]


def solve_lstsq(A: np.ndarray, y: np.ndarray):
    """The published formulation: lstsq on the masked design matrix, rcond = float32's epsilon (on singular values: the square
    root of the eigenvalue cut).  ``gelsd`` on purpose: torch's default ``gelsy`` (pivoted QR) is no minimum-norm solver for a
    rank-deficient matrix and lands 0.37 away on the gray and empty-channel scenes."""
    import torch
    if A.shape[0] == 0:
        return np.zeros(10), None
    sol = torch.linalg.lstsq(torch.from_numpy(np.ascontiguousarray(A)), torch.from_numpy(np.ascontiguousarray(y))[:, None],
                             rcond=2.0 ** -23, driver="gelsd").solution
    return sol[:10, 0].numpy().astype(np.float64), None


def color_correct(pred: np.ndarray, gt: np.ndarray, num_iters: int = NUM_ITERS, eps: float = EPS, solver=solve_eigh, order=None):
    """-> {"image" [.., 3] float32, "warps" [num_iters, 10, 3] float64, "counts" [num_iters, 3] int64,
    "iterates": the float32 images x_0 .. x_num_iters ([P, 3]), "masks" [num_iters, 3, P] bool,
    "ratios": per iteration and channel lambda / lambda_max (or None)}."""
    shape = pred.shape
    pred = np.ascontiguousarray(pred, dtype=np.float32).reshape(-1, 3)
    gt = np.ascontiguousarray(gt, dtype=np.float32).reshape(-1, 3)
    m0, mg = unclipped(pred, eps), unclipped(gt, eps)
    x = pred.copy()
    warps = np.zeros((num_iters, 10, 3))
    counts = np.zeros((num_iters, 3), dtype=np.int64)
    iterates, masks, ratios = [x], [], []
    for it in range(num_iters):
        a = monomials(x)
        m = m0 & unclipped(x, eps) & mg
        rat = []
        for c in range(3):
            rows = np.flatnonzero(m[:, c])
            if order is not None:
                rows = rows[np.argsort(order[rows], kind="stable")]
            w, lam = solver(a[rows], gt[rows, c].astype(np.float64))
            warps[it, :, c] = w
            counts[it, c] = rows.size
            rat.append(lam)
        x = apply_warp(x, warps[it])
        iterates.append(x)
        masks.append(m.T.copy())
        ratios.append(rat)
    return {"image": x.reshape(shape), "warps": warps, "counts": counts, "iterates": iterates,
            "masks": np.array(masks, dtype=bool).reshape(num_iters, 3, x.shape[0]), "ratios": ratios}


def apply_chain(pred: np.ndarray, warps: np.ndarray) -> np.ndarray:
    """pred [.., 3] float32 through the warps [num_iters, 10, 3] one after the other, float32 in between."""
    x = np.ascontiguousarray(pred, dtype=np.float32).reshape(-1, 3)
    for w in np.asarray(warps, dtype=np.float64):
        x = apply_warp(x, w)
    return x.reshape(pred.shape)
