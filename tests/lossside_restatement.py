"""Numpy fp64 restatement of the depth -> normal stencil (a4) and its adjoint, written from the formulas in the
comments of csrc/blend.hip -- independent of the torch restatement in oracle/camera_oracle.py and of the reference.

    P(y,x)  = z(y,x) * ray(y,x),  ray = (rx, ry, 1)
    a       = P(y+1,x) - P(y-1,x)           (along rows)
    b       = P(y,x+1) - P(y,x-1)           (along columns)
    c       = a x b,  n = c / max(|c|, 1e-12)            interior pixels; n = 0 on the border
    err_k   = 1 - <n_render, n_k>

    v_n     = v_normals - v_err * n_render,  v_n_render = -sum_k v_err_k * n_k
    v_c     = (v_n - n <n, v_n>) / |c|   if |c| > 1e-12   else   v_n * 1e12
    v_a     = b x v_c,  v_b = v_c x a
    v_P(y+1,x) += v_a, v_P(y-1,x) -= v_a, v_P(y,x+1) += v_b, v_P(y,x-1) -= v_b,  v_z = <v_P, ray>

The ray table is an argument ([H,W,2]: rx, ry): the goldens store the fp32 table the reference built, so the two
evaluations agree to fp64 rounding.
"""
import numpy as np

EPS = 1e-12


def ray_table(W, H, fx, fy):
    """K^-1 [x + .5, y + .5, 1] with the principal point at the image centre, fp64."""
    xs = (np.arange(W) + 0.5) / fx - W / (2 * fx)
    ys = (np.arange(H) + 0.5) / fy - H / (2 * fy)
    return np.stack(np.broadcast_arrays(xs[None, :], ys[:, None]), -1)


def _points(d, rays):
    return np.stack([d * rays[..., 0], d * rays[..., 1], d], -1)


def differences(d, rays):
    """a, b [H-2,W-2,3] of the interior pixels (empty when there is none)."""
    P = _points(np.asarray(d, np.float64), np.asarray(rays, np.float64))
    return P[2:, 1:-1] - P[:-2, 1:-1], P[1:-1, 2:] - P[1:-1, :-2]


def forward(d1, d2, n_render, rays):
    """-> normals2 [2,H,W,3], err [2,H,W]"""
    H, W = d1.shape
    n2 = np.zeros((2, H, W, 3))
    if H >= 3 and W >= 3:
        for k, d in enumerate((d1, d2)):
            a, b = differences(d, rays)
            c = np.cross(a, b)
            n2[k, 1:-1, 1:-1] = c / np.maximum(np.linalg.norm(c, axis=-1, keepdims=True), EPS)
    err = 1.0 - (np.asarray(n_render, np.float64)[None] * n2).sum(-1)
    return n2, err


def adjoint(d1, d2, n_render, rays, v_n2=None, v_err=None):
    """-> v_d1 [H,W], v_d2 [H,W], v_n_render [H,W,3]; an absent upstream is zero."""
    H, W = d1.shape
    nr = np.asarray(n_render, np.float64)
    rays = np.asarray(rays, np.float64)
    v_n2 = np.zeros((2, H, W, 3)) if v_n2 is None else np.asarray(v_n2, np.float64)
    v_err = np.zeros((2, H, W)) if v_err is None else np.asarray(v_err, np.float64)
    n2, _ = forward(d1, d2, nr, rays)
    v_nr = -(v_err[..., None] * n2).sum(0)
    v_d = []
    ray3 = np.concatenate([rays, np.ones((H, W, 1))], -1)
    for k, d in enumerate((d1, d2)):
        vP = np.zeros((H, W, 3))
        if H >= 3 and W >= 3:
            a, b = differences(d, rays)
            ln = np.linalg.norm(np.cross(a, b), axis=-1, keepdims=True)
            n = n2[k, 1:-1, 1:-1]
            vn = v_n2[k, 1:-1, 1:-1] - v_err[k, 1:-1, 1:-1, None] * nr[1:-1, 1:-1]
            healthy = ln > EPS
            vc = np.where(healthy, (vn - n * (n * vn).sum(-1, keepdims=True)) / np.where(healthy, ln, 1.0), vn * 1e12)
            va, vb = np.cross(b, vc), np.cross(vc, a)
            vP[2:, 1:-1] += va
            vP[:-2, 1:-1] -= va
            vP[1:-1, 2:] += vb
            vP[1:-1, :-2] -= vb
        v_d.append((vP * ray3).sum(-1))
    return v_d[0], v_d[1], v_nr

