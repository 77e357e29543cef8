"""The bilateral-grid slice and the grids' TV loss restated in plain tensor indexing (test infrastructure; DESIGN.md
section 24 has the definition).  Parameterised by dtype: the luma z = 0.299 r + 0.587 g + 0.114 b and the interval index
floor(gz) are ALWAYS evaluated in fp32, left to right (they choose a cell: a choice is not a rounding error, the same device
as the ray table that stays fp32 in the loss-side restatement); everything after that runs in the requested dtype.  The fp64
run is the oracle of the GPU tests, the fp32 run their yardstick.  Gradients come from autograd over these lines.

``luma_dtype`` (default fp32, as stated) exists for one test: finite differences need the luma in fp64 as well, because an
fp32-rounded z is a staircase at the scale of a finite-difference step."""
import torch

LUMA = (0.299, 0.587, 0.114)


def luma(rgb: torch.Tensor, luma_dtype=torch.float32) -> torch.Tensor:
    """[H, W, 3] -> [H, W]: (0.299 r + 0.587 g) + 0.114 b with the fp32 constants, evaluated in ``luma_dtype``."""
    c = rgb.to(luma_dtype)
    w = [torch.tensor(v, dtype=torch.float32).to(luma_dtype) for v in LUMA]
    return (w[0] * c[..., 0] + w[1] * c[..., 1]) + w[2] * c[..., 2]


class _Luma(torch.autograd.Function):
    """The luma's VALUE from ``luma_dtype`` (cast to the dtype of ``rgb``: exact for fp32 -> fp64), its gradient -- the three
    constants -- in the dtype of ``rgb``: autograd through the cast would round the oracle's gradient to fp32."""

    @staticmethod
    def forward(ctx, rgb, luma_dtype):
        ctx.dtype = rgb.dtype
        return luma(rgb, luma_dtype).to(rgb.dtype)

    @staticmethod
    def backward(ctx, g):
        w = torch.tensor(LUMA, dtype=torch.float32).to(ctx.dtype)
        return g[..., None] * w, None


def _axis(n_pix: int, n_grid: int, dtype):
    """Positions of the pixels of one image axis on a grid axis: (i0, i1, t)."""
    p = torch.arange(n_pix, dtype=dtype)
    u = p / (n_pix - 1) if n_pix > 1 else torch.zeros(n_pix, dtype=dtype)
    c = (u * (n_grid - 1)).clamp(0, n_grid - 1)
    i0 = torch.floor(c).long()
    return i0, (i0 + 1).clamp(max=n_grid - 1), c - i0.to(dtype)


def z_position(rgb: torch.Tensor, L: int, dtype, luma_dtype=torch.float32):
    """(z0, z1, tz, gz in luma_dtype): the interval from the ``luma_dtype`` evaluation, the fraction in ``dtype``.  The fraction
    carries a gradient only where 0 < gz < L - 1 (the slope of the interval floor(gz); 0 at and beyond the border planes)."""
    gz_sel = (luma(rgb.detach(), luma_dtype) * (L - 1)).clamp(0, L - 1)
    z0 = torch.floor(gz_sel).long()
    z1 = (z0 + 1).clamp(max=L - 1)
    gz = (_Luma.apply(rgb.to(dtype), luma_dtype) * (L - 1)).clamp(0, L - 1)
    tz = gz - z0.to(dtype)
    inside = (gz_sel > 0) & (gz_sel < L - 1)
    return z0, z1, torch.where(inside, tz, tz.detach()), gz_sel


def affine_field(rgb: torch.Tensor, grid: torch.Tensor, dtype, luma_dtype=torch.float32) -> torch.Tensor:
    """[12, H, W]: one camera's grid [12, L, GH, GW] interpolated at every pixel, lerp form a + t (b - a) along x, y, z."""
    H, W = rgb.shape[:2]
    _, L, GH, GW = grid.shape
    G = grid.to(dtype)
    x0, x1, tx = _axis(W, GW, dtype)
    y0, y1, ty = _axis(H, GH, dtype)
    z0, z1, tz, _ = z_position(rgb, L, dtype, luma_dtype)
    Y0, Y1, X0, X1 = y0[:, None], y1[:, None], x0[None, :], x1[None, :]
    tx, ty = tx[None, None, :], ty[None, :, None]

    def plane(zi):
        a00, a01, a10, a11 = G[:, zi, Y0, X0], G[:, zi, Y0, X1], G[:, zi, Y1, X0], G[:, zi, Y1, X1]
        r0 = a00 + tx * (a01 - a00)
        r1 = a10 + tx * (a11 - a10)
        return r0 + ty * (r1 - r0)

    P0, P1 = plane(z0), plane(z1)
    return P0 + tz[None] * (P1 - P0)


def slice_image(rgb: torch.Tensor, grids: torch.Tensor, cam: int, dtype, luma_dtype=torch.float32) -> torch.Tensor:
    """[H, W, 3]: out_c = A[c,0] r + A[c,1] g + A[c,2] b + A[c,3], left to right, not clamped."""
    A = affine_field(rgb, grids[cam], dtype, luma_dtype)
    c = rgb.to(dtype)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    return torch.stack([A[4 * k] * r + A[4 * k + 1] * g + A[4 * k + 2] * b + A[4 * k + 3] for k in range(3)], dim=-1)


def tv(grids: torch.Tensor, dtype) -> torch.Tensor:
    """(1 / num) sum over the axes L, GH, GW of sum (G[i + 1] - G[i])^2 / (the differences of one camera along that axis)."""
    G = grids.to(dtype)
    num = G.shape[0]
    total = torch.zeros((), dtype=dtype)
    for axis in (2, 3, 4):
        n = G.shape[axis]
        if n < 2:
            continue
        d = G.narrow(axis, 1, n - 1) - G.narrow(axis, 0, n - 1)
        total = total + (d * d).sum() / (d.numel() // num)
    return total / num


def run_slice(rgb, grids, v_out, cam: int, dtype, luma_dtype=torch.float32):
    """{"out", "v_rgb", "v_grids"} of one scene and camera in ``dtype`` (inputs are fp32 tensors: they are exact in both)."""
    r = rgb.to(dtype).clone().requires_grad_(True)
    g = grids.to(dtype).clone().requires_grad_(True)
    out = slice_image(r, g, cam, dtype, luma_dtype)
    (out * v_out.to(dtype)).sum().backward()
    return {"out": out.detach(), "v_rgb": r.grad, "v_grids": g.grad}


def run_tv(grids, dtype):
    g = grids.to(dtype).clone().requires_grad_(True)
    loss = tv(g, dtype)
    loss.backward()
    return {"loss": loss.detach(), "v_grids": g.grad}
