"""Generates tests/golden/metrics_goldens.npz by RUNNING THE REFERENCE's own ``mean_angular_error`` in the build container, as
make_depthcloud_goldens.py does: only the input and output arrays are committed, nothing of the reference's text.

``collab_splats/utils/utils.py`` imports packages that are not installed here, so it is parsed and the one function definition
alone is executed.  The input is [2, 3, 5, 7] float32: unit vectors in view 0, vectors of length up to 2 in view 1 -- dot products
beyond +-1, which the function clamps -- with a few exactly parallel and exactly opposite pairs.

    python tests/golden/make_metrics_goldens.py
"""
import ast
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
UTILS = "/root/reference/collab_splats/utils/utils.py"
OUT = os.path.join(HERE, "metrics_goldens.npz")


def load_mean_angular_error():
    tree = ast.parse(open(UTILS).read())
    wanted = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "mean_angular_error"]
    assert len(wanted) == 1
    ns = {"torch": torch}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), UTILS, "exec"), ns)
    return ns["mean_angular_error"]


def main():
    fn = load_mean_angular_error()
    g = torch.Generator().manual_seed(2024)
    pred = torch.randn(2, 3, 5, 7, generator=g)
    gt = torch.randn(2, 3, 5, 7, generator=g)
    pred = pred / pred.norm(dim=1, keepdim=True)
    gt = gt / gt.norm(dim=1, keepdim=True)
    pred[1] *= 0.5 + 1.5 * torch.rand(5, 7, generator=g)
    gt[1] *= 0.5 + 1.5 * torch.rand(5, 7, generator=g)
    gt[:, :, 0, 0] = pred[:, :, 0, 0]                                  # parallel
    gt[:, :, 0, 1] = -pred[:, :, 0, 1]                                 # opposite
    gt[1, :, 1, 0] = 1.5 * pred[1, :, 1, 0]                            # dot > 1 for certain
    gt[1, :, 1, 1] = -1.5 * pred[1, :, 1, 1]                           # dot < -1
    out = fn(pred, gt)
    dots = (pred * gt).sum(1)
    assert out.shape == (2, 5, 7) and bool(torch.isfinite(out).all())
    assert int((dots > 1).sum()) >= 1 and int((dots < -1).sum()) >= 1
    np.savez_compressed(OUT, pred=pred.numpy(), gt=gt.numpy(), angles=out.numpy())
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", int((dots.abs() > 1).sum()), "dot products beyond +-1")


if __name__ == "__main__":
    main()
