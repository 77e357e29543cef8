"""Generates tests/golden/depthcloud_goldens.npz by RUNNING THE REFERENCE's own code in the build container, as
make_camera_goldens.py does: only the input and output arrays are committed, nothing of the reference's text.

  * ``camera_utils.py`` is loaded by path (``get_colored_points_from_depth``, ``get_means3d_backproj``, ``project_pix``).
  * ``mesh.py`` cannot be imported here (Open3D, nerfstudio, MeshLib): it is parsed, and the two function definitions
    ``find_depth_edges`` and ``pick_indices_at_random`` alone are executed; the normal-map statements of
    ``DepthAndNormalMapsPoisson.main`` (mesh.py:937-954) are cut out of the parsed source at generation time and executed on
    the scene's maps.

The edge goldens are only meaningful when no pixel's Laplacian sits at the threshold (the reference's conv2d sums in its own
order): the generator asserts that the fp64 Laplacian of every pixel is at least 1e-4 from every threshold used.

    python tests/golden/make_depthcloud_goldens.py
"""
import ast
import os
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import depthcloud_restatement as R  # noqa: E402
import depthcloud_scenes as Q  # noqa: E402
from make_camera_goldens import load_reference  # noqa: E402

MESH = "/root/reference/collab_splats/utils/mesh.py"
OUT = os.path.join(HERE, "depthcloud_goldens.npz")
EDGE_CASES = [(0.004, 10), (0.004, 3), (0.01, 1), (0.01, 0)]


def load_mesh_functions():
    """find_depth_edges, pick_indices_at_random and the normal-map statements of mesh.py, by parsing it."""
    source = open(MESH).read()
    tree = ast.parse(source)
    ns = {"torch": torch, "F": torch.nn.functional}
    wanted = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("find_depth_edges", "pick_indices_at_random")]
    assert len(wanted) == 2
    exec(compile(ast.Module(body=wanted, type_ignores=[]), MESH, "exec"), ns)
    lines = source.splitlines()
    first, last = 937 - 1, 954 - 1                                  # mesh.py:937-954, checked by shape below
    assert "normals_name" in lines[first] and lines[first].strip().startswith("normal_map =") and lines[last].strip().endswith("[indices]")
    normal_code = compile(textwrap.dedent("\n".join(lines[first:last + 1])), MESH, "exec")

    def normals_of(normal_map, c2w, indices):
        env = {"torch": torch, "outputs": {"normals": normal_map}, "self": types.SimpleNamespace(normals_name="normals"),
               "c2w": c2w, "indices": indices}
        exec(normal_code, env)
        return env["normal_map"]

    return ns["find_depth_edges"], ns["pick_indices_at_random"], normals_of


def lap64(depth):
    inv = 1.0 / (depth.astype(np.float64) + 1e-6)
    pad = np.pad(inv, 1)
    return pad[:-2, 1:-1] + pad[2:, 1:-1] + pad[1:-1, :-2] + pad[1:-1, 2:] - 4 * inv


def main():
    cam = load_reference()
    find_depth_edges, pick_indices_at_random, normals_of = load_mesh_functions()
    out = {"edge_cases": np.array(EDGE_CASES)}
    worst_margin, worst_pts, worst_inv, worst_nrm = np.inf, 0.0, 0.0, 0.0
    for i in range(3):
        c2w, intr, W, H = Q.pose(i)
        # ---- edges
        depth = Q.edge_scene(H, W, seed=10 + i)
        out[f"edge{i}_depth"] = depth
        lap = lap64(depth)
        for j, (thr, dil) in enumerate(EDGE_CASES):
            worst_margin = min(worst_margin, float(np.abs(lap - thr).min()))
            ref = find_depth_edges(torch.from_numpy(depth)[..., None], threshold=thr, dilation_itr=dil)
            ref = ref.numpy()[..., 0] > 0
            assert np.array_equal(R.depth_edges(depth[None], thr, dil)[0], ref), (i, thr, dil)
            out[f"edge{i}_{j}"] = np.packbits(ref)
        # ---- candidates: pick_indices_at_random with room for all returns nonzero(ravel(valid_mask)) in order
        picked = pick_indices_at_random(torch.from_numpy(depth)[..., None], H * W + 1).numpy()
        out[f"pick{i}_all"] = picked.astype(np.int32)
        torch.manual_seed(i)
        out[f"pick{i}_some"] = pick_indices_at_random(torch.from_numpy(depth)[..., None], 37).numpy().astype(np.int32)
        # ---- back-projection
        rng = np.random.default_rng(20 + i)
        d = rng.uniform(1.5, 4.5, (H, W)).astype(np.float32)
        rgb = rng.random((H, W, 3)).astype(np.float32)
        nrm = rng.random((H, W, 3)).astype(np.float32)
        indices = np.nonzero(d.ravel())[0][::3]
        c2w4 = torch.eye(4)
        c2w4[:3, :4] = torch.from_numpy(c2w)
        c2w_cv = (c2w4 @ torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0])))[:3, :4]                  # mesh.py:896-901
        fx, fy, cx, cy = (float(x) for x in intr)
        pts, cols = cam.get_colored_points_from_depth(depths=torch.from_numpy(d)[..., None], rgbs=torch.from_numpy(rgb), fx=fx, fy=fy,
                                                      cx=cx, cy=cy, img_size=(W, H), c2w=c2w_cv, mask=torch.from_numpy(indices))
        nout = normals_of(torch.from_numpy(nrm), c2w_cv, torch.from_numpy(indices))
        out.update({f"bp{i}_c2w": c2w, f"bp{i}_intr": intr, f"bp{i}_depth": d, f"bp{i}_rgb": rgb, f"bp{i}_normals": nrm,
                    f"bp{i}_indices": indices.astype(np.int32), f"bp{i}_points": pts.numpy(), f"bp{i}_colors": cols.numpy(),
                    f"bp{i}_out_normals": nout.numpy()})
        # what the restatement is from the reference, in the units of the tests' bounds
        f = np.zeros(len(indices), np.int32)
        rp, rn, rc = R.backproject(d[None], rgb[None], nrm[None], c2w[None], intr[None], f, indices)
        unit = 2.0 ** -24 * (R.camera_abs(d[None], intr[None], f, indices) + np.abs(c2w[:, 3]).max())
        worst_pts = max(worst_pts, float((np.abs(rp.astype(np.float64) - pts.numpy()).max(1) / unit).max()))
        worst_nrm = max(worst_nrm, float(np.abs(rn.astype(np.float64) - nout.numpy()).max() / 2.0 ** -24))
        assert np.array_equal(rc, cols.numpy())
        # the reference's inv(R) against R^T, same units
        Rm = c2w_cv[:3, :3].double()
        cam_pts = (pts.double() - c2w_cv[:3, 3].double()) @ Rm                                     # back to the camera frame
        diff = (cam_pts @ torch.linalg.inv(c2w_cv[:3, :3]).double() - cam_pts @ Rm.T).abs().max(1).values.numpy()
        worst_inv = max(worst_inv, float((diff / unit).max()))
        # ---- project_pix, for the Gaussian mask filter's restatement
        P = (rng.uniform(-1, 1, (200, 3)) * 3).astype(np.float32) + c2w[:, 3] + (c2w[:, :3] @ np.array([0, 0, -4.0], np.float32))
        uvz = cam.project_pix(torch.from_numpy(P), fx, fy, cx, cy, c2w_cv, device=torch.device("cpu"), return_z_depths=True)
        out[f"proj{i}_points"], out[f"proj{i}_uvz"] = P, uvz.numpy()
    assert worst_margin >= 1e-4, worst_margin
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(out), "arrays,", os.path.getsize(OUT), "bytes")
    print(f"smallest |lap64 - threshold| {worst_margin:.3g}; restatement vs reference: points {worst_pts:.3g} units, "
          f"normals {worst_nrm:.3g} x 2^-24; inv(R) vs R^T {worst_inv:.3g} units")


if __name__ == "__main__":
    main()
