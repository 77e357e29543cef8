"""Build recipe for libmisplat.so (hipcc, gfx950 only, in-tree).

``python -m collab_splats_amd.build`` or ``build()``.  The library is written next to this
file so it travels with the source tree; it is git-ignored (history stays source-only).
hipcc cross-compiles without a GPU.
"""
from __future__ import annotations

import glob
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(ROOT, "include")
OBJ = os.path.join(HERE, "_obj")
LIB = os.path.join(HERE, "libmisplat.so")

ARCH = "gfx950"
COMMON = ["--offload-arch=" + ARCH, "-O3", "-fPIC", "-std=c++17", "-I", INCLUDE,
          "-Wall", "-Wno-unused-function", "-fno-fast-math"]
# project.hip: fixed IEEE operation order (no FMA contraction) so the integer binning stage is
# reproducible bit for bit against an independent fp32 implementation of the same order.
SOURCES = {
    "project.hip": ["-ffp-contract=off"],
    "binning.hip": [],
    "bucket.hip": [],
    "raster.hip": [],
    # blend.hip: the compositing loops are written for the issue slots they cost -- packed (v_pk_*) where two pixels run, plain
    # where one does; the SLP vectoriser re-packs the one-pixel bodies across unrelated values (103 packed + 83 moves in the
    # backward's trip loop, 154 registers; without it 37 + 17 and 115)
    "blend.hip": ["-fno-slp-vectorize"],
    "epilogue.hip": [],
    "ssim.hip": [],
    # featloss.hip: contraction allowed (the decoder's dot products are multiply-add chains; the test oracle is fp64)
    "featloss.hip": [],
    # textquery.hip: contraction allowed, as featloss.hip (multiply-add chains; the test oracle is fp64)
    "textquery.hip": [],
    "optim.hip": [],
    # tsdf.hip: fixed IEEE operation order, as project.hip: the voxel grids equal the fp32 restatement (tests/) bit for bit
    "tsdf.hip": ["-ffp-contract=off"],
    # meshmap.hip: the same: the neighbour lists equal the fp32 restatement (tests/) bit for bit
    "meshmap.hip": ["-ffp-contract=off"],
    # cluster.hip: the same: the radius graph's edge test d2 < r2 equals the fp32 restatement (tests/) bit for bit
    "cluster.hip": ["-ffp-contract=off"],
    # pointcloud.hip: the same: the k smallest d2, the radius rule d2 < r2 and the fp64 voxel sums equal the restatement (tests/)
    "pointcloud.hip": ["-ffp-contract=off"],
    # meshclean.hip: the same: edge lengths, plane hypotheses and the inlier rule equal the restatement (tests/) bit for bit
    "meshclean.hip": ["-ffp-contract=off"],
    # depthcloud.hip: the same: edge bits, sampled pixels, back-projected points and normals equal the restatement (tests/)
    "depthcloud.hip": ["-ffp-contract=off"],
    # poisson.hip: the same: the splat's int64 grids, the right-hand side and the diagonal equal the restatement (tests/)
    "poisson.hip": ["-ffp-contract=off"],
    # grouping.hip: integer work throughout; its one double product (front_percentage n) has nothing to contract with
    "grouping.hip": [],
    # bilagrid.hip: fixed IEEE operation order: the luma z (black exactly 0, white exactly 1), the interval floor(gz) and the
    # lerp form a + t (b - a) equal the fp32 restatement (tests/); a locally constant grid is reproduced bit for bit
    "bilagrid.hip": ["-ffp-contract=off"],
    # density.hip: fixed IEEE operation order: the Gaussians' frames, unit ranges and slab tests, hence the unit lists, equal
    # the fp32 restatement (tests/) bit for bit; the accumulation's multiply-adds are written as explicit fma
    "density.hip": ["-ffp-contract=off"],
    # decimate.hip: the same: quadrics, collapse targets and cost bits (the selection's priority) equal the fp64 restatement (tests/)
    "decimate.hip": ["-ffp-contract=off"],
    # meshfill.hip: the same: edge lengths (the split priority), midpoints and the fp64 neighbour means equal the restatement (tests/)
    "meshfill.hip": ["-ffp-contract=off"],
    # meshtri.hip: the same: triangle areas and the fp64 sums of the triangulation's table, the cotangents and normals of the flip
    # test equal the restatement (tests/) bit for bit
    "meshtri.hip": ["-ffp-contract=off"],
    # pointtsdf.hip: the same: the rays' voxel walks and fixed-point sdf terms, hence the integer planes, equal the restatement (tests/)
    "pointtsdf.hip": ["-ffp-contract=off"],
    # identity.hip: contraction allowed, as featloss.hip (the logits are multiply-add chains; the test oracle is fp64)
    "identity.hip": [],
    # evalmetrics.hip: contraction allowed, as ssim.hip, whose filter it runs (multiply-add chains; the test oracle is fp64);
    # the per-pixel normal and depth arithmetic is fp64 and the integer counts do not depend on it
    "evalmetrics.hip": [],
    # colorcorrect.hip: fixed IEEE operation order: the warp's sum ((a0 w0 + a1 w1) + a2 w2) + ... rounds every product and sum
    # on its own, so the numpy fp64 restatement (tests/) reproduces the image bit for bit from the device's fit; the
    # accumulation's multiply-adds are written as explicit fma
    "colorcorrect.hip": ["-ffp-contract=off"],
    # mcmc.hip: fixed IEEE operation order: the noise step rounds its displacement d to fp32 on its own and then adds it, so
    # the update equals fl32(mean + d) bit for bit; the sampler is integer work and the relocation's sums are fp64 in written order
    "mcmc.hip": ["-ffp-contract=off"],
}


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def headers() -> list:
    """What every object depends on: the public header and every header next to the sources."""
    return [os.path.join(INCLUDE, "misplat.h")] + sorted(glob.glob(os.path.join(CSRC, "*.h")))


def build(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(OBJ, exist_ok=True)
    hipcc = _hipcc()
    jobs = []
    objs = []
    for src, extra in SOURCES.items():
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s, __file__] + headers()):
            jobs.append([hipcc] + COMMON + extra + ["-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    if jobs:
        with ThreadPoolExecutor(max_workers=min(4, len(jobs))) as ex:
            list(ex.map(run, jobs))
    if force or jobs or _stale(LIB, objs):
        run([hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs)
    try:                                              # the source revision travels with the library (the GPU box has no .git)
        rev = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        dirty = subprocess.call(["git", "-C", ROOT, "diff", "--quiet", "HEAD", "--", "collab_splats_amd", "include", "bench.py"]) != 0
        with open(os.path.join(HERE, "_build_rev.txt"), "w") as f:
            f.write(rev + ("+" if dirty else "") + "\n")
    except Exception:
        pass
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
