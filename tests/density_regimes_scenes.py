"""Scenes for the regimes of the density field that the model and scripts/density_bench.py reach and the scenes of
density_scenes.py do not: a cut-off other than 3, a min_opacity other than 1 / 255, the bench's voxel
size 0.01 at the far corner of its frustum (unit coordinates 46, -27, 72), a lattice hundreds of metres out with an h = 0.013 whose
products k h round, and Gaussians a hundredth of a voxel thick.  Every scene is a crop of TWO units drawn with
synthetic.random_scene's distributions (one of them with eight plates added that need the sub-brick test's slack), so the fp64 oracle costs about a second; density_scenes.scene() / restated() / oracle() / oracle_map() take the
names.  tests/test_density_regimes_host.py asserts on the restatement that each scene meets the conditions the GPU tests rest on,
tests/test_density_regimes_gpu.py compares the device with it."""
import functools
import math

import numpy as np

import density_scenes as S

F = np.float32
SHELL = 1e-4                                 # |m - r^2| <= SHELL r^2: where skipping and not skipping may round apart
SHELL_SHARE = 2e-3                           # at most this share of a scene's voxels may lie in such a shell


def workload(lo_units, dims, n, h, cutoff, seed, min_opacity=1.0 / 255.0, zero_opacities=0):
    """n Gaussians of synthetic.random_scene's distributions (log-uniform scales in [0.004, 0.04] with one randomly chosen axis
    ten times thinner, normal quaternions, opacities sigmoid(U(-2, 4))), their means uniform in the box of `dims` units at
    `lo_units` padded by the reach of the largest of them, min(cutoff, 3) 0.04 + h.  The bounds are that box shrunk by 1e-3 L: the
    map is exactly `dims` units at `lo_units`.  zero_opacities: that many opacities (evenly spread) are set to exactly 0."""
    rng = np.random.default_rng(seed)
    L = float(F(h) * F(16))
    lo_w, hi_w = np.asarray(lo_units, np.float64) * L, (np.asarray(lo_units, np.float64) + np.asarray(dims, np.float64)) * L
    pad = min(cutoff, 3.0) * 0.04 + h
    means = rng.uniform(lo_w - pad, hi_w + pad, (n, 3))
    log_s = rng.uniform(math.log(0.004), math.log(0.04), (n, 3))
    log_s[np.arange(n), rng.integers(0, 3, n)] += math.log(0.1)
    quats = rng.standard_normal((n, 4))
    opac = 1.0 / (1.0 + np.exp(-rng.uniform(-2.0, 4.0, n)))
    if zero_opacities:
        opac[:: n // zero_opacities][:zero_opacities] = 0.0
    return S._scene(means, quats, np.exp(log_s), opac, bounds=[(lo_w + 1e-3 * L).tolist(), (hi_w - 1e-3 * L).tolist()], h=h,
                    cutoff=cutoff, min_opacity=min_opacity)


BENCH_CORNER = (46, -27, 72)                 # the far corner of the bench scene's frustum (means reach 12 m) in units of 0.16 m
FAR = (-1900, 1300, 2500)                    # 395 m, 270 m, 520 m out at h = 0.013, where an fp32 coordinate resolves 3e-5 m
N_ZERO = 20

# name: (lo, dims, n, h, cutoff, seed, min_opacity, zero_opacities)
SCENES = {
    "bench_corner": (BENCH_CORNER, (2, 1, 1), 1000, 0.01, 3.0, 0, 1.0 / 255.0, 0),
    "bench_corner_r1.5": (BENCH_CORNER, (2, 1, 1), 1000, 0.01, 1.5, 0, 1.0 / 255.0, 0),
    "bench_corner_r6": (BENCH_CORNER, (2, 1, 1), 600, 0.01, 6.0, 0, 1.0 / 255.0, 0),
    "far_h13": (FAR, (2, 1, 1), 1000, 0.013, 3.0, 0, 1.0 / 255.0, 0),
    "far_h13_z": (FAR, (1, 1, 2), 1000, 0.013, 3.0, 1, 1.0 / 255.0, 0),
    "coarse": ((0, 0, 0), (2, 1, 1), 1000, 0.05, 3.0, 0, 1.0 / 255.0, 0),
    "bench_corner_mo0": (BENCH_CORNER, (2, 1, 1), 1000, 0.01, 3.0, 0, 0.0, N_ZERO),
    # (1600, not 1000: min_opacity = 0.5 removes a third of the Gaussians, and every list must still span three LDS batches)
    "bench_corner_mo.5": (BENCH_CORNER, (2, 1, 1), 1600, 0.01, 3.0, 0, 0.5, 0),
}
EDGES = "far_h13_edges"                      # far_h13 with brick_edge_gaussians behind its 1000
NAMES = tuple(SCENES) + (EDGES,)
QUERY = ("bench_corner", "bench_corner_r1.5", "bench_corner_r6", "far_h13")
CHANNELS = (1, 4, 5, 8, 16)                  # query's values: one walk of the list per four channels, up to 16


def _bricks(lo_units, dims):
    """The accumulate kernel's wave bricks: (unit coords, wave, per axis (first voxel, voxels, centre offset, half side))."""
    for uz in range(lo_units[2], lo_units[2] + dims[2]):
        for uy in range(lo_units[1], lo_units[1] + dims[1]):
            for ux in range(lo_units[0], lo_units[0] + dims[0]):
                for w in range(4):
                    yield (ux, uy, uz), w, ((ux * 16 + 8 * (w & 1), 8, 4.0, 3.5), (uy * 16 + 8 * (w >> 1), 8, 4.0, 3.5),
                                            (uz * 16, 16, 8.0, 7.5))


def brick_edge_gaussians(lo_units, dims, h, cutoff, steps=40):
    """Plates that each reach ONE voxel, the outermost of a wave's brick along the plate's thin axis, from beyond it -- and only
    just: what the brick test's slack is there for.  The kernel has the brick as fl(centre) +- fl(half side) and the voxel as
    fl(position), three roundings of half an ulp of the coordinate each (3e-5 m at 400 m); with 1 / s = 2500 that is 0.04 in
    the plate's own metric, twenty times the test's relative margin of 2^-16.  For every brick, axis and side whose roundings
    put the voxel `delta` >= 0.4 ulp OUTSIDE the brick as the kernel has it: a plate (identity quaternion, 0.004 in its plane,
    opacity 0.9) with its mean `steps` ulp beyond the voxel's centre and s = (steps ulp + delta / 2) / r along the axis, so the
    voxel sits delta / 2 inside the cut-off (a term of about 0.06 o exp(-r^2 / 2), a hundredth of its m away from r^2) and the
    brick, without the slack, delta / 2 outside.  (means, scales, cases [(axis, side, unit, wave, voxel index)])."""
    hf, means, scales, cases = F(h), [], [], []
    for unit, w, axes in _bricks(lo_units, dims):
        for a in range(3):
            first, n, off, half = axes[a]
            for side in (-1, 1):
                b = F(F(first) + F(off)) * hf
                e = F(F(first + (n - 1 if side > 0 else 0)) + F(0.5)) * hf
                delta = side * (float(e) - (float(b) + side * float(F(half) * hf)))
                ulp = float(np.spacing(np.abs(e)))
                mu_a = F(float(e) + side * steps * ulp)
                if delta < 0.4 * ulp or float(mu_a) != float(e) + side * steps * ulp:
                    continue
                local = [axes[c][0] + axes[c][1] // 2 - 1 for c in range(3)]          # (a voxel in the middle of the brick)
                local[a] = first + (n - 1 if side > 0 else 0)
                mu = [F(F(v) + F(0.5)) * hf for v in local]
                mu[a] = mu_a
                sc = [0.004, 0.004, 0.004]
                sc[a] = (steps * ulp + 0.5 * delta) / cutoff
                l = [local[c] - 16 * unit[c] for c in range(3)]
                means.append(mu)
                scales.append(sc)
                cases.append((a, side, unit, w, l[0] + 16 * l[1] + 256 * l[2]))
    return np.array(means, F), np.array(scales, F), cases


def build(name):
    if name == EDGES:
        lo, dims, n, h, cutoff = SCENES["far_h13"][:5]
        base = build("far_h13")
        mu, sc, _ = brick_edge_gaussians(lo, dims, h, cutoff)
        quats = np.tile(np.array([[1, 0, 0, 0]], F), (len(mu), 1))
        return S._scene(np.concatenate([base["means"], mu]), np.concatenate([base["quats"], quats]),
                        np.concatenate([base["scales"], sc]), np.concatenate([base["opacities"], np.full(len(mu), 0.9, F)]),
                        bounds=base["bounds"], h=h, cutoff=cutoff)
    lo, dims, n, h, cutoff, seed, mo, zeros = SCENES[name]
    return workload(lo, dims, n, h, cutoff, seed, min_opacity=mo, zero_opacities=zeros)


def edge_cases():
    """EDGES' plates: [(g, axis, side, map index, wave, voxel index)]."""
    lo, dims, n, h, cutoff = SCENES["far_h13"][:5]
    cases = brick_edge_gaussians(lo, dims, h, cutoff)[2]
    return [(n + i, a, side, (u[0] - lo[0]) + dims[0] * ((u[1] - lo[1]) + dims[1] * (u[2] - lo[2])), w, v)
            for i, (a, side, u, w, v) in enumerate(cases)]


def brick_test_skips(R, g, m, wave, slack=True):
    """The accumulate kernel's sub-brick test for record g and a wave of map unit m, in its fp32 operations (the fused
    multiply-adds restated in fp64 and rounded once: the products are exact there); slack=False: without the 2^-20 pad."""
    nx, ny = int(R.dims[0]), int(R.dims[1])
    ux, uy, uz = m % nx + int(R.lo[0]), (m // nx) % ny + int(R.lo[1]), m // (nx * ny) + int(R.lo[2])
    vs = R.h
    bx, by = F(F(ux * 16 + 8 * (wave & 1)) + F(4)) * vs, F(F(uy * 16 + 8 * (wave >> 1)) + F(4)) * vs
    bz = F(F(uz * 16) + F(8)) * vs
    pad = F(9.5367431640625e-7) * F(F(F(np.abs(bx) + np.abs(by)) + np.abs(bz)) + F(16) * vs) if slack else F(0)
    hx, hz = F(F(3.5) * vs + pad), F(F(7.5) * vs + pad)
    rec = R.records[g]
    c = np.array([bx - rec[0], by - rec[1], bz - rec[2]], F).astype(np.float64)
    half = np.array([hx, hx, hz], np.float64)
    A = rec[3:12].reshape(3, 3).astype(np.float64)

    def fma3(row, v):                                     # fma(row[2], v[2], fma(row[1], v[1], fl(row[0] v[0])))
        return F(row[2] * v[2] + float(F(row[1] * v[1] + float(F(row[0] * v[0])))))

    for a in range(3):
        p, wd = fma3(A[a], c), fma3(np.abs(A[a]), half)
        if np.abs(p) > F(F(R.r + wd) * F(1.0000152587890625)):
            return True
    return False


def rel(got, ref):
    """The standing rule's err: max |got - ref| / max |ref| over everything."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)) if ref.size else 0.0


def rel_local(got, ref, scale):
    """The local-scale rule's err: max over the entries with scale > 0 of |got - ref| / scale; an entry with scale 0 (no Gaussian
    within a thousandth of its cut-off) must be exactly 0."""
    got, ref, scale = (np.asarray(v, np.float64) for v in (got, ref, scale))
    pos = scale > 0
    assert not np.any(got[~pos]), "a non-zero value where no Gaussian reaches"
    return float((np.abs(got - ref)[pos] / scale[pos]).max()) if pos.any() else 0.0


def bound(e32):
    return min(8.0 * max(e32, 2.0 ** -23), 1e-4)


@functools.lru_cache(maxsize=None)
def scale_map(name):
    """Oracle.scale at the voxel centres of every unit of the map [n_map,4096] (the positions of S.oracle_map)."""
    c, _ = S.restated(name).map_voxel_centres()
    return S.oracle(name).scale(c.reshape(-1, 3)).reshape(c.shape[:2])


@functools.lru_cache(maxsize=None)
def shell_map(name):
    """bool [n_map,4096]: the voxels where the oracle puts a Gaussian OF THE UNIT'S LIST within |m - r^2| <= SHELL r^2.  Only
    there may the kernel that skips sub-bricks and the one that does not differ: a term next to its cut-off, where it vanishes,
    may fall on either side of `m < r^2` in a test whose rounding differs."""
    R, O = S.restated(name), S.oracle(name)
    c, _ = R.map_voxel_centres()
    out = np.zeros(c.shape[:2], bool)
    for m, lst in R.lists.items():
        t = O.terms(c[m])[1][:, np.isin(O.ids, lst)]
        out[m] = (np.abs((t * t).sum(-1) - O.r2) <= SHELL * O.r2).any(1)
    return out


# ------------------------------------------------------------------------------------------------------------ query
def _faces(R, rng, per_axis=96):
    """Points with one coordinate exactly on a voxel face k h or a unit face k L (fp32 products, the map's own outer faces among
    them; k is negative where the map's lo is), the other two inside the map; then the same points with that coordinate one
    ulp below and one ulp above."""
    lo_w, hi_w = R.lo * float(R.L), (R.lo + R.dims) * float(R.L)
    rows = []
    for a in range(3):
        kv = rng.integers(R.lo[a] * 16, (R.lo[a] + R.dims[a]) * 16 + 1, per_axis)
        ku = np.arange(R.lo[a], R.lo[a] + R.dims[a] + 1)
        on = np.concatenate([kv.astype(F) * R.h, ku.astype(F) * R.L, (ku * 16).astype(F) * R.h])
        p = rng.uniform(lo_w, hi_w, (len(on), 3)).astype(F)
        for v in (on, np.nextafter(on, F(-np.inf)), np.nextafter(on, F(np.inf))):
            q = p.copy()
            q[:, a] = v
            rows.append(q)
    return np.concatenate(rows)


@functools.lru_cache(maxsize=None)
def query_set(name):
    """The points of the query test (fp32) with the oracle and the restatement at them, computed once: a sample of voxel
    centres, 2048 random points inside the map, and the face points; values [N,16]; in_map: the points whose voxel the
    restatement puts inside the map (all but the face points on the map's outer faces or an ulp beyond them: the field ends
    there, the oracle, which knows no bounds, does not)."""
    R, O = S.restated(name), S.oracle(name)
    rng = np.random.default_rng(23)
    centres = R.voxel_centres().reshape(-1, 3).astype(F)
    centres = centres[rng.choice(len(centres), 2048, replace=False)]
    lo_w, hi_w = R.lo * float(R.L), (R.lo + R.dims) * float(R.L)
    inside = rng.uniform(lo_w, hi_w, (2048, 3)).astype(F)
    faces = _faces(R, rng)
    pts = np.concatenate([centres, inside, faces])
    values = rng.uniform(-1.0, 2.0, (len(S.scene(name)["means"]), max(CHANNELS))).astype(F)
    p64 = pts.astype(np.float64)
    return dict(pts=pts, values=values, in_map=R.map_index(pts) >= 0, oracle=O.evaluate(p64, values), scale=O.scale(p64), restated=R.query(pts, values),
                sets=(("voxel centres", slice(0, 2048)), ("random points", slice(2048, 4096)), ("face points", slice(4096, None))))
