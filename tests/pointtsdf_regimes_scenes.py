"""Scenes for the regimes of the point-cloud TSDF fusion that the reference workload reaches and the scenes of
pointtsdf_scenes.py, as tests/test_pointtsdf_gpu.py uses them, do not: voxel sizes and truncations
other than 0.02 / 0.06, a sphere at the workload's voxel 0.01 at the world origin and 5210 voxels out, ray bundles up to 4e6
voxels out, rays of 400 to 700 voxels, rays that end or start within a voxel of the padded unit map's edge, a bounds box cut
through every face, fans of exactly one and two pieces of the accumulate kernel, colours at the edges of the uint8 cast.
tests/test_pointtsdf_regimes_host.py asserts on the restatement that each scene is in the regime it is there for,
tests/test_pointtsdf_regimes_gpu.py compares the device with the restatement (numpy only here)."""
import functools

import numpy as np

import pointtsdf_scenes as PS
from pointtsdf_restatement import RestatedPointTSDF, make_rays, walk

F = np.float32
WORK = (0.01, 0.03)                          # the workload's voxel size and truncation


# ------------------------------------------------------------------------------------------------------- the pair count
def pairs(points, origins, vs, trunc, carve, bounds=None):
    """The distinct (ray, unit) pairs of the restatement's plain walk, after its clip: int64 [n, 4] = (the ray's position in
    the input, unit x, y, z), sorted.  What one ``integrate`` call adds to ``PointTSDFVolume.n_pairs`` is their number."""
    ref = RestatedPointTSDF(vs, trunc, carve, bounds=bounds)
    R = make_rays(points, origins, ref.vs, ref.trunc, ref.carve)
    ray, g = walk(R)
    u = g >> 4
    if ref.clip is not None:
        keep = np.all((u >= ref.clip[0]) & (u <= ref.clip[1]), 1)
        ray, u = ray[keep], u[keep]
    if not len(ray):
        return np.zeros((0, 4), np.int64)
    return np.unique(np.concatenate([R["index"][ray][:, None], u], 1), axis=0)


def pair_count(points, origins, vs, trunc, carve, bounds=None):
    return len(pairs(points, origins, vs, trunc, carve, bounds))


def held_units(x, vs):
    """The units that hold the positions x [n,3] (fp32 world), as the product places a world position: floor(x / (16 fp32(vs)))
    in float64.  A set of tuples."""
    ulen = float(F(F(vs) * F(16)))
    return set(map(tuple, np.floor(np.asarray(x, np.float64).reshape(-1, 3) / ulen).astype(np.int64).tolist()))


# ------------------------------------------------------------------------------------- 1: voxel size x truncation
VOXEL_TRUNC = (WORK, (0.02, 0.01), (0.02, 0.5), (0.013, 0.0377), (0.25, 0.75))
THIN, WIDE = VOXEL_TRUNC[1], VOXEL_TRUNC[2]  # a band thinner than a voxel; one of 25 voxels, wider than a unit


def bundle(vs, offset=0.0, n=320, seed=0):
    """pointtsdf_scenes.edge_rays with a colour per ray: (points, origins [n,3], colours [n,3])."""
    p, o = PS.edge_rays(vs, n=n, offset=offset, seed=seed)
    return p, o, np.random.default_rng(1000 + seed).random(p.shape).astype(np.float32)


# --------------------------------------------------------------------------------- 2: a sphere at the workload's voxel
SHIFT = (37.3, -52.1, 18.7)                  # metres: up to 5210 voxels of 0.01 from the world origin


@functools.lru_cache(maxsize=None)
def scan(shifted):
    """pointtsdf_scenes.sphere_scan at half its size: with voxel 0.01 the voxel geometry of the scan at 0.02."""
    return PS.sphere_scan(n=8, W=48, H=36, centre=(0.05, -0.025, 0.1), radius=0.25, dist=0.8,
                          shift=SHIFT if shifted else (0.0, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def restated_scan(shifted, carve):
    """The restatement after one call per view (shared: leave it unchanged)."""
    r = RestatedPointTSDF(*WORK, carve)
    for p, o, c in scan(shifted)["views"]:
        r.integrate(p, o, c)
    return r


def off_sphere(v, sc):
    """The largest distance of the vertices v from the scan's sphere, in world units (float64)."""
    return float(np.abs(np.linalg.norm(np.asarray(v, np.float64) - sc["centre"], axis=1) - sc["radius"]).max())


# ------------------------------------------------------------------------------------------------------- 3: far out
OFFSETS = (4051.0, -1.0e5 + 0.5, 2.0e6, -4.0e6)   # voxels; the last sits at the 2^22 skip rule, where ol keeps half a voxel


# ------------------------------------------------------------------------------------------------------ 4: long rays
def long_rays(vs=WORK[0], n=16, seed=4):
    """n rays with origins within +-5 voxels of the world origin, random directions, 400 to 700 voxels long: (points,
    origins [n,3])."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-5, 5, (n, 3))
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = o + d * rng.uniform(400, 700, (n, 1))
    return (p * vs).astype(np.float32), (o * vs).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 5: the map's padding
PAD_UNIT = (2, -3, 1)                        # the unit that holds every point (and, with carving, every origin) at offset 0
PAD_OFFSET = float(1 << 21)                  # voxels: one fp32 step of a world coordinate is 2^-9 m there, a fifth of a voxel of 0.01


def padding_rays(carve, offset=0.0, vs=WORK[0], trunc_voxels=3.0, per=17, seed=5):
    """Rays that leave the box of their points and origins only within the padding of ``PointTSDFVolume._box_units`` (the
    points by sdf_trunc and a voxel, the origins by a voxel).  Every point lies in unit PAD_UNIT (shifted by ``offset`` voxels,
    a multiple of 16); per face of that unit, ``per`` rays of each of two groups:
    * towards the face, the far end p + trunc d less than a voxel past it (both with and without carving);
    * without carving: away from the face, the start p - trunc d less than a voxel past it, the origin two units out (no
      origin enters the map without carving);
    * with carving: the origin less than a quarter voxel inside the face (every third on the last fp32 value inside it), the
      ray pointing away from it.  These rays end well inside the unit, their points' padding included: integrated alone,
      only the origins' voxel of padding reaches past the unit.
    (points, origins [6 * 2 * per, 3], second bool [6 * 2 * per]: the ray belongs to the second or third group)."""
    rng = np.random.default_rng(seed)
    base = np.asarray(PAD_UNIT, np.float64) * 16 + offset
    P, O, G = [], [], []
    for a in range(3):
        for s in (1.0, -1.0):
            face = base[a] + (16.0 if s > 0 else 0.0)
            for group in (0, 1):
                for j in range(per):
                    d = rng.uniform(-0.25, 0.25, 3) if group == 0 else rng.uniform(-0.1, 0.1, 3)
                    d[a] = s if group == 0 else -s
                    d /= np.linalg.norm(d)
                    x = base + (rng.uniform(5.0, 11.0, 3) if group == 0 else rng.uniform(6.0, 10.0, 3))
                    if group == 0:                                              # x: the far end
                        x[a] = face + s * rng.uniform(0.02, 0.98)
                        p = x - trunc_voxels * d
                        o = p - rng.uniform(4.0, 8.0) * d
                    elif not carve:                                             # x: the start
                        x[a] = face + s * rng.uniform(0.02, 0.98)
                        p = x + trunc_voxels * d
                        o = x - d * (25.0 / abs(d[a]))
                    else:                                                       # x: the origin
                        x[a] = face - s * (0.0 if j % 3 == 0 else rng.uniform(0.0, 0.25))   # (every third ON the face)
                        o = x
                        p = o + rng.uniform(6.0, 9.0) * d
                    P.append(p)
                    O.append(o)
                    G.append(group == 1)
    P, O = (np.array(P) * vs).astype(np.float32), (np.array(O) * vs).astype(np.float32)
    if carve:
        # The cast may have put an origin of the third group on or beyond its face.  Step it back, an fp32 step at a time,
        # until the product's own rule (held_units) places it in the points' unit: the origins closest to a face are then
        # the closest that fp32 has, and no unit but the points' holds an origin.
        ulen, home = float(F(F(vs) * F(16))), base / 16
        for a in range(3):
            for s in (1.0, -1.0):                                               # (below the unit: step up; above it: down)
                out = (np.floor(O[:, a].astype(np.float64) / ulen) - home[a]) * s < 0
                while out.any():
                    O[out, a] = np.nextafter(O[out, a], F(s * np.inf))
                    out = (np.floor(O[:, a].astype(np.float64) / ulen) - home[a]) * s < 0
    return P, O, np.array(G)


# -------------------------------------------------------------------------------------- 6: bounds through every face
BOUNDS_VS = 0.02
BOUNDS_VOXELS = ((-6.5, -4.5, -7.5), (9.5, 12.5, 5.5))   # strictly inside the bundle, aligned to no unit: the map is units -1 .. 0
BOUNDS_SEEDS = (0, 1)                        # the bundle of the first call and of the second


def bounds_box():
    return (np.asarray(BOUNDS_VOXELS, np.float64) * BOUNDS_VS).tolist()


def bounds_bundle(k):
    return bundle(BOUNDS_VS, n=640, seed=BOUNDS_SEEDS[k])


def map_entries(points, origins, vs, trunc, carve, bounds):
    """How each ray of the restatement's plain walk meets the clipped map: (started_inside, never_inside, crosses bool [n]
    -- crosses: the walk has voxels inside and outside --, first int64 [n,3]: the first voxel of the walk inside the map,
    where there is one), n the rays of the input (a skipped ray counts as never inside), and the map's voxel box (lo, hi
    inclusive)."""
    ref = RestatedPointTSDF(vs, trunc, carve, bounds=bounds)
    R = make_rays(points, origins, ref.vs, ref.trunc, ref.carve)
    ray, g = walk(R)                                                             # (rays step side by side: in walk order per ray)
    inside = np.all(((g >> 4) >= ref.clip[0]) & ((g >> 4) <= ref.clip[1]), 1)
    n = len(np.asarray(points).reshape(-1, 3))
    started, never, first = np.zeros(n, bool), np.ones(n, bool), np.zeros((n, 3), np.int64)
    seen = np.zeros(len(R["index"]), bool)
    for k in np.argsort(ray, kind="stable"):
        r = ray[k]
        i = R["index"][r]
        if inside[k] and never[i]:
            never[i], first[i], started[i] = False, g[k], not seen[r]
        seen[r] = True
    crosses = ~never & (np.bincount(R["index"][ray[~inside]], minlength=n) > 0)
    return started, never, crosses, first, (ref.clip[0] * 16, ref.clip[1] * 16 + 15)


# --------------------------------------------------------------------------------- 7: pieces of the accumulate kernel
PIECE = 8192                                 # rays of a unit's list per workgroup (pointtsdf.hip kChunk)
FAN_VS, FAN_TRUNC = 0.02, 0.06
FANS = (PIECE, PIECE + 1, 2 * PIECE)         # one full piece (plain flush), a full piece and one ray, two full pieces
FAN_VOXEL = 2 | (4 << 4) | (7 << 8)          # the origin's voxel in unit (0, 0, 0)


# ------------------------------------------------------------------------------------- 8: colours at the cast's edges
EDGE_COLOURS = (-0.5, 0.0, 0.5 / 255, 1.0 / 255, 0.999999, 1.0, 1.5, np.nan, np.inf, -np.inf)
EDGE_U8 = (0, 0, 0, 1, 254, 255, 255, 0, 255, 0)   # uint8(rgb * 255) in fp32: truncated, clamped, NaN to 0


def edge_colours(n):
    """[n,3] fp32: ray i's channel k takes EDGE_COLOURS[(i + 3 k) % 10]."""
    i = (np.arange(n)[:, None] + 3 * np.arange(3)[None]) % len(EDGE_COLOURS)
    return np.asarray(EDGE_COLOURS, np.float32)[i]
