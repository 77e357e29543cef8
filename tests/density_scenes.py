"""Scenes for the Gaussian density field: the smallest at which each mechanism can fail.  Every scene is
a dict of fp32 numpy arrays (means, quats, scales, opacities), the voxel size h, optional bounds, the isos its mesh is
extracted at, and the field's cutoff and min_opacity (the defaults here).  h = 0.02 throughout: a unit is 0.32 m.  The scenes
off the defaults and at workload coordinates are density_regimes_scenes.py's; scene() knows their names too."""
import functools

import numpy as np

H = 0.02
F = np.float32
BATCH = 64                                   # records the accumulate kernel stages at a time (MISPLAT_DENSITY_BATCH)


def _quat_axis(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.radians(deg) / 2
    return np.concatenate([[np.cos(t)], np.sin(t) * a])


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def _scene(means, quats, scales, opacities, bounds=None, isos=(), h=H, cutoff=3.0, min_opacity=1.0 / 255.0):
    return dict(means=np.ascontiguousarray(means, F).reshape(-1, 3), quats=np.ascontiguousarray(quats, F).reshape(-1, 4),
                scales=np.ascontiguousarray(scales, F).reshape(-1, 3), opacities=np.ascontiguousarray(opacities, F).reshape(-1),
                h=h, bounds=bounds, isos=tuple(isos), cutoff=float(cutoff), min_opacity=float(min_opacity))


def _normalise32(q):
    """fp32 normalisation in the kernel's operation order."""
    q = np.asarray(q, F)
    n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return q / n


def idempotent_quat(seed=0, factor=3.7):
    """A generic unit quaternion q (fp32) for which fp32 normalisation is exact both ways: normalise(q) == q and
    normalise(fp32(factor q)) == q, bit for bit.  Only for such a q can an unnormalised quaternion and its normalised twin give
    the same bits; rounding decides for the others.  A deterministic search (about one candidate in fifty qualifies)."""
    rng = np.random.default_rng(seed)
    for _ in range(20000):
        q = _normalise32(rng.standard_normal(4))
        if np.array_equal(_normalise32(q), q) and np.array_equal(_normalise32(q * F(factor)), q) and np.abs(q).min() > 0.2:
            return q, q * F(factor)
    raise AssertionError("no idempotent quaternion found")


def single():
    # one isotropic Gaussian on a unit corner: its support reaches the 8 units around it, across all three faces
    L = float(F(H) * F(16))
    return _scene([[L, L, L]], [[1, 0, 0, 0]], [[0.1, 0.1, 0.1]], [1.0], isos=(0.5, 0.1))


def tilted_disc():
    # thinner than a voxel, 45 degrees about two axes: most units of its AABB miss the slabs
    q = _qmul(_quat_axis([1, 0, 0], 45), _quat_axis([0, 1, 0], 45))
    return _scene([[0.11, 0.05, -0.07]], [q], [[0.2, 0.2, 0.004]], [0.9])


def tiny():
    # s = 0.3 h on the centre of a voxel with local x = 15: the next voxel along x lies in the next unit, which only the
    # one-voxel pad allocates.  One voxel above iso: the mesh is an octahedron.
    return _scene([[15.5 * H, 8.5 * H, 8.5 * H]], [[1, 0, 0, 0]], [[0.3 * H] * 3], [1.0], isos=(0.5,))


def batches(n):
    # n small Gaussians inside one unit (their padded support stays inside it): one list of n entries
    rng = np.random.default_rng(100 + n)
    means = rng.uniform(0.07, 0.25, (n, 3))
    quats = rng.standard_normal((n, 4))
    scales = np.exp(rng.uniform(np.log(0.004), np.log(0.0125), (n, 3)))
    return _scene(means, quats, scales, rng.uniform(0.1, 1.0, n))


BATCH_SIZES = (1, BATCH - 1, BATCH, BATCH + 1, 3 * BATCH + 1)


def negative():
    # the map's lo is negative on every axis and the Gaussians straddle 0: floor, not truncation
    rng = np.random.default_rng(7)
    n = 12
    means = rng.uniform(-0.2, 0.2, (n, 3))
    means[0] = [-0.001, 0.001, -0.0005]
    return _scene(means, rng.standard_normal((n, 4)), np.exp(rng.uniform(np.log(0.02), np.log(0.08), (n, 3))),
                  rng.uniform(0.2, 1.0, n))


def clipped():
    # bounds of one unit: Gaussian 0 is wider than the whole map, 1 lies wholly outside (no pairs), 2 hangs over the edge
    return _scene([[0.15, 0.15, 0.15], [2.0, 2.0, 2.0], [0.3, 0.1, 0.12]], [[1, 0, 0, 0], [1, 0, 0, 0], [0.9, 0.1, 0.3, 0.2]],
                  [[0.2, 0.25, 0.2], [0.05, 0.05, 0.05], [0.05, 0.03, 0.04]], [0.7, 1.0, 0.8],
                  bounds=[[0.0, 0.0, 0.0], [0.3, 0.3, 0.3]])


def culled():
    # opacity 0, just below and just above min_opacity = 1 / 255 (0.0039216); a NaN mean; the quaternion twins (4: normalised,
    # 5: x 3.7) at one place with one shape: their records must be equal bit for bit
    qn, qu = idempotent_quat()
    means = [[0.1, 0.1, 0.1], [0.2, 0.1, 0.1], [0.1, 0.2, 0.1], [np.nan, 0.1, 0.1], [0.15, 0.18, 0.12], [0.15, 0.18, 0.12]]
    quats = [[1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], qn, qu]
    scales = [[0.05] * 3, [0.05] * 3, [0.05] * 3, [0.05] * 3, [0.06, 0.02, 0.01], [0.06, 0.02, 0.01]]
    return _scene(means, quats, scales, [0.0, 0.0039, 0.00395, 1.0, 0.5, 0.5])


def empty():
    return _scene([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2]], [[1, 0, 0, 0], [0, 0, 0, 0]], [[0.05] * 3, [0.05] * 3], [0.0, 1.0])


RANDOM_SEED = 0


def random_scene(seed=None):
    # 300 Gaussians in a 1.28 m cube: 4^3 = 64 units, 2.6e5 voxels.  Opacities are random and fall with size (large Gaussians are
    # faint, as in trained scenes): u min(1, 0.025 / max s), u uniform in [0.4, 1].  The level set 0.5 then wraps small, steep
    # Gaussians, and a seed exists (RANDOM_SEED, found by search) for which no voxel centre lies within 1e-3 of it -- what
    # the mesh test needs to count crossings from the oracle.  (With size-independent opacities some 150 of the 2.6e5 voxels
    # do, for every seed.)
    rng = np.random.default_rng(RANDOM_SEED if seed is None else seed)
    n = 300
    means = rng.uniform(0.08, 1.2, (n, 3))                       # (the bounds below still cut the large Gaussians' support)
    scales = np.exp(rng.uniform(np.log(0.01), np.log(0.15), (n, 3)))
    opac = rng.uniform(0.4, 1.0, n) * np.minimum(1.0, 0.025 / scales.max(1))
    return _scene(means, rng.standard_normal((n, 4)), scales, opac,
                  bounds=[[0.0, 0.0, 0.0], [1.27, 1.27, 1.27]], isos=(0.5,))


def wide_map(dims):
    """Seven small Gaussians in a map of dims units (the bounds give it): in the first unit, in the last and in the middle one,
    interleaved, so that every unit's list must be brought into ascending g and the map indices reach from 0 to the last.  Not
    in NAMES: the map is far too large for the oracle, only the integer structures are compared."""
    L = float(F(H) * F(16))
    d = np.asarray(dims, np.float64)
    first, mid, last = 0.5 * L * np.ones(3), (d // 2 + 0.5) * L, (d - 0.5) * L
    rng = np.random.default_rng(int(np.prod(dims)) % 1000)
    centres = np.stack([last, first, last, mid, first, last, mid])
    means = centres + rng.uniform(-0.05, 0.05, (7, 3))
    return _scene(means, rng.standard_normal((7, 4)), np.exp(rng.uniform(np.log(0.01), np.log(0.03), (7, 3))),
                  rng.uniform(0.3, 1.0, 7), bounds=[[0.0, 0.0, 0.0], ((d - 0.5) * L).tolist()])


@functools.lru_cache(maxsize=None)
def scene(name):
    if name.startswith("batches_"):
        return batches(int(name.split("_")[1]))
    own = {"single": single, "tilted_disc": tilted_disc, "tiny": tiny, "negative": negative, "clipped": clipped,
           "culled": culled, "empty": empty, "random": random_scene}
    if name in own:
        return own[name]()
    import density_regimes_scenes as RS                      # (imports this module: only here)
    return RS.build(name)


NAMES = ("single", "tilted_disc", "tiny") + tuple(f"batches_{n}" for n in BATCH_SIZES) + ("negative", "clipped", "culled",
                                                                                           "empty", "random")
MESH = tuple((n, iso) for n in ("single", "tiny", "random") for iso in scene(n)["isos"])


@functools.lru_cache(maxsize=None)
def restated(name):
    from density_restatement import Restated
    sc = scene(name)
    return Restated(sc["means"], sc["quats"], sc["scales"], sc["opacities"], sc["h"], cutoff=sc["cutoff"],
                    min_opacity=sc["min_opacity"], bounds=sc["bounds"])


@functools.lru_cache(maxsize=None)
def oracle(name):
    from density_restatement import Oracle
    sc = scene(name)
    return Oracle(sc["means"], sc["quats"], sc["scales"], sc["opacities"], cutoff=sc["cutoff"], min_opacity=sc["min_opacity"])


@functools.lru_cache(maxsize=None)
def oracle_map(name):
    """The fp64 oracle at the voxel centres of EVERY unit of the map (the fp32 positions the kernel evaluates at, widened):
    (d [n_map,4096], allocated [n_map] bool by the restatement, kmax [n_map,G'] = each participating Gaussian's largest term in
    the unit (0: none of its voxels lies inside the cut-off), ids [G'])."""
    R, O = restated(name), oracle(name)
    c, alloc = R.map_voxel_centres()
    d = np.zeros(c.shape[:2])
    kmax = np.zeros((c.shape[0], len(O.ids)))
    if len(O.ids):
        for u0 in range(0, c.shape[0], 4):
            k = O.terms(c[u0:u0 + 4].reshape(-1, 3))[0].reshape(-1, 4096, len(O.ids))
            d[u0:u0 + 4] = k.sum(2)
            kmax[u0:u0 + 4] = k.max(1)
    return d, alloc, kmax, O.ids


def to_dense(per_unit, dims):
    """[n_map,4096] (voxel i = lx + 16 ly + 256 lz, units x fastest) -> [Dz 16, Dy 16, Dx 16]."""
    dx, dy, dz = (int(v) for v in dims)
    a = np.asarray(per_unit).reshape(dz, dy, dx, 16, 16, 16)
    return a.transpose(0, 3, 1, 4, 2, 5).reshape(dz * 16, dy * 16, dx * 16)


@functools.lru_cache(maxsize=None)
def restated_map(name):
    """The restatement's fp32 field on the whole map [n_map,4096]: 0 in unallocated units."""
    R = restated(name)
    out = np.zeros((int(np.prod(R.dims)), 4096), F)
    if R.lists:
        out[np.array(sorted(R.lists))] = R.unit_fields()
    return out


def crossings(dense, iso):
    """Per axis (x, y, z) the bool array of lattice edges (voxel, voxel + 1 along the axis) whose ends lie on opposite sides of
    iso; dense is [Z,Y,X]."""
    above = dense > iso
    return [above[:, :, :-1] != above[:, :, 1:], above[:, :-1, :] != above[:, 1:, :], above[:-1, :, :] != above[1:, :, :]]
