"""Ray sets for the level-set search on the scenes of density_scenes.py, the fp64 search on them
(computed once), and the small meshes of the smoothing tests."""
import functools

import numpy as np

import density_scenes as S
import levelset_restatement as LR

F = np.float32
LEVELS = (0.1, 0.3, 0.5)
RES = 32
FOV_DEG = 50.0

# scene -> (eye, target, t0, t1): a 32 x 32 pinhole fan, pixel centres (i + 1/2) / 32 * 2 - 1, 50 degrees, up = +y; the long
# rays span 3 to 6 units each, so one wave holds several unit groups
LONG = {"random": ((0.64, 0.7, -0.9), (0.64, 0.64, 0.64), 0.8, 2.4),
        "single": ((0.32, 0.32, -0.5), (0.32, 0.32, 0.32), 0.3, 1.3),
        "negative": ((0.05, 0.0, -0.8), (0.0, 0.0, 0.0), 0.4, 1.2),
        "tilted_disc": ((0.11, 0.05, -0.9), (0.11, 0.05, -0.07), 0.4, 1.3)}
# the fp64 oracle's hits per level (0.1, 0.3, 0.5) on the long sets
HITS = {"random": (800, 137, 8), "single": (256, 124, 76), "negative": (329, 144, 65), "tilted_disc": (513, 220, 98)}


def fan(eye, target, res=RES, fov_deg=FOV_DEG):
    """(origins [res^2,3], unit dirs [res^2,3]) fp32, rows of pixels from the top, x fastest."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    c = (np.arange(res) + 0.5) / res * 2.0 - 1.0
    x, y = np.meshgrid(c, -c)
    k = np.tan(np.radians(fov_deg) / 2.0)
    d = fwd[None, :] + k * x.reshape(-1, 1) * right[None, :] + k * y.reshape(-1, 1) * up[None, :]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile(eye.astype(F), (res * res, 1)), d.astype(F)


@functools.lru_cache(maxsize=None)
def long_set(name):
    eye, target, t0, t1 = LONG[name]
    o, v = fan(eye, target)
    m = o.shape[0]
    return dict(origins=o, dirs=v, t0=np.full(m, t0, F), t1=np.full(m, t1, F))


@functools.lru_cache(maxsize=None)
def long_oracle(name):
    """The fp64 search on the long set at LEVELS."""
    r = long_set(name)
    return LR.search(LR.oracle_density(S.oracle(name), S.restated(name)), r["origins"], r["dirs"], r["t0"], r["t1"], LEVELS)


@functools.lru_cache(maxsize=None)
def short_set(name):
    """The long set's rays re-centred on their own fp64 hit at level 0.3 (the rays that hit it): t0 = t - 0.067, t1 = t + 0.093:
    a short ray touches one or two units."""
    r, O = long_set(name), long_oracle(name)
    hit = O["hit"][1]
    t = O["t"][1][hit]
    return dict(origins=r["origins"][hit], dirs=r["dirs"][hit], t0=(t - 0.067).astype(F), t1=(t + 0.093).astype(F))


def edge_rays():
    """Rays on the `random` scene (h = 0.02, map [0, 1.28]^3) that take the search's side paths: name -> dict."""
    h16 = float(F(S.H) * F(16))
    base = long_set("random")
    one = lambda o, v, t0, t1: dict(origins=np.array([o], F), dirs=np.array([v], F), t0=np.array([t0], F), t1=np.array([t1], F))  # noqa: E731
    first = lambda m: {k: a[300:300 + m].copy() for k, a in base.items()}                                                     # noqa: E731
    out = {f"partial_workgroup_{m}": first(m) for m in (1, 3, 5)}
    out["in_a_unit_face"] = one((0.1, h16, 0.05), (0.6, 0.0, 0.8), 0.0, 1.4)              # p_y = 16 h exactly, all along
    out["leaving_the_map"] = one((0.64, 0.64, 0.9), (0.0, 0.0, 1.0), 0.0, 1.5)
    out["outside_the_map"] = one((3.0, 3.0, 3.0), (1.0, 0.0, 0.0), 0.0, 2.0)
    O = long_oracle("random")                                                             # starting inside level 0.1: t0 just
    hit = O["hit"][0]                                                                     # behind the first crossing
    out["starting_inside"] = dict(origins=base["origins"][hit], dirs=base["dirs"][hit], t0=(O["t"][0][hit] + 0.01).astype(F),
                                  t1=base["t1"][hit])
    out["t1_below_t0"] = one((0.64, 0.7, -0.9), (0.0, 0.0, 1.0), 1.5, 1.0)
    out["t1_equals_t0"] = one((0.64, 0.7, -0.9), (0.0, 0.0, 1.0), 1.5, 1.5)
    out["nan_origin"] = one((np.nan, 0.7, -0.9), (0.0, 0.0, 1.0), 0.8, 2.4)
    long37 = {k: a[:256].copy() for k, a in base.items()}                                 # |v| = 3.7: t in units of |v|
    long37["dirs"] = (long37["dirs"] * F(3.7)).astype(F)
    long37["t0"], long37["t1"] = (long37["t0"] / F(3.7)).astype(F), (long37["t1"] / F(3.7)).astype(F)
    out["unnormalised_dirs"] = long37
    return out


def unallocated_rays(name="tilted_disc"):
    """Rays that stay inside units of the map that no Gaussian reaches (one per such unit, along x through its centre)."""
    R = S.restated(name)
    c, alloc = R.map_voxel_centres()
    assert (~alloc).sum() >= 8
    centres = c[~alloc].mean(1)
    m = len(centres)
    return dict(origins=(centres - [0.1, 0.0, 0.0]).astype(F), dirs=np.tile(np.array([[1.0, 0.0, 0.0]], F), (m, 1)),
                t0=np.zeros(m, F), t1=np.full(m, 0.2, F))


# ------------------------------------------------------------------------------------------------------------ meshes
def tetrahedron():
    """Regular: every edge has length 2 sqrt(2); closed."""
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], F)
    t = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    return v, t


def grid_patch(n=3, isolated=True):
    """An n x n patch of unit squares in z = 0, two triangles a square, the centre lifted; with `isolated` one more vertex that
    no triangle names."""
    x, y = np.meshgrid(np.arange(n), np.arange(n))
    v = np.stack([x.ravel(), y.ravel(), np.zeros(n * n)], 1).astype(F)
    v[(n // 2) * n + n // 2, 2] = 1.0
    t = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            t += [[a, a + 1, a + n], [a + 1, a + n + 1, a + n]]
    if isolated:
        v = np.concatenate([v, np.array([[5.0, 5.0, 5.0]], F)])
    return v, np.array(t, np.int32)


def bumpy_sphere(n_lat=12, n_lon=17, seed=4):
    """A closed, irregular mesh of a few hundred vertices with a repeated triangle and a degenerate one (corner repeated):
    the gather must meet every neighbour once and never the vertex itself."""
    rng = np.random.default_rng(seed)
    v = [[0.0, 0.0, 1.0]]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            v.append([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    v.append([0.0, 0.0, -1.0])
    v = np.array(v) * (1.0 + 0.1 * rng.standard_normal((len(v), 1)))
    t = []
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon                                   # noqa: E731
    for j in range(n_lon):
        t.append([0, ring(1, j), ring(1, j + 1)])
        t.append([len(v) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)])
        for i in range(1, n_lat - 1):
            t += [[ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)], [ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)]]
    t += [t[5], [7, 7, 9]]
    return v.astype(F), np.array(t, np.int32)
