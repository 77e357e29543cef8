"""One small holed grid at vertex indices of one, two and three key bytes, for the callers of csrc/meshadj.h whose later call
names the buffer an earlier call's radix sort left its result in (the parity of radix_passes(M - 1)): Laplacian smoothing and
quadric decimation.  (The fairing and the subdivision reach the same pass counts in tests/meshfill_regimes_scenes.py: FAIR's
passes_*, SUBDIVIDE's cut_m255, cut_m256 and cut_5000_padded.)  tests/test_meshadj_host.py asserts on the restatements that each
size reaches its regime, tests/test_meshadj_gpu.py compares the device with them (references: computed once per process)."""
from __future__ import annotations

import numpy as np

import decimate_scenes as DS
from meshclean_scenes import F, sheet
from meshfill_regimes_scenes import padded, radix_passes  # noqa: F401  (re-exported)

SIZES = (200, 300, 70000)               # M: the largest key M - 1 has one, two and three bytes
N_GRID = 100
_MESHES, _REFERENCES = {}, {}


def holed_grid(M, seed=4):
    """A 10 x 10-vertex grid without its vertices 3 <= i, j < 6 (the 4 x 4 quads that touch them: one hole, 130 faces), off
    its lattice (N(0,1) 0.03 on z, uniform +- 0.03 on the x and y of the inner vertices: no two costs, no two weights equal),
    behind M - 100 unreferenced vertices.  (V, T, an attribute of width 2)."""
    if M not in _MESHES:
        V, T = sheet(9, [(2, 6, 2, 6)])
        rng = np.random.default_rng(seed)
        V = V.astype(np.float64)
        inner = ((V[:, :2] > 0) & (V[:, :2] < 1)).all(1)
        V[:, 2] += 0.03 * rng.standard_normal(len(V))
        V[:, :2] += np.where(inner[:, None], rng.uniform(-0.03, 0.03, (len(V), 2)), 0.0)
        att = rng.uniform(0, 1, (len(V), 2)).astype(F)
        _MESHES[M] = padded(V.astype(F), T, M - N_GRID, att)
    return _MESHES[M]


def decimate_reference(M):
    """(the restatement's result of halving the faces, one round_account per round)."""
    if M not in _REFERENCES:
        import decimate_restatement as R
        V, T, att = holed_grid(M)
        rounds = []
        result = R.simplify(V, T, len(T) // 2, (att,), on_round=lambda *a: rounds.append(DS.round_account(*a)))
        _REFERENCES[M] = (result, rounds)
    return _REFERENCES[M]
