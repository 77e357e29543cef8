"""GPU: the callers of csrc/meshadj.h whose sorted adjacency is named again by a later call, on the holed grid of
tests/meshadj_scenes.py at vertex indices of one, two and three key bytes (the radix sort leaves its result in the second pair
of buffers after an odd number of passes, in the first after an even one).  Decimation compares with
tests/decimate_restatement.py for equality; smoothing with tests/levelset_restatement.py as tests/test_levelset_gpu.py does.
That each size reaches its regime is asserted on the restatements, on the CPU (tests/test_meshadj_host.py)."""
import numpy as np
import pytest
import torch

import levelset_restatement as LR
import meshadj_scenes as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(x):
    return x.detach().cpu().numpy().view(np.int32)


@pytest.mark.parametrize("M", S.SIZES)
def test_smoothing_finds_its_rows_after_every_pass_count(M):
    """Two iterations and an attribute of width 2.  The bound is test_levelset_gpu.py's: one iteration adds the restatement's
    fp64 terms in its order (at most 8 neighbours here) and rounds once to fp32, so the results differ by at most one fp32 ulp
    where a value falls on a rounding boundary, 2^-23 max |x|; the second iteration is compared from the first one's own output."""
    from collab_splats_amd import smooth_laplacian
    V, T, att = S.holed_grid(M)

    def close(got, ref):
        assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref).max()
        print(M, "max error", err, "bound", 2.0 ** -23 * np.abs(ref).max())
        assert err <= 2.0 ** -23 * np.abs(ref).max()

    one = smooth_laplacian(_t(V), _t(T), 1, 0.5, attributes=(_t(att),))
    ref_v, (ref_a,) = LR.smooth_laplacian(V, T, 1, 0.5, [att])
    close(one[0], ref_v)
    close(one[1][0], ref_a)
    both = smooth_laplacian(_t(V), _t(T), 2, 0.5, attributes=(_t(att),))
    again = smooth_laplacian(_t(V), _t(T), 2, 0.5, attributes=(_t(att),))
    assert np.array_equal(_bits(both[0]), _bits(again[0])) and np.array_equal(_bits(both[1][0]), _bits(again[1][0]))
    ref2_v, (ref2_a,) = LR.smooth_laplacian(one[0].cpu().numpy(), T, 1, 0.5, [one[1][0].cpu().numpy()])
    close(both[0], ref2_v)
    close(both[1][0], ref2_a)
    pad = M - S.N_GRID
    assert np.array_equal(_bits(both[0][:pad]), V[:pad].view(np.int32)) and not np.array_equal(_bits(both[0][pad:]), V[pad:].view(np.int32))


@pytest.mark.parametrize("M", S.SIZES)
def test_decimation_names_its_tables_after_every_pass_count(M):
    from collab_splats_amd import simplify_quadric_decimation
    V, T, att = S.holed_grid(M)
    v, t, a, vm, r = simplify_quadric_decimation(_t(V), _t(T), len(T) // 2, (_t(att),))
    (rv, rt, ra, rvm, rr), _ = S.decimate_reference(M)
    print(M, "rounds", r, "restated", rr, "faces", tuple(t.shape), "restated", rt.shape)
    assert r == rr and tuple(t.shape) == rt.shape and np.array_equal(t.cpu().numpy(), rt)
    assert tuple(v.shape) == rv.shape and np.array_equal(_bits(v), rv.view(np.int32))
    assert np.array_equal(vm.cpu().numpy(), rvm)
    assert len(a) == 1 and tuple(a[0].shape) == ra[0].shape and np.array_equal(_bits(a[0]), ra[0].view(np.int32))
