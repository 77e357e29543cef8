"""GPU: the rasterizer call's layout against what the calls really take from their arena slots -- the reserved figure IS
the demand, in every form of the call -- and the rule that a plan is cached only after a build that the slot served whole."""
import pytest
import torch

from helpers import upstream

pytestmark = pytest.mark.gpu
N, W, H, F = 3000, 96, 64, 13


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from collab_splats_amd import load_library
    load_library()
    return torch.device("cuda:0")


def _call(dev, cams=1, grad=True, features=False, seed=5, **kw):
    """(step, leaves): ``step()`` runs one forward (+ backward) of the reference's call and returns the five images."""
    from collab_splats_amd import rasterization
    from collab_splats_amd.synthetic import random_scene, view_matrix
    sc = random_scene(N, W, H, seed=seed)
    leaves = [sc[k].to(dev).requires_grad_(grad) for k in ("means", "quats", "log_scales", "opacity_logits", "sh")]
    f_leaf = torch.rand(N, F, generator=torch.Generator().manual_seed(seed + 1)).to(dev).requires_grad_(grad) if features else None
    V = torch.cat([view_matrix(v) for v in range(cams)]).to(dev)
    K = sc["Ks"].repeat(cams, 1, 1).to(dev)
    cd = 4 + (F if features else 0)
    ups = [u.to(dev) for u in upstream([(cams, H, W, cd), (cams, H, W, 1), (cams, H, W, 1), (cams, H, W, 1), (cams, H, W, 3)],
                                       dtype=torch.float32)]
    kw = dict(dict(sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased", return_depth_normal=True, scales_are_log=True,
                   opacities_are_logit=True, features=f_leaf), **kw)

    def forward():
        for l in leaves + ([f_leaf] if f_leaf is not None else []):
            l.grad = None
        return rasterization(*leaves, V, K, W, H, **kw)

    def backward(out):
        torch.autograd.backward(list(out[:5]), ups)
    return forward, backward


CASES = {
    "grad": dict(),
    "absgrad": dict(absgrad=True),
    "no_grad": dict(grad=False),
    "features_lazy": dict(features=True, lazy="1"),
    "features_eager": dict(features=True, lazy="0"),
    "front_only": dict(front="1"),
    "two_cameras": dict(cams=2),
}


@pytest.mark.parametrize("case", list(CASES))
def test_reserved_figure_is_the_demand_of_the_call(dev, monkeypatch, case):
    """From an empty arena, three training steps: no take ever leaves its slot and no slot is regrown, and whenever a call
    reserves -- the forward on every build, the backward on its ring's first call -- the slot's demand afterwards is exactly
    the reserved figure (a step whose capacity fell short takes a second set of lists and is not counted)."""
    from collab_splats_amd import arena, ops
    spec = dict(CASES[case])
    monkeypatch.setattr(ops, "LAZY_SH", spec.pop("lazy", ops.LAZY_SH))
    monkeypatch.setattr(ops, "FRONT_ONLY", spec.pop("front", ops.FRONT_ONLY))
    grad = spec.get("grad", True)
    forward, backward = _call(dev, **spec)
    reserved = []
    real = arena.Carver.reserve

    def reserve(self, nbytes):
        reserved.append((self, int(nbytes)))
        real(self, nbytes)
    monkeypatch.setattr(arena.Carver, "reserve", reserve)
    arena.reset()
    before, checked = dict(arena.STATS), {"fwd": 0, "bwd": 0}
    for step in range(3):
        for phase in ("fwd", "bwd") if grad else ("fwd",):
            del reserved[:]
            redo = ops.PATH_STATS["capacity_redo"]
            if phase == "fwd":
                out = forward()
            else:
                backward(out)
            for cv, nbytes in reserved:
                assert cv.slot is not None, (phase, step)
                print(case, phase, step, "reserved", nbytes, "demand", cv.slot.demand, "slot", cv.slot.size)
                if ops.PATH_STATS["capacity_redo"] == redo:
                    assert cv.slot.demand == nbytes, (phase, step)
                    checked[phase] += 1
        if case == "front_only":
            assert out[5]["flatten_ids"].numel() > 0                 # (the lists are completed on access: still readable)
        del out
    torch.cuda.synchronize()
    assert arena.STATS["fallbacks"] == before.get("fallbacks", 0) and arena.STATS["regrown"] == before.get("regrown", 0)
    assert checked["fwd"] >= 1 and checked["bwd"] >= int(grad), checked


def test_no_plan_is_cached_after_a_build_that_left_its_slot(dev, monkeypatch):
    """A cached plan holds raw pointers into its slot.  With the layout's demand one array short and slots of exactly the
    demanded size, the last take of every build falls back to the allocator: such a call runs as ever -- the same images bit
    for bit -- but leaves no plan behind, forward or backward."""
    from collab_splats_amd import arena, ops
    forward, backward = _call(dev, seed=9, absgrad=True)

    def steps(n):
        imgs = []
        for _ in range(n):
            out = forward()
            out[5]["means2d"].retain_grad()
            backward(out)
            imgs.append([t.detach().clone() for t in out[:5]])
            del out
        torch.cuda.synchronize()
        return imgs

    arena.reset()
    ref = steps(3)
    assert any(s.plans for r in arena._RINGS.values() for s in r.slots)             # (the unpatched loop does cache plans)
    arena.reset()
    real = ops._demand
    monkeypatch.setattr(ops, "_demand", lambda takes: real(takes[:-1]))
    monkeypatch.setattr(arena.Ring, "_padded", staticmethod(lambda n: int(n)))
    monkeypatch.setattr(arena.Carver, "done", lambda self: None)                   # (the rings never learn the real demand)
    before = dict(arena.STATS), dict(ops.PATH_STATS)
    got = steps(3)
    assert arena.STATS["fallbacks"] - before[0].get("fallbacks", 0) >= 6           # one take per build, forward and backward
    assert arena._RINGS and all(s.size < s.demand and not s.plans for r in arena._RINGS.values() for s in r.slots)
    assert ops.PATH_STATS["forward_plan_hit"] == before[1].get("forward_plan_hit", 0)
    assert ops.PATH_STATS["backward_plan_hit"] == before[1].get("backward_plan_hit", 0)
    for a, b in zip(got, ref):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    arena.reset()
