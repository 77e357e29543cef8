"""CPU: what tests/test_lossside_gpu.py stands on -- the goldens are what a second, independent implementation computes,
they contain every kind of centre a holed render has, and the bounds the GPU tests derive are attainable (the oracle in
fp32 and torch's own fp32 Adam stay inside them)."""
import os

import numpy as np
import pytest
import torch

import lossside_restatement as lr
import test_lossside_gpu as tg

GOLD = os.path.join(os.path.dirname(__file__), "golden", "lossside_goldens.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _close(got, want, tol=1e-12):
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape
    s = np.abs(want).max() if want.size else 0.0
    return np.abs(got - want).max() <= tol * s if s > 0 else not np.any(got)


def test_goldens_hold_the_listed_cases_and_only_finite_numbers(gold):
    want = [(32, 8, 40, 37), (33, 9, 40, 37), (65, 17, 100, 80), (9, 7, 300.5, 310.25), (3, 3, 5, 5), (2, 5, 5, 5),
            (5, 2, 5, 5), (1, 1, 5, 5)]
    assert [tuple(c) for c in gold["cases"].tolist()] == want and len(want) == tg.N_CASES
    assert [tuple(gold["cases"][i][:2]) for i in gold["fused"]] == [(33, 9), (65, 17)] and len(gold["fused"]) == tg.N_FUSED
    for k, a in gold.items():
        assert np.isfinite(a).all(), k
    for i, (W, H, fx, fy) in enumerate(want):
        assert gold[f"c{i}_d1"].shape == (H, W) and gold[f"c{i}_d1"].dtype == np.float32
        assert np.allclose(gold[f"c{i}_fxfy"], [fx, fy], rtol=1e-6)     # (through the reference's fp32 field of view)
        # the reference's fp32 ray table is the formula of csrc/blend.hip's dn_point to fp32 rounding
        assert np.abs(gold[f"c{i}_rays"] - lr.ray_table(W, H, *gold[f"c{i}_fxfy"])).max() <= 4 * tg.U * max(W / fx, H / fy)
        assert (gold[f"c{i}_e32"] < 2e-6).all()                          # the reference itself in fp32: rounding level


@pytest.mark.parametrize("i", range(tg.N_CASES))
def test_numpy_restatement_reproduces_every_golden(gold, i):
    """Forward and adjoint written from the kernel's comments, in numpy fp64, against the reference's autograd run in fp64:
    1e-12 of each tensor's scale, no pixel excluded."""
    c = {k: gold[f"c{i}_{k}"] for k in ("d1", "d2", "nrm", "rays", "v_n2", "v_err", "normals2", "err", "g_d1", "g_d2", "g_nrm")}
    n2, err = lr.forward(c["d1"], c["d2"], c["nrm"], c["rays"])
    assert _close(n2, c["normals2"]) and _close(err, c["err"])
    v_d1, v_d2, v_nr = lr.adjoint(c["d1"], c["d2"], c["nrm"], c["rays"], c["v_n2"], c["v_err"])
    assert _close(v_d1, c["g_d1"]) and _close(v_d2, c["g_d2"]) and _close(v_nr, c["g_nrm"])


@pytest.mark.parametrize("j", range(tg.N_FUSED))
def test_fused_node_goldens_are_the_post_processing_plus_the_stencil_adjoint(gold, j):
    """The get_outputs goldens against oracle/camera_oracle.outputs_post under autograd plus the numpy adjoint with
    v_err alone -- the composition the GPU test uses for the runs with part of the outputs in the loss."""
    from oracle import camera_oracle as co
    i = int(gold["fused"][j])
    ins = tg._fused_inputs(gold, j, torch.float64)
    outs = co.outputs_post(*ins, torch.from_numpy(gold["bg"]))
    names = ("rgb", "depth", "median", "normals", "depth_im")
    for n, o in zip(names, outs):
        assert _close(o.detach().numpy()[0], gold[f"f{j}_o_{n}"])
    torch.autograd.backward(list(outs), [tg._fused_upstream(gold, j, n, torch.float64) for n in names])
    grads = [t.grad.numpy()[0] if t.grad is not None else np.zeros(t.shape[1:]) for t in ins]
    v_d1, v_d2, v_nr = lr.adjoint(gold[f"c{i}_d1"], gold[f"c{i}_d2"], gold[f"c{i}_nrm"], gold[f"c{i}_rays"], v_err=gold[f"f{j}_u_err"])
    grads[2], grads[3], grads[4] = grads[2] + v_d1[..., None], grads[3] + v_d2[..., None], grads[4] + v_nr
    for n, g in zip(tg.G_NAMES, grads):
        assert _close(g, gold[f"f{j}_g_{n}"]), n
    a = gold[f"f{j}_alpha"]
    hole = (gold[f"c{i}_d1"] == 0) | (gold[f"c{i}_d2"] == 0)
    assert np.array_equal(a == 0, hole) and a[~hole].min() >= 0.3 and a.max() < 1.0
    assert gold[f"f{j}_render"].shape[-1] == 4 and gold[f"f{j}_render"].min() >= -0.2 and gold[f"f{j}_render"].max() <= 1.2


@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_holed_cases_contain_every_class_of_centre(gold, i):
    W, H = int(gold["cases"][i][0]), int(gold["cases"][i][1])
    seen = set()
    for k, name in enumerate(("d1", "d2")):
        d = gold[f"c{i}_{name}"]
        a, b = lr.differences(d, gold[f"c{i}_rays"])
        a0, b0 = (a == 0).all(-1), (b == 0).all(-1)
        zero_normal = (gold[f"c{i}_normals2"][k, 1:-1, 1:-1] == 0).all(-1)
        assert np.array_equal(zero_normal, a0 | b0)                      # a zero normal comes from a hole, nothing else
        z = d == 0
        empty_nb = (z[2:, 1:-1].astype(int) + z[:-2, 1:-1] + z[1:-1, 2:] + z[1:-1, :-2])
        seen |= {"inside" for _ in [0] if (a0 & b0).any()}
        seen |= {"a=0,b!=0" for _ in [0] if (a0 & ~b0).any()}
        seen |= {"a!=0,b=0" for _ in [0] if (~a0 & b0).any()}
        seen |= {"edge" for _ in [0] if ((empty_nb == 1) & ~zero_normal).any()}
        healthy = ~zero_normal
        for tag, line in (("x=1", healthy[:, 0]), ("x=W-2", healthy[:, -1]), ("y=1", healthy[0]), ("y=H-2", healthy[-1])):
            if line.any():
                seen.add(tag)
            if (~line).any():
                seen.add(tag + " dead")
        # the 1e-12 on the upstreams sits on the zero-normal centres and nowhere else
        small = np.abs(gold[f"c{i}_v_err"][k, 1:-1, 1:-1]) < 1e-9
        assert np.array_equal(small, zero_normal)
        # holes of the listed shapes
        assert z[0, 0] and z[H - 2].all() and z[1:4, 1:4].all() and z[1, W - 2] and not z[0, W - 2] and not z[1, W - 3]
    d1, d2 = gold[f"c{i}_d1"], gold[f"c{i}_d2"]
    assert d1[1, W - 4] == 0 and d1[3, W - 4] == 0 and d1[2, W - 5] > 0 and d1[2, W - 3] > 0
    assert d2[3, W - 3] == 0 and d2[3, W - 1] == 0 and d2[2, W - 2] > 0 and d2[4, W - 2] > 0
    # (the empty row IS y = H-2: its centres have b = 0 and send their gradient sideways only; healthy centres at y = H-2 are
    # those of the 3 x 3 case and of the plane goldens)
    assert seen >= {"inside", "a=0,b!=0", "a!=0,b=0", "edge", "x=1", "x=W-2", "y=1", "y=H-2 dead"}, seen
    # border pixels receive gradient
    g = gold[f"c{i}_g_d1"]
    assert np.any(g[0]) and np.any(g[:, 0]) and np.any(g[:, -1]) and np.any(gold[f"c{i}_g_nrm"][1:-1, 1:-1])


@pytest.mark.parametrize("H,W", tg.SSIM_SIZES)
def test_render_like_ssim_images_leave_fp32_room_under_the_project_bar(H, W):
    """The oracle in fp32 against itself in fp64 on the images the GPU test uses: below 5e-5 of the gradient's max, half the
    1e-4 bar, so a kernel within 4 x of fp32 rounding... the flat regions and exact values the maker promises are there."""
    gt, pred = tg.ssim_images(H, W)
    assert gt.shape == (H, W, 3) and gt.dtype == torch.float32 and float(gt.min()) >= 0 and float(gt.max()) <= 1
    white = (gt == 1).all(-1)
    black = (gt == 0).all(-1)
    assert white[:2].all() and bool((pred[white[:, 0] & white[:, -1]] == 0).all())
    assert int(black.sum()) >= 4 and bool((pred[black] == 0).all())
    rest = ~white & ~black
    assert int((pred[rest] == 0).sum()) + int((pred[rest] == 1).sum()) > 0 or H * W < 200
    e32 = tg.ssim_e32(gt, pred, 0.2)
    print(f"ssim images {H}x{W}: e32 {e32:.3e}")
    assert e32 < 5e-5
    assert tg.ssim_e32(gt, pred, 1.0) < 5e-5


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("kind", tg.ADAM_KINDS)
def test_torch_fp32_adam_stays_inside_the_derived_one_step_bounds(kind, half):
    """If torch's own fp32 Adam left the bounds the GPU test holds the kernel to, the bounds would be wrong."""
    for k, (p, g, m, v, step, lr_) in enumerate(tg.adam_config(kind, half)):
        q = p.clone().requires_grad_(True)
        q.grad = g.clone()
        o = torch.optim.Adam([q], lr=lr_, betas=(tg.ADAM_B1, tg.ADAM_B2), eps=tg.ADAM_EPS, foreach=False)
        o.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
        o.step()
        st = o.state[q]
        assert int(st["step"]) == step
        tg.adam_check(f"torch {kind} tensor {k}", tg.adam_reference(p, g, m, v, step, lr_), p, q, st["exp_avg"], st["exp_avg_sq"])


def test_adam_configurations_cover_what_they_claim():
    numels = {n for row in tg.ADAM_NUMELS for n in row}
    assert numels == {1, 3, 4, 5, 2047, 2048, 2049, 4097, 10007 * 3}
    assert all(set(row) == {1, 2, 1000, 30000} for row in tg.ADAM_STEPS)
    for half in (0, 1):
        for p, g, m, v, step, lr_ in tg.adam_config("sparse_rows", half):
            if p.numel() > 2000:
                frac = float((g == 0).float().mean())
                assert 0.85 < frac < 0.95
                nz = g[g != 0].abs()
                assert float(nz.min()) < 1e-6 and float(nz.max()) > 1e-2 and bool(m.any()) and bool(v.any())
        for p, g, m, v, step, lr_ in tg.adam_config("tiny_1e-25", half):
            assert float((g * g).abs().max()) == 0.0 and float(g.abs().min()) > 0
