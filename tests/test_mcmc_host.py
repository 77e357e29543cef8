"""CPU: the restatement of the MCMC densification (tests/mcmc_restatement.py) against the method's own identities, the scenes
of tests/mcmc_scenes.py against the launch regimes they are meant to reach, and the model's ``strategy`` switch.  The GPU
tests (tests/test_mcmc_gpu.py) hold the kernels to this restatement: bit for bit where it is integer work."""
import math

import numpy as np
import pytest
import torch

import collab_splats_amd.mcmc as mcmc
import mcmc_restatement as R
import mcmc_scenes as S


# ------------------------------------------------------------------------------------------------------------ relocation
def test_relocation_with_one_copy_changes_nothing():
    """n = 1: o' = o and D = o analytically, so s' = s."""
    o = np.array([0.005, 0.1, 0.5, 0.9, 0.99, S.RELOC_NEAR_ONE], np.float32)
    s = np.array([[1e-3, 1.0, 1e3]] * 6, np.float32)
    new_o, new_s = R.relocation(o, s, np.ones(6, np.int32))
    assert np.abs(new_o - o.astype(np.float64)).max() <= 2.0 ** -50
    assert np.abs(new_s / s.astype(np.float64) - 1).max() <= 2.0 ** -48


@pytest.mark.parametrize("n", [2, 3, 7, 51])
def test_new_opacity_composes(n):
    """n copies of o' on top of each other have the joint opacity o: 1 - (1 - o')^n = o."""
    o = np.array([0.005, 0.1, 0.5, 0.9, 0.99, S.RELOC_NEAR_ONE], np.float32)
    new_o, _ = R.relocation(o, np.ones((6, 3), np.float32), np.full(6, n, np.int32))
    joint = 1.0 - (1.0 - new_o) ** n
    assert np.abs(joint / o.astype(np.float64) - 1).max() <= 2.0 ** -40


def test_ratios_clamp_to_n_max():
    o, s = np.array([0.3], np.float32), np.ones((1, 3), np.float32)
    a, b = R.relocation(o, s, np.array([200])), R.relocation(o, s, np.array([51]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(mcmc.binomial_table().numpy(), R.binomial_table())
    assert R.binomial_table()[50, 25] == float(math.comb(50, 25)) < 2.0 ** 53


def test_fp32_restatement_agrees_with_fp64_on_the_relocation_scenes():
    """The GPU bound is 8 x the fp32 restatement's error, capped at 1e-4.  On ``grid`` that error is below 1e-4 / 8: the
    bound is built on fp32's own rounding and the cap decides nothing.  On ``near_one`` (o = 1 - 2^-20) the alternating
    sum's terms add up to (1 + o')^50 = 4e4 in absolute value at n = 51 against a sum of order 1: the fp32 sum of those rows
    loses more than two of its seven digits (at least 100 roundings of 2^-24), which is what the kernel's fp64 sum is for;
    the fp32 restatement still agrees to 1e-4, and the cap is the GPU's bound there."""
    for name, most in (("grid", 1e-4 / 8), ("near_one", 1e-4)):
        for k in (0, 1):
            e = R.rel_err(S.relocation_restated(name, True)[k], S.relocation_restated(name, False)[k])
            print(f"{name} tensor {k}: fp32 restatement error {e:.3e}")
            assert e < most
    o, s, n = S.relocation_scene("near_one")
    f32, f64 = S.relocation_restated("near_one", True)[1], S.relocation_restated("near_one", False)[1]
    assert np.isfinite(f64).all() and (f64 > 0).all()
    worst = {k: float(np.abs(f32[n == k] / f64[n == k] - 1).max()) for k in (1, 51)}
    print(f"near_one: the fp32 scales are off by {worst[1]:.3e} at n = 1 and {worst[51]:.3e} at n = 51")
    assert worst[1] <= 4 * 2.0 ** -24 and worst[51] > 100 * 2.0 ** -24


# --------------------------------------------------------------------------------------------------------------- sampler
@pytest.mark.parametrize("seed,step", [(0, 100), (1, 200), (12345, 7)])
def test_draw_frequencies_match_the_weights(seed, step):
    """Chi-square of 2^16 draws over the alive rows of the 64-row scene (d degrees of freedom: mean d, standard deviation
    sqrt(2 d)): below d + 4 sigma for these seeds.  The GPU equals the restatement bit for bit, so this needs no repeat there."""
    o = S.sample_opacities(64)
    m = 1 << 16
    idx, counts = R.sample(o, m, seed, step, S.MIN_OPACITY)
    q = R.weights(o, S.MIN_OPACITY)
    assert counts.sum() == m and not counts[q == 0].any()
    live = q > 0
    expect = m * q[live] / q.sum()
    chi2 = float(((counts[live] - expect) ** 2 / expect).sum())
    dof = int(live.sum()) - 1
    print(f"seed {seed} step {step}: chi-square {chi2:.1f} at {dof} degrees of freedom")
    assert chi2 < dof + 4 * math.sqrt(2 * dof)


def test_weights_are_exact_and_zero_rows_are_never_drawn():
    o = np.array([0.0, 1.0, 0.5, 2.0 ** -24, 2.0 ** -25, np.nan, -1.0, 0.005, 3.0], np.float32)
    assert R.weights(o).tolist() == [0, 1 << 24, 1 << 23, 1, 0, 0, 0, int(np.float32(0.005) * np.float32(2 ** 24)), 1 << 24]
    assert R.weights(o, 0.005).tolist()[7] == 0
    assert R.sample(np.zeros(5, np.float32), 3, 0, 0) is None
    idx, counts = R.sample(o, 4096, 3, 9)
    assert set(idx.tolist()) <= {1, 2, 3, 7, 8}


def test_two_streams_of_one_step_differ():
    o = S.sample_opacities(1023)
    a = R.sample(o, 65, 4, 100)[0]
    assert not np.array_equal(a, R.sample(o, 65, 4 + R.ADD_STREAM, 100)[0])
    assert not np.array_equal(a, R.sample(o, 65, 4, 101)[0])
    assert R.ADD_STREAM == mcmc._ADD_STREAM and R.N_MAX == mcmc.N_MAX


# ---------------------------------------------------------------------------------------------------------------- normals
def test_restated_normals_are_finite_and_standard():
    """2^16 Gaussians, 3 normals each, n = 196608 values.  The mean of n standard normals has standard deviation 1 / sqrt(n)
    and their sample variance sqrt(2 / n): both are held to 5 of those.  The largest value Box-Muller can return from a 24-bit
    uniform is sqrt(-2 log 2^-24) = 5.77."""
    for dtype in (np.float64, np.float32):
        z = R.normals(R.noise_words(11, 300, 1 << 16), dtype)
        n = z.size
        assert z.dtype == dtype and np.isfinite(z).all()
        assert np.abs(z).max() <= math.sqrt(2 * 24 * math.log(2)) + 1e-5
        assert abs(z.astype(np.float64).mean()) <= 5 / math.sqrt(n)
        assert abs(z.astype(np.float64).var() - 1) <= 5 * math.sqrt(2 / n)
        for a in range(3):
            for b in range(a + 1, 3):                                      # the three components are uncorrelated
                assert abs(float(np.mean(z[:, a].astype(np.float64) * z[:, b]))) <= 5 / math.sqrt(1 << 16)


def test_gate_is_zero_for_opaque_rows_and_never_nan():
    for dtype in (np.float64, np.float32):
        g = R.gate(np.array([30.0, -30.0, 0.0, -5.3, 88.0, -88.0, 200.0, -200.0], np.float32), dtype)
        assert np.isfinite(g).all() and (g >= 0).all() and (g <= 1).all()
        assert g[0] < 1e-40 and g[2] < 1e-20 and g[4] < 1e-40
        assert abs(g[1] - 1 / (1 + math.exp(-0.5))) < 1e-6                 # o -> 0: the gate's largest value, 0.62


# ------------------------------------------------------------------------------------------------------------- the scenes
def test_every_scene_reaches_its_regime():
    b = S.scan_block()
    sizes = S.sample_sizes()
    assert [S.scan_level(n) for n in sizes] == [1, 1, 1, 1, 1, 1, 2, 3]
    assert b - 1 in sizes and b in sizes and b + 1 in sizes               # one block's span +- 1
    assert min(n for n in sizes if S.scan_level(n) == 2) == b + 1         # the smallest n of each further level
    assert min(n for n in sizes if S.scan_level(n) == 3) == b * b + 1
    assert (b * b + 1 + b - 1) // b > b                                    # ... whose block totals need a second trip
    assert S.SAMPLE_DRAWS == [1, 65, 3000]
    for n in sizes[1:]:
        q = R.weights(S.sample_opacities(n), S.MIN_OPACITY)
        q0 = R.weights(S.sample_opacities(n))
        assert q[0] == 0 and q[-1] == 0 and q[n // 3] == 0 and q[n // 2] == 0 and (q > 0).any()     # prefix, suffix, interior
        assert (q0 == 0).any() and (q0 > q).any()                                               # exact zeros; the threshold kills more
    noise = S.noise_sizes()
    assert noise[:4] == [1, 64, 65, 257] and noise[4] > S.stream_span() and all(n <= S.stream_span() for n in noise[:4])
    logits, log_scales, quats = S.noise_scene(257)
    assert (logits == 30).any() and (logits == -30).any()
    assert log_scales.max() - log_scales.min() > math.log(1e5)
    lengths = np.linalg.norm(quats, axis=1)
    assert lengths.max() / lengths.min() > 100
    o, s, n = S.relocation_scene("grid")
    assert sorted(set(n.tolist())) == S.RELOC_RATIOS and s.max() / s.min() >= 1e6
    assert np.float32(S.RELOC_NEAR_ONE) == 1 - 2.0 ** -20 < 1


# ---------------------------------------------------------------------------------------------------------- model, C ABI
def _tiny_model(**kw):
    from collab_splats_amd import radegs
    n = 8
    cfg = radegs.RadegsModelConfig(**kw)
    return radegs.RadegsModel(cfg, torch.zeros(n, 3), torch.zeros(n, 3), torch.ones(n, 4), torch.zeros(n), torch.zeros(n, 1, 3),
                              torch.zeros(n, 15, 3))


def test_unknown_strategy_raises():
    from collab_splats_amd import radegs
    with pytest.raises(ValueError, match="strategy"):
        radegs.RadegsModelConfig(strategy="bogus")
    cfg = radegs.RadegsModelConfig()
    cfg.strategy = "bogus"
    with pytest.raises(ValueError, match="strategy"):
        radegs.RadegsModel(cfg, *(torch.zeros(1, k) for k in (3, 3, 4)), torch.zeros(1), torch.zeros(1, 1, 3), torch.zeros(1, 15, 3))


def test_default_config_builds_the_default_strategy_and_keeps_the_loss_keys():
    import collab_splats_amd as m
    model = _tiny_model(ssim_lambda=0.0).train()                          # (plain L1: the SSIM term has no CPU path)
    assert m.radegs.RadegsModelConfig().strategy == "default"
    assert type(model.strategy) is m.DefaultStrategy and set(model.strategy_state) == {"grad2d", "count", "scene_scale"}
    rgb = torch.rand(4, 4, 3)
    losses = model.get_loss_dict({"rgb": rgb}, {"image": torch.rand(4, 4, 3)})
    assert set(losses) == {"main_loss", "scale_reg"} and float(losses["scale_reg"]) == 0.0


def test_mcmc_config_builds_the_relocation_strategy_and_adds_the_regularisers():
    import collab_splats_amd as m
    model = _tiny_model(strategy="mcmc", cap_max=1234, noise_lr=7.0, ssim_lambda=0.0).train()
    assert isinstance(model.strategy, m.RelocationStrategy) and model.strategy.cap_max == 1234 and model.strategy.noise_lr == 7.0
    assert tuple(model.strategy_state["binoms"].shape) == (51, 51)
    model.strategy.check_sanity(model.gauss_params, {})
    model.strategy.step_pre_backward(model.gauss_params, {}, model.strategy_state, 0, {})       # no means2d needed
    losses = model.get_loss_dict({"rgb": torch.rand(4, 4, 3)}, {"image": torch.rand(4, 4, 3)})
    assert set(losses) == {"main_loss", "scale_reg", "opacity_reg"}
    assert float(losses["opacity_reg"].detach()) == pytest.approx(0.01 * 0.5)
    assert float(losses["scale_reg"].detach()) == pytest.approx(0.01 * 1.0)
    assert set(model.eval().get_loss_dict({"rgb": torch.rand(4, 4, 3)}, {"image": torch.rand(4, 4, 3)})) == {"main_loss", "scale_reg"}
    d = m.RelocationStrategy()
    assert (d.cap_max, d.noise_lr, d.refine_start_iter, d.refine_stop_iter, d.refine_every, d.min_opacity, d.verbose, d.seed) == \
        (1_000_000, 5e5, 500, 25_000, 100, 0.005, False, 0)


def test_the_placeholder_still_raises():
    import collab_splats_amd as m
    with pytest.raises(NotImplementedError):
        m.strategy.MCMCStrategy()
    assert m.MCMCStrategy is m.strategy.MCMCStrategy and m.RelocationStrategy is not m.MCMCStrategy


def test_no_cpu_fallback():
    import collab_splats_amd as m
    with pytest.raises(m.MisplatError):
        m.sample_by_opacity(torch.rand(8), 4, 0, 0)
    with pytest.raises(m.MisplatError):
        m.compute_relocation(torch.rand(8), torch.rand(8, 3), torch.ones(8, dtype=torch.int32))
    params = {k: torch.nn.Parameter(torch.zeros(4, d)) for k, d in (("means", 3), ("scales", 3), ("quats", 4), ("opacities", 1))}
    with pytest.raises(m.MisplatError):
        m.inject_noise_to_position(params, {}, {}, 1.0, 0, 0)


def test_bad_arguments_are_refused_before_any_launch(built_lib):
    from collab_splats_amd import _lib
    for label, status in S.abi_bad_calls(_lib.load()):
        assert status in (-1, -3), (label, status)                         # EINVAL / EWORKSPACE: refused, not a failed launch (-2)
