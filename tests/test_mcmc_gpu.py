"""GPU: the MCMC densification (csrc/mcmc.hip, collab_splats_amd/mcmc.py, the model's ``strategy="mcmc"``) against the
restatement (tests/mcmc_restatement.py) on the scenes of tests/mcmc_scenes.py.

The sampler is integer work: indices and counts equal the restatement bit for bit.  The float kernels are held to the fp64
restatement under DESIGN.md section 21.4's rule: max |got - oracle| / max |oracle| at most 8 x the error the fp32 restatement
makes on the same scene, that bound floored at 2^-23 and capped at 1e-4 (``mcmc_restatement.bound_from``), computed from the
restatement and never from the code under test.  The noise step's update is held to bits against its own displacement.
The gate at an opacity logit of +30 is an exact 0; at -30 the published formula gives its largest value, 1 / (1 + e^-0.5) =
0.62, not 1: the kernel is held to the formula (tests/test_mcmc_host.py checks the restated gate at both ends), never a NaN.
(The figures of a GPU run belong in DESIGN.md section 36; these tests print them.)"""
import numpy as np
import pytest
import torch

import mcmc_restatement as R
import mcmc_scenes as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.int32),
                                                                      b.reshape(-1).contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- sample
@pytest.mark.parametrize("m", S.SAMPLE_DRAWS)
@pytest.mark.parametrize("n", S.sample_sizes())
def test_sample_equals_the_restatement_bit_for_bit(dev, n, m):
    import collab_splats_amd as cs
    o = torch.from_numpy(S.sample_opacities(n)).to(dev)
    seed, step = 17, 300
    for thresholded in (False, True):
        ref = S.sample_restated(n, m, seed, step, thresholded)
        kw = {"min_opacity": S.MIN_OPACITY} if thresholded else {}
        if ref is None:                                                    # (n = 1 has one alive row: never empty)
            with pytest.raises(cs.mcmc.NothingToSample):
                cs.sample_by_opacity(o, m, seed, step, **kw)
            continue
        idx, counts = cs.sample_by_opacity(o, m, seed, step, **kw)
        assert idx.dtype == torch.int64 and counts.dtype == torch.int32 and idx.shape == (m,) and counts.shape == (n,)
        assert np.array_equal(idx.cpu().numpy(), ref[0]), (n, m, thresholded)
        assert np.array_equal(counts.cpu().numpy(), ref[1]), (n, m, thresholded)
        q = R.weights(S.sample_opacities(n), S.MIN_OPACITY if thresholded else None)
        assert (q[ref[0]] > 0).all()                                       # a zero-weight row is never returned
        idx2, counts2 = cs.sample_by_opacity(o, m, seed, step, **kw)
        assert torch.equal(idx, idx2) and torch.equal(counts, counts2)


def test_all_zero_weights_give_nothing_to_sample(dev):
    import collab_splats_amd as cs
    for o, kw in ((torch.zeros(1025, device=dev), {}), (torch.full((65,), 0.004, device=dev), {"min_opacity": S.MIN_OPACITY}),
                  (torch.full((3,), float("nan"), device=dev), {})):
        with pytest.raises(cs.mcmc.NothingToSample, match="nothing to sample"):
            cs.sample_by_opacity(o, 7, 0, 0, **kw)


# ------------------------------------------------------------------------------------------------------------ relocation
@pytest.mark.parametrize("name", ["grid", "near_one"])
def test_relocation_against_the_fp64_restatement(dev, name):
    import collab_splats_amd as cs
    o, s, n = S.relocation_scene(name)
    new_o, new_s = cs.compute_relocation(torch.from_numpy(o).to(dev), torch.from_numpy(s).to(dev), torch.from_numpy(n).to(dev))
    assert new_o.dtype == torch.float32 and new_o.shape == (len(o),) and new_s.shape == (len(o), 3)
    ora, yard = S.relocation_restated(name, False), S.relocation_restated(name, True)
    for k, (got, what) in enumerate(((new_o, "opacities"), (new_s, "scales"))):
        got = got.cpu().numpy()
        e, bound = R.rel_err(got, ora[k]), R.bound_from(R.rel_err(yard[k], ora[k]))
        print(f"{name:8s} {what:9s} gpu - fp64 restatement {e:.3e}  bound {bound:.3e}")
        assert np.isfinite(got).all() and e <= bound, (name, what, e, bound)
    one = n == 1                                                           # one copy: nothing changes, to fp32's rounding
    assert np.abs(new_o.cpu().numpy()[one] / o[one].astype(np.float64) - 1).max() <= 2.0 ** -23
    assert np.abs(new_s.cpu().numpy()[one] / s[one].astype(np.float64) - 1).max() <= 2.0 ** -23
    clamped = cs.compute_relocation(torch.from_numpy(o).to(dev), torch.from_numpy(s).to(dev),
                                    torch.from_numpy(np.minimum(n, 51)).to(dev))               # 200 clamps to 51
    assert (n == 200).any() and _bits_equal(clamped[0], new_o) and _bits_equal(clamped[1], new_s)


# ----------------------------------------------------------------------------------------------------------------- noise
def _noise(dev, n, means, seed, step):
    import collab_splats_amd as cs
    logits, log_scales, quats = (torch.from_numpy(t).to(dev) for t in S.noise_scene(n))
    params = {"means": torch.nn.Parameter(means.clone()), "opacities": torch.nn.Parameter(logits),
              "scales": torch.nn.Parameter(log_scales), "quats": torch.nn.Parameter(quats)}
    cs.inject_noise_to_position(params, {}, {}, S.NOISE_SCALER, seed, step)
    return params["means"].detach()


@pytest.mark.parametrize("n", S.noise_sizes())
def test_noise_against_the_restatement(dev, n):
    seed, step = 21, 1000
    zero = torch.zeros(n, 3, device=dev)
    d = _noise(dev, n, zero, seed, step)
    ora, yard = S.noise_restated(n, seed, step, False), S.noise_restated(n, seed, step, True)
    got = d.cpu().numpy()
    assert np.isfinite(got).all()
    e, bound = R.rel_err(got, ora), R.bound_from(R.rel_err(yard, ora))
    print(f"noise n = {n}: gpu - fp64 restatement {e:.3e}  bound {bound:.3e}  max |d| {np.abs(ora).max():.3e}")
    assert e <= bound, (n, e, bound)
    logits = S.noise_scene(n)[0].reshape(-1)
    assert not got[logits == 30].any()                                     # opaque: the gate is an exact 0, not a NaN
    if n >= 64:
        assert got[logits == -30].any()
    # the update is fl32(old + d) bit for bit
    old = torch.from_numpy(np.random.default_rng(n).normal(size=(n, 3)).astype(np.float32) * 100).to(dev)
    moved = _noise(dev, n, old, seed, step)
    assert _bits_equal(moved, old + d)
    # the same bits twice; another step and another seed move something else
    assert _bits_equal(_noise(dev, n, zero, seed, step), d)
    assert not _bits_equal(_noise(dev, n, zero, seed, step + 1), d)
    assert not _bits_equal(_noise(dev, n, zero, seed + 1, step), d)


# -------------------------------------------------------------------------------------------------------------- strategy
def _toy(dev, cap_max, seed=3, n=300):
    import collab_splats_amd as cs
    arrays, dead = S.toy_model(n)
    params = torch.nn.ParameterDict({k: torch.nn.Parameter(torch.from_numpy(v).to(dev)) for k, v in arrays.items()})
    optimizers = {k: cs.FusedAdam([v], lr=1e-3, eps=1e-15) for k, v in params.items()}
    g = torch.Generator().manual_seed(1)
    for v in params.values():                                              # one Adam step: every moment is non-zero
        v.grad = (torch.rand(v.shape, generator=g) + 0.5).to(dev)
    cs.fused_adam_step_all(optimizers)
    strategy = cs.RelocationStrategy(cap_max=cap_max, refine_start_iter=0, refine_every=10, seed=seed)
    return strategy, params, optimizers, strategy.initialize_state(), dead


def _moments(optimizers, params):
    return {k: {m: optimizers[k].state[params[k]][m].clone() for m in ("exp_avg", "exp_avg_sq")} for k in params}


def test_refine_step_relocates_the_dead_and_grows(dev):
    n, step = 300, 10
    strategy, params, optimizers, state, dead = _toy(dev, cap_max=1000)
    n_dead = int(dead.sum())
    assert 80 <= n_dead <= 120
    before = {k: v.detach().clone() for k, v in params.items()}
    moments = _moments(optimizers, params)
    assert all(bool((m != 0).all()) for ms in moments.values() for m in ms.values())
    # what the restatement draws from the device's own activations
    act = torch.sigmoid(before["opacities"].reshape(-1))
    w = act.masked_fill(torch.from_numpy(dead).to(dev), 0.0).cpu().numpy()
    idx, counts = R.sample(w, n_dead, strategy.seed, step, strategy.min_opacity)
    got = strategy.step_post_backward(params, optimizers, state, step, {}, lr=0.0)         # lr 0: the noise adds exact zeros
    n_new = min(1000, int(1.05 * n)) - n
    assert got == (n_dead, n_new) and n_new == 15
    assert all(v.shape[0] == n + n_new for v in params.values())
    now = {k: v.detach() for k, v in params.items()}
    assert int((torch.sigmoid(now["opacities"].reshape(-1)) <= strategy.min_opacity).sum()) == 0           # no dead row is left
    dead_rows, src = torch.from_numpy(np.where(dead)[0]).to(dev), torch.from_numpy(idx).to(dev)
    for k in ("means", "quats", "features_dc"):                            # each dead row took its sampled row's parameters
        assert _bits_equal(now[k][dead_rows], before[k][src]), k
        assert _bits_equal(now[k][:n][~torch.from_numpy(dead).to(dev)], before[k][~torch.from_numpy(dead).to(dev)]), k
    # the growth: the restatement's second draw, from the activations after the relocation, names the appended rows' sources
    idx2, _ = R.sample(_after_relocation_activations(before, dead, idx, counts, strategy.min_opacity, dev), n_new,
                       strategy.seed + R.ADD_STREAM, step)
    src2 = torch.from_numpy(idx2).to(dev)
    assert _bits_equal(now["means"][n:], now["means"][:n][src2])
    assert _bits_equal(now["opacities"][n:], now["opacities"][:n][src2]) and _bits_equal(now["scales"][n:], now["scales"][:n][src2])
    # moments: zero at the relocation's sampled rows and at the appended rows, untouched everywhere else
    sampled = torch.zeros(n, dtype=torch.bool, device=dev)
    sampled[src] = True
    for k in params:
        for m in ("exp_avg", "exp_avg_sq"):
            v = optimizers[k].state[params[k]][m]
            assert v.shape[0] == n + n_new and not v[n:].any() and not v[:n][sampled].any(), (k, m)
            assert _bits_equal(v[:n][~sampled], moments[k][m][~sampled]), (k, m)


def _after_relocation_activations(before, dead, idx, counts, min_opacity, dev) -> np.ndarray:
    """The activated opacities after the relocation, as the device computes them (torch ops on the device's own results of
    ``compute_relocation``): what ``sample_add`` then draws from."""
    import collab_splats_amd as cs
    src = torch.from_numpy(idx).to(dev)
    logits = before["opacities"].reshape(-1).clone()
    new_o, _ = cs.compute_relocation(torch.sigmoid(logits[src]), torch.exp(before["scales"][src]),
                                     torch.from_numpy(counts).to(dev)[src] + 1)
    logits[src] = torch.logit(torch.clamp(new_o, min=min_opacity, max=1.0 - torch.finfo(torch.float32).eps))
    logits[torch.from_numpy(np.where(dead)[0]).to(dev)] = logits[src]
    return torch.sigmoid(logits).cpu().numpy()


def test_growth_stops_at_the_cap_and_corner_cases_change_nothing(dev):
    strategy, params, optimizers, state, dead = _toy(dev, cap_max=305)
    assert strategy.step_post_backward(params, optimizers, state, 10, {}, lr=0.0) == (int(dead.sum()), 5)
    assert params["means"].shape[0] == 305
    before = {k: v.detach().clone() for k, v in params.items()}
    moments = _moments(optimizers, params)
    # at the cap with no dead row: nothing is relocated, nothing added, nothing launched but the noise (lr 0: exact zeros)
    assert strategy.step_post_backward(params, optimizers, state, 20, {}, lr=0.0) == (0, 0)
    # every row dead: nothing to relocate onto, and at the cap nothing to add
    with torch.no_grad():
        saved = params["opacities"].detach().clone()
        params["opacities"].fill_(-9.0)
    assert strategy.step_post_backward(params, optimizers, state, 30, {}, lr=0.0) == (0, 0)
    with torch.no_grad():
        params["opacities"].copy_(saved)
    # outside the refine window and off the refine steps
    assert strategy.step_post_backward(params, optimizers, state, 35, {}, lr=0.0) == (0, 0)
    assert strategy.step_post_backward(params, optimizers, state, strategy.refine_stop_iter, {}, lr=0.0) == (0, 0)
    for k in params:
        assert _bits_equal(params[k].detach(), before[k]), k
        for m in ("exp_avg", "exp_avg_sq"):
            assert _bits_equal(optimizers[k].state[params[k]][m], moments[k][m]), (k, m)


def test_two_replicas_with_one_seed_stay_bitwise_equal(dev):
    import collab_splats_amd as cs
    runs = []
    for _ in range(2):
        strategy, params, optimizers, state, _ = _toy(dev, cap_max=340, seed=9)
        log = []
        for step in (9, 10, 11, 20, 30):                                   # refine steps at 10, 20 and 30, the last at the cap
            for v in params.values():
                v.grad = torch.full_like(v, 0.25)
            cs.fused_adam_step_all(optimizers)
            log.append(strategy.step_post_backward(params, optimizers, state, step, {}, lr=1.6e-4))
        runs.append((log, {k: v.detach().clone() for k, v in params.items()}, _moments(optimizers, params)))
    (log_a, par_a, mom_a), (log_b, par_b, mom_b) = runs
    assert log_a == log_b and [c[1] for c in log_a] == [0, 15, 0, 15, 10] and par_a["means"].shape[0] == 340
    for k in par_a:
        assert _bits_equal(par_a[k], par_b[k]), k
        assert all(_bits_equal(mom_a[k][m], mom_b[k][m]) for m in mom_a[k]), k
    other, params, optimizers, state, _ = _toy(dev, cap_max=340, seed=10)
    other.step_post_backward(params, optimizers, state, 10, {}, lr=1.6e-4)
    strategy, params9, optimizers9, state9, _ = _toy(dev, cap_max=340, seed=9)
    strategy.step_post_backward(params9, optimizers9, state9, 10, {}, lr=1.6e-4)
    assert not _bits_equal(params["means"].detach(), params9["means"].detach())            # another seed, other draws


def test_torch_adam_takes_the_same_surgery(dev):
    """``relocate`` / ``sample_add`` edit a ``torch.optim.Adam`` as they edit ``FusedAdam`` (the interface ``duplicate`` and
    ``split`` use)."""
    import collab_splats_amd as cs
    arrays, dead = S.toy_model(300)
    params = torch.nn.ParameterDict({k: torch.nn.Parameter(torch.from_numpy(v).to(dev)) for k, v in arrays.items()})
    optimizers = {k: torch.optim.Adam([v], lr=1e-3) for k, v in params.items()}
    for k, v in params.items():
        v.grad = torch.ones_like(v)
        optimizers[k].step()
    strategy = cs.RelocationStrategy(cap_max=1000, refine_start_iter=0, refine_every=10)
    assert strategy.step_post_backward(params, optimizers, strategy.initialize_state(), 10, {}, lr=1.6e-4) == (int(dead.sum()), 15)
    for k, v in params.items():
        st = optimizers[k].state[v]
        assert v.shape[0] == 315 and st["exp_avg"].shape == v.shape and not st["exp_avg"][300:].any()
        v.grad = torch.ones_like(v)
        optimizers[k].step()                                               # and the optimizer goes on stepping


# ----------------------------------------------------------------------------------------------------------------- model
def test_model_trains_three_steps_under_mcmc(dev):
    import importlib.util
    import os
    import collab_splats_amd as cs
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    spec = importlib.util.spec_from_file_location("train_synthetic", os.path.join(S.ROOT, "examples", "train_synthetic.py"))
    ts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ts)
    n, W, H = 2000, 160, 100
    sc = random_scene(n, W, H, seed=42)
    cfg = radegs.RadegsModelConfig(rasterize_mode="antialiased", sh_degree_interval=1, strategy="mcmc", cap_max=2150)
    truth = ts.build_model(sc, radegs.RadegsModelConfig(rasterize_mode="antialiased", sh_degree_interval=1), dev).eval()
    cams = [ts.ring_camera(i, 3, W, H) for i in range(3)]
    with torch.no_grad():
        targets = [truth.get_outputs(c)["rgb"].clone() for c in cams]
    model = ts.build_model(sc, cfg, dev, noise={"means": 0.05, "opacity_logits": 1.0}, generator=torch.Generator().manual_seed(0)).train()
    assert isinstance(model.strategy, cs.RelocationStrategy) and model.strategy.cap_max == 2150
    model.strategy.refine_start_iter, model.strategy.refine_every = 0, 1
    model.optimizers = {k: cs.FusedAdam([v], lr=ts.LRS[k], eps=1e-15) for k, v in model.gauss_params.items()}
    counts = [n]
    for it in range(3):
        model.step = 10 + it
        for o in model.optimizers.values():
            o.zero_grad(set_to_none=True)
        losses = model.get_loss_dict(model.get_outputs(cams[it]), {"image": targets[it]})
        assert {"main_loss", "scale_reg", "opacity_reg"} <= set(losses)
        op64 = torch.sigmoid(model.opacities.detach().double()).mean().item()
        sc64 = torch.exp(model.scales.detach().double()).mean().item()
        # an fp32 mean of N values in a pairwise-or-better order: N roundings of 2^-24 at the very most
        tol = 2.0 ** -24 * (model.num_points + 8)
        assert abs(losses["opacity_reg"].item() / (0.01 * op64) - 1) <= tol
        assert abs(losses["scale_reg"].item() / (0.01 * sc64) - 1) <= tol
        sum(losses.values()).backward()
        cs.fused_adam_step_all(model.optimizers)
        lr = model.optimizers["means"].param_groups[0]["lr"]
        n_rel, n_add = model.strategy.step_post_backward(model.gauss_params, model.optimizers, model.strategy_state, it + 1,
                                                         model.info, lr=lr)
        counts.append(model.num_points)
        assert n_add == counts[-1] - counts[-2] and torch.isfinite(model.means).all()
    assert counts == [2000, 2100, 2150, 2150]                              # min(cap_max, int(1.05 N)) every refine step


# ----------------------------------------------------------------------------------------------------------------- C ABI
def test_bad_arguments_are_refused_before_any_launch(dev):
    from collab_splats_amd import _lib
    for label, status in S.abi_bad_calls(_lib.load()):
        assert status in (-1, -3), (label, status)                         # EINVAL / EWORKSPACE: refused, not a failed launch (-2)
    torch.cuda.synchronize()                                               # nothing was launched: nothing can have faulted
