"""CPU (no kernel runs): the row-selective Adam restatement (tests/selective_adam_restatement.py) against
``torch.optim.Adam`` in fp64 on the gathered rows, the conditions the case generator (tests/selective_adam_cases.py)
promises, the visibility rule, and the strategy's optimizer-state surgery on a ``SelectiveAdam``."""
import pytest
import torch

import adam_cases as A
import adam_restatement as R
import selective_adam_cases as SC
import selective_adam_restatement as S


@pytest.mark.parametrize("n,steps", [c for c in SC.CASES if c[0] <= 2049])
def test_selected_rows_equal_torch_adam_on_the_gathered_rows_in_fp64(n, steps):
    """Selected rows: ``torch.optim.Adam`` in fp64 on the gathered rows with the state of step t - 1 injected, to 1e-12 (the
    bar of test_adam_host.py).  Unselected rows: the inputs exactly."""
    cases = SC.make(n, steps)
    for name, mask in SC.masks(n).items():
        for i, (c, got) in enumerate(zip(cases, SC.masked_oracle(n, steps, mask))):
            for k in ("p", "m", "v"):
                assert got[k].dtype == torch.float64 and got[k].shape == c["p"].shape
                assert torch.equal(got[k][~mask], c[k][~mask].double()), (n, steps, name, i, k)
            if not bool(mask.any()):
                continue
            ref = dict(zip(("p", "m", "v"), R.torch_adam_step(c["p"][mask], c["g"][mask], c["m"][mask], c["v"][mask], c["lr"],
                                                               *c["betas"], SC.EPS, c["t"], torch.float64)))
            for k in ("p", "m", "v"):
                assert A.rel_err(got[k][mask], ref[k]) <= 1e-12, (n, steps, name, i, k)
            before = c["p"][mask].double()
            assert A.rel_err(got["p"][mask] - before, ref["p"] - before) <= 1e-12, (n, steps, name, i)


def test_the_masked_restatement_is_the_dense_one_on_the_selected_rows():
    n, steps = 2049, "mixed"
    for mask in SC.masks(n).values():
        for a, b in zip(SC.masked_oracle(n, steps, mask), SC.under_mask(SC.oracle(n, steps), SC.make(n, steps), mask)):
            for k in ("p", "m", "v"):
                assert torch.equal(a[k], b[k])


def test_the_cases_cover_what_they_are_there_for():
    assert SC.SIZES == (1, 7, 64, 2047, 2048, 2049, 10007) and sum(SC.WIDTHS) == 59
    assert {(n, s) for n in SC.SIZES for s in ("t1", "t1000")} <= set(SC.CASES) and (2049, "mixed") in SC.CASES
    for n, steps in SC.CASES:
        cases = SC.make(n, steps)
        assert [tuple(c["p"].shape) for c in cases] == [(n,) + r for r in SC.ROW_SHAPES]
        assert [c["p"].numel() // n for c in cases] == list(SC.WIDTHS) == [3, 3, 45, 1, 3, 4]
        assert [c["lr"] for c in cases] == [1.6e-4, 0.0025, 0.0025 / 20, 0.05, 0.005, 0.001]
        assert [c["t"] for c in cases] == [SC.STEPS[steps][i % len(SC.STEPS[steps])] for i in range(6)]
        for c in cases:
            assert all(c[k].dtype == torch.float32 and c[k].is_contiguous() for k in ("p", "g", "m", "v"))
    assert [c["t"] for c in SC.make(2049, "mixed")] == [1, 1000] * 3
    assert SC.EPS == 1e-15


def test_the_masks_are_what_their_names_say():
    for n in SC.SIZES:
        ms = SC.masks(n)
        assert set(ms) <= set(SC.MASKS) and all(m.shape == (n,) and m.dtype == torch.bool for m in ms.values())
        assert int(ms["none"].sum()) == 0 and int(ms["all"].sum()) == n
        assert ms["first"].nonzero().flatten().tolist() == [0] and ms["last"].nonzero().flatten().tolist() == [n - 1]
        assert ms["alternating"].nonzero().flatten().tolist() == list(range(0, n, 2))
        assert ("rows_2047_2048" in ms) == (n >= 2049) and ("random_2" in ms) == ("random_50" in ms) == (n >= 2)
        if n >= 2049:
            assert ms["rows_2047_2048"].nonzero().flatten().tolist() == [2047, 2048]
        for name, density in (("random_2", 0.02), ("random_50", 0.5)):
            if name in ms:
                m = ms[name]
                assert bool(m[0]) and not bool(m[-1])
                if n >= 2047:
                    assert 0.6 * density < float(m.float().mean()) < 1.4 * density
    assert set(SC.masks(10007)) == set(SC.MASKS)


@pytest.mark.parametrize("n,steps", [(2049, "t1000"), (10007, "t1")])
def test_generated_states_are_consistent(n, steps):
    """As test_adam_host.py asks of adam_cases: v = s^2 >= 0, |m| <= sqrt(v), untouched elements all zero, idle ones with a zero
    gradient and a state, every other with a gradient; the shares over the case."""
    n_all = n_untouched = n_idle = 0
    for c in SC.make(n, steps):
        p, g, m, v, un, idle = (c[k].reshape(-1) for k in ("p", "g", "m", "v", "untouched", "idle"))
        assert bool((v >= 0).all()) and bool(torch.isfinite(torch.stack([p, g, m, v])).all())
        assert bool((m.double().abs() <= v.double().sqrt() * (1 + 2.0 ** -22)).all())
        assert not bool(((v == 0) & (m != 0)).any()) and not bool((un & idle).any())
        assert bool((g[un] == 0).all() and (m[un] == 0).all() and (v[un] == 0).all())
        assert bool((g[idle] == 0).all() and (v[idle] > 0).all())
        active = ~(un | idle)
        assert bool((g[active] != 0).all() and (v[active] > 0).all()) and bool(active[0]) and bool(active[-1])
        n_all, n_untouched, n_idle = n_all + p.numel(), n_untouched + int(un.sum()), n_idle + int(idle.sum())
    assert 0.30 < n_untouched / n_all < 0.37 and 0.13 < n_idle / n_all < 0.20


def test_visibility_restatement_on_a_hand_written_example():
    radii = torch.tensor([[[3, 2], [0, 5], [4, 0], [-1, 6], [0, 0], [1, 1]],
                          [[0, 0], [2, 2], [0, 9], [7, -2], [0, 0], [0, 0]]], dtype=torch.int32)    # [C=2, N=6, 2]
    assert S.visibility_from_radii(radii).tolist() == [True, True, False, False, False, True]
    assert S.visibility_from_radii(radii[:1]).tolist() == [True, False, False, False, False, True]


def test_selective_adam_is_constructed_like_fused_adam_and_refuses_the_cpu():
    from collab_splats_amd import FusedAdam, MisplatError, SelectiveAdam, selective_adam_step_all
    p = torch.zeros(4, 3, requires_grad=True)
    opt = SelectiveAdam([p], lr=0.01, betas=(0.8, 0.99), eps=1e-15)
    assert isinstance(opt, FusedAdam) and opt.param_groups[0]["lr"] == 0.01 and opt.param_groups[0]["betas"] == (0.8, 0.99)
    with pytest.raises(ValueError):
        SelectiveAdam([p], lr=-1.0)
    p.grad = torch.ones(4, 3)
    with pytest.raises(MisplatError):                                                  # no CPU fallback
        opt.step(torch.ones(4, dtype=torch.bool))
    with pytest.raises(TypeError):
        selective_adam_step_all([FusedAdam([p])], torch.ones(4, dtype=torch.bool))
    assert len(opt.state[p]) == 0 or int(opt.state[p]["step"]) == 0


def test_update_param_with_optimizer_edits_a_selective_adam_as_it_edits_torch_adam():
    """The densification's state surgery (duplicate-like: the selected rows appended, their moments zero) on CPU tensors."""
    from collab_splats_amd import SelectiveAdam
    from collab_splats_amd.strategy import _update_param_with_optimizer
    c = SC.make(7, "t1000")
    sel = torch.tensor([1, 4, 6])
    edited = []
    for cls in (SelectiveAdam, torch.optim.Adam):
        params = {name: torch.nn.Parameter(x["p"].clone()) for name, x in zip(SC.NAMES, c)}
        opts = {name: cls([params[name]], lr=x["lr"], eps=SC.EPS) for name, x in zip(SC.NAMES, c)}
        for name, x in zip(SC.NAMES, c):
            opts[name].state[params[name]] = {"step": torch.tensor(float(x["t"] - 1)), "exp_avg": x["m"].clone(),
                                              "exp_avg_sq": x["v"].clone()}
        _update_param_with_optimizer(lambda n, p: torch.cat([p, p[sel]]),
                                     lambda k, v: torch.cat([v, torch.zeros((len(sel), *v.shape[1:]))]), params, opts)
        edited.append((params, opts))
    (pa, oa), (pb, ob) = edited
    for name, x in zip(SC.NAMES, c):
        assert oa[name].param_groups[0]["params"][0] is pa[name]
        assert pa[name].shape[0] == 10 and torch.equal(pa[name], pb[name]) and torch.equal(pa[name][:7], x["p"])
        sa, sb = oa[name].state[pa[name]], ob[name].state[pb[name]]
        assert set(sa) == set(sb) == {"step", "exp_avg", "exp_avg_sq"} and len(oa[name].state) == 1
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (name, k)
        assert torch.equal(sa["exp_avg"][:7], x["m"]) and bool((sa["exp_avg_sq"][7:] == 0).all())


def test_bad_c_arguments_are_refused_before_any_launch(built_lib):
    """Bad sizes, null pointers and counts out of range: ``MISPLAT_EINVAL`` (-1), not a failed launch (-2).  Every call here
    returns before it launches, so the addresses are never dereferenced and no GPU is needed."""
    import ctypes as C
    from collab_splats_amd import _lib
    lib = _lib.load()
    FAKE = 4096                                                                        # 16-byte aligned, never read

    def rows(n=1, tensors=(FAKE, FAKE, FAKE, FAKE), width=3, n_rows=8, step=1, ids=FAKE, cap=8, count=FAKE, arrays=True):
        k = max(n, 1)
        vp = lambda a: (C.c_void_p * k)(*[a] * k) if arrays else None
        return lib.misplat_adam_step_rows(C.c_int32(n), vp(tensors[0]), vp(tensors[1]), vp(tensors[2]), vp(tensors[3]),
                                          (C.c_int32 * k)(*[width] * k), C.c_int64(n_rows), (C.c_float * k)(*[1e-3] * k),
                                          (C.c_int64 * k)(*[step] * k), C.c_double(0.9), C.c_double(0.999), C.c_double(1e-15),
                                          C.c_void_p(ids), C.c_int64(cap), C.c_void_p(count), C.c_void_p(0))

    bad = {"too many tensors": rows(n=9), "negative tensors": rows(n=-1), "negative rows": rows(n_rows=-1, cap=0),
           "rows past int32": rows(n_rows=2 ** 31), "negative capacity": rows(cap=-1), "capacity above the rows": rows(cap=9),
           "null arrays": rows(arrays=False), "width 0": rows(width=0), "width past 2^30": rows(width=2 ** 30),
           "step 0": rows(step=0), "null parameter": rows(tensors=(0, FAKE, FAKE, FAKE)),
           "null gradient": rows(tensors=(FAKE, 0, FAKE, FAKE)), "null exp_avg": rows(tensors=(FAKE, FAKE, 0, FAKE)),
           "null exp_avg_sq": rows(tensors=(FAKE, FAKE, FAKE, 0)), "null ids": rows(ids=0), "null count": rows(count=0)}
    vis = lambda radii=FAKE, cams=1, n=8, flags=FAKE: lib.misplat_visible_rows(C.c_void_p(radii), C.c_int32(cams), C.c_int64(n),
                                                                              C.c_void_p(flags), C.c_void_p(0))
    bad.update({"no camera": vis(cams=0), "negative visible rows": vis(n=-1), "null radii": vis(radii=0),
                "null flags": vis(flags=0), "radii at an odd address": vis(radii=FAKE + 4)})
    assert all(status == -1 for status in bad.values()), bad
    # nothing to do is not an error, and launches nothing either
    assert rows(n=0) == 0 and rows(cap=0, ids=0, count=0) == 0 and rows(n_rows=0, cap=0) == 0 and vis(n=0, radii=0, flags=0) == 0
