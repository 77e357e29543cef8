"""CPU: the restatement of the identity losses (tests/identity_restatement.py) against autograd through torch's own operators,
the rules it states for the empty cases, the conditions the GPU tests rely on in the scenes (tests/identity_scenes.py), and
the Python-side validation of collab_splats_amd/identity.py (no launch happens: there is no GPU here)."""
import pytest
import torch
import torch.nn.functional as F

import identity_restatement as R
import identity_scenes as S


def _autograd_2d(sc):
    f = sc["features"].double().requires_grad_(True)
    w, b = sc["weight"].double().requires_grad_(True), sc["bias"].double().requires_grad_(True)
    z = F.conv2d(f.permute(2, 0, 1)[None], w[:, :, None, None], b)                  # [1, K, H, W]
    loss = F.cross_entropy(z, sc["target"].long()[None] - 1, ignore_index=-1)
    loss.backward()
    return loss.detach(), {"features": f.grad, "weight": w.grad, "bias": b.grad}


@pytest.mark.parametrize("name", ["d1", "d16_k16", "k17", "d32", "d13", "k2", "one_pixel", "splits_2"])
def test_restatement_equals_conv2d_cross_entropy(name):
    sc = S.make(name)
    ref_loss, ref = _autograd_2d(sc)
    got = S.oracle(name)
    assert abs(float(got["loss"]) - float(ref_loss)) <= 1e-12 * max(abs(float(ref_loss)), 1.0)
    for k, v in ref.items():
        assert got["grads"][k].shape == v.shape
        assert float((got["grads"][k] - v).abs().max()) <= 1e-12 * max(float(v.abs().max()), 1.0), k


@pytest.mark.parametrize("name", list(S.SCENES_3D))
def test_3d_restatement_equals_the_log_softmax_form(name):
    sc = S.make_3d(name)
    e = sc["identities"].double().requires_grad_(True)
    w, b = sc["weight"].double().requires_grad_(True), sc["bias"].double().requires_grad_(True)
    s, t, ok = R.valid_pairs(sc["sample"], sc["table"], e.shape[0])
    lps, lpt = F.log_softmax(F.linear(e[s[ok]], w, b), dim=-1), F.log_softmax(F.linear(e[t[ok]], w, b), dim=-1)
    loss = (lps.exp() * (lps - lpt)).sum() / max(int(ok.sum()), 1)
    loss.backward()
    got = S.oracle_3d(name)
    assert got["n"] == int(ok.sum()) and got["n"] >= 1
    assert abs(float(got["loss"]) - float(loss.detach())) <= 1e-12 * max(abs(float(loss.detach())), 1.0)
    for k, v in {"identities": e.grad, "weight": w.grad, "bias": b.grad}.items():
        assert float((got["grads"][k] - v).abs().max()) <= 1e-12 * max(float(v.abs().max()), 1.0), k


def test_no_labelled_pixel_gives_zero_and_zero_gradients():
    got = S.oracle("unlabelled")
    assert got["n"] == 0 and float(got["loss"]) == 0.0
    for k, v in got["grads"].items():
        assert bool((v == 0).all()), k
    # (torch's own cross-entropy gives NaN there: the rule is this project's)
    assert bool(torch.isnan(_autograd_2d(S.make("unlabelled"))[0]))


def test_one_class_gives_zero_and_zero_gradients():
    got = S.oracle("k1")
    assert got["n"] > 0 and float(got["loss"]) == 0.0
    for k, v in got["grads"].items():
        assert bool((v == 0).all()), k


def test_out_of_range_targets_count_as_unlabelled():
    sc = dict(S.make("k17"))
    t = sc["target"].clone()
    t[0, 0], t[1, 1] = 18, -3
    base = R.loss_2d(sc["features"].double(), sc["weight"].double(), sc["bias"].double(), t)
    t[0, 0], t[1, 1] = 0, 0
    zero = R.loss_2d(sc["features"].double(), sc["weight"].double(), sc["bias"].double(), t)
    assert float(base["loss"]) == float(zero["loss"]) and base["n"] == zero["n"]


@pytest.mark.parametrize("name", list(S.ALL_SCENES))
def test_scene_conditions(name):
    """What the GPU tests take for granted: the margin of every pixel, labelled and unlabelled pixels where the scene promises
    them, the class nobody carries, and the launch regime of the LAUNCH scenes."""
    sc = S.make(name)
    (H, W), D, K, unl, _ = S.ALL_SCENES[name]
    assert sc["features"].shape == (H, W, D) and sc["weight"].shape == (K, D) and sc["target"].dtype == torch.int32
    _, _, margin, top = S.oracle_labels(name)
    if K > 1:
        assert float(margin.min()) >= S.MARGIN * top, (float(margin.min()), top)
    t = sc["target"]
    assert int(t.min()) >= 0 and int(t.max()) <= K
    if unl == 1.0:
        assert int((t > 0).sum()) == 0
    elif unl > 0 and H * W > 1:
        assert int((t > 0).sum()) > 0 and int((t == 0).sum()) > 0
    if name == "d16_k16":
        assert int((t == S.MISSING_CLASS).sum()) == 0 and W % 64 != 0
    if name in S.LAUNCH:
        assert S.plan(H * W, K) == S.LAUNCH[name]
        tiles, ps = S.LAUNCH[name]
        assert (H * W) % 256 != 0                                                    # a ragged last tile
    else:
        assert S.plan(H * W, K)[0] == S.plan(H * W, K)[1]                            # below every cap


def test_tie_scene_is_an_exact_tie_of_classes_3_and_7():
    sc = S.make("tie")
    for dt in (torch.float64, torch.float32):
        z = R.logits(sc["features"].to(dt), sc["weight"].to(dt), sc["bias"].to(dt))
        assert bool((z[..., 3] == z[..., 7]).all())
        others = z.clone()
        others[..., [3, 7]] = -float("inf")
        assert bool((others.max(-1)[0] < z[..., 3] - 0.5).all())
    assert bool((S.oracle_labels("tie")[0] == 4).all())


def test_3d_scene_conditions():
    sh = S.make_3d("shared")
    rows = torch.cat((sh["sample"], sh["table"].reshape(-1).long()))
    assert int((rows == 0).sum()) >= 4 and 0 in sh["sample"].tolist()                # a sample and several samples' neighbour
    k16 = S.make_3d("k16")
    assert k16["table"].shape[1] == 16 and int((k16["table"] == -1).sum()) > 0
    assert int((k16["table"].long() == k16["sample"][:, None]).sum()) > 0
    assert S.make_3d("k1")["table"].shape[1] == 1 and S.make_3d("m1")["sample"].shape[0] == 1
    N, D, K, M, k, _ = S.SCENES_3D["big"]
    assert S.plan(2 * M * k, K) == (47, 32)
    for name in S.SCENES_3D:
        assert S.oracle_3d(name)["n"] >= 1 and float(S.oracle_3d(name)["loss"]) > 1e-3


def test_validation_raises_before_any_launch():
    import collab_splats_amd as m
    from collab_splats_amd import identity
    z = torch.zeros
    i32 = torch.int32
    ok_cls = (z(4, 3), z(4))
    with pytest.raises(m.MisplatError):                                              # CPU tensors
        m.identity_loss(z(2, 2, 3), ok_cls, z(2, 2, dtype=i32))
    with pytest.raises(m.MisplatError):
        m.identity_labels(z(2, 2, 3), ok_cls)
    with pytest.raises(ValueError, match="width"):                                   # D outside 1..32
        m.identity_loss(z(2, 2, 33), (z(4, 33), z(4)), z(2, 2, dtype=i32))
    with pytest.raises(ValueError, match="classes"):                                 # K outside 1..4096
        m.identity_loss(z(2, 2, 3), (z(4097, 3), z(4097)), z(2, 2, dtype=i32))
    with pytest.raises(ValueError, match="classes"):
        m.identity_labels(z(2, 2, 3), (z(0, 3), z(0)))
    with pytest.raises(ValueError):                                                  # width mismatch
        m.identity_loss(z(2, 2, 3), (z(4, 5), z(4)), z(2, 2, dtype=i32))
    with pytest.raises(ValueError):                                                  # bias shape
        m.identity_loss(z(2, 2, 3), (z(4, 3), z(5)), z(2, 2, dtype=i32))
    with pytest.raises(ValueError, match="target"):                                  # target shape
        m.identity_loss(z(2, 2, 3), ok_cls, z(2, 3, dtype=i32))
    with pytest.raises(ValueError, match="int32"):                                   # target dtype
        m.identity_loss(z(2, 2, 3), ok_cls, z(2, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="float32"):                                 # features dtype
        m.identity_loss(z(2, 2, 3, dtype=torch.float64), ok_cls, z(2, 2, dtype=i32))
    with pytest.raises(ValueError, match="float32"):                                 # classifier dtype
        m.identity_loss(z(2, 2, 3), (z(4, 3, dtype=torch.float16), z(4)), z(2, 2, dtype=i32))
    with pytest.raises(ValueError):                                                  # not a classifier
        m.identity_loss(z(2, 2, 3), z(4, 3), z(2, 2, dtype=i32))
    with pytest.raises(ValueError, match="k must be"):                               # k outside 1..16
        m.IdentityNeighbours(z(3, dtype=torch.int64), z(3, 17, dtype=i32), 10)
    with pytest.raises(ValueError, match="k must be"):
        m.IdentityNeighbours(z(3, dtype=torch.int64), z(3, 0, dtype=i32), 10)
    with pytest.raises(ValueError, match="int32"):
        m.IdentityNeighbours(z(3, dtype=torch.int64), z(3, 4, dtype=torch.int64), 10)
    with pytest.raises(ValueError, match="int64"):
        m.IdentityNeighbours(z(3, dtype=i32), z(3, 4, dtype=i32), 10)
    with pytest.raises(m.MisplatError):
        m.IdentityNeighbours(z(3, dtype=torch.int64), z(3, 4, dtype=i32), 10)
    with pytest.raises(ValueError, match="IdentityNeighbours"):
        m.identity_3d_loss(z(5, 3), ok_cls, None)
    with pytest.raises(ValueError, match="k must be"):
        m.identity_neighbours(z(20, 3), 5, 16, 1.0, 0)
    with pytest.raises(m.MisplatError):
        m.identity_neighbours(z(20, 3), 5, 3, 1.0, 0)
    with pytest.raises(ValueError):
        m.IdentityField(10, 5000)
    with pytest.raises(ValueError):
        m.IdentityField(10, 5, identity_dim=33)
    field = m.IdentityField(10, 5, identity_dim=16)
    assert field.identities.shape == (10, 16) and bool((field.identities == 0).all())
    assert field.classifier.weight.shape == (5, 16, 1, 1)
    w, b = field.flat()
    assert w.shape == (5, 16) and b.shape == (5,) and w.data_ptr() == field.classifier.weight.data_ptr()
    assert all(p.is_contiguous() and p.dtype == torch.float32 for p in field.parameters())
    with pytest.raises(m.MisplatError):
        field.loss_2d(z(2, 2, 16), z(2, 2, dtype=i32))
    assert identity.MAX_DIM == 32 and identity.MAX_CLASSES == 4096 and identity.MAX_NEIGHBOURS == 16


def test_scratch_query_follows_the_plan(built_lib):
    """``misplat_identity_scratch_floats``: no K x P term -- per-row scalars plus PS partial [K, D + 1] blocks; -1 outside the
    limits."""
    import ctypes as C
    from collab_splats_amd import _lib
    lib = _lib.load()
    q = lambda rows, d, k, mode: int(lib.misplat_identity_scratch_floats(C.c_int64(rows), C.c_int32(d), C.c_int32(k), C.c_int32(mode)))  # noqa: E731
    r4 = lambda v: (v + 3) // 4 * 4                                                   # noqa: E731
    for rows, d, k in ((1, 16, 7), (6720, 32, 300), (1080 * 1920, 16, 256)):
        tiles, ps = S.plan(rows, k)
        assert q(rows, d, k, 0) == r4(6 * tiles) + r4(rows) + r4(ps * k * (d + 1))
    assert q(1080 * 1920, 16, 256, 0) < 3 * 1080 * 1920                               # nothing like 256 floats a pixel
    pairs = 6000
    tiles, ps = S.plan(2 * pairs, 256)
    assert q(pairs, 16, 256, 1) == r4(6 * ((pairs + 255) // 256)) + r4(3 * pairs) + r4(2 * pairs * 16) + r4(ps * 256 * 17)
    for bad in ((0, 16, 4, 0), (10, 0, 4, 0), (10, 33, 4, 0), (10, 16, 0, 0), (10, 16, 4097, 0), (10, 16, 4, 2), (2 ** 28 + 1, 16, 4, 0)):
        assert q(*bad) == -1
