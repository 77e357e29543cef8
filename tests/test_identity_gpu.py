"""GPU: identity training for Gaussian grouping (csrc/identity.hip, collab_splats_amd/identity.py) against the fp64 restatement
(tests/identity_restatement.py) on the scenes of tests/identity_scenes.py.

Error measure, per tensor: max |got - oracle| / max |oracle|, nothing left out.  The bound of a tensor is ``MULTIPLE`` times the
error the fp32 run of the restatement makes on the same scene against the same oracle (never a figure of the code under test),
that error floored at 2^-23 and the bound capped at 1e-4: the rule of test_featureloss_gpu.py.

MULTIPLE = 8, as there.  The kernels' sums are no longer than the feature loss's: a logit is D <= 32 products in two chains; the
softmax denominator adds K <= 1040 exponentials (all positive: no cancellation) 16 at a time; a weight-gradient entry adds the
rows of a tile in 8 or 16 groups of 16 or 32 rows (fp32), the groups in order (fp32) and the at most 64 row splits in fp64, where
the restatement's matmul adds all rows of the image in fp32; the loss adds its per-pixel terms in fp64.  Different orders over n
terms differ by about sqrt(n) roundings of the terms' size: for the longest fp32 chains here (32 rows, 16 groups) that is below
8 roundings, the floor's worth.  (The figures of a GPU run belong in DESIGN.md section 33; this test prints them.)"""
import pytest
import torch

import identity_restatement as R
import identity_scenes as S

pytestmark = pytest.mark.gpu

MULTIPLE = 8.0
FLOOR = 2.0 ** -23
CAP = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def bound(yard: float) -> float:
    return min(MULTIPLE * max(yard, FLOOR), CAP)


def run_2d(scene, dev, features=None, target=None, validate=True):
    import collab_splats_amd as m
    f = (scene["features"].to(dev) if features is None else features).detach().requires_grad_(True)
    w, b = scene["weight"].to(dev).requires_grad_(True), scene["bias"].to(dev).requires_grad_(True)
    t = scene["target"].to(dev) if target is None else target
    loss = m.identity_loss(f, (w, b), t, validate)
    loss.backward()
    torch.cuda.synchronize()
    return {"loss": loss.detach(), "grads": {"features": f.grad, "weight": w.grad, "bias": b.grad}}


def run_3d(scene, dev):
    import collab_splats_amd as m
    e = scene["identities"].to(dev).requires_grad_(True)
    w, b = scene["weight"].to(dev).requires_grad_(True), scene["bias"].to(dev).requires_grad_(True)
    nb = m.IdentityNeighbours(scene["sample"].to(dev), scene["table"].to(dev), e.shape[0])
    loss = m.identity_3d_loss(e, (w, b), nb)
    loss.backward()
    torch.cuda.synchronize()
    return {"loss": loss.detach(), "grads": {"identities": e.grad, "weight": w.grad, "bias": b.grad}}


def _check(tag, name, got, ora, y32):
    rows = [("loss", S.rel_err(got["loss"], ora["loss"]), S.rel_err(y32["loss"], ora["loss"]))]
    for k, ref in ora["grads"].items():
        assert got["grads"][k].shape == ref.shape and bool(torch.isfinite(got["grads"][k]).all()), k
        rows.append((k, S.rel_err(got["grads"][k], ref), S.rel_err(y32["grads"][k], ref)))
    for k, e_gpu, e_32 in rows:
        print(f"{tag} {name:10s} {k:10s} gpu {e_gpu:.3e}  fp32 restatement {e_32:.3e}  bound {bound(e_32):.3e}")
    for k, e_gpu, e_32 in rows:
        assert e_gpu <= bound(e_32), (name, k, e_gpu, e_32)


@pytest.mark.parametrize("name", list(S.ALL_SCENES))
def test_loss_and_gradients_against_the_fp64_oracle(dev, name):
    _check("identity2d", name, run_2d(S.make(name), dev), S.oracle(name), S.yardstick(name))


@pytest.mark.parametrize("name", list(S.SCENES_3D))
def test_3d_loss_and_gradients_against_the_fp64_oracle(dev, name):
    got = run_3d(S.make_3d(name), dev)
    _check("identity3d", name, got, S.oracle_3d(name), S.yardstick_3d(name))
    touched = S.oracle_3d(name)["grads"]["identities"].abs().sum(-1) > 0
    assert bool((got["grads"]["identities"].cpu()[~touched] == 0).all())            # written whole: zeros on the other rows


@pytest.mark.parametrize("name", list(S.ALL_SCENES) + ["tie"])
def test_labels_equal_the_oracle_at_every_pixel(dev, name):
    import collab_splats_amd as m
    sc = S.make(name)
    cls = (sc["weight"].to(dev), sc["bias"].to(dev))
    labels, conf = m.identity_labels(sc["features"].to(dev), cls, return_confidence=True)
    only = m.identity_labels(sc["features"].to(dev), cls)
    ref_l, ref_c, _, _ = S.oracle_labels(name)
    y_c = S.oracle_labels(name, torch.float32)[1]
    assert labels.dtype == torch.int32 and labels.shape == ref_l.shape and torch.equal(labels, only)
    assert torch.equal(labels.cpu().long(), ref_l)
    e_gpu, e_32 = S.rel_err(conf, ref_c), S.rel_err(y_c, ref_c)
    print(f"identity labels {name:10s} confidence gpu {e_gpu:.3e}  fp32 restatement {e_32:.3e}  bound {bound(e_32):.3e}")
    assert e_gpu <= bound(e_32)
    if name == "tie":
        assert bool((labels == 4).all())                                             # classes 3 and 7 tie: the smaller index, + 1


def test_labels_of_rows(dev):
    """[N, 1, D] rows, as ``IdentityField.gaussian_labels`` passes them."""
    import collab_splats_amd as m
    sc = S.make_3d("k16")
    field = m.IdentityField(300, 20, 16, identities=sc["identities"])
    with torch.no_grad():
        field.classifier.weight.copy_(sc["weight"][:, :, None, None])
        field.classifier.bias.copy_(sc["bias"])
    field = field.to(dev)
    got = field.gaussian_labels()
    ref = R.labels(sc["identities"].double()[:, None, :], sc["weight"].double(), sc["bias"].double())
    assert float(ref[2].min()) > 1e-5 * ref[3]
    assert got.shape == (300,) and torch.equal(got.cpu().long(), ref[0][:, 0])


@pytest.mark.parametrize("name", ["d16_k16", "d32", "cap_64", "cap_mid"])
def test_two_runs_are_equal_bit_for_bit(dev, name):
    a, b = run_2d(S.make(name), dev), run_2d(S.make(name), dev)
    assert torch.equal(a["loss"], b["loss"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


@pytest.mark.parametrize("name", ["shared", "k16", "big"])
def test_3d_two_runs_are_equal_bit_for_bit(dev, name):
    a, b = run_3d(S.make_3d(name), dev), run_3d(S.make_3d(name), dev)
    assert torch.equal(a["loss"], b["loss"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


@pytest.mark.parametrize("name", ["d16_k16", "d13"])
def test_strided_features_equal_the_contiguous_run(dev, name):
    """``features`` as a channel slice of a wider image: read in place through the pixel stride, the contiguous run's bits."""
    import collab_splats_amd as m
    from collab_splats_amd import featureloss
    sc = S.make(name)
    H, W, D = sc["features"].shape
    wide = torch.randn(H, W, D + 4, generator=torch.Generator().manual_seed(5))
    wide[..., 3:3 + D] = sc["features"]
    view = wide.to(dev)[..., 3:3 + D]
    assert not view.is_contiguous()
    kept, stride = featureloss._features_view(view, "test")
    assert kept.data_ptr() == view.data_ptr() and stride == D + 4                    # no copy
    a, b = run_2d(sc, dev), run_2d(sc, dev, features=view)
    assert torch.equal(a["loss"], b["loss"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    cls = (sc["weight"].to(dev), sc["bias"].to(dev))
    assert torch.equal(m.identity_labels(view, cls), m.identity_labels(sc["features"].to(dev), cls))


def test_one_class_gives_exact_zeros(dev):
    got = run_2d(S.make("k1"), dev)
    assert float(got["loss"]) == 0.0
    for k, v in got["grads"].items():
        assert bool((v == 0).all()), k


def test_unlabelled_image_gives_exact_zeros(dev):
    """Gradient buffers start from garbage (NaN left in the allocator's freed blocks): still exact zeros everywhere."""
    sc = S.make("unlabelled")
    junk = [torch.full(sc["features"].shape, float("nan"), device=dev) for _ in range(4)]
    del junk
    got = run_2d(sc, dev)
    assert float(got["loss"]) == 0.0
    for k, v in got["grads"].items():
        assert bool((v == 0).all()), k


def test_unlabelled_pixels_get_zero_gradient_and_do_not_count(dev):
    """Whatever lies under an unlabelled pixel (here: NaN) reaches neither the loss nor any gradient."""
    sc = S.make("k17")
    f = sc["features"].clone()
    f[sc["target"] == 0] = float("nan")
    a, b = run_2d(sc, dev), run_2d(sc, dev, features=f.to(dev))
    assert torch.equal(a["loss"], b["loss"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    assert bool((a["grads"]["features"].cpu()[sc["target"] == 0] == 0).all())


def test_validate_raises_on_a_target_out_of_range(dev):
    sc = S.make("k17")
    t = sc["target"].clone()
    t[2, 3] = 18                                                                      # K + 1
    with pytest.raises(ValueError, match="outside"):
        run_2d(sc, dev, target=t.to(dev))
    got = run_2d(sc, dev, target=t.to(dev), validate=False)                           # no host read: the pixel is unlabelled
    t[2, 3] = 0
    ref = run_2d(sc, dev, target=t.to(dev))
    assert torch.equal(got["loss"], ref["loss"])
    for k in got["grads"]:
        assert torch.equal(got["grads"][k], ref["grads"][k]), k


def test_identity_neighbours_come_from_the_exact_knn(dev):
    """The builder: a seeded sample, the k nearest OTHER Gaussians within the radius, -1 beyond it."""
    import collab_splats_amd as m
    means = torch.rand(400, 3, generator=torch.Generator().manual_seed(21))
    means[0] = 50.0                                                                   # an outlier: nothing within the radius
    nb = m.identity_neighbours(means.to(dev), num_samples=400, k=4, radius=0.5, seed=3)
    again = m.identity_neighbours(means.to(dev), num_samples=400, k=4, radius=0.5, seed=3)
    assert torch.equal(nb.sample, again.sample) and torch.equal(nb.table, again.table)
    assert nb.table.shape == (400, 5) and nb.table.dtype == torch.int32 and sorted(nb.sample.tolist()) == list(range(400))
    d = torch.cdist(means.double(), means.double())
    for j in (1, 17, 399):
        row = int(nb.sample[j])
        got = [int(v) for v in nb.table[j].tolist() if v >= 0 and v != row]
        if row == 0:
            continue
        want = [v for v in torch.argsort(d[row])[1:5].tolist() if float(d[row, v]) <= 0.5]
        assert got == want
    j0 = nb.sample.tolist().index(0)
    assert all(v in (-1, 0) for v in nb.table[j0].tolist())
    # the reverse table: every valid slot once, under its own row, ascending
    s, t, ok = R.valid_pairs(nb.sample.cpu(), nb.table.cpu(), 400)
    rows = torch.stack((s, t), -1).reshape(-1)
    okk = torch.stack((ok, ok), -1).reshape(-1)
    off, slots = nb.rev_offsets.cpu(), nb.rev_slots.cpu().long()
    assert int(off[-1]) == int(okk.sum())
    for n in (0, 5, 123):
        mine = slots[int(off[n]):int(off[n + 1])]
        assert torch.equal(mine, torch.nonzero(okk & (rows == n))[:, 0])


def _model(dev, n=300, size=64):
    from collab_splats_amd import radegs
    from collab_splats_amd.synthetic import random_scene
    sc = random_scene(n, size, size, seed=4)
    model = radegs.RadegsModel(radegs.RadegsModelConfig(), sc["means"], sc["log_scales"], sc["quats"], sc["opacity_logits"],
                               sc["sh"][:, 0], sc["sh"][:, 1:]).to(dev)
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 0]])
    cam = radegs.PinholeCamera.make(c2w, 0.9 * size, 0.9 * size, size, size)
    return model, cam


def test_render_identities_is_attached_to_the_field_only(dev):
    import collab_splats_amd as m
    model, cam = _model(dev)
    field = m.IdentityField(300, 2, 16, identities=torch.randn(300, 16, generator=torch.Generator().manual_seed(1))).to(dev)
    out = model.render_identities(cam, field)
    assert out.shape == (64, 64, 16) and out.requires_grad
    out.square().sum().backward()
    assert field.identities.grad is not None and float(field.identities.grad.abs().sum()) > 0
    assert all(p.grad is None for p in model.parameters())
    assert all(p.grad is None for p in field.classifier.parameters())
    model.set_crop(object())
    with pytest.raises(ValueError, match="crop box"):
        model.render_identities(cam, field)


def test_fit_identities_lowers_the_loss(dev):
    """Two labels on the halves of a 64 x 64 view: thirty steps end below the starting loss, and every parameter of the field
    (identities, classifier weight and bias) steps through the one FusedAdam."""
    import collab_splats_amd as m
    model, cam = _model(dev)
    matched = torch.zeros(64, 64, dtype=torch.int32)
    matched[:, :32], matched[:, 32:] = 1, 2
    matched[:4] = 0
    torch.manual_seed(7)
    field = m.IdentityField(300, 2, 16).to(dev)
    before = {k: p.detach().clone() for k, p in field.named_parameters()}
    with torch.no_grad():
        start = float(field.loss_2d(model.render_identities(cam, field), matched.to(dev)))
    out = model.fit_identities([cam], [matched], num_classes=2, steps=30, lr=1e-2, lambda_3d=2.0, every_3d=5, field=field)
    assert out is field
    with torch.no_grad():
        end = float(field.loss_2d(model.render_identities(cam, field), matched.to(dev)))
    print(f"fit_identities: loss {start:.4f} -> {end:.4f}")
    assert end < start
    for k, p in field.named_parameters():
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[k]), k
    labels = field.pixel_labels(model.render_identities(cam, field).detach())
    assert labels.shape == (64, 64) and int(labels.min()) >= 1 and int(labels.max()) <= 2
    assert field.gaussian_labels().shape == (300,)
