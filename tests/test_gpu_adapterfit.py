"""CLIP-Adapter's training on the GPU (csrc/adapter_train.hip, clip_calibration_amd/adapterfit.py) against the float64 oracle of
tests/adapterfit_ref.py (torch's autograd and torch.optim.SGD in float64), which tests/test_adapterfit_cpu.py holds to the formulas the
kernels implement.  The tolerance of every compared quantity is measured: adapterfit_ref.tolerance takes FACTOR (4) times the distance of
torch's own fp32 CPU run of the same restatement from the oracle, with a floor of 2^-22 of the quantity's largest value.  Every test prints
its figures on lines that start with "adapterfit-parity:"; profiles/adapterfit_parity.txt is one run's lines."""
import functools

import numpy as np
import pytest
import torch

import adapterfit_ref as ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import adapterfit, ops  # noqa: E402

S = ref.scale_of()
RATIO = 0.2


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()             # a copy: the cached cases are read-only


def say(line):
    print("adapterfit-parity: " + line)


@functools.lru_cache(maxsize=None)
def case(shape, seed=None):
    c = ref.make_case(*shape, seed=ref.SHAPES[shape] if seed is None else seed)
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def step_oracle(shape, ratio=RATIO, s=S):
    """(float64 step, torch's fp32 step, keep masks of dw1 and dw2, excluded share), computed once per case."""
    B, E, H, C = shape
    o64, o32 = ref.torch_step(case(shape), ratio, s, "float64"), ref.torch_step(case(shape), ratio, s, "float32")
    x1, x2 = ref.excluded(ref.kinks(o64["p1"], o64["p2"]), E, H)
    return o64, o32, ~x1, ~x2, ref.excluded_share(x1, x2)


def device_step(c, ratio=RATIO, s=S, lr=1.0, momentum=0.0, weight_decay=0.0, y=None):
    """One step from the case's weights: (w1', w2', m1, m2, batch loss) as numpy."""
    st = adapterfit.AdapterFitState(cuda(c["T"]), torch.from_numpy(np.array(c["w1"])), torch.from_numpy(np.array(c["w2"])), ratio=ratio,
                                    logit_scale=float(np.log(s)), momentum=momentum, weight_decay=weight_decay)
    st.scale = s
    loss = st.step(cuda(c["f"]), c["y"] if y is None else y, lr, want_loss=True)
    m = (None, None) if st.m1 is None else (st.m1.cpu().numpy(), st.m2.cpu().numpy())
    return st.w1.cpu().numpy(), st.w2.cpu().numpy(), m[0], m[1], float(loss.cpu()[0])


def device_row_losses(c, ratio=RATIO, s=S):
    """Every row as a batch of its own at rate 0: the loss history is the row losses, the weights stay."""
    n = c["f"].shape[0]
    w1, w2 = cuda(c["w1"]), cuda(c["w2"])
    losses = ops.adapter_fit(cuda(c["f"]), cuda(c["y"]), cuda(c["T"]), w1, w2, None, None, torch.zeros(n).cuda(), ratio, s, 1, 1, want_losses=True)
    assert np.array_equal(w1.cpu().numpy(), c["w1"]) and np.array_equal(w2.cpu().numpy(), c["w2"])
    return losses.cpu().numpy()


@pytest.mark.parametrize("shape", list(ref.SHAPES))
def test_one_step_gradient(shape):
    """With momentum 0, weight decay 0 and lr 1 the step is W' = W - g.  The gradient itself is read where the kernel leaves it
    unrounded -- the momentum buffers after a first step with a momentum hold g exactly -- and W - W' is held to it bit for bit:
    W' == fl(W - g) in both runs, so nothing but the one rounding of that subtraction separates W - W' from the compared gradient.  g
    is compared with the float64 autograd element-wise, over the entries that depend on no ReLU at its kink (at most 1 % may be left out;
    tests/test_adapterfit_cpu.py holds the seeds to that by the oracle alone); the row losses and the batch loss likewise."""
    c = case(shape)
    o64, o32, keep1, keep2, share = step_oracle(shape)
    assert share <= ref.EXCLUDED_CAP
    w1a, w2a, _, _, loss = device_step(c)
    w1b, w2b, g1, g2, loss_b = device_step(c, momentum=0.9)
    assert np.array_equal(w1a, w1b) and np.array_equal(w2a, w2b) and loss == loss_b
    assert np.array_equal(w1a, c["w1"] - g1) and np.array_equal(w2a, c["w2"] - g2)          # fp32 arithmetic: fl(W - g)
    rows = device_row_losses(c)
    for name, got, keep in (("dw1", g1, keep1), ("dw2", g2, keep2), ("row_loss", rows, None)):
        tol, d = ref.tolerance(o32[name], o64[name], keep)
        err = np.abs(got.astype(np.float64) - o64[name])
        err = float((err if keep is None else err[keep]).max())
        say(f"step B,E,H,C={shape} {name}: max|value| {np.abs(o64[name]).max():.4g}  device {err:.3e}  torch-fp32 d {d:.3e}  "
            f"ratio {err / d if d else float('inf'):.2f}  tolerance {tol:.3e}  excluded {share:.4f}")
        assert np.isfinite(got).all() and err <= tol, name
    tol, d = ref.tolerance(o32["row_loss"].mean(dtype=np.float64), o64["row_loss"].mean())
    assert abs(loss - o64["row_loss"].mean()) <= tol
    assert loss == float(np.float32(rows.astype(np.float64).mean()))                          # the float64 mean of the fp32 row losses


def test_ratio_zero_moves_the_weights_by_weight_decay_only():
    """ratio = 0 takes the adapter out of the loss: both gradients are exactly zero, the step is W' = W - lr * wd * W."""
    c = case((5, 64, 16, 3))
    w1, w2, g1, g2, loss = device_step(c, ratio=0.0, momentum=0.9)
    assert not g1.any() and not g2.any() and np.array_equal(w1, c["w1"]) and np.array_equal(w2, c["w2"]) and np.isfinite(loss)
    wd, lr = np.float32(5e-4), np.float32(0.5)
    w1, w2, _, _, _ = device_step(c, ratio=0.0, lr=0.5, weight_decay=5e-4)
    assert np.array_equal(w1, c["w1"] - lr * (wd * c["w1"])) and np.array_equal(w2, c["w2"] - lr * (wd * c["w2"]))


def test_a_dead_hidden_unit_has_exactly_zero_gradients():
    """A hidden unit whose pre-activation is negative for every row: its row of dW1 and its column of dW2 are exactly zero."""
    shape = (33, 128, 32, 65)
    c = dict(case(shape))
    f64 = c["f"].astype(np.float64)
    w = np.linalg.pinv(f64) @ -np.ones(f64.shape[0])          # B < E: f w = -1 has a solution; the fp32 rounding of w is then checked
    w1 = c["w1"].copy()
    w1[7] = (w / np.linalg.norm(w)).astype(np.float32)
    c["w1"] = w1
    p1 = f64 @ w1.astype(np.float64).T
    assert (p1[:, 7] < -1e-3 * np.abs(p1).max()).all()
    _, _, g1, g2, _ = device_step(c, momentum=0.9)
    assert not g1[7].any() and not g2[:, 7].any()
    assert g1[6].any() and g2[:, 6].any() and np.isfinite(g1).all() and np.isfinite(g2).all()


def test_ratio_one():
    """ratio = 1: the raw features enter through the adapter alone."""
    shape = (5, 64, 16, 3)
    c = case(shape)
    o64, o32 = ref.torch_step(c, 1.0, S, "float64"), ref.torch_step(c, 1.0, S, "float32")
    assert not ref.kinks(o64["p1"], o64["p2"])
    _, _, g1, g2, loss = device_step(c, ratio=1.0, momentum=0.9)
    for name, got in (("dw1", g1), ("dw2", g2)):
        tol, d = ref.tolerance(o32[name], o64[name])
        err = float(np.abs(got - o64[name]).max())
        say(f"ratio 1 B,E,H,C={shape} {name}: device {err:.3e}  torch-fp32 d {d:.3e}  tolerance {tol:.3e}")
        assert err <= tol
    assert abs(loss - o64["row_loss"].mean()) <= ref.tolerance(o32["row_loss"].mean(dtype=np.float64), o64["row_loss"].mean())[0]


def test_saturated_softmax_gives_no_nan():
    """Every label the row's argmax and s = exp(8) = 2981: the softmax saturates (the other classes underflow), the loss and the
    gradient are tiny or zero and hold no NaN; exp(s u . T) without the shift by the maximum would overflow fp32."""
    shape = (33, 128, 32, 65)
    c = dict(case(shape))
    s = ref.scale_of(8.0)
    z64 = ref.torch_forward(*(torch.from_numpy(np.array(c[k])).double() for k in ("f", "T", "w1", "w2")), RATIO, s)[0].numpy()
    c["y"] = z64.argmax(axis=1).astype(np.int64)
    assert z64.max() > 89.0                                   # expf overflows beyond 88.7
    _, _, g1, g2, loss = device_step(c, s=s, momentum=0.9)
    o64 = ref.torch_step(c, RATIO, s, "float64")
    assert np.isfinite(g1).all() and np.isfinite(g2).all() and np.isfinite(loss) and loss >= 0.0
    say(f"saturated s={s:.1f}: loss64 {o64['row_loss'].mean():.3e} device {loss:.3e}  max|dw1| 64 {np.abs(o64['dw1']).max():.3e} device {np.abs(g1).max():.3e}")
    o32 = ref.torch_step(c, RATIO, s, "float32")
    for name, got in (("dw1", g1), ("dw2", g2)):
        assert float(np.abs(got - o64[name]).max()) <= ref.tolerance(o32[name], o64[name])[0]


def test_a_label_outside_the_classes_is_not_an_address():
    """Labels that arrive on the device are not range-checked by the host: a label outside [0, C) is never dereferenced, it makes the
    step's loss and the weights NaN."""
    c = case((5, 64, 16, 3))
    y = c["y"].copy()
    y[2] = 1 << 40
    w1, w2, _, _, loss = device_step(c, y=cuda(y))
    assert np.isnan(loss) and np.isnan(w1).any() and np.isnan(w2).any()
    with pytest.raises(ValueError, match="labels span"):
        device_step(c, y=y)                                   # host labels are checked


N_TRAJ, TRAJ_SHAPE = 70, (70, 128, 32, 10)
TRAJ_RATES = [0.002, 0.004, 0.001]
TRAJ_KW = dict(momentum=0.9, weight_decay=5e-4)


def _order(n, seed=5, epochs=3):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n) for _ in range(epochs)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def trajectory_oracle(drop_last):
    c = case(TRAJ_SHAPE, seed=7)
    kw = dict(TRAJ_KW, order=_order(N_TRAJ), drop_last=drop_last)
    return ref.torch_fit(c, RATIO, S, TRAJ_RATES, 32, dtype="float64", **kw), ref.torch_fit(c, RATIO, S, TRAJ_RATES, 32, dtype="float32", **kw)


def device_fit(drop_last):
    c = case(TRAJ_SHAPE, seed=7)
    return adapterfit.fit_adapter(cuda(c["f"]), c["y"], cuda(c["T"]), cuda(c["w1"]), cuda(c["w2"]), ratio=RATIO, epochs=3, batch_size=32,
                                  lr_per_epoch=TRAJ_RATES, order=_order(N_TRAJ), drop_last=drop_last, return_history=True, **TRAJ_KW)


@pytest.mark.parametrize("drop_last", [True, False])
def test_trajectory_and_determinism(drop_last):
    """N = 70 in batches of 32 for three epochs over a permuted order, momentum 0.9 and weight decay 5e-4: six steps with drop_last,
    nine (a short batch of 6 per epoch) without.  The final weights and the loss history against torch.optim.SGD in float64, inside the
    measured tolerance; a second run returns the same bits, in the weights and in the losses."""
    (w1_64, w2_64, l64), (w1_32, w2_32, l32) = trajectory_oracle(drop_last)
    w1, w2, losses = device_fit(drop_last)
    w1b, w2b, losses_b = device_fit(drop_last)
    assert torch.equal(w1, w1b) and torch.equal(w2, w2b) and np.array_equal(losses, losses_b)
    assert w1.dtype == w2.dtype == torch.float32 and losses.dtype == np.float32 and len(losses) == len(l64) == (6 if drop_last else 9)
    for name, got, t32, t64 in (("w1", w1.cpu().numpy(), w1_32, w1_64), ("w2", w2.cpu().numpy(), w2_32, w2_64), ("losses", losses, l32, l64)):
        tol, d = ref.tolerance(t32, t64)
        err = float(np.abs(got.astype(np.float64) - t64).max())
        say(f"trajectory drop_last={drop_last} {name}: max|value| {np.abs(t64).max():.4g}  device {err:.3e}  torch-fp32 d {d:.3e}  "
            f"ratio {err / d if d else float('inf'):.2f}  tolerance {tol:.3e}")
        assert err <= tol, name
    assert np.abs(w1_64 - case(TRAJ_SHAPE, seed=7)["w1"]).max() > 1e-4            # the run went somewhere


def test_train_step_gives_the_bits_of_fit():
    """AdapterFitState.step called batch by batch on gathered rows gives the bits adapter_fit leaves over the same order: weights,
    momentum buffers and every loss."""
    c = case(TRAJ_SHAPE, seed=7)
    order = _order(N_TRAJ)
    w1, w2, losses = device_fit(False)
    st = adapterfit.AdapterFitState(cuda(c["T"]), cuda(c["w1"]), cuda(c["w2"]), ratio=RATIO, **TRAJ_KW)
    f, y = cuda(c["f"]), cuda(c["y"])
    got = []
    for e, idx in ref.batches(N_TRAJ, 32, 3, order, False):
        idx = cuda(idx.astype(np.int64))
        got.append(st.step(f[idx], y[idx], TRAJ_RATES[e], want_loss=True))
    assert st.steps == 9
    assert torch.equal(st.w1, w1) and torch.equal(st.w2, w2) and np.array_equal(torch.cat(got).cpu().numpy(), losses)


def test_fit_adapter_end_to_end_on_the_tiny_model():
    """CustomCLIP.fit_adapter on 16 random images for two epochs: the second epoch's mean loss is below the first's, the module holds
    the fitted weights in its dtype, and the inference mirror uses them: _image_features is adapter_blend with the module's weights."""
    from clip_calibration_amd import synthetic as syn
    from clip_calibration_amd.model import build_model
    from clip_calibration_amd.trainers import CLIPAdapterCLIP
    model = build_model(dict(syn.synthetic_state_dict("tiny", seed=0)), {"trainer": "CoOp"}).cuda()
    Cn = 5
    ids = syn.synthetic_token_ids(Cn, "tiny", seed=90, n_ctx_placeholders=4)
    images = syn.synthetic_images(16, "tiny", seed=90)
    labels = torch.arange(16) % Cn
    loader = [(images[i:i + 8].cuda(), labels[i:i + 8]) for i in (0, 8)]
    torch.manual_seed(0)
    ad = CLIPAdapterCLIP(model, ids, n_ctx=4, ratio=0.2, seed=6)
    before = [ad.adapter.fc[i].weight.detach().clone() for i in (0, 2)]
    w1, w2, losses = ad.fit_adapter(loader, epochs=2, lr_per_epoch=[0.002, 0.002], batch_size=8, return_history=True)
    assert losses.shape == (4,) and np.isfinite(losses).all()
    say(f"end to end tiny: losses {losses.tolist()}")
    assert losses[2:].mean() < losses[:2].mean()
    assert all(p.grad is None for p in model.parameters()) and all(p.grad is None for p in ad.adapter.parameters())
    for i, fitted, old in ((0, w1, before[0]), (2, w2, before[1])):
        w = ad.adapter.fc[i].weight
        assert w.dtype == model.dtype and torch.equal(w, fitted.to(w.dtype)) and not torch.equal(w, old)
    img = images[:4].cuda()
    want = ops.adapter_blend(model.image_features_f32(img), ad.adapter.fc[0].weight.float(), ad.adapter.fc[2].weight.float(), 0.2)
    assert torch.equal(ad._image_features(img), want)
