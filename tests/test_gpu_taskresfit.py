"""TaskRes' training on the GPU (csrc/taskres_train.hip, clip_calibration_amd/taskresfit.py) against the float64 oracle of
tests/taskresfit_ref.py (torch's autograd, torch.optim.Adam and torch.optim.SGD in float64), which tests/test_taskresfit_cpu.py holds to
the formulas the kernels implement.  The tolerance of every compared quantity is measured: taskresfit_ref.tolerance takes FACTOR (4) times
the distance of torch's own fp32 CPU run of the same restatement from the oracle, with a floor of 2^-22 of the quantity's largest value.
Every test prints its figures on lines that start with "taskresfit-parity:"; profiles/taskresfit_parity.txt is one run's lines."""
import functools

import numpy as np
import pytest
import torch

import taskresfit_ref as ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import ops, taskresfit  # noqa: E402

S = ref.scale_of()
ALPHA = ref.ALPHA


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()             # a copy: the cached cases are read-only


def say(line):
    print("taskresfit-parity: " + line)


@functools.lru_cache(maxsize=None)
def case(shape, seed=11, zero_residuals=False):
    c = ref.make_case(*shape, seed=seed, zero_residuals=zero_residuals)
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def step_oracle(shape, alpha=ALPHA, s=S):
    """(float64 step, torch's fp32 step), computed once per case."""
    return ref.torch_step(case(shape), alpha, s, "float64"), ref.torch_step(case(shape), alpha, s, "float32")


def device_step(c, alpha=ALPHA, s=S, lr=1.0, optimizer="sgd", momentum=0.0, weight_decay=0.0, y=None, f=None):
    """One step from the case's residuals: (r', state1, state2, batch loss) as numpy."""
    st = taskresfit.TaskResFitState(cuda(c["base"]), torch.from_numpy(np.array(c["r"])), alpha=alpha, logit_scale=float(np.log(s)),
                                    optimizer=optimizer, momentum=momentum, weight_decay=weight_decay)
    st.scale = s
    loss = st.step(cuda(c["f"]) if f is None else f, c["y"] if y is None else y, lr, want_loss=True)
    s1, s2 = (None if t is None else t.cpu().numpy() for t in (st.state1, st.state2))
    return st.residuals.cpu().numpy(), s1, s2, float(loss.cpu()[0])


def device_row_losses(c, alpha=ALPHA, s=S):
    """Every row as a batch of its own at rate 0 (SGD, no momentum): the loss history is the row losses, the residuals stay."""
    n = c["f"].shape[0]
    r = cuda(c["r"])
    losses = ops.taskres_fit(cuda(c["f"]), cuda(c["y"]), cuda(c["base"]), r, None, None, torch.zeros(n).cuda(), alpha, s, 1, 1, optimizer="sgd",
                             want_losses=True)
    assert np.array_equal(r.cpu().numpy(), c["r"])
    return losses.cpu().numpy()


def compare(what, name, got, t32, t64):
    tol, d = ref.tolerance(t32, t64)
    err = float(np.abs(np.asarray(got, np.float64) - t64).max())
    say(f"{what} {name}: max|value| {np.abs(t64).max():.4g}  device {err:.3e}  torch-fp32 d {d:.3e}  ratio {err / d if d else float('inf'):.2f}  "
        f"tolerance {tol:.3e}")
    assert np.isfinite(got).all() and err <= tol, (what, name, err, tol)
    return tol


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_one_step_gradient(shape):
    """With momentum 0, weight decay 0 and lr 1 the SGD step is r' = r - g.  The gradient itself is read where the kernel leaves it
    unrounded -- the momentum buffer after a first step with a momentum holds g exactly -- and r' == fl(r - g) bit for bit.  g, the row
    losses and the batch loss against the float64 autograd; the batch loss is the float32 of the float64 mean of the device's row
    losses; g is tangent to the normalised row."""
    c = case(shape)
    o64, o32 = step_oracle(shape)
    ra, _, _, loss = device_step(c)
    rb, g, _, loss_b = device_step(c, momentum=0.9)
    assert np.array_equal(ra, rb) and loss == loss_b
    assert np.array_equal(ra, c["r"] - g)                                                    # fp32 arithmetic: fl(r - g)
    rows = device_row_losses(c)
    tol_g = compare(f"step B,E,C={shape}", "dr", g, o32["dr"], o64["dr"])
    compare(f"step B,E,C={shape}", "row_loss", rows, o32["row_loss"], o64["row_loss"])
    tol, _ = ref.tolerance(o32["row_loss"].mean(dtype=np.float64), o64["row_loss"].mean())
    assert abs(loss - o64["row_loss"].mean()) <= tol
    assert loss == float(np.float32(rows.astype(np.float64).mean()))                          # the float64 mean of the fp32 row losses
    u = ref.backward(c, ALPHA, S)["u"]
    tangent = float(np.abs((u * g.astype(np.float64)).sum(axis=1)).max())
    say(f"step B,E,C={shape} max|u . dr| {tangent:.3e}  (tolerance of dr {tol_g:.3e})")
    assert tangent <= tol_g


def test_alpha_zero_moves_the_residuals_by_weight_decay_only():
    """alpha = 0 takes the residuals out of the loss: the gradient is exactly zero, SGD's step is r' = r - lr * (wd * r), and Adam's
    moments stay zero without weight decay."""
    c = case((5, 64, 3))
    r, g, _, loss = device_step(c, alpha=0.0, momentum=0.9)
    assert not g.any() and np.array_equal(r, c["r"]) and np.isfinite(loss)
    wd, lr = np.float32(5e-4), np.float32(0.5)
    r, _, _, _ = device_step(c, alpha=0.0, lr=0.5, weight_decay=5e-4)
    assert np.array_equal(r, c["r"] - lr * (wd * c["r"]))
    r, m, v, _ = device_step(c, alpha=0.0, lr=0.5, optimizer="adam")
    assert not m.any() and not v.any() and np.array_equal(r, c["r"])


def test_first_adam_step_moves_by_the_rate():
    """One Adam step from zero residuals without weight decay: m / (1 - b1) = g and sqrt(v / (1 - b2)) = |g|, so every element whose
    gradient is not tiny moves by lr against the gradient's sign; then every element against torch.optim.Adam in float64."""
    shape, lr = (33, 128, 65), 2e-3
    c = case(shape, zero_residuals=True)
    g64 = ref.torch_step(c, ALPHA, S)["dr"]
    r, m, v, _ = device_step(c, lr=lr, optimizer="adam")
    big = np.abs(g64) > 1e-4
    assert big.sum() > 100
    want = {dt: ref.torch_fit(c, ALPHA, S, [lr], shape[0], "adam", dtype=dt)[0] for dt in ("float64", "float32")}
    tol = compare(f"adam first step B,E,C={shape}", "r", r, want["float32"], want["float64"])
    assert np.abs(r[big] + lr * np.sign(g64[big])).max() <= tol + lr * 1e-8 / 1e-4              # eps / |g| of the rate stays behind
    assert (np.sign(r[big]) == -np.sign(g64[big])).all()


def test_saturated_softmax_gives_no_nan():
    """Every label the row's argmax and s = exp(8) = 2981: the softmax saturates (the other classes underflow), the loss and the
    gradient are tiny or zero and hold no NaN; exp(z) without the shift by the maximum would overflow fp32."""
    shape = (33, 128, 65)
    c = dict(case(shape))
    s = ref.scale_of(8.0)
    z64 = ref.torch_step(c, ALPHA, s)["z"]
    c["y"] = z64.argmax(axis=1).astype(np.int64)
    assert z64.max() > 89.0                                   # expf overflows beyond 88.7
    _, g, _, loss = device_step(c, s=s, momentum=0.9)
    o64, o32 = ref.torch_step(c, ALPHA, s, "float64"), ref.torch_step(c, ALPHA, s, "float32")
    assert np.isfinite(g).all() and np.isfinite(loss) and loss >= 0.0
    say(f"saturated s={s:.1f}: loss64 {o64['row_loss'].mean():.3e} device {loss:.3e}")
    compare(f"saturated B,E,C={shape}", "dr", g, o32["dr"], o64["dr"])


def test_a_label_outside_the_classes_is_not_an_address():
    """Labels that arrive on the device are not range-checked by the host: a label outside [0, C) is never dereferenced, it makes the
    step's loss and the residuals NaN."""
    c = case((5, 64, 3))
    y = c["y"].copy()
    y[2] = 1 << 40
    r, _, _, loss = device_step(c, y=cuda(y))
    assert np.isnan(loss) and np.isnan(r).any()
    with pytest.raises(ValueError, match="labels span"):
        device_step(c, y=y)                                   # host labels are checked


def test_a_column_slice_gives_the_bits_of_the_contiguous_copy():
    """Features passed as a column slice of a wider matrix (ld > E) are read in place."""
    shape = (40, 96, 130)
    c = case(shape)
    wide = torch.full((40, 96 + 37), float("nan")).cuda()
    wide[:, 5:5 + 96] = cuda(c["f"])
    sl = wide[:, 5:5 + 96]
    assert sl.stride(0) == 133 and not sl.is_contiguous()
    for opt in ("sgd", "adam"):
        a, b = device_step(c, optimizer=opt, lr=0.01, momentum=0.9), device_step(c, optimizer=opt, lr=0.01, momentum=0.9, f=sl)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3] and np.isfinite(a[0]).all()


N_TRAJ, TRAJ_SHAPE = 70, (70, 128, 10)
TRAJ_RATES = [2e-4, 4e-4, 1e-4]
TRAJ_KW = {"adam": dict(optimizer="adam", weight_decay=5e-4), "sgd": dict(optimizer="sgd", momentum=0.9, weight_decay=5e-4)}


def _order(n, seed=5, epochs=3):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n) for _ in range(epochs)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def trajectory_oracle(optimizer, drop_last):
    c = case(TRAJ_SHAPE, seed=7)
    kw = dict(TRAJ_KW[optimizer], order=_order(N_TRAJ), drop_last=drop_last)
    return ref.torch_fit(c, ALPHA, S, TRAJ_RATES, 32, dtype="float64", **kw), ref.torch_fit(c, ALPHA, S, TRAJ_RATES, 32, dtype="float32", **kw)


def device_fit(optimizer, drop_last):
    c = case(TRAJ_SHAPE, seed=7)
    return taskresfit.fit_residuals(cuda(c["f"]), c["y"], cuda(c["base"]), cuda(c["r"]), alpha=ALPHA, epochs=3, batch_size=32,
                                    lr_per_epoch=TRAJ_RATES, order=_order(N_TRAJ), drop_last=drop_last, return_history=True, **TRAJ_KW[optimizer])


@pytest.mark.parametrize("drop_last", [True, False])
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_trajectory_and_determinism(optimizer, drop_last):
    """N = 70 in batches of 32 for three epochs over a permuted order with weight decay 5e-4: six steps with drop_last, nine (a short
    batch of 6 per epoch) without.  The final residuals and the loss history against torch's optimiser in float64, inside the measured
    tolerance; a second run returns the same bits, in the residuals and in the losses."""
    (r64, l64), (r32, l32) = trajectory_oracle(optimizer, drop_last)
    r, losses = device_fit(optimizer, drop_last)
    rb, losses_b = device_fit(optimizer, drop_last)
    assert torch.equal(r, rb) and np.array_equal(losses, losses_b)
    assert r.dtype == torch.float32 and losses.dtype == np.float32 and len(losses) == len(l64) == (6 if drop_last else 9)
    what = f"trajectory {optimizer} drop_last={drop_last}"
    compare(what, "r", r.cpu().numpy(), r32, r64)
    compare(what, "losses", losses, l32, l64)
    assert np.abs(r64 - case(TRAJ_SHAPE, seed=7)["r"]).max() > 1e-4                            # the run went somewhere


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_train_step_gives_the_bits_of_fit(optimizer):
    """TaskResFitState.step called batch by batch on gathered rows gives the bits taskres_fit leaves over the same order: residuals,
    optimiser state and every loss."""
    c = case(TRAJ_SHAPE, seed=7)
    order = _order(N_TRAJ)
    kw = dict(TRAJ_KW[optimizer])
    name = kw.pop("optimizer")
    f, y, base = cuda(c["f"]), cuda(c["y"]), cuda(c["base"])
    # the fit with its state in hand: ops.taskres_fit on buffers of the test's own
    r = cuda(c["r"])
    s1, s2 = torch.zeros_like(r), (torch.zeros_like(r) if name == "adam" else None)
    rates = torch.from_numpy(np.repeat(np.asarray(TRAJ_RATES, np.float64), 3).astype(np.float32)).cuda()
    losses = ops.taskres_fit(f, y, base, r, s1, s2, rates, ALPHA, S, 32, 3, name, order=cuda(order), drop_last=False, want_losses=True, **kw)
    r_fit, losses_fit = device_fit(optimizer, False)
    assert torch.equal(r, r_fit) and np.array_equal(losses.cpu().numpy(), losses_fit)
    st = taskresfit.TaskResFitState(base, cuda(c["r"]), alpha=ALPHA, optimizer=name, **kw)
    got = []
    for e, idx in ref.batches(N_TRAJ, 32, 3, order, False):
        idx = cuda(idx.astype(np.int64))
        got.append(st.step(f[idx], y[idx], TRAJ_RATES[e], want_loss=True))
    assert st.steps == 9
    assert torch.equal(st.residuals, r) and torch.equal(st.state1, s1) and (s2 is None or torch.equal(st.state2, s2))
    assert np.array_equal(torch.cat(got).cpu().numpy(), losses_fit)


def test_fit_residuals_end_to_end_on_the_tiny_model():
    """TaskResCLIP.fit_residuals on 16 random images for two epochs with three templates per class: the second epoch's mean loss is
    below the first's, no .grad is set, the module holds the fitted residuals, and the inference forward uses them."""
    from clip_calibration_amd import synthetic as syn
    from clip_calibration_amd.model import build_model
    from clip_calibration_amd.trainers import TaskResCLIP
    model = build_model(dict(syn.synthetic_state_dict("tiny", seed=0)), {"trainer": "CoOp"}).cuda()
    Cn, T = 5, 3
    ids = torch.stack([syn.synthetic_token_ids(Cn, "tiny", seed=90 + i) for i in range(T)], dim=1)      # [C, T, 77]
    images = syn.synthetic_images(16, "tiny", seed=90)
    labels = torch.arange(16) % Cn
    loader = [(images[i:i + 8].cuda(), labels[i:i + 8]) for i in (0, 8)]
    tr = TaskResCLIP(model, ids, alpha=0.5)
    res = tr.prompt_learner.text_feature_residuals
    assert not res.detach().any()
    fitted, losses = tr.fit_residuals(loader, epochs=2, lr_per_epoch=[2e-3, 2e-3], batch_size=8, return_history=True)
    assert losses.shape == (4,) and np.isfinite(losses).all()
    say(f"end to end tiny: losses {losses.tolist()}")
    assert losses[2:].mean() < losses[:2].mean()
    assert all(p.grad is None for p in model.parameters()) and all(p.grad is None for p in tr.parameters())
    assert fitted.dtype == torch.float32 and torch.equal(res.detach(), fitted.to(res.dtype)) and res.detach().any()
    img = images[:4].cuda()
    text = ops.l2_normalize(ops.scale_add(tr.prompt_learner.base_text_features, res.detach(), 0.5))
    want = ops.fused_tail(model.image_features_f32(img), text, tr.scale, None, False)[0]
    assert torch.equal(tr.forward(img)[0], want)
