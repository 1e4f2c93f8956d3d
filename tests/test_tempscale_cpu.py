"""TempScaling's fit without a GPU: the float64 restatement (tests/tempscale_ref.py) against torch's own step, the schedule helper
against torch's CosineAnnealingLR, the C entries' argument validation and the host-side checks of clip_calibration_amd/tempfit.py."""
import ctypes

import numpy as np
import pytest
import torch

import tempscale_ref as ref
from clip_calibration_amd import _lib, ops, tempfit

N, C = 150, 23
SCHED = ref.cosine_warmup_schedule(0.005, 3)


def _order(seed, epochs=3, n=N):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n) for _ in range(epochs)]).astype(np.int32)


@pytest.mark.parametrize("batching", ["short_last", "drop_last", "order", "whole"])
@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.9, False), (0.9, True)])
@pytest.mark.parametrize("weight_decay", [0.0, 5e-4])
def test_restatement_is_torchs_step(momentum, nesterov, weight_decay, batching):
    """The step the reference performs (tempscaling.py:156-160) -- F.cross_entropy, backward, torch.optim.SGD.step, in float64 on the CPU --
    against the numpy restatement: the final theta and every step's loss to 1e-12 relative.  Batches of 32 (150 rows: a last batch of 22,
    or dropped), of 150, and a shuffled order.  The batches hold rows with a wrong label, so every batch loss is of order 1 or more: the
    loss of a single confidently right row is log(1 + 1e-7), which float64 gives to 1e-9 relative only, in torch as in numpy."""
    c, y = ref.make_case(N, C, seed=3)
    kw = dict(momentum=momentum, weight_decay=weight_decay, nesterov=nesterov, drop_last=batching == "drop_last",
              order=_order(5) if batching == "order" else None)
    batch = N if batching == "whole" else 32
    theta, losses = ref.fit(c, y, 4.6052, SCHED, batch, **kw)
    t_theta, t_losses = ref.torch_fit(c, y, 4.6052, SCHED, batch, dtype="float64", **kw)
    assert len(losses) == len(t_losses) == 3 * {"short_last": 5, "drop_last": 4, "order": 5, "whole": 1}[batching]
    assert min(losses) > 0.5
    assert abs(theta - t_theta) <= 1e-12 * abs(t_theta)
    np.testing.assert_allclose(losses, t_losses, rtol=1e-12, atol=0)
    assert abs(theta - 4.6052) > 1e-3                       # the run went somewhere


def test_restatement_applies_dampening():
    c, y = ref.make_case(N, C, seed=4)
    theta, losses = ref.fit(c, y, 4.6052, SCHED, 32, momentum=0.9, dampening=0.3)
    t_theta, t_losses = ref.torch_fit(c, y, 4.6052, SCHED, 32, momentum=0.9, dampening=0.3)
    assert abs(theta - t_theta) <= 1e-12 * abs(t_theta)
    np.testing.assert_allclose(losses, t_losses, rtol=1e-12, atol=0)


def test_gradient_is_autograds():
    c, y = ref.make_case(40, 11, seed=6)
    for theta in (0.0, 4.6052, 6.5):
        t = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
        loss = torch.nn.functional.cross_entropy(t.exp() * torch.from_numpy(c).double(), torch.from_numpy(y))
        loss.backward()
        got = ref.batch_loss_grad(c, y, theta)
        assert got[0] == pytest.approx(float(loss.detach()), rel=1e-12) and got[1] == pytest.approx(float(t.grad), rel=1e-11)


@pytest.mark.parametrize("epochs,warmup", [(20, 1), (3, 1), (7, 0), (10, 3)])
def test_schedule_is_cosine_annealing_after_the_warmup(epochs, warmup):
    """Hand-over rule (tempfit.cosine_warmup_schedule): the warm-up epochs run at the constant rate; the cosine scheduler is stepped for
    the first time at the end of the last warm-up epoch, so epoch e >= warmup runs at torch's CosineAnnealingLR(T_max=epochs) value of
    index e - warmup + 1 (index e without a warm-up).  torch's values come from its recursive form: 1e-12 relative, 1e-18 absolute at
    the zero of the cosine."""
    lr = 0.05
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, epochs)
    cos = []
    for _ in range(epochs + 1):
        cos.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    for got in (tempfit.cosine_warmup_schedule(lr, epochs, warmup, 1e-5), ref.cosine_warmup_schedule(lr, epochs, warmup, 1e-5)):
        assert len(got) == epochs and got[:warmup] == [1e-5] * warmup
        want = [cos[e - warmup + 1 if warmup else e] for e in range(warmup, epochs)]
        np.testing.assert_allclose(got[warmup:], want, rtol=1e-12, atol=1e-18)
    assert tempfit.cosine_warmup_schedule(lr, 0) == []
    with pytest.raises(ValueError):
        tempfit.cosine_warmup_schedule(lr, -1)


def test_entries_validate_arguments_without_a_gpu():
    L = _lib.lib
    p = ctypes.c_void_p(4096)
    assert L.clipmi_tempscale_workspace_bytes(100) >= 800 and L.clipmi_tempscale_workspace_bytes(0) == 0
    big = 1 << 20

    def fit(cos=p, ld=37, lab=p, order=None, n=300, C=37, batch=100, epochs=3, drop=0, lr=p, mom=0.9, damp=0.0, wd=5e-4, nest=0, state=p,
            losses=None, ws=p, ws_bytes=big):
        return L.clipmi_tempscale_fit(cos, ld, lab, order, n, C, batch, epochs, drop, lr, mom, damp, wd, nest, state, losses, ws, ws_bytes, None)
    for null in ("cos", "lab", "lr", "state", "ws"):
        assert fit(**{null: None}) == _lib.ERR_ARG and "null" in _lib.last_error(), null
    assert fit(C=1, ld=1) == _lib.ERR_SHAPE and "C=1" in _lib.last_error()
    assert fit(n=0) == _lib.ERR_SHAPE
    assert fit(batch=0) == _lib.ERR_SHAPE and "batch=0" in _lib.last_error()
    assert fit(epochs=-1) == _lib.ERR_ARG and "epochs=-1" in _lib.last_error()
    assert fit(ld=36) == _lib.ERR_SHAPE and "ld=36" in _lib.last_error()
    for bad in (-0.1, 1.0, float("nan")):
        assert fit(mom=bad) == _lib.ERR_ARG and "momentum" in _lib.last_error()
        assert fit(damp=bad) == _lib.ERR_ARG and "dampening" in _lib.last_error()
    assert fit(wd=-1e-3) == _lib.ERR_ARG and fit(wd=float("inf")) == _lib.ERR_ARG
    assert fit(nest=1, mom=0.0) == _lib.ERR_ARG and "nesterov" in _lib.last_error()
    assert fit(nest=1, mom=0.9, damp=0.1) == _lib.ERR_ARG and "nesterov" in _lib.last_error()
    assert fit(ws_bytes=100 * 8 - 1) == _lib.ERR_WORKSPACE
    assert fit(ws=ctypes.c_void_p(4100)) == _lib.ERR_ARG and "aligned" in _lib.last_error()
    assert fit(epochs=0) == _lib.OK                                                     # nothing to launch
    assert fit(batch=400, drop=1) == _lib.OK                                            # every batch dropped

    def batch(cos=p, ld=37, lab=p, order=None, rows=8, n=300, C=37, theta=p, out=p, ws=p, ws_bytes=big):
        return L.clipmi_tempscale_batch(cos, ld, lab, order, rows, n, C, theta, out, ws, ws_bytes, None)
    for null in ("cos", "lab", "theta", "out", "ws"):
        assert batch(**{null: None}) == _lib.ERR_ARG and "null" in _lib.last_error(), null
    assert batch(C=1, ld=1) == _lib.ERR_SHAPE and batch(rows=0) == _lib.ERR_SHAPE and batch(ld=36) == _lib.ERR_SHAPE
    assert batch(rows=301) == _lib.ERR_SHAPE and "without an order" in _lib.last_error()
    assert batch(ws_bytes=8) == _lib.ERR_WORKSPACE
    if not torch.cuda.is_available():                  # valid arguments reach the launch, which fails loudly without a device
        assert fit() == _lib.ERR_HIP and _lib.last_error()
        assert batch() == _lib.ERR_HIP and _lib.last_error()
        assert batch(rows=301, order=p) == _lib.ERR_HIP


def test_host_checks_come_before_any_launch():
    """Labels outside [0, C), a wrong order and bad optimiser settings are refused on the host -- with CPU tensors too, so before the
    device is looked at; valid CPU input then meets the library's no-CPU-fallback error."""
    c, y = ref.make_case(20, 5, seed=1)
    ct = torch.from_numpy(c)
    for bad in (5, -1):
        yb = y.copy()
        yb[7] = bad
        with pytest.raises(ValueError, match="labels span"):
            tempfit.fit_logit_scale(ct, torch.from_numpy(yb), epochs=2)
    with pytest.raises(ValueError, match="labels"):
        tempfit.fit_logit_scale(ct, y[:-1])
    with pytest.raises(TypeError):
        tempfit.fit_logit_scale(ct, y.astype(np.float32))
    with pytest.raises(ValueError, match="order"):
        tempfit.fit_logit_scale(ct, y, epochs=2, order=np.zeros((2, 19), np.int32))
    with pytest.raises(ValueError, match="order"):
        tempfit.fit_logit_scale(ct, y, epochs=1, order=np.full((1, 20), 20, np.int32))
    with pytest.raises(ValueError, match="Nesterov"):
        tempfit.fit_logit_scale(ct, y, nesterov=True, momentum=0.0)
    with pytest.raises(ValueError, match="momentum"):
        tempfit.fit_logit_scale(ct, y, momentum=1.0)
    with pytest.raises(ValueError, match="learning rates"):
        tempfit.fit_logit_scale(ct, y, epochs=3, lr_per_epoch=[0.1, 0.1])
    with pytest.raises(ValueError):
        tempfit.fit_logit_scale(ct[:, :1], np.zeros(20, np.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tempfit.fit_logit_scale(ct, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tempscale_batch(ct, torch.from_numpy(y), torch.tensor([4.6052]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tempscale_fit(ct, torch.from_numpy(y), torch.zeros(4), torch.zeros(3), 20, 3)
