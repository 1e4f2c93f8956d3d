"""CLIP-Adapter's training without a GPU: the hand-derived backward (tests/adapterfit_ref.py) against torch's autograd in float64, the
seeds of the GPU test against the ReLU-kink cap, the host-side checks of clip_calibration_amd/adapterfit.py and the C entries' argument
validation."""
import ctypes

import numpy as np
import pytest
import torch

import adapterfit_ref as ref
from clip_calibration_amd import _lib, adapterfit, ops

S = ref.scale_of()


@pytest.mark.parametrize("ratio", [0.2, 1.0, 0.0])
@pytest.mark.parametrize("shape", sorted(ref.SHAPES))
def test_hand_derived_backward_is_autograds(shape, ratio):
    """dW1, dW2 of the mean loss and the row losses: numpy float64 by the formulas the kernels implement against torch's float64
    autograd of the restated forward, to 1e-12 of each matrix's largest entry."""
    case = ref.make_case(*shape, seed=ref.SHAPES[shape])
    got, want = ref.backward(case, ratio, S), ref.torch_step(case, ratio, S)
    np.testing.assert_allclose(got["row_loss"], want["row_loss"], rtol=1e-12, atol=1e-12)
    for k in ("dw1", "dw2"):
        scale = float(np.abs(want[k]).max())
        assert float(np.abs(got[k] - want[k]).max()) <= 1e-12 * scale, k
        assert (scale > 0) == (ratio != 0.0)            # ratio 0 takes the adapter out of the loss: both gradients vanish identically


@pytest.mark.parametrize("shape", sorted(ref.SHAPES))
def test_seeds_keep_the_kink_exclusion_below_the_cap(shape):
    """The GPU test leaves out the gradient entries that depend on a ReLU whose float64 pre-activation lies below 1e-4 of its matrix's
    largest: with the seeds of adapterfit_ref.SHAPES that is at most 1 % of the entries, by the oracle alone."""
    B, E, H, C = shape
    o = ref.torch_step(ref.make_case(*shape, seed=ref.SHAPES[shape]), 0.2, S)
    x1, x2 = ref.excluded(ref.kinks(o["p1"], o["p2"]), E, H)
    assert ref.excluded_share(x1, x2) <= ref.EXCLUDED_CAP
    # the report itself: a planted pre-activation at the kink is found, and its dependants are the documented ones
    p1, p2 = o["p1"].copy(), o["p2"].copy()
    p1[0, 3] = 0.5 * ref.KINK * np.abs(p1).max()
    planted = ref.kinks(p1, p2)
    assert ("p1", 0, 3) in planted
    x1, x2 = ref.excluded([("p1", 0, 3)], E, H)
    assert x1[3].all() and x1.sum() == E and not x2.any()
    x1, x2 = ref.excluded([("p2", 0, 5)], E, H)
    assert x1.all() and x2[5].all() and x2.sum() == H


@pytest.mark.parametrize("momentum,nesterov,dampening", [(0.0, False, 0.0), (0.9, False, 0.0), (0.9, True, 0.0), (0.9, False, 0.3)])
def test_sgd_rule_on_the_hand_derived_gradient_is_torchs_fit(momentum, nesterov, dampening):
    """Three epochs over N = 23 in batches of 8 (a short batch of 7) with a permuted order: torch.optim.SGD in float64 against the rule
    of include/clipmi.h applied in numpy to the hand-derived gradients, 1e-11 of the largest weight."""
    N, E, H, C = 23, 32, 8, 5
    case = ref.make_case(N, E, H, C, seed=2)
    rng = np.random.default_rng(3)
    order = np.stack([rng.permutation(N) for _ in range(3)]).astype(np.int32)
    rates, wd = [0.01, 0.02, 0.005], 5e-4
    w1t, w2t, losses_t = ref.torch_fit(case, 0.2, S, rates, 8, momentum, dampening, wd, nesterov, order)
    w = {k: case[k].astype(np.float64) for k in ("w1", "w2")}
    buf, losses = {}, []
    for step, (e, idx) in enumerate(ref.batches(N, 8, 3, order)):
        b = ref.backward(dict(case, f=case["f"][idx], y=case["y"][idx], **w), 0.2, S)
        losses.append(b["row_loss"].mean())
        for k in ("w1", "w2"):
            g = b["d" + k] + wd * w[k]
            if momentum:
                buf[k] = g if step == 0 else momentum * buf[k] + (1 - dampening) * g
                g = g + momentum * buf[k] if nesterov else buf[k]
            w[k] = w[k] - rates[e] * g
    np.testing.assert_allclose(losses, losses_t, rtol=1e-11)
    assert np.abs(w["w1"] - w1t).max() <= 1e-11 * np.abs(w1t).max() and np.abs(w["w2"] - w2t).max() <= 1e-11 * np.abs(w2t).max()
    assert np.abs(w1t - case["w1"]).max() > 1e-4                      # the run went somewhere


def _host_case():
    case = ref.make_case(20, 16, 4, 5, seed=1)
    return tuple(torch.from_numpy(case[k]) for k in ("f", "T", "w1", "w2")) + (case["y"],)


def test_host_checks_come_before_any_launch():
    """Labels outside [0, C), a wrong order, shapes that do not chain and bad optimiser settings are refused on the host -- with CPU
    tensors too, so before the device is looked at; valid CPU input then meets the library's no-CPU-fallback error."""
    f, T, w1, w2, y = _host_case()
    fit = adapterfit.fit_adapter
    for bad in (5, -1):
        yb = y.copy()
        yb[7] = bad
        with pytest.raises(ValueError, match="labels span"):
            fit(f, torch.from_numpy(yb), T, w1, w2, epochs=2)
    with pytest.raises(ValueError, match="labels"):
        fit(f, y[:-1], T, w1, w2)
    with pytest.raises(TypeError):
        fit(f, y.astype(np.float32), T, w1, w2)
    with pytest.raises(ValueError, match="order"):
        fit(f, y, T, w1, w2, epochs=2, order=np.zeros((2, 19), np.int32))
    with pytest.raises(ValueError, match="order"):
        fit(f, y, T, w1, w2, epochs=1, order=np.full((1, 20), 20, np.int32))
    with pytest.raises(ValueError, match="order"):
        fit(f, y, T, w1, w2, epochs=1, order=np.full((1, 20), -1, np.int32))
    with pytest.raises(ValueError, match="do not chain"):
        fit(f, y, T, w1, w2[:, :3])
    with pytest.raises(ValueError, match="do not chain"):
        fit(f, y, T, w1[:, :15], w2)
    with pytest.raises(ValueError, match="text features"):
        fit(f, y, T[:, :15], w1, w2)
    with pytest.raises(ValueError, match="text features"):
        fit(f, y, T[:1], w1, w2)
    with pytest.raises(ValueError, match="Nesterov"):
        fit(f, y, T, w1, w2, nesterov=True, momentum=0.0)
    with pytest.raises(ValueError, match="Nesterov"):
        fit(f, y, T, w1, w2, nesterov=True, dampening=0.1)
    with pytest.raises(ValueError, match="momentum"):
        fit(f, y, T, w1, w2, momentum=1.0)
    with pytest.raises(ValueError, match="learning rates"):
        fit(f, y, T, w1, w2, epochs=3, lr_per_epoch=[0.1, 0.1])
    with pytest.raises(ValueError, match="batch_size"):
        fit(f, y, T, w1, w2, batch_size=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit(f, y, T, w1, w2, epochs=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        adapterfit.AdapterFitState(T, w1, w2)
    yt = torch.from_numpy(y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.adapter_train_step(f, yt, T, w1.clone(), w2.clone(), None, None, torch.zeros(1), 0.2, 100.0, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.adapter_fit(f, yt, T, w1.clone(), w2.clone(), None, None, torch.zeros(3), 0.2, 100.0, 8, 1)
    assert adapterfit.steps_per_epoch(70, 32, True) == 2 and adapterfit.steps_per_epoch(70, 32, False) == 3


P = ctypes.c_void_p(4096)


def test_entries_validate_arguments_without_a_gpu():
    """clipmi_adapter_train_step and clipmi_adapter_fit refuse, before any launch: null or misaligned pointers, C < 2, H < 1, E or H
    beyond the kernel's LDS plan, bad optimiser settings and a workspace too small for the batch."""
    L = _lib.lib
    need = L.clipmi_adapter_train_workspace_bytes
    assert need(32, 512, 128, 100) >= 32 * (512 + 2 * 128 + 100 + 1) * 4 and need(32, 512, 128, 100) % 256 == 0
    assert need(0, 512, 128, 100) == 0 and need(32, 0, 128, 100) == 0 and need(32, 512, 0, 100) == 0 and need(32, 512, 128, 1) == 0
    big = 1 << 24

    def fit(feats=P, ld=512, lab=P, order=None, text=P, w1=P, w2=P, m1=P, m2=P, n=70, E=512, H=128, C=100, batch=32, epochs=3, drop=0,
            ratio=0.2, scale=100.0, lr=P, first=1, mom=0.9, damp=0.0, wd=5e-4, nest=0, losses=None, ws=P, ws_bytes=big):
        return L.clipmi_adapter_fit(feats, ld, lab, order, text, w1, w2, m1, m2, n, E, H, C, batch, epochs, drop, ratio, scale, lr, first, mom,
                                    damp, wd, nest, losses, ws, ws_bytes, None)

    def step(feats=P, ld=512, lab=P, text=P, w1=P, w2=P, m1=P, m2=P, rows=32, E=512, H=128, C=100, ratio=0.2, scale=100.0, lr=P, first=1,
             mom=0.9, damp=0.0, wd=5e-4, nest=0, loss=None, ws=P, ws_bytes=big):
        return L.clipmi_adapter_train_step(feats, ld, lab, text, w1, w2, m1, m2, rows, E, H, C, ratio, scale, lr, first, mom, damp, wd, nest,
                                           loss, ws, ws_bytes, None)

    for f in (fit, step):
        for null in ("feats", "lab", "text", "w1", "w2", "lr", "ws", "m1", "m2"):
            assert f(**{null: None}) == _lib.ERR_ARG and "null" in _lib.last_error(), null
        for odd in ("feats", "text", "w1", "w2", "m1", "m2", "lr"):
            assert f(**{odd: ctypes.c_void_p(4098)}) == _lib.ERR_ARG and "aligned" in _lib.last_error(), odd
        assert f(lab=ctypes.c_void_p(4100)) == _lib.ERR_ARG and "aligned" in _lib.last_error()
        assert f(ws=ctypes.c_void_p(4100)) == _lib.ERR_ARG and "aligned" in _lib.last_error()
        assert f(C=1) == _lib.ERR_SHAPE and "C=1" in _lib.last_error()
        assert f(H=0) == _lib.ERR_SHAPE and "H=0" in _lib.last_error()
        assert f(E=0, ld=0) == _lib.ERR_SHAPE
        assert f(E=16384, ld=16384) == _lib.ERR_SHAPE and "LDS" in _lib.last_error()
        assert f(H=1 << 16) == _lib.ERR_SHAPE and "LDS" in _lib.last_error()
        assert f(ld=511) == _lib.ERR_SHAPE and "ld=511" in _lib.last_error()
        for bad in (-0.1, 1.0, float("nan")):
            assert f(mom=bad) == _lib.ERR_ARG and "momentum" in _lib.last_error()
            assert f(damp=bad) == _lib.ERR_ARG and "dampening" in _lib.last_error()
        assert f(wd=-1e-3) == _lib.ERR_ARG and f(wd=float("inf")) == _lib.ERR_ARG
        assert f(nest=1, mom=0.0) == _lib.ERR_ARG and "nesterov" in _lib.last_error()
        assert f(nest=1, mom=0.9, damp=0.1) == _lib.ERR_ARG and "nesterov" in _lib.last_error()
        assert f(ratio=float("nan")) == _lib.ERR_ARG and f(scale=float("inf")) == _lib.ERR_ARG
        assert f(ws_bytes=need(32, 512, 128, 100) - 1) == _lib.ERR_WORKSPACE and "needed" in _lib.last_error()
    assert fit(n=0) == _lib.ERR_SHAPE and step(rows=0) == _lib.ERR_SHAPE
    assert fit(batch=0) == _lib.ERR_SHAPE and "batch=0" in _lib.last_error()
    assert fit(epochs=-1) == _lib.ERR_ARG and "epochs=-1" in _lib.last_error()
    # arguments that pass every check stop short of a launch here (every batch dropped): nothing in this test may reach a device
    assert fit(m1=None, m2=None, mom=0.0, batch=400, drop=1) == _lib.OK                  # no momentum, no buffers
    assert fit(n=20, batch=32, drop=1, ws_bytes=need(20, 512, 128, 100)) == _lib.OK      # the widest batch is the whole set
    assert fit(n=20, batch=32, drop=1, ws_bytes=need(20, 512, 128, 100) - 1) == _lib.ERR_WORKSPACE
    assert fit(E=64, ld=64, H=256, batch=400, drop=1) == _lib.OK                         # H > E is inside the LDS plan
    assert fit(epochs=0) == _lib.OK                                                      # nothing to launch
    assert fit(batch=400, drop=1) == _lib.OK                                             # every batch dropped
    if not torch.cuda.is_available():                  # valid arguments reach the launch, which fails loudly without a device
        assert fit() == _lib.ERR_HIP and _lib.last_error()
        assert step() == _lib.ERR_HIP and _lib.last_error()
        assert step(m1=None, m2=None, mom=0.0) == _lib.ERR_HIP                           # no momentum, no buffers
