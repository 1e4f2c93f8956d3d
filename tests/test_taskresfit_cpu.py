"""TaskRes' training without a GPU: the hand-derived backward and the Adam rule (tests/taskresfit_ref.py) against torch in float64, the
host-side checks of clip_calibration_amd/taskresfit.py and the C entries' argument validation."""
import ctypes

import numpy as np
import pytest
import torch

import taskresfit_ref as ref
from clip_calibration_amd import _lib, ops, taskresfit

S = ref.scale_of()


@pytest.mark.parametrize("alpha", [0.5, 1.0, 0.0])
@pytest.mark.parametrize("shape", ref.CPU_SHAPES)
def test_hand_derived_backward_is_autograds(shape, alpha):
    """dr of the mean loss and the row losses: numpy float64 by the formulas the kernels implement against torch's float64 autograd of
    the restated forward, to 1e-12 of the gradient's largest entry; the gradient is tangent to the normalised row."""
    case = ref.make_case(*shape, seed=3)
    got, want = ref.backward(case, alpha, S), ref.torch_step(case, alpha, S)
    np.testing.assert_allclose(got["row_loss"], want["row_loss"], rtol=1e-12, atol=1e-12)
    scale = float(np.abs(want["dr"]).max())
    assert float(np.abs(got["dr"] - want["dr"]).max()) <= 1e-12 * scale
    assert (scale > 0) == (alpha != 0.0)                # alpha 0 takes the residuals out of the loss
    assert float(np.abs((got["u"] * got["dr"]).sum(axis=1)).max()) <= 1e-12 * max(scale, 1e-300)


@pytest.mark.parametrize("weight_decay", [0.0, 5e-4])
def test_adam_rule_is_torchs(weight_decay):
    """Seven steps of torch.optim.Adam in float64 on fixed gradients with changing rates against the numpy restatement of the rule in
    include/clipmi.h, to 1e-13 of the largest weight."""
    rng = np.random.default_rng(0)
    w0 = rng.normal(size=(6, 9))
    grads = [rng.normal(size=(6, 9)) * 10.0 ** rng.integers(-4, 1) for _ in range(7)]
    rates = [2e-4, 4e-4, 1e-4, 1e-3, 1e-5, 2e-3, 3e-4]
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.Adam([p], lr=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    w, m, v = w0.copy(), np.zeros_like(w0), np.zeros_like(w0)
    for t, (g, lr) in enumerate(zip(grads, rates), start=1):
        opt.param_groups[0]["lr"] = lr
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        w, m, v = ref.adam_rule(w, g, m, v, t, lr, weight_decay=weight_decay)
        assert np.abs(w - p.detach().numpy()).max() <= 1e-13 * np.abs(w).max(), t
    st = opt.state[p]
    assert np.abs(m - st["exp_avg"].numpy()).max() <= 1e-13 * np.abs(m).max()
    assert np.abs(v - st["exp_avg_sq"].numpy()).max() <= 1e-13 * np.abs(v).max()
    assert np.abs(w - w0).max() > 1e-4


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_rule_on_the_hand_derived_gradient_is_torchs_fit(optimizer):
    """Three epochs over N = 23 in batches of 8 (a short batch of 7) with a permuted order: torch's optimiser in float64 against the
    rules of include/clipmi.h applied in numpy to the hand-derived gradients."""
    N, E, C = 23, 32, 5
    case = ref.make_case(N, E, C, seed=2)
    rng = np.random.default_rng(3)
    order = np.stack([rng.permutation(N) for _ in range(3)]).astype(np.int32)
    rates, wd = [0.01, 0.02, 0.005], 5e-4
    rt, losses_t = ref.torch_fit(case, 0.5, S, rates, 8, optimizer, weight_decay=wd, momentum=0.9, order=order)
    r = case["r"].astype(np.float64)
    m, v, losses = np.zeros_like(r), np.zeros_like(r), []
    for step, (e, idx) in enumerate(ref.batches(N, 8, 3, order)):
        b = ref.backward(dict(case, f=case["f"][idx], y=case["y"][idx], r=r), 0.5, S)
        losses.append(b["row_loss"].mean())
        if optimizer == "adam":
            r, m, v = ref.adam_rule(r, b["dr"], m, v, step + 1, rates[e], weight_decay=wd)
        else:
            g = b["dr"] + wd * r
            m = g if step == 0 else 0.9 * m + g
            r = r - rates[e] * m
    np.testing.assert_allclose(losses, losses_t, rtol=1e-10)
    assert np.abs(r - rt).max() <= 1e-10 * np.abs(rt).max()
    assert np.abs(rt - case["r"]).max() > 1e-4                       # the run went somewhere


def _host_case():
    case = ref.make_case(20, 16, 5, seed=1)
    return tuple(torch.from_numpy(case[k]) for k in ("f", "base", "r")) + (case["y"],)


def test_host_checks_come_before_any_launch():
    """Labels outside [0, C), a wrong order, shapes that do not fit and bad optimiser settings are refused on the host -- with CPU tensors
    too, so before the device is looked at; valid CPU input then meets the library's no-CPU-fallback error."""
    f, base, r, y = _host_case()
    fit = taskresfit.fit_residuals
    for bad in (5, -1):
        yb = y.copy()
        yb[7] = bad
        with pytest.raises(ValueError, match="labels span"):
            fit(f, torch.from_numpy(yb), base, r, epochs=2)
    with pytest.raises(ValueError, match="labels"):
        fit(f, y[:-1], base, r)
    with pytest.raises(TypeError):
        fit(f, y.astype(np.float32), base, r)
    with pytest.raises(ValueError, match="order"):
        fit(f, y, base, r, epochs=2, order=np.zeros((2, 19), np.int32))
    with pytest.raises(ValueError, match="order"):
        fit(f, y, base, r, epochs=1, order=np.full((1, 20), 20, np.int32))
    with pytest.raises(ValueError, match="order"):
        fit(f, y, base, r, epochs=1, order=np.full((1, 20), -1, np.int32))
    with pytest.raises(ValueError, match="residuals"):
        fit(f, y, base, r[:, :15])
    with pytest.raises(ValueError, match="residuals"):
        fit(f, y, base, r[:4])
    with pytest.raises(ValueError, match="base text features"):
        fit(f, y, base[:, :15])
    with pytest.raises(ValueError, match="base text features"):
        fit(f, y, base[:1])
    with pytest.raises(ValueError, match="features"):
        fit(f[0], y, base)
    with pytest.raises(ValueError, match="optimizer"):
        fit(f, y, base, r, optimizer="adamw")
    with pytest.raises(ValueError, match="betas"):
        fit(f, y, base, r, betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="betas"):
        fit(f, y, base, r, betas=(-0.1, 0.999))
    with pytest.raises(ValueError, match="eps"):
        fit(f, y, base, r, eps=-1e-8)
    with pytest.raises(ValueError, match="weight_decay"):
        fit(f, y, base, r, weight_decay=-1e-4)
    with pytest.raises(ValueError, match="Nesterov"):
        fit(f, y, base, r, optimizer="sgd", nesterov=True, momentum=0.0)
    with pytest.raises(ValueError, match="Nesterov"):
        fit(f, y, base, r, optimizer="sgd", nesterov=True, dampening=0.1)
    with pytest.raises(ValueError, match="momentum"):
        fit(f, y, base, r, optimizer="sgd", momentum=1.0)
    with pytest.raises(ValueError, match="alpha"):
        fit(f, y, base, r, alpha=float("nan"))
    with pytest.raises(ValueError, match="learning rates"):
        fit(f, y, base, r, epochs=3, lr_per_epoch=[0.1, 0.1])
    with pytest.raises(ValueError, match="batch_size"):
        fit(f, y, base, r, batch_size=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit(f, y, base, r, epochs=2, batch_size=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit(f, y, base, epochs=2, batch_size=8)
    State = taskresfit.TaskResFitState
    with pytest.raises(ValueError, match="optimizer"):
        State(base, optimizer="rmsprop")
    with pytest.raises(ValueError, match="betas"):
        State(base, betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="residuals"):
        State(base, r[:3])
    with pytest.raises(ValueError, match="base text features"):
        State(base[:1])
    with pytest.raises(ValueError, match="momentum"):
        State(base, optimizer="sgd", momentum=-0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        State(base, r)
    yt = torch.from_numpy(y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.taskres_train_step(f, yt, base, r.clone(), r.clone(), r.clone(), torch.zeros(1), 0.5, 100.0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.taskres_fit(f, yt, base, r.clone(), r.clone(), r.clone(), torch.zeros(3), 0.5, 100.0, 8, 1)
    with pytest.raises(ValueError, match="optimizer"):
        ops.taskres_fit(f, yt, base, r.clone(), None, None, torch.zeros(3), 0.5, 100.0, 8, 1, optimizer="lion")


P = ctypes.c_void_p(4096)


def test_entries_validate_arguments_without_a_gpu():
    """clipmi_taskres_train_step and clipmi_taskres_fit refuse, before any launch: null or misaligned pointers, C < 2, E < 1, ld < E, a
    batch or class count beyond the grid's 65 535 tiles, bad optimiser settings and a workspace too small for the batch."""
    L = _lib.lib
    need = L.clipmi_taskres_train_workspace_bytes
    assert need(256, 512, 1000) >= (2 * 256 * 1000 + 2 * 256 + 1000) * 4 and need(256, 512, 1000) % 256 == 0
    assert need(0, 512, 100) == 0 and need(32, 0, 100) == 0 and need(32, 512, 1) == 0
    big = 1 << 26

    def fit(feats=P, ld=512, lab=P, order=None, base=P, res=P, s1=P, s2=P, n=70, E=512, C=100, batch=32, epochs=3, drop=0, alpha=0.5, scale=100.0,
            lr=P, opt=_lib.OPTIM_ADAM, done=0, wd=5e-4, mom=0.9, damp=0.0, nest=0, b1=0.9, b2=0.999, eps=1e-8, losses=None, ws=P, ws_bytes=big):
        return L.clipmi_taskres_fit(feats, ld, lab, order, base, res, s1, s2, n, E, C, batch, epochs, drop, alpha, scale, lr, opt, done, wd, mom,
                                    damp, nest, b1, b2, eps, losses, ws, ws_bytes, None)

    def step(feats=P, ld=512, lab=P, base=P, res=P, s1=P, s2=P, rows=32, E=512, C=100, alpha=0.5, scale=100.0, lr=P, opt=_lib.OPTIM_ADAM, done=0,
             wd=5e-4, mom=0.9, damp=0.0, nest=0, b1=0.9, b2=0.999, eps=1e-8, loss=None, ws=P, ws_bytes=big):
        return L.clipmi_taskres_train_step(feats, ld, lab, base, res, s1, s2, rows, E, C, alpha, scale, lr, opt, done, wd, mom, damp, nest, b1, b2,
                                           eps, loss, ws, ws_bytes, None)

    sgd = _lib.OPTIM_SGD
    for f in (fit, step):
        for null in ("feats", "lab", "base", "res", "lr", "ws", "s1", "s2"):
            assert f(**{null: None}) == _lib.ERR_ARG and "null" in _lib.last_error(), null
        assert f(opt=sgd, s1=None) == _lib.ERR_ARG and "null" in _lib.last_error()      # a momentum needs its buffer
        for odd in ("feats", "base", "res", "s1", "s2", "lr"):
            assert f(**{odd: ctypes.c_void_p(4098)}) == _lib.ERR_ARG and "aligned" in _lib.last_error(), odd
        assert f(lab=ctypes.c_void_p(4100)) == _lib.ERR_ARG and "aligned" in _lib.last_error()
        assert f(ws=ctypes.c_void_p(4100)) == _lib.ERR_ARG and "aligned" in _lib.last_error()
        assert f(C=1) == _lib.ERR_SHAPE and "C=1" in _lib.last_error()
        assert f(C=65535 * 64 + 1) == _lib.ERR_SHAPE and "C=" in _lib.last_error()
        assert f(E=0, ld=0) == _lib.ERR_SHAPE and "E=0" in _lib.last_error()
        assert f(ld=511) == _lib.ERR_SHAPE and "ld=511" in _lib.last_error()
        assert f(opt=2) == _lib.ERR_ARG and "optimizer" in _lib.last_error()
        assert f(done=-1) == _lib.ERR_ARG and "steps_done" in _lib.last_error()
        for bad in (-0.1, 1.0, float("nan")):
            assert f(b1=bad) == _lib.ERR_ARG and "beta1" in _lib.last_error()
            assert f(b2=bad) == _lib.ERR_ARG and "beta2" in _lib.last_error()
            assert f(opt=sgd, mom=bad) == _lib.ERR_ARG and "momentum" in _lib.last_error()
            assert f(opt=sgd, damp=bad) == _lib.ERR_ARG and "dampening" in _lib.last_error()
        assert f(eps=-1e-8) == _lib.ERR_ARG and "eps" in _lib.last_error() and f(eps=float("inf")) == _lib.ERR_ARG
        assert f(wd=-1e-3) == _lib.ERR_ARG and f(wd=float("inf")) == _lib.ERR_ARG
        assert f(opt=sgd, nest=1, mom=0.0) == _lib.ERR_ARG and "nesterov" in _lib.last_error()
        assert f(opt=sgd, nest=1, mom=0.9, damp=0.1) == _lib.ERR_ARG and "nesterov" in _lib.last_error()
        assert f(alpha=float("nan")) == _lib.ERR_ARG and f(scale=float("inf")) == _lib.ERR_ARG
        assert f(ws_bytes=need(32, 512, 100) - 1) == _lib.ERR_WORKSPACE and "needed" in _lib.last_error()
    assert fit(n=0) == _lib.ERR_SHAPE and step(rows=0) == _lib.ERR_SHAPE
    assert step(rows=65535 * 64 + 1, ws_bytes=1 << 60) == _lib.ERR_SHAPE and "rows" in _lib.last_error()
    assert fit(batch=0) == _lib.ERR_SHAPE and "batch=0" in _lib.last_error()
    assert fit(epochs=-1) == _lib.ERR_ARG and "epochs=-1" in _lib.last_error()
    # arguments that pass every check stop short of a launch here (every batch dropped): nothing in this test may reach a device
    assert fit(opt=sgd, s1=None, s2=None, mom=0.0, batch=400, drop=1) == _lib.OK         # no momentum, no buffers
    assert fit(opt=sgd, s2=None, batch=400, drop=1) == _lib.OK                           # SGD has no second buffer
    assert fit(n=20, batch=32, drop=1, ws_bytes=need(20, 512, 100)) == _lib.OK           # the widest batch is the whole set
    assert fit(n=20, batch=32, drop=1, ws_bytes=need(20, 512, 100) - 1) == _lib.ERR_WORKSPACE
    assert fit(epochs=0) == _lib.OK                                                      # nothing to launch
    assert fit(batch=400, drop=1) == _lib.OK                                             # every batch dropped
    if not torch.cuda.is_available():                  # valid arguments reach the launch, which fails loudly without a device
        assert fit() == _lib.ERR_HIP and _lib.last_error()
        assert step() == _lib.ERR_HIP and _lib.last_error()
        assert step(opt=sgd, s1=None, s2=None, mom=0.0) == _lib.ERR_HIP                  # no momentum, no buffers


def test_the_translation_unit_is_vector_code_and_joins_the_library():
    """taskres_train.hip ships the LDS-tiled fp32 vector form of both products (DESIGN.md "TaskRes fit"): it names no matrix-core
    instruction, so the hazard scan of the matrix-core translation units has nothing to walk in it; the symbols are exported and the
    header declares them."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "taskres_train.hip")).read()
    assert not re.search(r"mfma|smfmac", src)
    assert "#pragma clang fp contract(off)" in src and not re.search(r"atomic[A-Z_(]", src)
    header = open(_lib.HEADER_PATH).read()
    for name in ("clipmi_taskres_train_workspace_bytes", "clipmi_taskres_train_step", "clipmi_taskres_fit"):
        assert name in _lib.exported_symbols() and hasattr(_lib.lib, name) and f" {name}(" in header
    assert (_lib.OPTIM_SGD, _lib.OPTIM_ADAM) == (0, 1) and "optimizer == 0" in header and "optimizer == 1" in header
