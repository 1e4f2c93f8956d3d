"""CPU checks of ProDA's dynamic loss scale (clip_calibration_amd/prodafit.py ``grad_scale="dynamic"``, csrc/proda_train.hip
clipmi_proda_ctx_step_scaled): the plain restatement (tests/prodascaler_ref.py) against torch's own GradScaler operators and
torch.optim.SGD on CPU tensors, the host-side argument checks, the library's refusals before any launch, the header."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import coopfit_ref
import prodafit_ref as dref
import prodascaler_ref as pref
import scalerfit_ref as sref

from clip_calibration_amd import _lib, ops, prodafit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C, PB, P, L, D, N_CTX = 3, 4, 8, 16, 16, 4
NAME_LENS = np.array([0, 3, 5])
POS = dref.positions(P)
SELS = [dref.ordered(s, POS) for s in ((1, 6, 2, 5), (0, 3, 4, 7), (7, 0, 3, 4), (5, 2, 1, 6))]    # every one holds all three positions
LR = 2.0 ** -3


def _poisoned(ints, scale, k, sel):
    """Step k's d_embed at `scale` with one inf, -inf or NaN: in a class row of a selected context (k even) or in the no-class row of a
    context outside the selection (k odd)."""
    d = pref.scaled(ints, scale).reshape(C * PB + P, L, D)
    if k % 2 == 0:
        q = k % PB
        c = k % C
        row = dref.ctx_row(int(POS[sel[q]]), k % N_CTX, int(NAME_LENS[c]), N_CTX // 2)
        d[c * PB + q, row, (5 * k) % D] = pref.POISON[k % 3]
    else:
        p = next(p for p in range(P) if p not in set(int(v) for v in sel))
        d[C * PB + p, 1 + k % N_CTX, (5 * k) % D] = pref.POISON[k % 3]
    return d.reshape(-1, D)


@pytest.mark.parametrize("momentum,wd,nesterov", [(0.5, 0.0, False), (0.0, 0.0, False), (0.5, 0.5, True)])
@pytest.mark.parametrize("name", sorted(sref.SEQUENCES))
def test_rule_equals_torch_on_the_cpu(name, momentum, wd, nesterov):
    """torch._amp_foreach_non_finite_check_and_unscale_, torch._amp_update_scale_ and torch.optim.SGD stepped only on clean steps, on the
    gradient prodafit_ref gathers, against the restatement, through scalerfit_ref's found-inf patterns with growth_interval = 2 and a
    selection that changes every step -- scale and counters after every step, ctx and buf as well, all exactly."""
    seq = sref.SEQUENCES[name]
    pattern = seq["pattern"][:4] if wd else seq["pattern"]        # weight decay adds bits per step: four steps stay exact in fp32
    ctx0, ints = pref.exact_inputs(C, PB, P, L, D, N_CTX, len(pattern), seed=1)
    r = pref.ProdaScalerRef(ctx0, C, POS, NAME_LENS, seq["init_scale"], 2.0, 0.5, 2, momentum, 0.0, wd, nesterov)
    p = torch.nn.Parameter(torch.from_numpy(ctx0.copy()))
    opt = torch.optim.SGD([p], lr=LR, momentum=momentum, weight_decay=wd, nesterov=nesterov)
    scale_t, tracker_t = torch.tensor([seq["init_scale"]], dtype=torch.float32), torch.zeros(1, dtype=torch.int32)
    skipped = applied = 0
    for k, poison in enumerate(pattern):
        sel = SELS[k % len(SELS)]
        d = _poisoned(ints[k], float(r.scale), k, sel) if poison else pref.scaled(ints[k], float(r.scale))
        grad_t = torch.from_numpy(pref.gather(d, sel, POS, NAME_LENS, C, P, N_CTX))
        found_t = torch.zeros(1)
        torch._amp_foreach_non_finite_check_and_unscale_([grad_t], found_t, (1.0 / scale_t))
        if float(found_t) == 0.0:
            p.grad = grad_t
            opt.step()
            applied += 1
        else:
            skipped += 1
        torch._amp_update_scale_(scale_t, tracker_t, found_t, 2.0, 0.5, 2)
        assert r.step(d, LR, sel) == bool(poison) == bool(float(found_t)), k
        assert r.state() == {"scale": float(scale_t), "growth_tracker": int(tracker_t), "skipped_steps": skipped, "applied_steps": applied,
                             "found_inf": int(poison)}, k
        assert np.array_equal(r.ctx, p.detach().numpy()), k
        buf_t = opt.state[p].get("momentum_buffer") if p in opt.state else None
        assert (r.buf is None) == (buf_t is None)
        if buf_t is not None:
            assert np.array_equal(r.buf, buf_t.numpy()), k
    assert applied >= 1 and skipped >= 1 and np.isfinite(r.ctx).all()


def test_found_looks_at_the_rows_the_gather_reads_and_at_the_sum():
    ctx0, ints = pref.exact_inputs(C, PB, P, L, D, N_CTX, 1)
    sel = SELS[0]
    mask = pref.read_rows(sel, POS, NAME_LENS, C, P, L, N_CTX)
    assert mask.sum() == C * PB * N_CTX + P * N_CTX and not mask[:, 0].any()
    for n, row in ((0, 0), (C * PB - 1, L - 1), (C * PB + 2, 1 + N_CTX)):           # SOS of a class prompt, a padding row, '.' of a no-class prompt
        assert not mask[n, row]
        d = pref.scaled(ints[0], 16.0)
        d[n * L + row, 3] = np.nan
        assert not pref.ProdaScalerRef(ctx0, C, POS, NAME_LENS, 16.0).step(d, LR, sel)
    # the rows of a selected front context move with the class's name length: row 1 of class 1 (three name tokens) is a name token
    q = int(np.argmax(POS[sel] == 0))
    assert not mask[1 * PB + q, 1] and mask[1 * PB + q, 1 + 3] and mask[0 * PB + q, 1]
    d = np.zeros(((C * PB + P) * L, D), np.float32)
    d[(0 * PB + 0) * L + 1, 0] = d[(1 * PB + 0) * L + 1, 0] = 3.0e38                # an end context: finite rows, the sum is not
    assert int(POS[sel[0]]) == 2 and np.isfinite(d).all() and pref.ProdaScalerRef(ctx0, C, POS, NAME_LENS, 16.0).step(d, LR, sel)
    assert pref.workspace_bytes(P, D, N_CTX) == 256 + 256 + 4 * P * D * N_CTX


@pytest.fixture(scope="module")
def cpu_model():
    return build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"})


def test_python_argument_checks(cpu_model):
    c = dref.make_case("tiny", 3, 4, 8, 4, 2)
    ids, ctx, f, y = c["ids"], c["ctx"], c["feats"], c["labels"]

    def state(**kw):
        return prodafit.ProDAFitState(cpu_model, ids, ctx, prompt_bs=4, **kw)

    def fit(**kw):
        return prodafit.fit_context(f, y, cpu_model, ids, ctx, prompt_bs=4, epochs=1, **kw)

    for make in (state, fit):
        for bad in ({"init_scale": 3.0}, {"init_scale": 0.0}, {"init_scale": -4.0}, {"init_scale": math.inf}, {"init_scale": math.nan},
                    {"growth_factor": 1.5}, {"backoff_factor": 0.3}, {"growth_factor": 2.0 ** 200}):
            with pytest.raises(ValueError, match="power of two"):
                make(grad_scale="dynamic", scaler=bad)
        with pytest.raises(ValueError, match="growth_factor"):
            make(grad_scale="dynamic", scaler={"growth_factor": 0.5})
        with pytest.raises(ValueError, match="backoff_factor"):
            make(grad_scale="dynamic", scaler={"backoff_factor": 2.0})
        for gi in (0, -1, 2.5):
            with pytest.raises(ValueError, match="growth_interval"):
                make(grad_scale="dynamic", scaler={"growth_interval": gi})
        with pytest.raises(ValueError, match="no option"):
            make(grad_scale="dynamic", scaler={"growth": 2.0})
        with pytest.raises(ValueError, match="must be a dict"):
            make(grad_scale="dynamic", scaler=[2.0 ** 12])
        with pytest.raises(ValueError, match="dynamic"):
            make(grad_scale="auto")
        with pytest.raises(ValueError, match="scaler"):
            make(grad_scale=4096.0, scaler={})
        with pytest.raises(ValueError, match="grad_scale"):                 # a number keeps today's message
            make(grad_scale=3.0)
        with pytest.raises(RuntimeError, match="GPU"):                      # everything checks out: the call needs the device
            make(grad_scale="dynamic", scaler={"init_scale": 2.0 ** 12, "growth_interval": 5})
        with pytest.raises(RuntimeError, match="GPU"):
            make(grad_scale="dynamic")
        with pytest.raises(RuntimeError, match="GPU"):                      # and a number behaves as today
            make(grad_scale=256.0)
    with pytest.raises(ValueError, match="needs a number"):
        prodafit.context_gradient(cpu_model, ids, ctx, f, y, grad_scale="dynamic")
    with pytest.raises(ValueError, match="dynamic"):
        prodafit.context_gradient(cpu_model, ids, ctx, f, y, grad_scale="auto")
    with pytest.raises(ValueError, match="return_scaler_state"):
        fit(grad_scale=256.0, return_scaler_state=True)
    # scaler= is the last argument of the state and, with return_scaler_state behind it, of the fit: positional callers keep working
    import inspect
    assert list(inspect.signature(prodafit.ProDAFitState.__init__).parameters)[-2:] == ["generator", "scaler"]
    assert list(inspect.signature(prodafit.fit_context).parameters)[-3:] == ["return_history", "scaler", "return_scaler_state"]
    out, untouched = prodafit.fit_context(f, y, cpu_model, ids, ctx, prompt_bs=4, epochs=0, grad_scale="dynamic", scaler={"init_scale": 64.0},
                                          return_scaler_state=True)
    assert torch.equal(out, ctx) and untouched == {"scale": 64.0, "growth_tracker": 0, "skipped_steps": 0, "applied_steps": 0, "found_inf": 0}


def test_header_declares_the_entries_with_the_abi_at_16():
    text = open(os.path.join(ROOT, "include", "clipmi.h")).read()
    assert re.search(r"#define CLIPMI_ABI_VERSION 16\b", text) and _lib.ABI_VERSION == 16 and _lib.lib.clipmi_abi_version() == 16
    for n in ("clipmi_proda_ctx_step_scaled_workspace_bytes", "clipmi_proda_ctx_step_scaled", "clipmi_proda_train_step_scaled_bytes",
              "clipmi_proda_train_step_scaled"):
        assert re.search(r"\b(int|size_t) " + n + r"\(", text), n
        assert n in _lib._SIGNATURES and n in _lib.exported_symbols() and hasattr(_lib.lib, n)
    assert callable(ops.proda_ctx_step_scaled)


def test_library_refuses_bad_calls_without_a_device():
    """Argument checks that return before anything is launched: with no device a launch would answer CLIPMI_ERR_HIP.  The refusals are
    clipmi_proda_ctx_step's together with clipmi_ctx_step_scaled's."""
    lib = _lib.lib
    p = ctypes.c_void_p(4096)

    def step(d=p, ctx=p, buf=None, sel=p, pos=p, nl=p, Cn=3, Pb=4, Pn=8, Ln=16, Dn=128, n_ctx=4, state=p, growth=2.0, backoff=0.5, interval=2000, lr=p,
             momentum=0.0, dampening=0.0, nesterov=0, ws=p, ws_bytes=1 << 20):
        return lib.clipmi_proda_ctx_step_scaled(d, ctx, buf, None, sel, pos, nl, Cn, Pb, Pn, Ln, Dn, n_ctx, state, growth, backoff, interval, lr, momentum,
                                                dampening, 0.0, nesterov, ws, ws_bytes, None)
    for null in ("d", "ctx", "sel", "pos", "nl", "state", "lr", "ws"):
        assert step(**{null: None}) == _lib.ERR_ARG, null
    assert step(momentum=0.9) == _lib.ERR_ARG and "buffer" in _lib.last_error()
    assert step(Cn=1) == _lib.ERR_SHAPE and step(Pn=1, Pb=1) == _lib.ERR_SHAPE and step(Pb=9) == _lib.ERR_SHAPE and step(Pb=0) == _lib.ERR_SHAPE
    assert step(Dn=0) == _lib.ERR_SHAPE and step(n_ctx=0) == _lib.ERR_SHAPE
    assert step(n_ctx=14) == _lib.ERR_SHAPE                                  # SOS, 14 vectors, '.' and EOT do not fit 16 rows
    assert step(n_ctx=13) != _lib.ERR_SHAPE
    for bad in (0.0, -2.0, math.inf, math.nan):
        assert step(growth=bad) == _lib.ERR_ARG and "growth_factor" in _lib.last_error()
        assert step(backoff=bad) == _lib.ERR_ARG and "backoff_factor" in _lib.last_error()
    assert step(interval=0) == _lib.ERR_ARG and "growth_interval" in _lib.last_error()
    assert step(momentum=1.0, buf=p) == _lib.ERR_ARG and step(nesterov=1) == _lib.ERR_ARG and step(dampening=-0.1) == _lib.ERR_ARG
    assert step(ws_bytes=64) == _lib.ERR_WORKSPACE
    assert step(ws=ctypes.c_void_p(4096 + 8)) == _lib.ERR_ARG and "aligned" in _lib.last_error()
    assert step(state=ctypes.c_void_p(4098)) == _lib.ERR_ARG
    by = lib.clipmi_proda_ctx_step_scaled_workspace_bytes
    assert by(1, 128, 4) == 0 and by(8, 0, 4) == 0 and by(8, 128, 0) == 0 and by(-1, 128, 4) == 0 and by(1 << 15, 1 << 15, 2) == 0
    assert by(8, 128, 4) == pref.workspace_bytes(8, 128, 4) and by(8, 16, 4) == pref.workspace_bytes(8, 16, 4)
    assert step(ws_bytes=by(8, 128, 4) - 1) == _lib.ERR_WORKSPACE

    def one_call(m=None, state=p, growth=2.0, backoff=0.5, interval=2000):
        return lib.clipmi_proda_train_step_scaled(m, None, p, p, 0, p, None, 4, p, p, p, p, 3, 4, 8, 0, p, 64, p, 2, 100.0, state, growth, backoff, interval,
                                                  0.1, p, 0.0, 0.0, 0.0, 0, p, None, p, 1 << 20, p, 1 << 20, None)
    assert one_call(state=None) == _lib.ERR_ARG and "state" in _lib.last_error()
    for bad in (0.0, -0.5, math.inf, math.nan):
        assert one_call(growth=bad) == _lib.ERR_ARG and "growth_factor" in _lib.last_error()
        assert one_call(backoff=bad) == _lib.ERR_ARG and "backoff_factor" in _lib.last_error()
    assert one_call(interval=0) == _lib.ERR_ARG and "growth_interval" in _lib.last_error()
    assert one_call() == _lib.ERR_ARG and "model" in _lib.last_error()
    assert lib.clipmi_proda_train_step_scaled_bytes(None, 3, 4, 8, 0, 2, 4) == 0


@pytest.mark.parametrize("geom", ["tiny", "tiny3"])
def test_one_call_refusals_and_sizes_with_a_model(geom):
    """With a model handle (no device needed for one): the scaler's and the optimiser's arguments are refused before any launch, and the
    sizing function is clipmi_proda_train_step_bytes plus the scaled step's workspace, 0 for what the call refuses."""
    lib = _lib.lib
    m = build_model(dict(coopfit_ref.state_dict(geom)), {"trainer": "CoOp"})
    m._ensure_handle()
    h, Dt = m._handle, int(m.geometry.transformer_width)
    by = lib.clipmi_proda_train_step_scaled_bytes
    for Cn, Pb, Pn, rows, B, n_ctx in ((3, 4, 8, 0, 2, 4), (37, 1, 4, 24, 1, 16), (2, 8, 8, 16, 4, 1)):
        assert by(h, Cn, Pb, Pn, rows, B, n_ctx) == (lib.clipmi_proda_train_step_bytes(h, Cn, Pb, Pn, rows, B) +
                                                      lib.clipmi_proda_ctx_step_scaled_workspace_bytes(Pn, Dt, n_ctx)) > 0
    assert by(h, 1, 4, 8, 0, 2, 4) == 0 and by(h, 3, 9, 8, 0, 2, 4) == 0 and by(h, 3, 4, 8, 0, 0, 4) == 0 and by(h, 3, 4, 8, 0, 2, 0) == 0
    p = ctypes.c_void_p(4096)

    def one_call(state=p, growth=2.0, feats=p, B=2, momentum=0.0, ws_bytes=1 << 30):
        return lib.clipmi_proda_train_step_scaled(h, None, p, p, 0, p, None, 4, p, p, p, p, 3, 4, 8, 0, feats, 64, p, B, 100.0, state, growth, 0.5, 2000, 0.1,
                                                  p, momentum, 0.0, 0.0, 0, p, None, p, ws_bytes, p, 1 << 30, None)
    assert one_call(state=None) == _lib.ERR_ARG and one_call(growth=math.nan) == _lib.ERR_ARG
    assert one_call(B=0) == _lib.ERR_SHAPE
    assert one_call(ws_bytes=64) == _lib.ERR_WORKSPACE
    assert one_call() != _lib.OK                                          # the weights are not bound / there is no device: never a launch that succeeds
