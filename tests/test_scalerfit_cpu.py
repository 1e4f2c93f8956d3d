"""CPU checks of the dynamic loss scale (clip_calibration_amd/coopfit.py ``grad_scale="dynamic"``, csrc/grad_scaler.hip): the plain
restatement of the rule (tests/scalerfit_ref.py) against torch's own GradScaler operators and torch.optim.SGD on CPU tensors, the
host-side argument checks, the library's refusals before any launch, the header."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import coopfit_ref
import scalerfit_ref as ref

from clip_calibration_amd import _lib, coopfit, fitoptim, ops  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C, L, D, N_CTX = 3, 8, 16, 2
LR = 2.0 ** -3


def _poisoned(ints, scale, k, per_class):
    """Step k's d_embed at `scale`, with one inf, -inf or NaN on a context row."""
    d = ref.scaled_embed(ints, scale)
    c = k % C if per_class else C - 1
    d[c * L + 1 + k % N_CTX, (5 * k) % D] = ref.POISON[k % 3]
    return d


@pytest.mark.parametrize("per_class", [False, True])
@pytest.mark.parametrize("momentum,wd,nesterov", [(0.5, 0.0, False), (0.0, 0.0, False), (0.5, 0.5, True)])
@pytest.mark.parametrize("name", sorted(ref.SEQUENCES))
def test_rule_equals_torch_on_the_cpu(name, momentum, wd, nesterov, per_class):
    """torch._amp_foreach_non_finite_check_and_unscale_, torch._amp_update_scale_ and torch.optim.SGD stepped only on clean steps, against
    the restatement, through a fixed found-inf pattern with growth_interval = 2: a skip on the very first step, two skips in a row, growth
    after a skip, a growth that would pass 2^127.  Scale and counters after every step, ctx and buf as well -- all exactly."""
    seq = ref.SEQUENCES[name]
    pattern = seq["pattern"][:4] if wd else seq["pattern"]        # weight decay adds bits per step: four steps stay exact in fp32
    ctx0, ints = ref.exact_inputs(C, L, D, N_CTX, per_class, len(pattern), seed=1)
    r = ref.ScalerRef(ctx0, C, L, N_CTX, per_class, seq["init_scale"], 2.0, 0.5, 2, momentum, 0.0, wd, nesterov)
    p = torch.nn.Parameter(torch.from_numpy(ctx0.copy()))
    opt = torch.optim.SGD([p], lr=LR, momentum=momentum, weight_decay=wd, nesterov=nesterov)
    scale_t, tracker_t = torch.tensor([seq["init_scale"]], dtype=torch.float32), torch.zeros(1, dtype=torch.int32)
    skipped = applied = 0
    scales = []
    for k, poison in enumerate(pattern):
        d = _poisoned(ints[k], float(r.scale), k, per_class) if poison else ref.scaled_embed(ints[k], float(r.scale))
        grad_t = torch.from_numpy(ref.context_sum(d, C, L, N_CTX, per_class))
        found_t = torch.zeros(1)
        torch._amp_foreach_non_finite_check_and_unscale_([grad_t], found_t, (1.0 / scale_t))
        if float(found_t) == 0.0:
            p.grad = grad_t
            opt.step()
            applied += 1
        else:
            skipped += 1
        torch._amp_update_scale_(scale_t, tracker_t, found_t, 2.0, 0.5, 2)
        assert r.step(d, LR) == bool(poison) == bool(float(found_t))
        assert r.state() == {"scale": float(scale_t), "growth_tracker": int(tracker_t), "skipped_steps": skipped, "applied_steps": applied,
                             "found_inf": int(poison)}, k
        assert np.array_equal(r.ctx, p.detach().numpy()), k
        buf_t = opt.state[p].get("momentum_buffer") if p in opt.state else None
        assert (r.buf is None) == (buf_t is None)
        if buf_t is not None:
            assert np.array_equal(r.buf, buf_t.numpy()), k
        scales.append(float(r.scale))
    if name == "A" and not wd:
        assert scales == [2.0 ** e for e in (9, 8, 8, 9, 8, 8, 9, 9)]
    if name == "B" and not wd:      # step 1 would grow to 2^128
        assert scales == [2.0 ** e for e in (127, 127, 126, 126, 127, 127, 127)]
    assert applied >= 1 and np.isfinite(r.ctx).all()


def test_found_looks_at_context_rows_only_and_at_the_sum():
    ctx0, ints = ref.exact_inputs(C, L, D, N_CTX, False, 1)
    for row in (0, 1 + N_CTX, L - 1):
        d = ref.scaled_embed(ints[0], 16.0)
        d[(C - 1) * L + row, 3] = np.nan
        assert not ref.ScalerRef(ctx0, C, L, N_CTX, False, 16.0).step(d, LR)
    d = np.zeros((C * L, D), np.float32)
    d[0 * L + 1, 0] = d[1 * L + 1, 0] = 3.0e38                       # finite rows, the sum is not
    assert np.isfinite(d).all() and ref.ScalerRef(ctx0, C, L, N_CTX, False, 16.0).step(d, LR)
    assert not ref.ScalerRef(np.zeros((C, N_CTX, D), np.float32), C, L, N_CTX, True, 16.0).step(d, LR)   # per class nothing is added


@pytest.fixture(scope="module")
def cpu_model():
    return build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"})


def test_python_argument_checks(cpu_model):
    c = coopfit_ref.make_case("tiny", 3, 4, 8, False)
    ids, ctx, f, y = c["ids"], c["ctx"], c["feats"], c["labels"]
    tea = torch.zeros(3, int(cpu_model.geometry.embed_dim))

    def state(**kw):
        return coopfit.CoOpFitState(cpu_model, ids, ctx, **kw)

    def fit(**kw):
        return coopfit.fit_context(f, y, cpu_model, ids, ctx, epochs=1, **kw)

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
        with pytest.raises(ValueError, match="ProGrad"):
            make(grad_scale="dynamic", method="prograd", teacher=tea)
        with pytest.raises(ValueError, match="dynamic"):
            make(grad_scale="auto")
        with pytest.raises(ValueError, match="scaler"):
            make(grad_scale=4096.0, scaler={})
        with pytest.raises(ValueError, match="power of two"):              # a number keeps today's message
            make(grad_scale=3.0)
        with pytest.raises(RuntimeError, match="GPU"):                      # everything checks out: the call needs the device
            make(grad_scale="dynamic", scaler={"init_scale": 2.0 ** 12, "growth_interval": 5})
        with pytest.raises(RuntimeError, match="GPU"):
            make(grad_scale="dynamic", method="kgcoop", teacher=tea)
    with pytest.raises(ValueError, match="needs a number"):
        coopfit.context_gradient(cpu_model, ids, ctx, f, y, grad_scale="dynamic")
    with pytest.raises(ValueError, match="power of two"):
        coopfit.context_gradient(cpu_model, ids, ctx, f, y, grad_scale="auto")
    assert ops.SCALER_DEFAULTS == {"init_scale": 2.0 ** 16, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000}
    assert fitoptim._check_scaler("t", None) == ops.SCALER_DEFAULTS
    assert fitoptim._check_scaler("t", {"growth_factor": 1.0, "backoff_factor": 1.0})["growth_factor"] == 1.0


def test_state_block_layout():
    assert ctypes.sizeof(_lib.ScalerState) == 20
    assert [(n, getattr(_lib.ScalerState, n).offset) for n, _ in _lib.ScalerState._fields_] == [
        ("scale", 0), ("growth_tracker", 4), ("skipped_steps", 8), ("applied_steps", 12), ("found_inf", 16)]
    block = ops.new_scaler_state(2.0 ** 12, "cpu")
    assert block.dtype == torch.int32 and block.shape == (5,)
    assert ops.scaler_state_dict(block) == {"scale": 4096.0, "growth_tracker": 0, "skipped_steps": 0, "applied_steps": 0, "found_inf": 0}
    text = open(os.path.join(ROOT, "include", "clipmi.h")).read()
    body = re.search(r"typedef struct clipmi_scaler_state \{(.*?)\} clipmi_scaler_state;", text, flags=re.S).group(1)
    assert re.findall(r"\b(float|int32_t) (\w+);", body) == [("float", "scale"), ("int32_t", "growth_tracker"), ("int32_t", "skipped_steps"),
                                                            ("int32_t", "applied_steps"), ("int32_t", "found_inf")]


def test_header_declares_the_entries_with_the_abi_at_16():
    text = open(os.path.join(ROOT, "include", "clipmi.h")).read()
    assert re.search(r"#define CLIPMI_ABI_VERSION 16\b", text) and _lib.ABI_VERSION == 16 and _lib.lib.clipmi_abi_version() == 16
    for n in ("clipmi_grad_scale_rows", "clipmi_ctx_step_scaled_workspace_bytes", "clipmi_ctx_step_scaled", "clipmi_prompt_train_step_scaled_bytes",
              "clipmi_prompt_train_step_scaled"):
        assert re.search(r"\b(int|size_t) " + n + r"\(", text), n
        assert n in _lib.exported_symbols() and hasattr(_lib.lib, n)


def test_library_refuses_bad_calls_without_a_device():
    """Argument checks that return before anything is launched: with no device a launch would answer CLIPMI_ERR_HIP."""
    lib = _lib.lib
    p = ctypes.c_void_p(4096)
    assert lib.clipmi_grad_scale_rows(None, 3, 64, p, None) == _lib.ERR_ARG and lib.clipmi_grad_scale_rows(p, 3, 64, None, None) == _lib.ERR_ARG
    assert lib.clipmi_grad_scale_rows(p, 0, 64, p, None) == _lib.ERR_SHAPE and lib.clipmi_grad_scale_rows(p, 3, 0, p, None) == _lib.ERR_SHAPE

    def step(d_embed=p, ctx=p, buf=None, Cn=3, Ln=8, Dn=64, n_ctx=4, state=p, growth=2.0, backoff=0.5, interval=2000, lr=p, momentum=0.0,
             dampening=0.0, nesterov=0, ws=p, ws_bytes=1 << 20):
        return lib.clipmi_ctx_step_scaled(d_embed, ctx, buf, None, Cn, Ln, Dn, n_ctx, 0, state, growth, backoff, interval, lr, momentum, dampening, 0.0,
                                          nesterov, ws, ws_bytes, None)
    for null in ("d_embed", "ctx", "state", "lr", "ws"):
        assert step(**{null: None}) == _lib.ERR_ARG, null
    assert step(momentum=0.9) == _lib.ERR_ARG and "buffer" in _lib.last_error()
    assert step(Cn=0) == _lib.ERR_SHAPE and step(Dn=0) == _lib.ERR_SHAPE and step(n_ctx=0) == _lib.ERR_SHAPE
    assert step(n_ctx=8) == _lib.ERR_SHAPE                                   # 1 + n_ctx > L
    assert step(n_ctx=7) != _lib.ERR_SHAPE
    for bad in (0.0, -2.0, math.inf, math.nan):
        assert step(growth=bad) == _lib.ERR_ARG and "growth_factor" in _lib.last_error()
        assert step(backoff=bad) == _lib.ERR_ARG
    assert step(interval=0) == _lib.ERR_ARG and "growth_interval" in _lib.last_error()
    assert step(momentum=1.0, buf=p) == _lib.ERR_ARG and step(nesterov=1) == _lib.ERR_ARG and step(dampening=-0.1) == _lib.ERR_ARG
    assert step(ws_bytes=64) == _lib.ERR_WORKSPACE
    assert step(ws=ctypes.c_void_p(4096 + 8)) == _lib.ERR_ARG and "aligned" in _lib.last_error()
    assert step(state=ctypes.c_void_p(4098)) == _lib.ERR_ARG
    by = lib.clipmi_ctx_step_scaled_workspace_bytes
    assert by(0, 64, 4, 0) == 0 and by(3, 0, 4, 0) == 0 and by(3, 64, 0, 0) == 0 and by(-1, 64, 4, 1) == 0
    assert by(3, 64, 4, 0) >= 8 + 4 + 4 * 64 * 4 and by(3, 64, 4, 1) >= 8 + 4 * 3 + 3 * 4 * 64 * 4 and by(3, 64, 4, 0) % 256 == 0
    assert step(ws_bytes=by(3, 64, 4, 0) - 1) == _lib.ERR_WORKSPACE

    def one_call(mode, state=p, growth=2.0, backoff=0.5, interval=2000):
        return lib.clipmi_prompt_train_step_scaled(None, None, p, 0, p, None, 4, 0, p, 3, 0, p, 64, p, 8, 100.0, state, growth, backoff, interval, mode, p,
                                                   8.0, p, 0.0, 0.0, 0.0, 0, p, None, p, 1 << 20, p, 1 << 20, None)
    assert one_call(_lib.PROMPT_PROGRAD) == _lib.ERR_ARG and "ProGrad" in _lib.last_error()
    assert one_call(3) == _lib.ERR_ARG and "mode" in _lib.last_error()
    assert one_call(_lib.PROMPT_COOP, state=None) == _lib.ERR_ARG and "state" in _lib.last_error()
    for bad in (0.0, -0.5, math.inf, math.nan):
        assert one_call(_lib.PROMPT_KGCOOP, growth=bad) == _lib.ERR_ARG and "growth_factor" in _lib.last_error()
        assert one_call(_lib.PROMPT_COOP, backoff=bad) == _lib.ERR_ARG and "backoff_factor" in _lib.last_error()
    assert one_call(_lib.PROMPT_COOP, interval=0) == _lib.ERR_ARG and "growth_interval" in _lib.last_error()
    assert one_call(_lib.PROMPT_COOP) == _lib.ERR_ARG and "model" in _lib.last_error()
    assert lib.clipmi_prompt_train_step_scaled_bytes(None, 3, 0, 8, 0, 4, 0) == 0


@pytest.mark.parametrize("geom", ["tiny", "tiny3"])
def test_one_call_refusals_and_sizes_with_a_model(geom):
    """With a model handle (no device needed for one): ProGrad's mode and the scaler's arguments are refused before any launch, and the
    sizing function is clipmi_prompt_train_step_bytes plus the scaled step's workspace, 0 for what the call refuses."""
    lib = _lib.lib
    m = build_model(dict(coopfit_ref.state_dict(geom)), {"trainer": "CoOp"})
    m._ensure_handle()
    h, Dt = m._handle, int(m.geometry.transformer_width)
    by = lib.clipmi_prompt_train_step_scaled_bytes
    for mode in (_lib.PROMPT_COOP, _lib.PROMPT_KGCOOP):
        for Cn, rows, B, n_ctx, pc in ((3, 0, 8, 4, 0), (37, 16, 1, 16, 1), (2, 16, 4, 1, 0)):
            assert by(h, Cn, rows, B, mode, n_ctx, pc) == (lib.clipmi_prompt_train_step_bytes(h, Cn, rows, B, mode, n_ctx, pc) +
                                                          lib.clipmi_ctx_step_scaled_workspace_bytes(Cn, Dt, n_ctx, pc))
    assert by(h, 3, 0, 8, _lib.PROMPT_PROGRAD, 4, 0) == 0 and by(h, 3, 0, 8, 3, 4, 0) == 0 and by(h, 3, 0, 8, -1, 4, 0) == 0
    assert by(h, 1, 0, 8, 0, 4, 0) == 0 and by(h, 3, 0, 0, 0, 4, 0) == 0 and by(h, 3, 0, 8, 0, 0, 0) == 0
    p = ctypes.c_void_p(4096)

    def one_call(mode=0, state=p, growth=2.0, backoff=0.5, interval=2000, feats=p, teacher=p, w=8.0, B=8, ws_bytes=1 << 30):
        return lib.clipmi_prompt_train_step_scaled(h, None, p, 0, p, None, 4, 0, p, 3, 0, feats, 64, p, B, 100.0, state, growth, backoff, interval, mode,
                                                   teacher, w, p, 0.0, 0.0, 0.0, 0, p, None, p, ws_bytes, p, 1 << 30, None)
    assert one_call(mode=_lib.PROMPT_PROGRAD) == _lib.ERR_ARG and "ProGrad" in _lib.last_error()
    assert one_call(feats=None) == _lib.ERR_ARG
    assert one_call(mode=_lib.PROMPT_KGCOOP, teacher=None) == _lib.ERR_ARG and one_call(mode=_lib.PROMPT_KGCOOP, w=-1.0) == _lib.ERR_ARG
    assert one_call(B=0) == _lib.ERR_SHAPE
    assert one_call(ws_bytes=64) == _lib.ERR_WORKSPACE
    assert one_call() != _lib.OK                                          # the weights are not bound / there is no device: never a launch that succeeds
