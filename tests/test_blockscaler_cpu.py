"""CPU checks of the dynamic loss scale of the block fits (CoCoOp, VPT, MaPLe, PromptSRC / IVLP; csrc/grad_scaler.hip
clipmi_block_step_scaled): the host-side argument handling of the eight entry points, the declarations, the library's refusals before any
launch and the workspace size."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import blockscaler_ref as bref
import cocoopfit_ref
import coopfit_ref
import maplefit_ref
import promptsrcfit_ref
import vptfit_ref

from clip_calibration_amd import _lib, cocoopfit, coopfit, maplefit, ops, promptsrcfit, vptfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("clipmi_block_step_scaled_workspace_bytes", "clipmi_block_step_scaled", "clipmi_cocoop_train_step_scaled_bytes",
       "clipmi_cocoop_train_step_scaled", "clipmi_vpt_train_step_scaled_bytes", "clipmi_vpt_train_step_scaled",
       "clipmi_maple_train_step_scaled_bytes", "clipmi_maple_train_step_scaled", "clipmi_promptsrc_train_step_scaled_bytes",
       "clipmi_promptsrc_train_step_scaled")


def entry_points():
    """name -> a callable of grad_scale / scaler keywords, on CPU models: everything but the device is there."""
    out = {}
    c = cocoopfit_ref.make_case("tiny", 3, 4, 1)
    m = build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"})
    out["cocoopfit.CoCoOpFitState"] = lambda **kw: cocoopfit.CoCoOpFitState(m, c["ids"], c["params"], **kw)
    out["cocoopfit.fit_prompt_learner"] = lambda **kw: cocoopfit.fit_prompt_learner(c["feats"], c["labels"], m, c["ids"], c["params"], epochs=1, **kw)
    v = vptfit_ref.make_case("tiny", 2, 2, 1, 3)
    mv = build_model(dict(v["sd"]), {"trainer": "VPT", "vision_depth": 2, "vision_ctx": 2, "language_depth": 0, "language_ctx": 0})
    out["vptfit.VPTFitState"] = lambda **kw: vptfit.VPTFitState(mv, v["text"], prompts=v["prompts"], **kw)
    out["vptfit.fit_prompts"] = lambda **kw: vptfit.fit_prompts(v["images"], v["labels"], mv, v["text"], v["prompts"], epochs=1, **kw)
    a = maplefit_ref.make_case("tiny3", 2, 1, 5, 3)
    ma = build_model(dict(a["sd"]), maplefit_ref.design(1))
    out["maplefit.MaPLeFitState"] = lambda **kw: maplefit.MaPLeFitState(ma, a["ids"], a["pl"], **kw)
    out["maplefit.fit_prompt_learner"] = lambda **kw: maplefit.fit_prompt_learner(a["images"], a["labels"], ma, a["ids"], a["pl"], epochs=1, **kw)
    p = promptsrcfit_ref.make_case("tiny", 2, 2, 3, 2, 3, 3)
    mp = build_model(dict(p["sd"]), promptsrcfit_ref.design(3, 2, 2, 2))
    for method in promptsrcfit.METHODS:
        out[f"promptsrcfit.PromptSRCFitState[{method}]"] = (
            lambda method=method, **kw: promptsrcfit.PromptSRCFitState(mp, p["ids"], p["p"], p["teacher"], method=method, **kw))
        out[f"promptsrcfit.fit_prompts[{method}]"] = (
            lambda method=method, **kw: promptsrcfit.fit_prompts(p["images"], p["labels"], mp, p["ids"], p["teacher"], p["p"], method=method, epochs=1, **kw))
    return out


ENTRY = None


@pytest.mark.parametrize("name", ["cocoopfit.CoCoOpFitState", "cocoopfit.fit_prompt_learner", "vptfit.VPTFitState", "vptfit.fit_prompts",
                                  "maplefit.MaPLeFitState", "maplefit.fit_prompt_learner", "promptsrcfit.PromptSRCFitState[promptsrc]",
                                  "promptsrcfit.fit_prompts[promptsrc]", "promptsrcfit.PromptSRCFitState[ivlp]", "promptsrcfit.fit_prompts[ivlp]"])
def test_python_argument_checks(name):
    """``grad_scale="dynamic"`` is accepted as far as "needs the GPU"; a bad scaler dict is refused with coopfit's messages, and so are a
    scaler beside a numeric scale and an unknown string."""
    global ENTRY
    ENTRY = ENTRY or entry_points()
    make = ENTRY[name]
    with pytest.raises(RuntimeError, match="GPU"):
        make(grad_scale="dynamic")
    with pytest.raises(RuntimeError, match="GPU"):
        make(grad_scale="dynamic", scaler={"init_scale": 2.0 ** 12, "growth_interval": 5, "backoff_factor": 2.0 ** -4})
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
        make(grad_scale="dynamic", scaler=[2.0])
    with pytest.raises(ValueError, match="dynamic"):
        make(grad_scale="auto")
    with pytest.raises(ValueError, match="scaler is an argument"):
        make(grad_scale=1024.0, scaler={})
    with pytest.raises(ValueError, match="power of two"):              # a number keeps today's message
        make(grad_scale=3.0)
    with pytest.raises(RuntimeError, match="GPU"):                      # and today's path
        make(grad_scale=1024.0)


def test_the_diagnostic_gradients_need_a_number():
    c = cocoopfit_ref.make_case("tiny", 3, 4, 1)
    m = build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"})
    v = vptfit_ref.make_case("tiny", 2, 2, 1, 3)
    mv = build_model(dict(v["sd"]), {"trainer": "VPT", "vision_depth": 2, "vision_ctx": 2, "language_depth": 0, "language_ctx": 0})
    a = maplefit_ref.make_case("tiny3", 2, 1, 5, 3)
    ma = build_model(dict(a["sd"]), maplefit_ref.design(1))
    p = promptsrcfit_ref.make_case("tiny", 2, 2, 3, 2, 3, 3)
    mp = build_model(dict(p["sd"]), promptsrcfit_ref.design(3, 2, 2, 2))
    calls = [lambda gs: cocoopfit.gradients(m, c["ids"], c["params"], c["feats"], c["labels"], grad_scale=gs),
             lambda gs: vptfit.prompt_gradient(mv, v["prompts"], v["images"], v["labels"], v["text"], grad_scale=gs),
             lambda gs: maplefit.gradients(ma, a["pl"], a["images"], a["labels"], a["ids"], grad_scale=gs),
             lambda gs: promptsrcfit.gradients(mp, p["p"], p["images"], p["labels"], p["ids"], p["teacher"], grad_scale=gs)]
    for call in calls:
        with pytest.raises(ValueError, match="needs a number"):
            call("dynamic")
        with pytest.raises(ValueError, match="power of two"):
            call("auto")


def test_header_declares_the_entries_with_the_abi_at_16():
    text = open(os.path.join(ROOT, "include", "clipmi.h")).read()
    assert re.search(r"#define CLIPMI_ABI_VERSION 16\b", text) and _lib.ABI_VERSION == 16 and _lib.lib.clipmi_abi_version() == 16
    for n in NEW:
        assert re.search(r"\b(int|size_t) " + n + r"\(", text), n
        assert n in _lib.exported_symbols() and hasattr(_lib.lib, n) and n in _lib._SIGNATURES
    assert callable(ops.block_step_scaled)


def test_workspace_size():
    by = _lib.lib.clipmi_block_step_scaled_workspace_bytes
    assert by(0) == 0 and by(-1) == 0 and by(2 ** 39) == 0 and by(2 ** 39 - 1) > 0
    for total, flags in ((1, 256), (256, 256), (257, 256), (65537, 1280)):
        assert by(total) == bref.workspace_bytes(total) == 256 + flags + (4 * total + 255) // 256 * 256, total
    assert by(1) == 768 and by(256) == 1536 and by(257) == 1792
    assert by(4 * 64) == _lib.lib.clipmi_ctx_step_scaled_workspace_bytes(3, 64, 4, 0)       # one layout for both steps


def test_library_refuses_bad_calls_without_a_device():
    """Every refusal returns before anything is launched: with no device a launch would answer CLIPMI_ERR_HIP."""
    lib = _lib.lib
    p = ctypes.c_void_p(4096)

    def step(grad=p, params=p, buf=None, grad_out=None, total=1000, state=p, growth=2.0, backoff=0.5, interval=2000, lr=p, momentum=0.0,
             dampening=0.0, weight_decay=0.0, nesterov=0, ws=p, ws_bytes=1 << 20):
        return lib.clipmi_block_step_scaled(grad, params, buf, grad_out, total, state, growth, backoff, interval, lr, momentum, dampening, weight_decay,
                                            nesterov, ws, ws_bytes, None)
    for null in ("grad", "params", "state", "lr", "ws"):
        assert step(**{null: None}) == _lib.ERR_ARG and "null pointer" in _lib.last_error(), null
    for odd in ("grad", "params", "buf", "grad_out", "lr", "state"):
        assert step(**{odd: ctypes.c_void_p(4098)}, momentum=0.5 if odd == "buf" else 0.0) == _lib.ERR_ARG and "aligned" in _lib.last_error(), odd
    assert step(ws=ctypes.c_void_p(4096 + 8)) == _lib.ERR_ARG and "256-byte aligned" in _lib.last_error()
    assert step(momentum=0.9) == _lib.ERR_ARG and "buffer" in _lib.last_error()
    assert step(total=0) == _lib.ERR_SHAPE and step(total=-5) == _lib.ERR_SHAPE and step(total=2 ** 39, ws_bytes=1 << 62) == _lib.ERR_SHAPE
    for bad in (0.0, -2.0, math.inf, math.nan):
        assert step(growth=bad) == _lib.ERR_ARG and "growth_factor" in _lib.last_error()
        assert step(backoff=bad) == _lib.ERR_ARG and "backoff_factor" in _lib.last_error()
    assert step(interval=0) == _lib.ERR_ARG and "growth_interval" in _lib.last_error()
    assert step(momentum=1.0, buf=p) == _lib.ERR_ARG or step(momentum=-0.1, buf=p) == _lib.ERR_ARG
    assert step(nesterov=1) == _lib.ERR_ARG and step(dampening=-0.1) == _lib.ERR_ARG and step(weight_decay=-1.0) == _lib.ERR_ARG
    need = lib.clipmi_block_step_scaled_workspace_bytes(1000)
    assert step(ws_bytes=need - 1) == _lib.ERR_WORKSPACE and step(ws_bytes=64) == _lib.ERR_WORKSPACE
    assert step(ws_bytes=need) not in (_lib.OK, _lib.ERR_ARG, _lib.ERR_SHAPE, _lib.ERR_WORKSPACE)      # all checks pass: the launch has no device
    for by in (lib.clipmi_cocoop_train_step_scaled_bytes, lib.clipmi_maple_train_step_scaled_bytes):
        assert by(None, 3, 0, 2, 4, 4) == 0
    assert lib.clipmi_vpt_train_step_scaled_bytes(None, 2, 4, 2, 3) == 0 and lib.clipmi_promptsrc_train_step_scaled_bytes(None, 3, 0, 2, 2, 2, 2, 2) == 0


def test_one_call_sizes_with_a_model():
    """The scaled one-call workspaces are the static ones plus the block step's (and, where the step's launches leave no gradient block in
    the workspace, that block), 0 for what the static sizing refuses."""
    lib = _lib.lib
    m = build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"})
    m._ensure_handle()
    h, g = m._handle, m.geometry
    Dt, Dv, E = int(g.transformer_width), int(g.vision_width), int(g.embed_dim)
    bs = lib.clipmi_block_step_scaled_workspace_bytes
    up = lambda n: (n + 255) // 256 * 256
    total = lib.clipmi_cocoop_block_floats(4, Dt, E, 8)
    assert lib.clipmi_cocoop_train_step_scaled_bytes(h, 3, 0, 2, 8, 4) == lib.clipmi_cocoop_train_step_bytes(h, 3, 0, 2, 8, 4) + bs(total)
    assert lib.clipmi_cocoop_train_step_scaled_bytes(h, 1, 0, 2, 8, 4) == 0
    assert lib.clipmi_vpt_train_step_scaled_bytes(h, 2, 3, 2, 5) == lib.clipmi_vpt_train_step_bytes(h, 2, 3, 5) + bs(2 * 3 * Dv)
    assert lib.clipmi_vpt_train_step_scaled_bytes(h, 2, 3, 0, 5) == 0 and lib.clipmi_vpt_train_step_scaled_bytes(h, 0, 3, 2, 5) == 0
    total = lib.clipmi_maple_block_floats(2, 2, Dt, Dv)
    assert lib.clipmi_maple_train_step_scaled_bytes(h, 3, 0, 2, 2, 2) == lib.clipmi_maple_train_step_bytes(h, 3, 0, 2, 2, 2) + up(4 * total) + bs(total)
    assert lib.clipmi_maple_train_step_scaled_bytes(h, 3, 0, 0, 2, 2) == 0
    total = lib.clipmi_promptsrc_block_floats(2, 2, Dt, 3, 2, Dv)
    assert lib.clipmi_promptsrc_train_step_scaled_bytes(h, 3, 0, 2, 2, 2, 3, 2) == (lib.clipmi_promptsrc_train_step_bytes(h, 3, 0, 2, 2, 2, 3) + up(4 * total) +
                                                                                  bs(total))
    assert lib.clipmi_promptsrc_train_step_scaled_bytes(h, 3, 0, 2, 2, 2, 3, 0) == 0


def test_restatement_against_torch_on_the_cpu():
    """blockscaler_ref.BlockRef against torch's own operators on a flat block: a skip on the first step, growth on the second clean one."""
    total, lr = 300, 2.0 ** -3
    params, ints = bref.exact_block(total, 4, seed=3)
    r = bref.BlockRef(params, 2.0 ** 10, 2.0, 0.25, 2, momentum=0.5)
    q = torch.nn.Parameter(torch.from_numpy(params.copy()))
    opt = torch.optim.SGD([q], lr=lr, momentum=0.5)
    scale_t, tracker_t = torch.tensor([2.0 ** 10]), torch.zeros(1, dtype=torch.int32)
    for k, poison in enumerate((1, 0, 0, 0)):
        g = bref.scaled(ints[k], float(r.scale))
        if poison:
            g[total - 1] = np.nan
        gt, found = torch.from_numpy(g.copy()), torch.zeros(1)
        torch._amp_foreach_non_finite_check_and_unscale_([gt], found, 1.0 / scale_t)
        if float(found) == 0.0:
            q.grad = gt
            opt.step()
        torch._amp_update_scale_(scale_t, tracker_t, found, 2.0, 0.25, 2)
        assert r.step(g, lr) == bool(poison)
        assert float(r.scale) == float(scale_t) and r.growth_tracker == int(tracker_t) and np.array_equal(r.params, q.detach().numpy()), k
    assert r.state() == {"scale": 512.0, "growth_tracker": 1, "skipped_steps": 1, "applied_steps": 3, "found_inf": 0}
