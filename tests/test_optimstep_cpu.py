"""The Adam / AdamW step of the prompt fits without a GPU: the references of tests/optimstep_ref.py against torch.optim on the CPU, the
bias table against Python's own doubles, the header and the binding, the C entry points' refusals (they precede the first launch and need
no device) and the fits' host-side refusals on CPU models."""
import math

import numpy as np
import pytest
import torch

import cocoopfit_ref
import coopfit_ref
import maplefit_ref
import optimstep_ref as oref
import prodafit_ref
import promptsrcfit_ref
import vptfit_ref

from clip_calibration_amd import _lib, cocoopfit, coopfit, fitloop, maplefit, ops, prodafit, promptsrcfit, vptfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

RULES = [(False, 0.0), (False, 5e-4), (True, 0.0), (True, 5e-4)]


@pytest.mark.parametrize("decoupled,wd", RULES)
def test_float64_form_equals_torch_in_float64(decoupled, wd):
    w, g = oref.make_block(1000)
    mine = oref.rule64_run(w, g, weight_decay=wd, decoupled=decoupled)
    theirs = oref.torch_run(w, g, torch.float64, weight_decay=wd, decoupled=decoupled)
    err = float(np.abs(mine - theirs).max())
    print(f"optimstep: float64 form vs torch float64, decoupled={decoupled} wd={wd}: {err:.3e}")
    assert err <= 8 * np.finfo(np.float64).eps * float(np.abs(theirs).max())      # a few float64 roundings of values of order max|w|


@pytest.mark.parametrize("decoupled,wd", RULES)
@pytest.mark.parametrize("total", oref.SEAMS)
def test_fp32_restatement_within_the_criterion_of_torch(total, decoupled, wd):
    w, g = oref.make_block(total)
    t64 = oref.torch_run(w, g, torch.float64, weight_decay=wd, decoupled=decoupled)
    t32 = oref.torch_run(w, g, torch.float32, weight_decay=wd, decoupled=decoupled)
    mine = np.stack([s[0] for s in oref.emulate_run(w, g, weight_decay=wd, decoupled=decoupled)])
    err, bound = oref.within_torch(mine, t32, t64)
    print(f"optimstep: fp32 restatement total={total} decoupled={decoupled} wd={wd}: {err:.3e} <= {bound:.3e}")
    assert np.isfinite(mine).all() and err <= bound


def test_the_scale_is_taken_out_exactly():
    w, g = oref.make_block(257)
    plain = oref.emulate_run(w, g, weight_decay=5e-4)
    scaled = oref.emulate_run(w, (g[:, :] * np.float32(4096.0)).astype(np.float32), grad_scale=4096.0, weight_decay=5e-4)
    finite = np.isfinite(g * np.float32(4096.0)).all()
    assert finite and all(np.array_equal(a[0], b[0]) for a, b in zip(plain, scaled))


def test_bias_table_is_pythons_own():
    for betas in ((0.9, 0.999), (0.5, 0.75), (0.0, 0.0)):
        table = fitloop.adam_bias_table(betas, 300)
        assert table.dtype == np.float64 and table.shape == (300, 2)
        for t in (1, 2, 7, 300):
            assert table[t - 1, 0] == 1 - betas[0] ** t and table[t - 1, 1] == math.sqrt(1 - betas[1] ** t)
        assert np.array_equal(table, oref.bias_table(betas, 300))
    with pytest.raises(ValueError, match="steps=0"):
        fitloop.adam_bias_table((0.9, 0.999), 0)


def test_threads_are_the_headers():
    assert oref.threads() == 256 and 256 in oref.SEAMS and 255 in oref.SEAMS and 257 in oref.SEAMS


def test_header_and_binding_carry_the_entry_points():
    header = open(_lib.HEADER_PATH).read()
    for name in ("clipmi_block_step_adam", "clipmi_block_step_adam_scaled_workspace_bytes", "clipmi_block_step_adam_scaled"):
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols() and hasattr(_lib.lib, name) and f" {name}(" in header
    for name in ("block_step_adam", "block_step_adam_scaled"):
        assert callable(getattr(ops, name))
    assert callable(fitloop.check_adam) and callable(fitloop.adam_bias_table)


def test_c_refusals_precede_every_launch():
    L = _lib.lib
    p, ws = 4096, 1 << 20           # never dereferenced: every call below is refused

    def static(**k):
        return L.clipmi_block_step_adam(k.get("grad", p), k.get("params", p), k.get("m", p), k.get("v", p), k.get("out", None), k.get("total", 10),
                                        k.get("gs", 1.0), k.get("lr", p), k.get("t", 1), k.get("table", p), k.get("rows", 4), k.get("b1", 0.9),
                                        k.get("b2", 0.999), k.get("eps", 1e-8), k.get("wd", 0.0), 0, None)

    def scaled(**k):
        return L.clipmi_block_step_adam_scaled(k.get("grad", p), k.get("params", p), k.get("m", p), k.get("v", p), k.get("out", None),
                                               k.get("total", 10), k.get("state", p), k.get("growth", 2.0), k.get("backoff", 0.5),
                                               k.get("interval", 2000), k.get("lr", p), k.get("table", p), k.get("rows", 4), k.get("b1", 0.9),
                                               k.get("b2", 0.999), k.get("eps", 1e-8), k.get("wd", 0.0), 0, k.get("ws", p), k.get("wsb", ws), None)

    for call in (static, scaled):
        for name in ("grad", "params", "m", "v", "lr", "table"):
            assert call(**{name: None}) == _lib.ERR_ARG and "null pointer" in _lib.last_error(), name
        for name in ("grad", "params", "m", "v", "lr", "out"):
            assert call(**{name: 4098}) == _lib.ERR_ARG and "4-byte aligned" in _lib.last_error(), name
        assert call(table=4100) == _lib.ERR_ARG and "8-byte aligned" in _lib.last_error()
        assert call(rows=0) == _lib.ERR_ARG and "table_len" in _lib.last_error()
        assert call(total=0) == _lib.ERR_SHAPE and "total=0" in _lib.last_error()
        assert call(total=1 << 39) == _lib.ERR_SHAPE and "too many" in _lib.last_error()
        for b in (-0.1, 1.0, math.nan):
            assert call(b1=b) == _lib.ERR_ARG and "beta1" in _lib.last_error()
            assert call(b2=b) == _lib.ERR_ARG and "beta2" in _lib.last_error()
        for e in (0.0, -1e-8, math.inf, math.nan):
            assert call(eps=e) == _lib.ERR_ARG and "eps" in _lib.last_error()
        for w in (-1e-4, math.inf, math.nan):
            assert call(wd=w) == _lib.ERR_ARG and "weight_decay" in _lib.last_error()
    for gs in (0.0, -1.0, math.inf, math.nan):
        assert static(gs=gs) == _lib.ERR_ARG and "grad_scale" in _lib.last_error()
    assert static(t=0) == _lib.ERR_ARG and "t=0" in _lib.last_error()
    assert static(t=5, rows=4) == _lib.ERR_ARG and "behind the bias table of 4 steps" in _lib.last_error()      # the table bound
    assert scaled(state=None) == _lib.ERR_ARG and "state block" in _lib.last_error()
    assert scaled(growth=0.0) == _lib.ERR_ARG and scaled(backoff=math.inf) == _lib.ERR_ARG and scaled(interval=0) == _lib.ERR_ARG
    assert scaled(ws=None) == _lib.ERR_ARG and "workspace" in _lib.last_error()
    assert scaled(ws=4096 + 128) == _lib.ERR_ARG and "256-byte aligned" in _lib.last_error()
    need = L.clipmi_block_step_adam_scaled_workspace_bytes(10)
    assert need == L.clipmi_block_step_scaled_workspace_bytes(10) > 0
    assert scaled(wsb=need - 1) == _lib.ERR_WORKSPACE
    assert L.clipmi_block_step_adam_scaled_workspace_bytes(0) == 0 and L.clipmi_block_step_adam_scaled_workspace_bytes(1 << 39) == 0


def test_ops_refuse_host_tensors():
    z = torch.zeros(4)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.block_step_adam(z, z, z, z, z[:1], 1, torch.zeros(2, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.block_step_adam_scaled(z, torch.zeros(5, dtype=torch.int32), z, z, z, z[:1], torch.zeros(2, 2, dtype=torch.float64))


def test_check_optimizer_and_check_adam():
    assert fitloop.check_optimizer("f", "sgd", 0.5, 0.1, False, 1e-3) == ("sgd", 0.5, 0.1, False, None)
    assert fitloop.check_optimizer("f", "adamw", 0.9, 0.0, False, 1e-3, (0.8, 0.9), 1e-6) == ("adamw", 0.0, 0.0, False, (0.8, 0.9))
    with pytest.raises(ValueError, match="f: optimizer='rmsprop' must be one of"):
        fitloop.check_optimizer("f", "rmsprop", 0.9, 0.0, False, 0.0)
    for bad in ((1.0, 0.9), (0.9, -0.1), (0.9,), "ab", 0.9):
        with pytest.raises(ValueError, match="betas"):
            fitloop.check_adam("f", bad, 1e-8, 0.0)
    for eps in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="eps"):
            fitloop.check_adam("f", (0.9, 0.999), eps, 0.0)
    for wd in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="weight_decay"):
            fitloop.check_adam("f", (0.9, 0.999), 1e-8, wd)


def entry_points():
    """name -> (a callable of optimiser keywords on CPU models, its ``who``): everything but the device is there."""
    out = {}
    k = coopfit_ref.make_case("tiny", 5, 4, 4)
    m = build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"})
    teacher = torch.randn(5, m.geometry.embed_dim, generator=torch.Generator().manual_seed(3))
    for method in coopfit.METHODS:
        extra = {} if method == "coop" else {"method": method, "teacher": teacher}
        out[f"coopfit.CoOpFitState[{method}]"] = lambda extra=extra, **kw: coopfit.CoOpFitState(m, k["ids"], k["ctx"], **extra, **kw)
        out[f"coopfit.fit_context[{method}]"] = lambda extra=extra, **kw: coopfit.fit_context(k["feats"], k["labels"], m, k["ids"], k["ctx"], epochs=1,
                                                                                              **extra, **kw)
    d = prodafit_ref.make_case("tiny", 3, 4, 8, 4, 2)
    out["prodafit.ProDAFitState"] = lambda **kw: prodafit.ProDAFitState(m, d["ids"], d["ctx"], prompt_bs=4, **kw)
    out["prodafit.fit_context"] = lambda **kw: prodafit.fit_context(d["feats"], d["labels"], m, d["ids"], d["ctx"], prompt_bs=4, epochs=1, **kw)
    c = cocoopfit_ref.make_case("tiny", 3, 4, 1)
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


def entry(name):
    global ENTRY
    if ENTRY is None:
        ENTRY = entry_points()
    return ENTRY[name]


NAMES = ([f"coopfit.{f}[{m}]" for f in ("CoOpFitState", "fit_context") for m in ("coop", "kgcoop", "prograd")]
         + ["prodafit.ProDAFitState", "prodafit.fit_context", "cocoopfit.CoCoOpFitState", "cocoopfit.fit_prompt_learner", "vptfit.VPTFitState",
            "vptfit.fit_prompts", "maplefit.MaPLeFitState", "maplefit.fit_prompt_learner"]
         + [f"promptsrcfit.{f}[{m}]" for f in ("PromptSRCFitState", "fit_prompts") for m in ("promptsrc", "ivlp")])


@pytest.mark.parametrize("name", NAMES)
def test_fits_refuse_by_name_before_any_device_call(name):
    call = entry(name)
    who = name.split(".")[1].split("[")[0]
    with pytest.raises(ValueError, match=f"{who}: optimizer='rmsprop' must be one of"):
        call(optimizer="rmsprop")
    for opt in ("adam", "adamw"):
        with pytest.raises(ValueError, match=f"{who}: momentum=0.5 is an argument of optimizer='sgd'"):
            call(optimizer=opt, momentum=0.5)
        with pytest.raises(ValueError, match="dampening=0.1 is an argument of optimizer='sgd'"):
            call(optimizer=opt, dampening=0.1)
        with pytest.raises(ValueError, match="nesterov=True is an argument of optimizer='sgd'"):
            call(optimizer=opt, nesterov=True)
        with pytest.raises(ValueError, match="betas"):
            call(optimizer=opt, betas=(0.9, 1.0))
        with pytest.raises(ValueError, match="eps=0"):
            call(optimizer=opt, eps=0.0)
        with pytest.raises(ValueError, match="weight_decay=-1"):
            call(optimizer=opt, weight_decay=-1.0)
        with pytest.raises(RuntimeError, match="GPU"):
            call(optimizer=opt)                                   # everything checks out: the call needs the device
    with pytest.raises(ValueError, match="momentum=1.5"):         # SGD's own checks are where they were
        call(optimizer="sgd", momentum=1.5)


def test_shard_and_one_call_stay_sgd():
    two = coopfit.Shard(2, 0, coopfit.LocalGather(2))
    for name in ("coopfit.CoOpFitState[coop]", "coopfit.fit_context[coop]", "coopfit.fit_context[prograd]"):
        with pytest.raises(ValueError, match="shard with optimizer='adam': the class-sharded fit stays SGD"):
            entry(name)(optimizer="adam", shard=two)
    for method in ("promptsrc", "ivlp"):
        with pytest.raises(ValueError, match="fit_prompts: one_call=True with optimizer='adamw': the one-call steps stay SGD"):
            entry(f"promptsrcfit.fit_prompts[{method}]")(optimizer="adamw", one_call=True)
