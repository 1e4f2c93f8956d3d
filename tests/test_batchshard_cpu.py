"""CPU checks of the batch-sharded image-tower fits (``shard=`` on clip_calibration_amd/vptfit.py, maplefit.py, promptsrcfit.py;
csrc/shard_train.hip): the restatement of the rank mean, the identity the sharded step rests on -- the mean over equal parts of the
per-part gradients is the whole batch's gradient -- on the fits' float64 torch mirrors, the refusals that need no device, and the new
symbols in the header and the binding."""
import os
import re

import numpy as np
import pytest
import torch

import batchshard_ref as ref
import maplefit_ref
import promptsrcfit_ref
import vptfit_ref

from clip_calibration_amd import _lib, coopfit, maplefit, promptsrcfit, shard, vptfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_restatement_distinguishes_the_rank_order():
    g = np.zeros((3, 2), np.float32)
    g[:, 0] = ref.ORDER_TRIPLE
    g[:, 1] = (0.25, 0.5, 0.75)
    fwd, back = ref.rank_mean(g), ref.rank_mean(g[::-1])
    assert fwd[0] == np.float32(1.0) * np.float32(1.0 / 3) and back[0] == 0.0          # ((1e8 - 1e8) + 1) / 3 against ((1 - 1e8) + 1e8) / 3
    assert fwd[1] == back[1] == np.float32(1.5) * np.float32(1.0 / 3)
    assert abs(ref.rank_mean64(g)[0] - 1.0 / 3) < 1e-15 and abs(ref.rank_mean64(g[::-1])[0] - 1.0 / 3) < 1e-15
    one = np.array([[1e-40, -0.0, 3.5, np.inf]], np.float32)
    assert ref.rank_mean(one).tobytes() == one[0].tobytes()                            # one rank: x * 1.0f
    wide = np.array([[1.0, np.nan], [3.0, np.nan]], np.float32)
    assert ref.rank_mean(wide, 1).tolist() == [2.0]                                    # the padding is not read
    assert np.isnan(ref.rank_mean(np.array([[1.0, 2.0], [np.nan, np.inf]], np.float32))).tolist() == [True, False]


def parts_mean(grads_of, B, G):
    """The mean over the G equal parts [r B / G, (r + 1) B / G) of ``grads_of(rows)`` = (losses, {name: gradient}), in rank order."""
    n = B // G
    outs = [grads_of(slice(r * n, (r + 1) * n)) for r in range(G)]
    losses = sum(torch.as_tensor(o[0]).double().reshape(-1) for o in outs) / G
    return losses, {k: sum(o[1][k] for o in outs) / G for k in outs[0][1]}


def assert_same(whole, parts, what):
    lw, gw = torch.as_tensor(whole[0]).double().reshape(-1), whole[1]
    assert float((parts[0] - lw).abs().max()) <= 1e-12 * float(lw.abs().max()), what
    for k in gw:
        assert float(gw[k].norm()) > 0, (what, k)
        assert float((parts[1][k] - gw[k]).norm()) <= 1e-12 * float(gw[k].norm()), (what, k)


@pytest.mark.parametrize("G", [2, 4])
def test_mean_of_per_part_gradients_is_the_batch_gradient(G):
    """float64, batch 4: VPT, MaPLe and PromptSRC with all four loss terms on.  Every term of every loss is a mean over the rows it is
    given or does not depend on them (the text L1 term), so with equal parts the mean of the parts' losses and gradients is the whole
    batch's to rounding: 1e-12 relative."""
    B = 4
    v = vptfit_ref.make_case("tiny", 2, 2, B, 5)
    vpt = lambda rows: (lambda o: (o[0], {"prompts": o[1]}))(vptfit_ref.loss_and_grad(v["sd"], v["images"][rows], v["prompts"], v["text"], v["labels"][rows]))
    assert_same(vpt(slice(0, B)), parts_mean(vpt, B, G), "vpt")
    a = maplefit_ref.make_case("tiny3", 2, 1, 5, B)
    maple = lambda rows: maplefit_ref.loss_and_grads(a["sd"], a["ids"], a["pl"], a["images"][rows], a["labels"][rows])
    assert_same(maple(slice(0, B)), parts_mean(maple, B, G), "maple")
    p = promptsrcfit_ref.make_case("tiny", 2, 2, 3, 2, 3, B)
    assert all(w > 0 for w in promptsrcfit_ref.WEIGHTS)
    src = lambda rows: promptsrcfit_ref.loss_and_grads(p["sd"], p["ids"], p["p"], p["images"][rows], p["labels"][rows], p["teacher"])
    whole = src(slice(0, B))
    assert all(float(x) > 0 for x in whole[0])                                         # total, CE and the three regularisers
    assert_same(whole, parts_mean(src, B, G), "promptsrc")


def entry_points():
    """name -> a callable of keywords on CPU models: everything but the device is there (tests/test_optimstep_cpu.py's way)."""
    out = {}
    v = vptfit_ref.make_case("tiny", 2, 2, 4, 3)
    mv = build_model(dict(v["sd"]), {"trainer": "VPT", "vision_depth": 2, "vision_ctx": 2, "language_depth": 0, "language_ctx": 0})
    out["VPTFitState"] = lambda **kw: vptfit.VPTFitState(mv, v["text"], prompts=v["prompts"], **kw)
    out["fit_prompts"] = lambda **kw: vptfit.fit_prompts(v["images"], v["labels"], mv, v["text"], v["prompts"], epochs=1, **kw)
    out["prompt_gradient"] = lambda **kw: vptfit.prompt_gradient(mv, v["prompts"], v["images"], v["labels"], v["text"], **kw)
    a = maplefit_ref.make_case("tiny3", 2, 1, 5, 4)
    ma = build_model(dict(a["sd"]), maplefit_ref.design(1))
    out["MaPLeFitState"] = lambda **kw: maplefit.MaPLeFitState(ma, a["ids"], a["pl"], **kw)
    out["fit_prompt_learner"] = lambda **kw: maplefit.fit_prompt_learner(a["images"], a["labels"], ma, a["ids"], a["pl"], epochs=1, **kw)
    out["maplefit.gradients"] = lambda **kw: maplefit.gradients(ma, a["pl"], a["images"], a["labels"], a["ids"], **kw)
    p = promptsrcfit_ref.make_case("tiny", 2, 2, 3, 2, 3, 4)
    mp = build_model(dict(p["sd"]), promptsrcfit_ref.design(3, 2, 2, 2))
    for method in promptsrcfit.METHODS:
        out[f"PromptSRCFitState[{method}]"] = lambda method=method, **kw: promptsrcfit.PromptSRCFitState(mp, p["ids"], p["p"], p["teacher"], method=method, **kw)
        out[f"promptsrcfit.fit_prompts[{method}]"] = (
            lambda method=method, **kw: promptsrcfit.fit_prompts(p["images"], p["labels"], mp, p["ids"], p["teacher"], p["p"], method=method, epochs=1, **kw))
        out[f"promptsrcfit.gradients[{method}]"] = (
            lambda method=method, **kw: promptsrcfit.gradients(mp, p["p"], p["images"], p["labels"], p["ids"], p["teacher"], method=method, **kw))
    return out


ENTRY = None
STATES = ["VPTFitState", "MaPLeFitState", "PromptSRCFitState[promptsrc]", "PromptSRCFitState[ivlp]"]
FITS = ["fit_prompts", "fit_prompt_learner", "promptsrcfit.fit_prompts[promptsrc]", "promptsrcfit.fit_prompts[ivlp]"]
GRADIENTS = ["prompt_gradient", "maplefit.gradients", "promptsrcfit.gradients[promptsrc]", "promptsrcfit.gradients[ivlp]"]


def entry(name):
    global ENTRY
    if ENTRY is None:
        ENTRY = entry_points()
    return ENTRY[name]


def two():
    return coopfit.Shard(2, 0, coopfit.LocalGather(2))


def who_of(name):
    return name.split("[")[0].replace("promptsrcfit.fit_prompts", "fit_prompts")


@pytest.mark.parametrize("name", STATES + FITS + GRADIENTS)
def test_shard_is_accepted_and_checked_before_any_device_call(name):
    call = entry(name)
    with pytest.raises(ValueError, match=f"{who_of(name)}: shard must be a coopfit.Shard"):
        call(shard=(2, 0))
    for opt in ("sgd", "adam", "adamw"):                             # all three optimisers and both loss scales pass the checks:
        for scale in ({}, {"grad_scale": "dynamic"}):                 # the call gets as far as needing the device
            if name in GRADIENTS and (opt != "sgd" or scale):
                continue
            with pytest.raises(RuntimeError, match="GPU"):
                call(shard=two(), **({} if name in GRADIENTS else {"optimizer": opt}), **scale)


@pytest.mark.parametrize("name", FITS)
def test_fit_functions_refuse_by_name(name):
    call, who = entry(name), who_of(name)
    with pytest.raises(ValueError, match=rf"{who}: a batch of B=3 images does not split over G=2 ranks"):
        call(shard=two(), batch_size=3)
    with pytest.raises(ValueError, match=rf"{who}: a batch of B=1 images does not split over G=2 ranks"):
        call(shard=two(), batch_size=1)
    with pytest.raises(RuntimeError, match="GPU"):                   # four images in batches of two: everything checks out
        call(shard=two(), batch_size=2)
    with pytest.raises(ValueError, match=f"{who}: shard has no validation: val="):
        call(shard=two(), val=(torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(ValueError, match=f"{who}: shard has no validation: val=.*best_val"):
        call(shard=two(), final_model="best_val")
    if "promptsrcfit" in name:
        with pytest.raises(ValueError, match=f"{who}: shard has no one-call step \\(one_call=True\\)"):
            call(shard=two(), one_call=True)


@pytest.mark.parametrize("name", GRADIENTS)
def test_gradients_refuse_operand_stats_by_name(name):
    with pytest.raises(ValueError, match=f"{who_of(name)}: shard returns no operand statistics \\(return_operand_stats=True\\)"):
        entry(name)(shard=two(), return_operand_stats=True)


def test_trainers_refuse_before_either_tower_runs():
    """``val_loader=`` under ``shard`` through the trainers' ``**fit_args``: this loader cannot be iterated."""
    from clip_calibration_amd.trainers import _fit
    for who in ("fit_prompts", "fit_prompt_learner"):
        with pytest.raises(ValueError, match=f"{who}: shard has no validation"):
            _fit.checked_shard(who, {"shard": two(), "val_loader": object()}, "block")
        with pytest.raises(ValueError, match=f"{who}: shard has no one-call step"):
            _fit.checked_shard(who, {"shard": two(), "one_call": True}, "block")
        assert _fit.checked_shard(who, {"lr": 1e-3}, "block") is None and isinstance(_fit.checked_shard(who, {"shard": two()}, "block"), coopfit.Shard)


def test_check_shard_batch():
    sh = coopfit.Shard(4, 1, coopfit.LocalGather(4))
    assert shard.check_batch("f", sh, 8) == 2 and shard.check_batch("f", sh, 4) == 1
    for B in (1, 3, 6):
        with pytest.raises(ValueError, match=f"f: a batch of B={B} images does not split over G=4 ranks"):
            shard.check_batch("f", sh, B)


def test_header_and_binding_carry_the_entry_points():
    header = open(os.path.join(ROOT, "include", "clipmi.h")).read()
    for name in ("clipmi_block_rank_mean", "clipmi_block_step_gathered"):
        assert re.search(rf"\bint {name}\(const float\* gathered, int world, size_t stride, size_t total,", header), name
        assert name in _lib.exported_symbols() and hasattr(_lib.lib, name)
    assert _lib.ABI_VERSION == 16 and re.search(r"#define CLIPMI_ABI_VERSION 16\b", header) and _lib.lib.clipmi_abi_version() == 16


def test_c_refusals_need_no_device():
    """Every refusal of clipmi_block_rank_mean comes before the launch: host addresses are refused the same way."""
    lib = _lib.lib
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    for args, rc in (((None, 2, 8, 8, p + 256), _lib.ERR_ARG), ((p, 2, 8, 8, None), _lib.ERR_ARG), ((p + 1, 2, 8, 8, p + 128), _lib.ERR_ARG),
                     ((p, 0, 8, 8, p + 128), _lib.ERR_SHAPE), ((p, 2, 8, 0, p + 128), _lib.ERR_SHAPE), ((p, 2, 2 ** 39, 2 ** 39, p + 128), _lib.ERR_SHAPE),
                     ((p, 2, 7, 8, p + 128), _lib.ERR_SHAPE), ((p, 2, 8, 8, p + 32), _lib.ERR_ARG)):
        assert lib.clipmi_block_rank_mean(*args, None) == rc, (args, _lib.last_error())
    assert "overlaps" in _lib.last_error()
    assert not buf.any()
