"""Nearest rows without a GPU: the three C symbols and the unchanged ABI, every refusal of clipmi_nearest_rows (shape before pointers,
all of it before a device is touched), the split rule and the workspace size, and the host side of clip_calibration_amd.interpret --
ClipTokenizer.symbol, prompt_layers, format_report -- plus the float64 restatement the GPU tests are held to."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import nearest_ref as ref
from clip_calibration_amd import _lib, interpret
from clip_calibration_amd.tokenizer import ClipTokenizer
from conftest import GOLDEN

L = _lib.lib
P = ctypes.c_void_p(4096)


def test_symbols_and_abi():
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define CLIPMI_ABI_VERSION 16\b", header) and _lib.ABI_VERSION == 16 and L.clipmi_abi_version() == 16
    for name in ("clipmi_nearest_rows", "clipmi_nearest_rows_workspace", "clipmi_nearest_rows_splits"):
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols() and hasattr(L, name) and f" {name}(" in header


def _call(Nq=8, Nr=100, E=64, K=10, splits=1, q=P, refs=P, dist=P, idx=P, ws=P, ws_bytes=1 << 30):
    return L.clipmi_nearest_rows(q, refs, dist, idx, Nq, Nr, E, K, splits, ws, ws_bytes, None)


def test_refusals_need_no_device():
    for kw in (dict(K=0), dict(K=33, Nr=100), dict(K=11, Nr=10), dict(E=96), dict(E=0), dict(Nq=-1), dict(Nr=-5), dict(Nr=0), dict(splits=-1)):
        assert _call(**kw) == _lib.ERR_SHAPE, kw
        assert "nearest_rows" in _lib.last_error()
    assert _call(K=33) == _lib.ERR_SHAPE and "K=33" in _lib.last_error()
    # shape before null pointers: a bad shape with null pointers is a shape error
    assert _call(E=96, q=None, refs=None) == _lib.ERR_SHAPE
    for name in ("q", "refs", "dist", "idx"):
        assert _call(**{name: None}) == _lib.ERR_ARG, name
        assert "null" in _lib.last_error()
    assert _call(q=ctypes.c_void_p(4100)) == _lib.ERR_ARG and "aligned" in _lib.last_error()
    need = L.clipmi_nearest_rows_workspace(8, 100, 10, 3)
    assert need == 3 * 8 * 10 * 8
    assert _call(splits=3, ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error()
    assert _call(splits=3, ws=None, ws_bytes=need) == _lib.ERR_WORKSPACE
    # splits = 0 resolves to the library's choice before the workspace is measured
    auto = L.clipmi_nearest_rows_splits(8, 100)
    assert _call(splits=0, ws_bytes=L.clipmi_nearest_rows_workspace(8, 100, 10, 0) - 1) == _lib.ERR_WORKSPACE
    assert L.clipmi_nearest_rows_workspace(8, 100, 10, 0) == L.clipmi_nearest_rows_workspace(8, 100, 10, auto)
    # no query rows: nothing to do, whatever the pointers
    assert _call(Nq=0, q=None, refs=None, dist=None, idx=None, ws=None, ws_bytes=0) == _lib.OK
    assert _call(Nq=0, K=0) == _lib.ERR_SHAPE                                       # ... but the shape is still checked


def test_split_rule_and_workspace():
    query_blocks = lambda nq: (nq + 15) // 16
    for nq in (4, 16, 144):
        s = L.clipmi_nearest_rows_splits(nq, 49408)
        assert s * query_blocks(nq) >= 256, (nq, s)
        assert s <= (49408 + 63) // 64                                               # never more slices than 64-row tiles
    assert L.clipmi_nearest_rows_splits(16000, 49408) == 3 and L.clipmi_nearest_rows_splits(1 << 20, 49408) == 1   # query blocks fill the chip by themselves
    assert L.clipmi_nearest_rows_splits(16, 64) == 1 and L.clipmi_nearest_rows_splits(1, 1) == 1
    assert L.clipmi_nearest_rows_splits(16, 65) == 2 and L.clipmi_nearest_rows_splits(16, 64 * 7) == 7
    one = L.clipmi_nearest_rows_workspace(144, 49408, 10, 1)
    assert one == 144 * 10 * 8
    for s in (2, 3, 7, 100, 1000):
        assert L.clipmi_nearest_rows_workspace(144, 49408, 10, s) == s * one
    for bad in ((144, 49408, 0, 1), (144, 49408, 33, 1), (144, 5, 10, 1), (-1, 49408, 10, 1), (144, 0, 10, 1), (144, 49408, 10, -1)):
        assert L.clipmi_nearest_rows_workspace(*bad) == 0, bad


def test_ops_refuses_host_and_half_tensors():
    from clip_calibration_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nearest_rows(torch.zeros(4, 64), torch.zeros(100, 64), 10)


def test_reference_restatement():
    """The float64 reference itself: stable ties, NaN rows last by index, distances not squared."""
    refs = np.zeros((6, 64), dtype=np.float32)
    refs[1, 0], refs[2, 0], refs[3, 0], refs[4, 0], refs[5, 0] = 3, 1, 3, np.nan, 1
    q = np.zeros((2, 64), dtype=np.float32)
    q[1, 5] = np.nan
    dist, idx, sq = ref.nearest_rows(q, refs, 6)
    assert idx[0].tolist() == [0, 2, 5, 1, 3, 4] and dist[0].tolist() == [0, 1, 1, 3, 3, np.inf]
    assert idx[1].tolist() == [0, 1, 2, 3, 4, 5] and np.isinf(dist[1]).all() and sq.shape == (2, 6)


def test_tokenizer_symbol_on_the_sparse_table():
    fx = json.load(open(os.path.join(GOLDEN, "tokenizer_cases.json")))
    tok = ClipTokenizer(merges={(a, b): r for a, b, r in fx["merges"]})
    assert tok.symbol(1125) == "photo</w>" and tok.symbol(320) == "a</w>" and tok.symbol(539) == "of</w>"
    assert tok.symbol(0) == "!" and tok.symbol(256) == "!</w>"
    assert tok.symbol(tok.sot) == "<|startoftext|>" and tok.symbol(torch.tensor(tok.eot)) == "<|endoftext|>"
    known = {512 + r for _, _, r in fx["merges"]}
    unknown = next(i for i in range(512, 49406) if i not in known)
    assert tok.symbol(unknown) == f"<{unknown}>" and tok.symbol(10 ** 6) == "<1000000>"
    a, b, r = fx["merges"][0]
    assert tok.symbol(512 + r) == a + b


def _t(*shape):
    return torch.zeros(*shape)


def test_prompt_layers_order_and_filtering():
    coop = {"ctx": _t(16, 512), "token_prefix": _t(3, 1, 512), "token_suffix": _t(3, 60, 512)}
    assert [k for k, _ in interpret.prompt_layers(coop)] == ["ctx"]
    csc = {"state_dict": {"prompt_learner.ctx": _t(5, 16, 512), "prompt_learner.token_prefix": _t(5, 1, 512)}, "epoch": 3}
    (name, value), = interpret.prompt_layers(csc)
    assert name == "prompt_learner.ctx" and value.shape == (5, 16, 512)
    maple = {"prompt_learner.token_prefix": _t(3, 1, 512), "prompt_learner.proj.weight": _t(768, 512), "prompt_learner.proj.bias": _t(768)}
    for i in (10, 2, 0, 1):                                                           # out of order on purpose: 10 sorts after 2
        maple[f"prompt_learner.compound_prompts_text.{i}"] = _t(2, 512)
        maple[f"prompt_learner.compound_prompt_projections.{i}.weight"] = _t(768, 512)
    maple["prompt_learner.ctx"] = _t(2, 512)
    assert [k for k, _ in interpret.prompt_layers(maple)] == ["prompt_learner.ctx"] + [f"prompt_learner.compound_prompts_text.{i}" for i in (0, 1, 2, 10)]
    assert [k for k, _ in interpret.prompt_layers({"state_dict": maple, "epoch": 5})] == [k for k, _ in interpret.prompt_layers(maple)]
    ivlp = {"image_encoder.VPT": _t(4, 768), "prompt_learner.ctx": _t(4, 512), "text_encoder.transformer.resblocks.11.VPT_shallow": _t(4, 512),
            "image_encoder.transformer.resblocks.1.VPT_shallow": _t(4, 768), "text_encoder.transformer.resblocks.2.VPT_shallow": _t(4, 512),
            "text_encoder.transformer.resblocks.1.VPT_shallow": _t(4, 512), "visual.transformer.resblocks.2.VPT_shallow": _t(4, 768)}
    assert [k for k, _ in interpret.prompt_layers(ivlp)] == ["prompt_learner.ctx"] + [f"text_encoder.transformer.resblocks.{i}.VPT_shallow" for i in (1, 2, 11)]
    assert interpret.prompt_layers({"visual.VPT": _t(4, 768), "epoch": 1}) == []
    with pytest.raises(ValueError):
        interpret.prompt_layers({"a.ctx": _t(2, 8), "b.ctx": _t(2, 8)})
    with pytest.raises(KeyError):
        interpret.interpret_prompt_learner({"visual.VPT": _t(4, 768)}, _t(100, 768))


def test_format_report_literal():
    two = interpret.NearestWords(indices=torch.tensor([[1125, 320], [7, 9]], dtype=torch.int32),
                                 distances=torch.tensor([[0.5, 1.25], [2.0, 3.14159]]), words=[["photo</w>", "a</w>"], ["(", "*"]])
    assert interpret.format_report(two) == (
        "SHOWING RESULTS FOR CTX Vectors of Layer:  1\n"
        "1: ['photo</w>', 'a</w>'] ['0.5000', '1.2500']\n"
        "2: ['(', '*'] ['2.0000', '3.1416']\n"
        "##############################\n"
        "##############################\n")
    csc = interpret.NearestWords(indices=torch.tensor([[[3], [4]], [[5], [6]]], dtype=torch.int32),
                                 distances=torch.tensor([[[1.0], [2.0]], [[3.0], [4.5]]]))
    assert interpret.format_report([two, csc]).splitlines()[5:] == [
        "SHOWING RESULTS FOR CTX Vectors of Layer:  2", "Class 0:", "1: [3] ['1.0000']", "2: [4] ['2.0000']",
        "Class 1:", "1: [5] ['3.0000']", "2: [6] ['4.5000']", "#" * 30, "#" * 30]
