"""The row-chunked validation score and the image-tower fits' validation arguments, without a GPU: the numpy restatement of the row
result and of the finish's order against tests/fitmonitor_ref.py for every chunking the GPU tests use, the argument checks of the new
keywords on the three fit functions, the new symbols and their host-side refusals."""
import inspect

import numpy as np
import pytest
import torch

import blockmonitor_ref as bref
import fitmonitor_ref as ref
from clip_calibration_amd import _lib, fitmonitor, maplefit, ops, promptsrcfit, vptfit

NEW_SYMBOLS = ("clipmi_val_score_rows", "clipmi_val_score_finish", "clipmi_val_score_finish_workspace_bytes", "clipmi_vision_val_chunk",
               "clipmi_vision_val_chunk_bytes")
FITS = [(vptfit.fit_prompts, 4), (maplefit.fit_prompt_learner, 4), (promptsrcfit.fit_prompts, 5)]     # (function, leading positionals)
NEW_KEYWORDS = ["val", "val_batch_size", "val_bins", "final_model", "val_criterion", "return_monitor"]


@pytest.mark.parametrize("N,C", [(1, 2), (63, 5), (64, 1), (65, 7), (129, 63), (257, 11)])
def test_the_restated_finish_equals_the_record_for_every_chunking(N, C):
    n_bins = 10
    z, y = ref.clean_logits(N, C, n_bins, seed=31 * N + C)
    want = ref.record(z, y, n_bins)
    rows = bref.row_results(z, y, n_bins)
    got_by = {name: bref.chunked_record(z, y, n_bins, sizes) for name, sizes in bref.chunkings(N).items()}
    assert set(got_by) == {"one", "ones", "seam", "partials", "straddle"}
    first = got_by["one"]
    for name, got in got_by.items():
        assert got["n"] == want["n"] == N and got["correct"] == want["correct"], name
        assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["hits"], want["hits"]), name
        assert abs(got["nll_sum"] - want["nll_sum"]) <= bref.sum_bound(rows["nll"]), name
        for b in range(n_bins + 1):
            assert abs(got["conf_sum"][b] - want["conf_sum"][b]) <= bref.sum_bound(rows["conf"][rows["bin"] == b]), (name, b)
        # the order of additions does not depend on the chunking: the same bits
        assert got["nll_sum"] == first["nll_sum"] and np.array_equal(got["conf_sum"], first["conf_sum"]), name


def test_chunkings_put_their_seams_where_they_say():
    c = bref.chunkings(129)
    assert c["seam"] == [5, 59, 1, 64] and c["straddle"] == [63, 2, 64] and c["partials"] == [64, 64, 1] and len(c["ones"]) == 129
    assert all(sum(v) == 1 for v in bref.chunkings(1).values())
    assert bref.chunkings(63)["seam"] == [5, 58] and bref.chunkings(64)["straddle"] == [63, 1]


def test_defined_outcomes_of_the_row_result():
    z = np.array([[1.0, 1.0, -3.0], [np.nan, 0.0, 0.0], [0.0, 2.0, 1.0], [0.0, 0.0, 0.0]], np.float32)
    y = np.array([1, 1, 3, -1])
    r = bref.row_results(z, y, 10)
    assert not r["hit"][0] and np.isfinite(r["nll"][0])                              # a tie: the lower index wins, the label sits on the higher
    assert not r["hit"][1] and np.isnan(r["nll"][1]) and np.isnan(r["conf"][1]) and r["bin"][1] == 10
    assert not r["hit"][2] and np.isnan(r["nll"][2]) and np.isfinite(r["conf"][2])   # labels outside [0, C)
    assert not r["hit"][3] and np.isnan(r["nll"][3])


def test_new_symbols_and_sizes():
    names = set(_lib.exported_symbols())
    for s in NEW_SYMBOLS:
        assert s in names and hasattr(_lib.lib, s), s
    L = _lib.lib
    for N, n_bins in ((1, 10), (64, 10), (65, 15), (257, 64)):
        assert L.clipmi_val_score_finish_workspace_bytes(N, n_bins) == L.clipmi_val_score_workspace_bytes(N, n_bins) > 0
    assert L.clipmi_val_score_finish_workspace_bytes(0, 10) == 0 and L.clipmi_val_score_finish_workspace_bytes(5, 65) == 0
    assert L.clipmi_vision_val_chunk_bytes(None, 4, 2, 3) == 0
    assert ops.VAL_ROW_BYTES == 16 and ops._ROW_DTYPE.itemsize == 16


def test_refusals_come_before_any_launch():
    L = _lib.lib
    p, q, ws = 4096, 4100, 1 << 16
    rows = lambda **k: L.clipmi_val_score_rows(k.get("z", p), k.get("ld", 4), k.get("y", p), k.get("rows", 2), k.get("C", 4), k.get("bins", 10),
                                               k.get("rr", p), None)
    assert rows(z=None) == _lib.ERR_ARG and rows(y=None) == _lib.ERR_ARG and rows(rr=None) == _lib.ERR_ARG
    assert rows(z=q) == _lib.ERR_ARG and "16-byte" in _lib.last_error()
    assert rows(rr=4104) == _lib.ERR_ARG and "16-byte" in _lib.last_error()
    assert rows(y=q) == _lib.ERR_ARG and "8-byte" in _lib.last_error()
    assert rows(rows=0) == _lib.ERR_SHAPE and rows(C=0) == _lib.ERR_SHAPE and rows(ld=3) == _lib.ERR_SHAPE
    assert rows(bins=0) == _lib.ERR_ARG and rows(bins=65) == _lib.ERR_ARG and "n_bins" in _lib.last_error()
    fin = lambda **k: L.clipmi_val_score_finish(k.get("rr", p), k.get("N", 2), k.get("bins", 10), k.get("rec", p), k.get("ws", p), k.get("wsb", ws), None)
    assert fin(rr=None) == _lib.ERR_ARG and fin(rec=None) == _lib.ERR_ARG and fin(ws=None) == _lib.ERR_ARG
    assert fin(rr=4104) == _lib.ERR_ARG and fin(rec=q) == _lib.ERR_ARG and fin(ws=4096 + 128) == _lib.ERR_ARG
    assert fin(N=0) == _lib.ERR_SHAPE and fin(bins=0) == _lib.ERR_ARG and fin(bins=65) == _lib.ERR_ARG
    assert fin(wsb=16) == _lib.ERR_WORKSPACE
    with pytest.raises(RuntimeError, match="GPU"):
        ops.val_score_rows(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), 10)
    with pytest.raises(ValueError, match="n_bins"):
        ops.val_score_rows(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), 0)
    with pytest.raises(ValueError, match="n_bins"):
        ops.val_score_finish(torch.zeros(2, 16, dtype=torch.uint8), 65)
    with pytest.raises(ValueError, match="row_results"):
        ops.val_score_finish(torch.zeros(0, 16, dtype=torch.uint8), 10)


@pytest.mark.parametrize("fn,lead", FITS, ids=["vpt", "maple", "promptsrc"])
def test_the_new_keywords_sit_at_the_end_and_are_checked_first(fn, lead):
    names = list(inspect.signature(fn).parameters)
    assert names[-len(NEW_KEYWORDS):] == NEW_KEYWORDS
    sig = inspect.signature(fn).parameters
    assert sig["val"].default is None and sig["val_batch_size"].default == 32 and sig["val_bins"].default == 10
    assert sig["final_model"].default == "last_step" and sig["val_criterion"].default == "accuracy" and sig["return_monitor"].default is False
    lead = (None,) * lead       # the checks of the validation arguments come before anything touches the model
    with pytest.raises(ValueError, match="final_model='best_val' needs val="):
        fn(*lead, final_model="best_val")
    with pytest.raises(ValueError, match="final_model='best' must be one of"):
        fn(*lead, final_model="best")
    with pytest.raises(ValueError, match="val_criterion='f1' must be one of"):
        fn(*lead, val=(None, None), val_criterion="f1")
    for bins in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="n_bins="):
            fn(*lead, val=(None, None), val_bins=bins)
    for val in ((1, 2, 3), "ab"[:1], torch.zeros(2)):
        with pytest.raises(ValueError, match=r"val must be \("):
            fn(*lead, val=val)
    for bs in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="val_batch_size="):
            fn(*lead, val=(None, None), val_batch_size=bs)


def test_check_args_keeps_fit_contexts_messages():
    with pytest.raises(ValueError, match=r"fit_context: final_model='best_val' needs val=\(val_features, val_labels\)"):
        fitmonitor.check_args("fit_context", None, 10, "best_val", "accuracy")
    with pytest.raises(ValueError, match=r"fit_context: val must be \(val_features, val_labels\)"):
        fitmonitor.check_args("fit_context", (1,), 10, "last_step", "accuracy")
    assert fitmonitor.empty_monitor()["best_epoch"] is None
