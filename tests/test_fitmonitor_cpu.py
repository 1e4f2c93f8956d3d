"""CPU checks of the fit monitor: the float64 restatement (tests/fitmonitor_ref.py) against torch, numpy and
clip_calibration_amd.metrics; the selection rule on hand-written sequences; the new C entry points in the header, the binding and the
build; the host-side refusals; and the arguments of coopfit.fit_context that need no GPU."""
import ctypes
import re

import numpy as np
import pytest
import torch

import coopfit_ref
import fitmonitor_ref as ref
from clip_calibration_amd import _lib, coopfit, fitloop, metrics, ops
from clip_calibration_amd.model import build_model

NEW_SYMBOLS = ("clipmi_val_score", "clipmi_val_score_workspace_bytes", "clipmi_best_select", "clipmi_best_select_workspace_bytes")


@pytest.mark.parametrize("N,C", [(1, 1), (67, 2), (65, 63), (40, 1000)])
@pytest.mark.parametrize("scale", [1.0, 100.0])
def test_restatement_against_torch_numpy_and_metrics(N, C, scale):
    rng = np.random.default_rng(N * 1000 + C)
    z = (scale * rng.standard_normal((N, C))).astype(np.float32)
    if C > 2:
        z[0, 1] = z[0, 2] = z[0].max() + 1.0             # a tie at the maximum: the lower index wins
        z[N - 1, :] = 0.25                                # a row of equal values
        z[N // 2, 0] = -np.inf
    y = rng.integers(0, C, N)
    hit, nll, conf = ref.score_rows(z, y)
    zt = torch.from_numpy(z).double()
    want = torch.nn.functional.cross_entropy(zt, torch.from_numpy(y), reduction="sum").item()
    assert nll.sum() == pytest.approx(want, rel=1e-12, abs=1e-12)
    pred = np.argmax(z.astype(np.float64), axis=1)
    assert np.array_equal(hit, pred == y)
    if C > 2:
        assert pred[0] == 1 and pred[N - 1] == 0
    np.testing.assert_allclose(conf, torch.softmax(zt, dim=1).max(dim=1).values.numpy(), rtol=1e-12)
    for n_bins in (1, 10, 15, 64):
        rec = ref.record(z, y, n_bins)
        want_bins = metrics.bin_statistics(conf, pred, y, n_bins)
        np.testing.assert_array_equal(ref.record_bins(rec)[0], want_bins[0])
        np.testing.assert_array_equal(ref.record_bins(rec)[2], want_bins[2])
        np.testing.assert_allclose(ref.record_bins(rec)[1], want_bins[1], rtol=1e-13, atol=0)
        assert rec["n"] == N and rec["count"].sum() == N and rec["correct"] == rec["hits"].sum() == int((pred == y).sum())
        assert ref.ece(rec) == pytest.approx(metrics.ECE(conf, pred, y, n_bins), abs=1e-13)


def test_restatement_defined_outcomes():
    """conf == 1.0 lands in the last bin; a label outside [0, C) and a row with a NaN count as wrong with a NaN nll."""
    z = np.array([[200.0, 0.0, 0.0], [0.0, 1.0, 0.5], [np.nan, 5.0, 0.0], [1.0, 2.0, 3.0]], np.float32)
    y = np.array([0, 1, 1, 7])
    hit, nll, conf = ref.score_rows(z, y)
    assert conf[0] == 1.0 and metrics.digitize_bins(conf[:1], 10)[0] == 10
    assert hit.tolist() == [True, True, False, False]
    assert np.isfinite(nll[:2]).all() and np.isnan(nll[2]) and np.isnan(nll[3]) and np.isnan(conf[2]) and np.isfinite(conf[3])
    rec = ref.record(z, y, 10)
    assert rec["correct"] == 2 and np.isnan(rec["nll_sum"]) and rec["count"][10] == 2 and rec["count"].sum() == 4
    assert np.isfinite(ref.ece(rec))                     # the last bin enters the ECE with its count alone


def test_clean_logits_keep_every_row_and_saturate():
    z, y = ref.clean_logits(67, 63, 10, seed=3)
    conf = ref.score_rows(z, y)[2]
    assert z.shape == (67, 63) and ref.off_the_edges(conf, 10) and (conf == 1.0).any() and (conf < 1.0).any()
    edge = np.linspace(0, 1, 11)[3]
    assert not ref.off_the_edges(np.array([edge * (1 + 2.0 ** -22)]), 10) and ref.off_the_edges(np.array([edge, 1.0, 0.35]), 10)


@pytest.mark.parametrize("name,seq,want_acc,want_nll", ref.SEQUENCES, ids=[s[0] for s in ref.SEQUENCES])
def test_selection_rule_on_hand_written_sequences(name, seq, want_acc, want_nll):
    recs = [{"correct": c, "nll_sum": v} for c, v in seq]
    assert ref.best_epoch(recs, "accuracy") == want_acc
    assert ref.best_epoch(recs, "nll") == want_nll
    for crit in ("accuracy", "nll"):
        steps = ref.select(recs, crit)
        assert [s[3] for s in steps].count(True) >= (0 if ref.best_epoch(recs, crit) < 0 else 1)
        for (e0, *_), (e1, _, _, better) in zip(steps, steps[1:]):
            assert (e1 != e0) == better and e1 >= e0


def test_new_entry_points_in_header_binding_and_build():
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols() and hasattr(_lib.lib, name)
    assert _lib.ABI_VERSION == 16 == _lib.lib.clipmi_abi_version()
    make = open(_lib.HEADER_PATH.replace("include/clipmi.h", "clip_calibration_amd/csrc/Makefile")).read()
    assert "fit_monitor.hip" in make


def test_record_and_best_block_layout():
    for n_bins in (1, 10, 64):
        assert ops.val_record_bytes(n_bins) == 16 + 16 * (n_bins + 1)
        assert _lib.lib.clipmi_val_score_workspace_bytes(65, n_bins) == (2 * ops.val_record_bytes(n_bins) + 255) // 256 * 256
    raw = np.zeros(ops.val_record_bytes(2), np.uint8)
    raw[0:4] = np.array([7], "<i4").view(np.uint8)
    raw[4:8] = np.array([5], "<i4").view(np.uint8)
    raw[8:16] = np.array([1.5], "<f8").view(np.uint8)
    raw[16 + 16 * 2:16 + 16 * 2 + 4] = np.array([3], "<i4").view(np.uint8)          # bin 2, the last: count
    raw[16 + 16 * 2 + 8:16 + 16 * 3] = np.array([3.0], "<f8").view(np.uint8)
    (rec,) = ops.decode_val_records(raw, 2)
    assert (rec["n"], rec["correct"], rec["nll_sum"]) == (7, 5, 1.5) and rec["count"].tolist() == [0, 0, 3] and rec["conf_sum"][2] == 3.0
    assert ops.val_record_bins(rec).shape == (3, 3)
    blk = ops.decode_best_block(ops.new_best_block("cpu"))
    assert blk == {"best_epoch": -1, "best_correct": -1, "best_nll_sum": float("inf"), "epochs_seen": 0}
    assert ops.new_best_block("cpu").numel() == 24
    assert _lib.lib.clipmi_val_score_workspace_bytes(0, 10) == 0 and _lib.lib.clipmi_val_score_workspace_bytes(5, 65) == 0
    assert _lib.lib.clipmi_best_select_workspace_bytes(0) == 0 and _lib.lib.clipmi_best_select_workspace_bytes(1) >= 4


def test_argument_refusals_need_no_gpu():
    L = _lib.lib
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)
    ws = 1 << 20
    assert L.clipmi_val_score(None, 4, p, 2, 4, 10, p, p, ws, None) == _lib.ERR_ARG
    assert L.clipmi_val_score(p, 4, p, 2, 4, 10, None, p, ws, None) == _lib.ERR_ARG
    assert L.clipmi_val_score(q, 4, p, 2, 4, 10, p, p, ws, None) == _lib.ERR_ARG and "16-byte" in _lib.last_error()
    assert L.clipmi_val_score(p, 4, p, 0, 4, 10, p, p, ws, None) == _lib.ERR_SHAPE
    assert L.clipmi_val_score(p, 4, p, 2, 0, 10, p, p, ws, None) == _lib.ERR_SHAPE
    assert L.clipmi_val_score(p, 3, p, 2, 4, 10, p, p, ws, None) == _lib.ERR_SHAPE          # ld < C
    assert L.clipmi_val_score(p, 4, p, 2, 4, 0, p, p, ws, None) == _lib.ERR_ARG and "n_bins" in _lib.last_error()
    assert L.clipmi_val_score(p, 4, p, 2, 4, 65, p, p, ws, None) == _lib.ERR_ARG
    assert L.clipmi_val_score(p, 4, p, 2, 4, 10, p, p, 16, None) == _lib.ERR_WORKSPACE
    assert L.clipmi_best_select(None, p, 0, 0, p, p, 4, p, 256, None) == _lib.ERR_ARG
    assert L.clipmi_best_select(p, p, 0, 0, p, None, 4, p, 256, None) == _lib.ERR_ARG
    assert L.clipmi_best_select(p, p, 0, 0, q, p, 4, p, 256, None) == _lib.ERR_ARG and "16-byte" in _lib.last_error()
    assert L.clipmi_best_select(p, p, 2, 0, p, p, 4, p, 256, None) == _lib.ERR_ARG and "criterion" in _lib.last_error()
    assert L.clipmi_best_select(p, p, 0, -1, p, p, 4, p, 256, None) == _lib.ERR_ARG
    assert L.clipmi_best_select(p, p, 0, 0, p, p, 0, p, 256, None) == _lib.ERR_SHAPE
    assert L.clipmi_best_select(p, p, 0, 0, p, p, 4, p, 2, None) == _lib.ERR_WORKSPACE
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.val_score(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), 10)
    with pytest.raises(ValueError, match="n_bins"):
        ops.val_score(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), 0)
    with pytest.raises(ValueError, match="criterion"):
        ops.best_select(None, None, "f1", 0, None, None)


def test_run_cached_calls_end_epoch_behind_each_epoch():
    seen = []
    f, y = torch.zeros(5, 4), torch.zeros(5, dtype=torch.int64)
    fitloop.run_cached(lambda a, b, r, want: seen.append(("step", a.shape[0])), f, y, None, 2, 3, 2, torch.zeros(6), False,
                       lambda e: seen.append(("end", e)))
    assert seen == [("step", 2), ("step", 2), ("step", 1), ("end", 0), ("step", 2), ("step", 2), ("step", 1), ("end", 1)]


def _case():
    c = coopfit_ref.make_case("tiny", 3, 4, 8)
    return c, build_model(dict(c["sd"]), {"trainer": "CoOp"})


def test_best_val_without_val_and_other_refusals():
    c, m = _case()
    args = (c["feats"], c["labels"], m, c["ids"], c["ctx"])
    with pytest.raises(ValueError, match="best_val"):
        coopfit.fit_context(*args, epochs=2, batch_size=4, final_model="best_val")
    with pytest.raises(ValueError, match="final_model"):
        coopfit.fit_context(*args, epochs=2, batch_size=4, final_model="best")
    with pytest.raises(ValueError, match="val_criterion"):
        coopfit.fit_context(*args, epochs=2, batch_size=4, val=(c["feats"], c["labels"]), val_criterion="f1")
    with pytest.raises(ValueError, match="n_bins"):
        coopfit.fit_context(*args, epochs=2, batch_size=4, val=(c["feats"], c["labels"]), val_bins=65)
    with pytest.raises(ValueError, match="labels span"):
        coopfit.fit_context(*args, epochs=2, batch_size=4, val=(c["feats"], c["labels"] + 3))


def test_no_epochs_returns_the_context_and_an_empty_monitor():
    c, m = _case()
    ctx, hist, mon = coopfit.fit_context(c["feats"], c["labels"], m, c["ids"], c["ctx"], epochs=0, batch_size=4, return_history=True,
                                         val=(c["feats"], c["labels"]), final_model="best_val", return_monitor=True)
    assert torch.equal(ctx, c["ctx"]) and hist.size == 0
    assert mon["accuracy"].size == mon["nll"].size == mon["ece"].size == 0 and mon["bins"].shape == (0, 3, 11) and mon["best_epoch"] is None
    ctx, mon = coopfit.fit_context(c["feats"], c["labels"], m, c["ids"], c["ctx"], epochs=0, batch_size=4, return_monitor=True)
    assert torch.equal(ctx, c["ctx"]) and mon["records"] == []
