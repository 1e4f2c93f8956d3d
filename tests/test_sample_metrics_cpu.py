"""Host side of the device sample metrics (clip_calibration_amd/metrics.py: quantile_ranks, percentiles_from_order_stats,
quantile_edges_from_order_stats, gap_from_groups, macro_f1_from_counts) against the functions they restate -- quantile_bin_index and
np.percentile exactly, AdaptiveECE / PIECE / macro_f1 on the reference-generated fixtures -- and the C-ABI surface of
csrc/sample_metrics.hip: symbols, ABI version, argument checks that need no GPU."""
import ctypes

import numpy as np
import pytest

from clip_calibration_amd import _lib, metrics
from conftest import load_golden

SIZES = (1, 2, 3, 10, 11, 37, 1000)
BINS = (1, 5, 10, 15)


def _vectors(n, seed):
    """name -> fp32 [n]: random, heavy ties at 1.0, constant, neighbours in the last mantissa bit, mixed signs."""
    rng = np.random.default_rng(seed)
    ties = rng.random(n).astype(np.float32)
    ties[rng.permutation(n)[: (n + 1) // 2]] = 1.0
    base = np.float32(0.7).view(np.uint32)
    return {"random": rng.random(n).astype(np.float32),
            "ties": ties,
            "equal": np.full(n, 0.37, np.float32),
            "last_bit": (base + rng.integers(0, 2, n).astype(np.uint32)).view(np.float32),
            "signed": (rng.standard_normal(n) * 3).astype(np.float32)}


def _edges(x, n_bins, **kw):
    ranks = metrics.quantile_ranks(x.shape[0], n_bins)
    return metrics.quantile_edges_from_order_stats(np.sort(x)[ranks], x.shape[0], n_bins, **kw)


@pytest.mark.parametrize("n", SIZES)
def test_bin_indices_equal_quantile_bin_index(n):
    for n_bins in BINS:
        ranks = metrics.quantile_ranks(n, n_bins)
        assert ranks.dtype == np.int32 and ranks.shape == (2 * (n_bins + 1),)
        assert ranks.min() >= 0 and ranks.max() < n and ranks[0] == 0 and ranks[-1] == n - 1
        for name, x in _vectors(n, 100 * n + n_bins).items():
            edges = _edges(x, n_bins)
            assert edges.dtype == np.float64
            got = np.searchsorted(edges, x, side="right").astype(np.int64)
            assert np.array_equal(got, metrics.quantile_bin_index(x, n_bins)), (name, n, n_bins)
            if name == "equal":
                assert edges.size == 0


@pytest.mark.parametrize("n", SIZES)
def test_edges_before_deduplication_are_numpys_percentiles(n):
    for n_bins in BINS:
        for name, x in _vectors(n, 200 * n + n_bins).items():
            ranks = metrics.quantile_ranks(n, n_bins)
            got = metrics.percentiles_from_order_stats(np.sort(x)[ranks], n, n_bins)
            want = np.asarray(np.percentile(x, np.linspace(0, 100, n_bins + 1)))
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (name, n, n_bins)
        x64 = np.random.default_rng(n).random(n)   # the fixtures' float64 confidences take the same road
        got = metrics.percentiles_from_order_stats(np.sort(x64)[metrics.quantile_ranks(n, n_bins)], n, n_bins)
        assert got.tobytes() == np.asarray(np.percentile(x64, np.linspace(0, 100, n_bins + 1))).tobytes()


def test_nan_collapses_to_one_bin():
    for n in (2, 11, 1000):
        x = np.random.default_rng(n).random(n).astype(np.float32)
        x[n // 2] = np.nan
        assert metrics.quantile_bin_index(x, 10).max() == 0                 # what the restated function does today
        assert _edges(x, 10).size == 0                                      # a NaN sorts last and the last element is always read
        clean = np.where(np.isnan(x), np.float32(0.5), x)
        assert n == 2 or _edges(clean, 10).size > 0
        assert _edges(clean, 10, nan_count=1).size == 0                     # ... or the kernel's count says so


def _group_sums(group, conf, correct, G):
    return np.stack([np.bincount(group, minlength=G).astype(np.float64), np.bincount(group, weights=conf, minlength=G),
                     np.bincount(group, weights=correct, minlength=G)])


def test_restatements_reproduce_the_reference_fixtures():
    g = load_golden("ece_cases.npz")
    for n in sorted({k.split(":")[0] for k in g}):
        conf, pred, gt, bins, prox = g[f"{n}:conf"], g[f"{n}:pred"], g[f"{n}:gt"], int(g[f"{n}:bins"]), g[f"{n}:prox"]
        tol = 1e-12 if conf.dtype == np.float64 else 2e-7           # tests/test_cabi_cpu.py, test_host_ece_matches_reference_goldens
        correct = (pred == gt).astype(np.float64)
        conf64 = conf.astype(np.float64)
        key_bin = np.searchsorted(_edges(conf, bins), conf, side="right")
        ace = metrics.gap_from_groups(_group_sums(key_bin, conf64, correct, bins))
        assert ace == pytest.approx(float(g[f"{n}:ace"]), abs=tol), n
        assert ace == pytest.approx(metrics.AdaptiveECE(conf, pred, gt, bins), abs=1e-15), n
        conf_edges = np.linspace(0, 1, bins + 1)[1:-1]
        group = np.searchsorted(_edges(prox, 10), prox, side="right") * bins + np.searchsorted(conf_edges, conf, side="right")
        piece = metrics.gap_from_groups(_group_sums(group, conf64, correct, 10 * bins))
        assert piece == pytest.approx(float(g[f"{n}:piece"]), abs=tol), n
        assert piece == pytest.approx(metrics.PIECE(conf, prox, pred, gt, 10, bins), abs=1e-15), n
        C = int(max(pred.max(), gt.max())) + 1
        counts = np.concatenate([np.bincount(gt[pred == gt], minlength=C), np.bincount(pred, minlength=C), np.bincount(gt, minlength=C), [0]])
        f1 = metrics.macro_f1_from_counts(counts.astype(np.int64))
        assert f1 == pytest.approx(float(g[f"{n}:f1"]), abs=1e-12), n
        assert f1 == metrics.macro_f1(pred, gt), n
    with pytest.raises(ValueError):
        metrics.macro_f1_from_counts(np.zeros(9, np.int64))


def test_sample_metric_symbols_exported_and_abi_unchanged():
    assert _lib.ABI_VERSION == 16 and _lib.lib.clipmi_abi_version() == 16
    header = open(_lib.HEADER_PATH).read()
    assert "#define CLIPMI_ABI_VERSION 16" in header
    for name in ("clipmi_order_stats", "clipmi_group_gap_accumulate", "clipmi_class_counts"):
        assert name in _lib.exported_symbols() and hasattr(_lib.lib, name) and f"int {name}(" in header
    assert "clipmi_order_stats_workspace_bytes" in _lib.exported_symbols() and "size_t clipmi_order_stats_workspace_bytes(" in header
    assert hasattr(_lib.lib, "clipmi_order_stats_workspace_bytes")
    assert f"#define CLIPMI_ORDER_STATS_MAX_RANKS {_lib.ORDER_STATS_MAX_RANKS}" in header
    assert f"#define CLIPMI_GROUP_GAP_MAX_GROUPS {_lib.GROUP_GAP_MAX_GROUPS}" in header


def test_sample_metric_arguments_are_checked_on_the_host():
    L = _lib.lib
    p = ctypes.c_void_p(4096)
    need = L.clipmi_order_stats_workspace_bytes
    assert need(0, 1) == 0 and need(10, 0) == 0 and need(10, 65) == 0 and need(10, 64) > need(10, 1) > 0

    def order(ranks=(0, 3), n=8, x=p, out=p, nans=p, ws=p, ws_bytes=None, give_ranks=True, k=None):
        arr = (ctypes.c_int32 * max(1, len(ranks)))(*ranks)
        k = len(ranks) if k is None else k
        ws_bytes = need(n, k) if ws_bytes is None else ws_bytes
        return L.clipmi_order_stats(x, n, arr if give_ranks else None, k, out, nans, ws, ws_bytes, None)
    assert order(n=0) == _lib.ERR_SHAPE and order(k=0) == _lib.ERR_SHAPE
    assert order(ranks=tuple(range(65)), n=100) == _lib.ERR_SHAPE and "k=65" in _lib.last_error()
    assert order(x=None) == _lib.ERR_ARG and order(out=None) == _lib.ERR_ARG and order(nans=None) == _lib.ERR_ARG
    assert order(give_ranks=False) == _lib.ERR_ARG and order(ws=None) == _lib.ERR_ARG
    assert order(ranks=(0, 8)) == _lib.ERR_ARG and "ranks[1]=8" in _lib.last_error()
    assert order(ranks=(-1, 3)) == _lib.ERR_ARG and order(ranks=(3, 2)) == _lib.ERR_ARG and "ascending" in _lib.last_error()
    assert order(ws_bytes=need(8, 2) - 1) == _lib.ERR_WORKSPACE
    assert order(ws=ctypes.c_void_p(4096 + 8)) == _lib.ERR_ARG and "aligned" in _lib.last_error()

    def gap(n=8, conf=p, pred=p, lab=p, key=p, ke=p, nk=3, ce=p, nc=2, groups=p):
        return L.clipmi_group_gap_accumulate(conf, pred, lab, key, ke, nk, ce, nc, groups, n, None)
    assert gap(n=0) == _lib.OK and gap(n=-1) == _lib.ERR_SHAPE and gap(nk=-1) == _lib.ERR_SHAPE and gap(nc=-1) == _lib.ERR_SHAPE
    assert gap(nk=31, nc=32) == _lib.ERR_SHAPE and "groups" in _lib.last_error()   # 32 x 33 > 1024
    assert gap(conf=None) == _lib.ERR_ARG and gap(pred=None) == _lib.ERR_ARG and gap(lab=None) == _lib.ERR_ARG and gap(groups=None) == _lib.ERR_ARG
    assert gap(key=None) == _lib.ERR_ARG and gap(ke=None) == _lib.ERR_ARG and gap(ce=None) == _lib.ERR_ARG

    def counts(n=8, C=4, pred=p, lab=p, out=p):
        return L.clipmi_class_counts(pred, lab, n, C, out, None)
    assert counts(n=0) == _lib.OK and counts(n=-1) == _lib.ERR_SHAPE and counts(C=0) == _lib.ERR_SHAPE
    assert counts(pred=None) == _lib.ERR_ARG and counts(lab=None) == _lib.ERR_ARG and counts(out=None) == _lib.ERR_ARG


def test_evaluator_refuses_a_device_mode_it_cannot_run():
    from clip_calibration_amd.evaluator import DeviceCalibrationEvaluator
    with pytest.raises(ValueError, match="n_classes"):
        DeviceCalibrationEvaluator(10, device="cpu", keep_samples=True, sample_metrics="device")
    with pytest.raises(ValueError, match="keep_samples"):
        DeviceCalibrationEvaluator(10, device="cpu", sample_metrics="device", n_classes=5)
    with pytest.raises(ValueError, match="sample_metrics"):
        DeviceCalibrationEvaluator(10, device="cpu", sample_metrics="gpu")
    ev = DeviceCalibrationEvaluator(10, device="cpu", keep_samples=True, sample_metrics="device", n_classes=5)
    assert ev.sample_metrics == "device" and ev.n_classes == 5
