"""CPU checks of multi-class isotonic calibration and Bin-Mean-Shift (clip_calibration_amd/isotonic.py, csrc/isotonic.hip): the
sort-based float64 restatement (tests/isotonic_ref.py) and the product's host pooling against sklearn's float64 thresholds recorded in
tests/golden/isotonic_cases.npz (tools/gen_isotonic_golden.py), the fixture's own float32-vs-float64 condition, VLCalibration's branch
table, and the C-ABI argument checks (no GPU needed)."""
import ctypes
import math
import os

import numpy as np
import pytest

import isotonic_ref as ref
from clip_calibration_amd import _lib
from clip_calibration_amd import isotonic as iso
from clip_calibration_amd.calibrator import VLCalibration

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "isotonic_cases.npz")
GOLDEN = np.load(GOLDEN_PATH)
CASES = [str(c) for c in GOLDEN["cases"]]
BINS = 5


def g(case, key):
    return GOLDEN[f"{case}_{key}"]


def _same_table(got, X, Y):
    np.testing.assert_array_equal(got[0], X)
    np.testing.assert_allclose(got[1], Y, rtol=1e-12, atol=0)


def _bin_rows(case):
    no = ref.bin_index(g(case, "bin_edges"), g(case, "val_prox"))
    return [no == b for b in range(BINS)]


def test_fixture_covers_the_cases_the_kernels_care_about():
    assert sorted(CASES) == ["c131", "c2", "c50", "ties"]
    assert g("c2", "val_logits").shape[1] == 2 and g("c131", "val_logits").shape[1] % 64 != 0
    x = g("ties", "x_test")
    top = x == x.max(axis=1, keepdims=True)
    assert (top.sum(axis=1) > 1).mean() > 0.2, "the tied case needs rows whose largest x is shared"
    assert os.path.getsize(GOLDEN_PATH) < 1 << 20


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_sklearn_float64_thresholds(case):
    """The sort-based restatement on the fixture's float32 x: X exactly, y to rtol 1e-12, plain and per proximity bin; its bin edges
    are the reference's."""
    x, y = g(case, "x_val"), g(case, "val_labels")
    _same_table(ref.fit_plain(x, y), g(case, "X64"), g(case, "y64"))
    edges, tables = ref.fit_bins(x, y, g(case, "val_prox"), BINS)
    np.testing.assert_array_equal(edges, g(case, "bin_edges"))
    for b in range(BINS):
        _same_table(tables[b], g(case, f"bms_X64_{b}"), g(case, f"bms_y64_{b}"))


@pytest.mark.parametrize("case", CASES)
def test_host_pooling_of_gap_statistics_reproduces_sklearn_float64_thresholds(case):
    """The product's pooling (isotonic.pool_gap_statistics), fed the gap statistics the device kernel accumulates but computed in numpy:
    the N positive keys and per-gap counts / extrema of the zeros determine the whole fit."""
    x, y = g(case, "x_val"), g(case, "val_labels")
    stats = ref.gap_statistics(x, y)
    assert stats[0].size <= x.shape[0] and stats[3].size == stats[0].size + 1
    assert stats[1].sum() == x.shape[0] and stats[2].sum() + stats[3].sum() == x.shape[0] * (x.shape[1] - 1)
    _same_table(iso.pool_gap_statistics(*stats), g(case, "X64"), g(case, "y64"))
    for b, rows in enumerate(_bin_rows(case)):
        _same_table(iso.pool_gap_statistics(*ref.gap_statistics(x[rows], y[rows])), g(case, f"bms_X64_{b}"), g(case, f"bms_y64_{b}"))


def test_split_gap_statistics_reads_the_device_layout():
    """The slot layout of include/clipmi.h, written here by hand for two bins, comes back as the arrays the pooling takes."""
    x = g("c50", "x_val")
    y = g("c50", "val_labels")
    rows = _bin_rows("c50")[:2]
    parts = [ref.gap_statistics(x[r], y[r]) for r in rows]
    off = [0, parts[0][0].size, parts[0][0].size + parts[1][0].size]
    total = 3 * off[-1] + 2
    stats = np.zeros((3, total), np.int32)
    for b, (keys, pos, zeq, gc, gmin, gmax) in enumerate(parts):
        m, base = keys.size, 3 * off[b] + b
        stats[0, base:base + m + 1] = gc
        stats[0, base + m + 1:base + 2 * m + 1] = zeq
        stats[0, base + 2 * m + 1:base + 3 * m + 1] = pos
        stats[1, base:base + m + 1] = gmin.view(np.int32)
        stats[2, base:base + m + 1] = gmax.view(np.int32)
    for b, (keys, *_) in enumerate(parts):
        _same_table(iso.pool_gap_statistics(keys, *iso.split_gap_statistics(stats, off, b)), g("c50", f"bms_X64_{b}"), g("c50", f"bms_y64_{b}"))


@pytest.mark.parametrize("case", CASES)
def test_fixture_float32_reference_and_float64_fit_agree_on_top1(case):
    """The condition the generator holds every case to, checked on what it wrote: the as-run float32 reference and the float64 fit pick
    the same class in every row (val, test, test with DAC; plain and Bin-Mean-Shift); and the recorded distance between the two is
    the one recomputed here."""
    tables = [(g(case, f"bms_X64_{b}"), g(case, f"bms_y64_{b}")) for b in range(BINS)]
    diffs = {"plain": [], "bms": []}
    for s in ("val", "test", "test_dac"):
        x = g(case, "x_" + s)
        prox = g(case, "val_prox" if s == "val" else "test_prox")
        for name, r64 in (("plain", ref.calibrate(g(case, "X64"), g(case, "y64"), x)),
                          ("bms", ref.calibrate_bins(g(case, "bin_edges"), tables, x, prox))):
            r32 = g(case, f"ref32_{name}_{s}")
            assert r32.dtype == np.float32 and r32.shape == x.shape
            np.testing.assert_array_equal(r32.argmax(axis=1), r64.argmax(axis=1))
            if s != "val":
                diffs[name].append(np.abs(r32.astype(np.float64) - r64).ravel())
    for i, name in enumerate(("plain", "bms")):
        d = np.concatenate(diffs[name])
        assert g(case, "ref32_vs_ref64_mean")[i] == pytest.approx(d.mean(), rel=1e-9)
        assert g(case, "ref32_vs_ref64_max")[i] == pytest.approx(d.max(), rel=1e-9)
        assert 0 < d.mean() < 0.01   # the float32 fit IS noisy, and only at isolated points


def test_pooling_edge_cases():
    # every positive key equal, zeros on both sides: one block in the middle can only pool with what violates monotonicity
    X, Y = iso.pool_gap_statistics([0.5], [4], [0], [3, 0], np.float32([0.1, np.inf]), np.float32([0.3, 0]))
    np.testing.assert_array_equal(X, np.float64(np.float32([0.1, 0.3, 0.5])))
    np.testing.assert_array_equal(Y, [0, 0, 1])
    _same_table(ref.fit_thresholds(np.float32([0.1, 0.2, 0.3, 0.5, 0.5, 0.5, 0.5]), [0, 0, 0, 1, 1, 1, 1]), X, Y)
    # zeros above the only key pool with it: one block from the key to the largest zero, then nothing
    X, Y = iso.pool_gap_statistics([0.5], [2], [1], [0, 2], np.float32([np.inf, 0.6]), np.float32([0, 0.7]))
    np.testing.assert_array_equal(X, np.float64(np.float32([0.5, 0.7])))
    np.testing.assert_allclose(Y, [0.4, 0.4], rtol=1e-15)
    # a single x altogether: one threshold
    X, Y = iso.pool_gap_statistics([0.5], [1], [1], [0, 0], np.float32([np.inf, np.inf]), np.float32([0, 0]))
    assert X.tolist() == [0.5] and Y.tolist() == [0.5]
    assert ref.calibrate(X, Y, np.float32([0.1, 0.9])).tolist() == pytest.approx([0.5, 0.5])


def _val_dict(n=60, C=5, seed=0):
    rng = np.random.default_rng(seed)
    logits = rng.normal(0, 2, (n, C)).astype(np.float32)
    labels = np.where(rng.random(n) < 0.6, logits.argmax(1), rng.integers(0, C, n))
    return {"val_logits": logits, "val_labels": labels, "val_image_features": rng.normal(size=(n, 8)).astype(np.float32),
            "val_image_knn_dists": rng.uniform(0.3, 1.2, (n, 3)).astype(np.float32)}


def test_branch_table():
    vd = _val_dict()
    for name in (None, "histogram_binning", "isotonic_regression", "platt"):   # the four refused spellings, at construction
        for flag in (True, False):
            with pytest.raises(NotImplementedError) as e:
                VLCalibration(vd, base_calibration_mode="bin_based", procal_flag=flag, base_bin_calibrator_name=name)
            assert ("netcal" in str(e.value)) == (name in ("histogram_binning", "isotonic_regression"))
    with pytest.raises(NotImplementedError):
        VLCalibration(vd, base_calibration_mode="tree_based", base_bin_calibrator_name="multi_isotonic_regression")
    for flag in (True, False):
        cal = VLCalibration(vd, base_calibration_mode="bin_based", procal_flag=flag, base_bin_calibrator_name="multi_isotonic_regression")
        assert cal.bin_based_active and not cal.procal_active and cal.procal_device() is None
        with pytest.raises(RuntimeError, match="fit"):    # on and not fitted: refused, not silently skipped
            cal.row_calibrator_device()
    # the name is ignored outside bin_based, and every earlier call keeps its behaviour
    cal = VLCalibration(vd, base_calibration_mode="scaling_based", procal_flag=False, base_bin_calibrator_name="multi_isotonic_regression")
    cal.fit()
    assert cal.base_calibrator is None and cal.row_calibrator_device() == (None, False) and not cal.bin_based_active
    assert VLCalibration(vd).row_calibrator_device() == (None, False)


def test_calibrator_classes_refuse_before_any_gpu_call():
    with pytest.raises(ValueError):
        iso.BinMeanShift(0)
    with pytest.raises(ValueError):
        iso.BinMeanShift(_lib.ISOTONIC_MAX_TABLES + 1)
    with pytest.raises(RuntimeError, match="fit"):
        iso.MultiIsotonicRegression().device_model()
    with pytest.raises(ValueError, match="labels outside"):
        iso._labels_1d([0, 5], 5)
    assert iso._labels_1d(np.eye(3)[[2, 0]], 3).tolist() == [2, 0]
    b = iso.BinMeanShift(2)
    b.set_thresholds([0.1, 0.2, 0.3], [([0.1, 0.2], [0.0, 1.0]), ([0.3], [0.5])])
    assert b.bin_index([0.05, 0.2, 0.25, 0.9]).tolist() == [0, 1, 1, 1]
    assert b.calibrators[1].y_thresholds_.tolist() == [0.5] and b.calibrators[0].X_thresholds_.dtype == np.float64
    with pytest.raises(_lib.ClipmiError, match="ascending"):
        iso.pack_tables([([0.2, 0.2], [0.0, 1.0])])
    packed = iso.pack_tables([([0.1, 0.2, 0.4], [0.0, 0.5, 1.0]), ([0.3], [0.5])])
    np.testing.assert_allclose(packed, [0.1, 0.2, 0.4, 0.0, 0.5, 1.0, 5.0, 2.5, 0.0, 0.3, 0.5, 0.0], rtol=1e-15)


def _model(n_tables=1, counts=(4,)):
    m = _lib.IsotonicModel()
    m.table, m.n_tables = 4096, n_tables
    off = 0
    for i, c in enumerate(counts):
        off += c
        m.offset[i + 1] = off
    for e in range(min(n_tables, _lib.ISOTONIC_MAX_TABLES) - 1):
        m.edges[e] = 0.1 * (e + 1)
    return m


def test_isotonic_abi_argument_checks():
    """Every argument is checked before anything touches a GPU (this box has none)."""
    L, p = _lib.lib, ctypes.c_void_p(4096)
    rows = lambda m, n=8, C=4, lg=p, dac=None, prox=None, fp=0, conf=p, pred=p: L.clipmi_isotonic_rows(m, lg, dac, prox, fp, None, None, conf,
                                                                                                       pred, n, C, None)
    assert rows(_model(), 0) == _lib.OK                                                   # empty N
    assert rows(None) == _lib.ERR_ARG and "null model" in _lib.last_error()
    assert rows(_model(), lg=None) == _lib.ERR_ARG and rows(_model(), conf=None) == _lib.ERR_ARG and rows(_model(), pred=None) == _lib.ERR_ARG
    assert rows(_model(), -1) == _lib.ERR_SHAPE and rows(_model(), C=0) == _lib.ERR_SHAPE
    assert rows(_model(), dac=p, fp=1) == _lib.ERR_ARG and "DAC" in _lib.last_error()
    m = _model()
    m.table = None
    assert rows(m) == _lib.ERR_ARG
    m = _model()
    m.table = 4100
    assert rows(m) == _lib.ERR_ARG and "aligned" in _lib.last_error()
    assert rows(_model(0, ())) == _lib.ERR_SHAPE and rows(_model(_lib.ISOTONIC_MAX_TABLES + 1, ())) == _lib.ERR_SHAPE
    assert rows(_model(2, (3, 0)), prox=p) == _lib.ERR_SHAPE and "table 1 has 0" in _lib.last_error()
    m = _model()
    m.offset[0] = 1
    assert rows(m) == _lib.ERR_SHAPE
    assert rows(_model(3, (2, 2, 2))) == _lib.ERR_ARG and "proximity" in _lib.last_error()   # several tables, no proximity
    for bad in (math.nan, math.inf):
        m = _model(3, (2, 2, 2))
        m.edges[1] = bad
        assert rows(m, prox=p) == _lib.ERR_ARG and "edges[1]" in _lib.last_error()
    m = _model(3, (2, 2, 2))
    m.edges[1] = 0.05
    assert rows(m, prox=p) == _lib.ERR_ARG and "ascending" in _lib.last_error()

    keys = lambda n=8, C=4, lg=p, lab=p, k=p: L.clipmi_isotonic_keys(lg, lab, k, n, C, 0, None)
    assert keys(0) == _lib.OK and keys(-1) == _lib.ERR_SHAPE and keys(C=0) == _lib.ERR_SHAPE
    assert keys(lg=None) == _lib.ERR_ARG and keys(lab=None) == _lib.ERR_ARG and keys(k=None) == _lib.ERR_ARG

    def stats(off=(0, 3), n=8, C=4, lg=p, lab=p, b=None, k=p, st=p, status=p, give_off=True):
        arr = (ctypes.c_int32 * len(off))(*off)
        return L.clipmi_isotonic_gap_stats(lg, lab, b, k, arr if give_off else None, len(off) - 1, st, status, n, C, 0, None)
    assert stats(give_off=False) == _lib.ERR_ARG and stats(k=None) == _lib.ERR_ARG and stats(st=None) == _lib.ERR_ARG
    assert stats(status=None) == _lib.ERR_ARG and stats(lg=None) == _lib.ERR_ARG and stats(lab=None) == _lib.ERR_ARG
    assert stats(n=-1) == _lib.ERR_SHAPE and stats(C=0) == _lib.ERR_SHAPE
    assert stats(off=(0,)) == _lib.ERR_SHAPE and stats(off=tuple(range(_lib.ISOTONIC_MAX_TABLES + 2)), b=p) == _lib.ERR_SHAPE
    assert stats(off=(1, 3)) == _lib.ERR_SHAPE
    assert stats(off=(0, 3, 3), b=p) == _lib.ERR_SHAPE and "bin 1 has 0 keys" in _lib.last_error()   # an empty val bin
    assert stats(off=(0, 3, 5)) == _lib.ERR_ARG and "bin index" in _lib.last_error()
    assert stats(off=(0, 9)) == _lib.ERR_SHAPE and "9 keys for 8 rows" in _lib.last_error()
    assert stats(n=1 << 20, C=1 << 12, off=(0, 3)) == _lib.ERR_SHAPE and "int32" in _lib.last_error()

    def pack(x, y, counts, out=True, n_tables=None):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        c = (ctypes.c_int32 * len(counts))(*counts)
        buf = np.zeros(3 * max(1, x.size))
        return L.clipmi_isotonic_pack(x.ctypes.data, y.ctypes.data, c, len(counts) if n_tables is None else n_tables,
                                      buf.ctypes.data if out else None)
    assert pack([0.1, 0.2], [0, 1], [2]) == _lib.OK
    assert pack([0.1, 0.2], [0, 1], [2], out=False) == _lib.ERR_ARG
    assert pack([0.1, 0.2], [0, 1], [2], n_tables=0) == _lib.ERR_SHAPE and pack([0.1, 0.2], [0, 1], [2, 0]) == _lib.ERR_SHAPE
    for x, y in (([0.1, math.nan], [0, 1]), ([0.1, 0.2], [0, math.inf]), ([-math.inf, 0.2], [0, 1])):   # non-finite table entries
        assert pack(x, y, [2]) == _lib.ERR_ARG and "finite" in _lib.last_error()
    assert pack([0.2, 0.1], [0, 1], [2]) == _lib.ERR_ARG and "ascending" in _lib.last_error()
    assert pack([0.1, 0.2], [0, 1], [1, 1]) == _lib.OK        # ascending is per table


def test_isotonic_symbols_exported_and_abi_unchanged():
    assert _lib.ABI_VERSION == 16 and _lib.lib.clipmi_abi_version() == 16
    header = open(_lib.HEADER_PATH).read()
    for name in ("clipmi_isotonic_pack", "clipmi_isotonic_rows", "clipmi_isotonic_keys", "clipmi_isotonic_gap_stats"):
        assert name in _lib.exported_symbols() and hasattr(_lib.lib, name) and f"int {name}(" in header
    assert "clipmi_isotonic_model" in header and "#define CLIPMI_ABI_VERSION 16" in header
    assert f"#define CLIPMI_ISOTONIC_MAX_TABLES {_lib.ISOTONIC_MAX_TABLES}" in header
    assert ctypes.sizeof(_lib.IsotonicModel) == 8 + 4 + 4 * (_lib.ISOTONIC_MAX_TABLES + 1) + 8 * (_lib.ISOTONIC_MAX_TABLES - 1)


def test_isotonic_translation_unit_has_no_matrix_core_code():
    """tests/test_cabi_cpu.py scans every translation unit that names a matrix-core instruction and fails when that set changes; this
    file must stay outside it, and the scanner itself, pointed at it, must compile it and report that there is nothing to walk."""
    import importlib.util
    import shutil
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "clip_calibration_amd", "csrc", "isotonic.hip")
    assert "mfma" not in open(src).read().lower()
    if shutil.which(os.environ.get("HIPCC", "hipcc")) is None:
        pytest.skip("no hipcc on this box: the ISA cannot be produced")
    spec = importlib.util.spec_from_file_location("mfma_hazard_scan", os.path.join(root, "tools", "mfma_hazard_scan.py"))
    hs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hs)
    with pytest.raises(hs.ScanError, match="no kernel with a v_mfma"):
        hs.scan("isotonic.hip")
