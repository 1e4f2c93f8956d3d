"""CPU checks of ProCal (clip_calibration_amd/procal.py, csrc/procal.hip): the float64 oracle (tests/procal_ref.py) against an
independent KDE, the fit's bandwidths and refusals, VLCalibration's branch table, and the C-ABI argument checks (no GPU needed)."""
import ctypes
import math

import numpy as np
import pytest

import procal_ref as ref
from clip_calibration_amd import _lib
from clip_calibration_amd.calibrator import VLCalibration
from clip_calibration_amd.procal import DensityRatioCalibration, normal_reference_bandwidth


def _val_dict(n=60, C=5, seed=0):
    rng = np.random.default_rng(seed)
    logits = rng.normal(0, 2, (n, C)).astype(np.float32)
    labels = np.where(rng.random(n) < 0.6, logits.argmax(1), rng.integers(0, C, n))
    return {"val_logits": logits, "val_labels": labels, "val_image_features": rng.normal(size=(n, 8)).astype(np.float32),
            "val_image_knn_dists": rng.uniform(0.3, 1.2, (n, 3)).astype(np.float32)}


def test_oracle_density_matches_sklearn():
    """The oracle's product-Gaussian KDE is sklearn's isotropic KernelDensity(bandwidth=1) on coordinates divided by h, divided
    by h_c h_p: an independent check of the restatement of statsmodels' gpke."""
    neighbors = pytest.importorskip("sklearn.neighbors")
    rng = np.random.default_rng(1)
    data = np.stack([rng.beta(5, 2, 300), rng.uniform(0.2, 0.6, 300)], axis=1)
    q = np.stack([rng.uniform(0, 1, 50), rng.uniform(0.1, 0.7, 50)], axis=1)
    bw = ref.bandwidth(data)
    kd = neighbors.KernelDensity(kernel="gaussian", bandwidth=1.0).fit(data / bw)
    expect = np.exp(kd.score_samples(q / bw)) / np.prod(bw)
    np.testing.assert_allclose(ref.kde_pdf(data, bw, q), expect, rtol=1e-10)


def test_bandwidths_match_the_hand_formula():
    rng = np.random.default_rng(2)
    pts = rng.normal(size=(37, 2)) * [0.1, 0.02] + [0.7, 0.4]
    n = pts.shape[0]
    for d in range(2):
        x = pts[:, d]
        h = 1.06 * math.sqrt(sum((v - x.mean()) ** 2 for v in x) / n) * n ** (-1 / 6)
        assert normal_reference_bandwidth(pts)[d] == pytest.approx(h, rel=1e-12)
        assert ref.bandwidth(pts)[d] == pytest.approx(h, rel=1e-12)
    probs = np.full((n, 3), 0.1)
    probs[:, 0] = pts[:, 0] * 0.5 + 0.45          # max prob: a function of pts[:, 0] kept inside [0, 1]
    preds = np.zeros(n, dtype=np.int64)
    true = np.where(np.arange(n) % 3 == 0, 1, 0)
    cal = DensityRatioCalibration()
    cal.fit(probs, preds, true, pts[:, 1])
    o = ref.ProCalRef(probs, preds, true, pts[:, 1])
    np.testing.assert_allclose(cal.bw_true, o.bw_true, rtol=1e-14)
    np.testing.assert_allclose(cal.bw_false, o.bw_false, rtol=1e-14)
    assert cal.false_true_ratio == pytest.approx(o.ratio, rel=1e-15)
    assert cal.data_false.shape[0] == 13 and cal.data_true.shape[0] == 24


def test_fit_refuses_degenerate_sets():
    rng = np.random.default_rng(3)
    probs = rng.dirichlet(np.ones(4), 20)
    preds = probs.argmax(1)
    prox = rng.uniform(0.2, 0.8, 20)
    cal = DensityRatioCalibration()
    with pytest.raises(ValueError, match="incorrect"):   # every sample correct: F is empty
        cal.fit(probs, preds, preds, prox)
    wrong = preds.copy()
    wrong[:19] = (preds[:19] + 1) % 4
    with pytest.raises(ValueError, match="correct val samples number 1"):
        cal.fit(probs, preds, wrong, prox)
    true = np.where(np.arange(20) % 2 == 0, preds, (preds + 1) % 4)
    with pytest.raises(ValueError, match="proximity"):
        cal.fit(probs, preds, true, np.full(20, 0.5))
    flat = np.full((20, 4), 0.25)
    with pytest.raises(ValueError, match="confidence"):
        cal.fit(flat, preds, true, prox)
    with pytest.raises(RuntimeError, match="fit"):
        DensityRatioCalibration().device_model()


def test_branch_table():
    vd = _val_dict()
    for mode, flag, built in (("scaling_based", True, True), ("scaling_based", False, False), (None, True, False), (None, False, False)):
        cal = VLCalibration(vd, base_calibration_mode=mode, procal_flag=flag)
        cal.fit()
        assert cal.procal_active is built
        assert isinstance(cal.base_calibrator, DensityRatioCalibration) if built else cal.base_calibrator is None
    for flag in (True, False):
        with pytest.raises(NotImplementedError):
            VLCalibration(vd, base_calibration_mode="bin_based", procal_flag=flag)
    # the fit runs on the val softmax WITHOUT DAC (vl_calibrator.py:60-62) and the val proximity
    cal = VLCalibration(vd, base_calibration_mode="scaling_based", procal_flag=True)
    cal.fit()
    p = ref.softmax(vd["val_logits"])
    o = ref.ProCalRef(p, p.argmax(1), vd["val_labels"], np.exp(-vd["val_image_knn_dists"].mean(1)))
    np.testing.assert_allclose(cal.base_calibrator.bw_true, o.bw_true, rtol=1e-12)
    np.testing.assert_allclose(cal.base_calibrator.bw_false, o.bw_false, rtol=1e-12)
    # ProCal on and not fitted: refused, not silently skipped
    with pytest.raises(RuntimeError, match="fit"):
        VLCalibration(vd, base_calibration_mode="scaling_based", procal_flag=True).procal_device()


def _model(n_true=4, n_false=4):
    m = _lib.ProcalModel()
    m.points_true, m.points_false = 4096, 8192
    m.n_true, m.n_false = n_true, n_false
    for k in range(2):
        for d in range(2):
            m.scale[k][d] = 10.0
        m.norm[k] = 1.0
    m.ratio = 0.5
    return m


def test_procal_abi_argument_checks():
    """Every argument is checked before anything touches a GPU (this box has none)."""
    L, p = _lib.lib, ctypes.c_void_p(4096)
    kde = lambda m, n=8: L.clipmi_procal_kde(m, p, p, p, n, None)
    rows = lambda m, n=8, C=4, lg=p, conf=p: L.clipmi_procal_rows(m, lg, None, p, None, conf, p, None, n, C, None)
    assert kde(_model(), 0) == _lib.OK and rows(_model(), 0) == _lib.OK            # empty N
    assert kde(None) == _lib.ERR_ARG and "null model" in _lib.last_error()
    assert rows(None) == _lib.ERR_ARG
    assert L.clipmi_procal_kde(_model(), None, p, p, 8, None) == _lib.ERR_ARG
    assert rows(_model(), lg=None) == _lib.ERR_ARG and rows(_model(), conf=None) == _lib.ERR_ARG
    assert kde(_model(), -1) == _lib.ERR_SHAPE and rows(_model(), C=0) == _lib.ERR_SHAPE
    assert kde(_model(n_true=1)) == _lib.ERR_SHAPE and "n_true=1" in _lib.last_error()
    assert rows(_model(n_false=0)) == _lib.ERR_SHAPE
    m = _model()
    m.points_false = 4104
    assert kde(m) == _lib.ERR_ARG and "aligned" in _lib.last_error()
    m = _model()
    m.points_true = None
    assert kde(m) == _lib.ERR_ARG
    for field, value in (("scale", 0.0), ("scale", math.inf), ("scale", math.nan)):
        m = _model()
        getattr(m, field)[1][0] = value
        assert kde(m) == _lib.ERR_ARG and field in _lib.last_error()
    for norm in (0.0, math.nan):
        m = _model()
        m.norm[0] = norm
        assert rows(m) == _lib.ERR_ARG and "norm" in _lib.last_error()
    for ratio in (-1.0, math.inf):
        m = _model()
        m.ratio = ratio
        assert kde(m) == _lib.ERR_ARG and "ratio" in _lib.last_error()


def test_procal_symbols_exported():
    assert _lib.ABI_VERSION == 16 and _lib.lib.clipmi_abi_version() == 16
    for name in ("clipmi_procal_kde", "clipmi_procal_rows"):
        assert name in _lib.exported_symbols() and hasattr(_lib.lib, name)
    header = open(_lib.HEADER_PATH).read()
    assert "clipmi_procal_model" in header and "#define CLIPMI_ABI_VERSION 16" in header
