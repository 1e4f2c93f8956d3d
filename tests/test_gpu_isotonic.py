"""Multi-class isotonic calibration and Bin-Mean-Shift on the GPU (csrc/isotonic.hip, clip_calibration_amd/isotonic.py) against the
numpy restatement (tests/isotonic_ref.py) and the fixtures of tests/golden/isotonic_cases.npz (the reference's own classes as run in
float32, and sklearn's float64 thresholds).  Measured figures of a run of this file: profiles/isotonic_parity.txt."""
import os

import numpy as np
import pytest
import torch

import isotonic_ref as ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import _lib, ops  # noqa: E402
from clip_calibration_amd import isotonic as iso  # noqa: E402
from clip_calibration_amd.proximity import knn_dists_device  # noqa: E402

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "isotonic_cases.npz"))
CASES = [str(c) for c in GOLDEN["cases"]]
BINS = 5


def g(case, key):
    return GOLDEN[f"{case}_{key}"]


def cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def device_x(logits, dac=None, from_probs=False):
    """The x values the kernels form (every kernel shares one device function): read back through the predict launch's optional output."""
    cal = iso.MultiIsotonicRegression()
    cal.set_thresholds([0.5], [0.5])
    lg = cuda(logits)
    return ops.isotonic_rows(cal.device_model(lg.device), lg, None, None if dac is None else cuda(dac), want_x=True,
                             from_probs=from_probs)[3].cpu().numpy()


def fixture_tables(case):
    return [(g(case, f"bms_X64_{b}"), g(case, f"bms_y64_{b}")) for b in range(BINS)]


def same_table(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_allclose(got[1], want[1], rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", CASES)
def test_device_x_is_the_reference_x_to_rounding(case):
    """softmax, then the second softmax, in fp32, against numpy's float32 values.  The first softmax is clipmi_softmax_rows' own:
    __expf(y - M) forms (y - M) * log2(e) in fp32 before v_exp_f32, a relative error of about |y - M| * 2^-24 in p; x = exp(p) / sum
    turns an absolute error of p (p <= 1) into a relative error of x, so x may be off by the row's logit range in ulp, plus a few for
    the two sums, the division and the exp.  The from_probs form skips the first softmax and keeps the few."""
    for key, dac in (("x_val", None), ("x_test", None), ("x_test_dac", g(case, "dac"))):
        lg = g(case, "val_logits" if key == "x_val" else "test_logits")
        x, want = device_x(lg, dac), g(case, key)
        y = lg if dac is None else lg * dac[lg.argmax(axis=1)][:, None]
        bound = 4 + float(np.ptp(y, axis=1).max())
        ulps = np.abs(x.astype(np.float64) - want) / np.spacing(want)
        print(f"{case} {key}: device x vs numpy x: max {ulps.max():.1f} ulp, {np.mean(x == want):.3f} of the values equal "
              f"(bound {bound:.0f})")
        assert ulps.max() <= bound
        xp = device_x(ref.softmax32(lg, dac), from_probs=True)
        assert (np.abs(xp.astype(np.float64) - want) / np.spacing(want)).max() <= bound


@pytest.mark.parametrize("case", CASES)
def test_fit_equals_the_restatement_on_the_device_x(case):
    """Device gap statistics -> host pooling, against the sort-based restatement fed the device's own x: X exactly, y to rtol 1e-12,
    plain and per proximity bin.  Against the fixture's float64 thresholds (numpy's x) only the fitted FUNCTIONS are compared, on the
    fixture's test points: their mean absolute difference stays inside the reference's own float32-vs-float64 distance."""
    lg, labels, prox = cuda(g(case, "val_logits")), g(case, "val_labels"), g(case, "val_prox")
    x = device_x(g(case, "val_logits"))
    plain = iso.MultiIsotonicRegression()
    plain.fit_device(lg, labels)
    same_table((plain.X_thresholds_, plain.y_thresholds_), ref.fit_plain(x, labels))
    bms = iso.BinMeanShift(BINS)
    bms.fit_device(lg, labels, prox)
    edges, tables = ref.fit_bins(x, labels, prox, BINS)
    np.testing.assert_array_equal(bms.bin_edges, edges)
    np.testing.assert_array_equal(bms.bin_edges, g(case, "bin_edges"))
    for b in range(BINS):
        same_table((bms.calibrators[b].X_thresholds_, bms.calibrators[b].y_thresholds_), tables[b])
    xt = np.concatenate([g(case, "x_test"), g(case, "x_test_dac")])
    pt = np.concatenate([g(case, "test_prox"), g(case, "test_prox")])
    d_plain = np.abs(ref.calibrate(plain.X_thresholds_, plain.y_thresholds_, xt).astype(np.float64)
                     - ref.calibrate(g(case, "X64"), g(case, "y64"), xt)).mean()
    d_bms = np.abs(ref.calibrate_bins(edges, bms._tables, xt, pt).astype(np.float64)
                   - ref.calibrate_bins(edges, fixture_tables(case), xt, pt)).mean()
    yard = g(case, "ref32_vs_ref64_mean")
    print(f"{case}: device fit vs float64 fixture fit, mean |d| on the test points: plain {d_plain:.3e} (yardstick {yard[0]:.3e}), "
          f"bin-mean-shift {d_bms:.3e} (yardstick {yard[1]:.3e})")
    assert d_plain <= yard[0] and d_bms <= yard[1]


@pytest.mark.parametrize("with_dac", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_predict_with_a_given_table(case, with_dac):
    """The fixture's float64 tables installed as they are: calibrated rows against float64 np.interp on the device's x at the fp32
    interpolation bound of the table, and (conf, pred) equal to the restatement's top-1 (lowest index among equal maxima) on every row."""
    lg, prox = g(case, "test_logits"), g(case, "test_prox")
    dac = g(case, "dac") if with_dac else None
    x = device_x(lg, dac)
    plain = iso.MultiIsotonicRegression()
    plain.set_thresholds(g(case, "X64"), g(case, "y64"))
    bms = iso.BinMeanShift(BINS)
    bms.set_thresholds(g(case, "bin_edges"), fixture_tables(case))
    dac_d = None if dac is None else cuda(dac)
    for name, cal, want, tol in (
            ("plain", plain, ref.calibrate(g(case, "X64"), g(case, "y64"), x), ref.interp_tolerance(g(case, "X64"), g(case, "y64"), x)),
            ("bms", bms, ref.calibrate_bins(g(case, "bin_edges"), fixture_tables(case), x, prox),
             max(ref.interp_tolerance(X, Y, x) for X, Y in fixture_tables(case)))):
        probs, conf, pred = cal.predict_device(cuda(lg), cuda(prox), dac_d, want_probs=True)
        _, conf2, pred2 = cal.predict_device(cuda(lg), cuda(prox), dac_d, want_probs=False)
        probs, conf, pred = probs.cpu().numpy(), conf.cpu().numpy(), pred.cpu().numpy()
        err = np.abs(probs.astype(np.float64) - want).max()
        print(f"{case} {name} dac={with_dac}: max |d row| {err:.3e} (bound {tol:.3e}), rows with a tied maximum "
              f"{np.mean((want == want.max(axis=1, keepdims=True)).sum(axis=1) > 1):.2f}")
        assert err <= tol
        wc, wp = ref.conf_pred(want)
        np.testing.assert_array_equal(pred, wp)
        np.testing.assert_array_equal(conf, probs[np.arange(len(pred)), pred])
        assert np.abs(conf - wc).max() <= tol
        np.testing.assert_array_equal(conf2.cpu().numpy(), conf)
        np.testing.assert_array_equal(pred2.cpu().numpy(), pred)


def test_large_table_is_read_from_global_memory():
    """More thresholds than the LDS copy holds (2048): same arithmetic from global memory."""
    rng = np.random.default_rng(7)
    lg = rng.normal(0, 3, (300, 77)).astype(np.float32)
    x = device_x(lg)
    X = np.unique(np.concatenate([rng.uniform(x.min() * 0.9, x.max() * 1.1, 3000).astype(np.float32), x.ravel()[::9]])).astype(np.float64)
    Y = np.sort(rng.uniform(0, 1, X.size))
    assert X.size > 2048
    cal = iso.MultiIsotonicRegression()
    cal.set_thresholds(X, Y)
    probs, conf, pred = cal.predict_device(cuda(lg), want_probs=True)
    want = ref.calibrate(X, Y, x)
    assert np.abs(probs.cpu().numpy().astype(np.float64) - want).max() <= ref.interp_tolerance(X, Y, x)
    np.testing.assert_array_equal(pred.cpu().numpy(), ref.conf_pred(want)[1])


def _metrics(out, labels):
    from oracle import clip_oracle as orc   # the reference's ECE (tools/metrics.py:90-130), conf == 1.0 quirk included
    conf, pred = ref.conf_pred(out)
    return np.array([np.mean(pred == labels), orc.ece(conf, pred, labels, 10), conf.astype(np.float64).mean()])


@pytest.mark.parametrize("with_dac", [False, True])
@pytest.mark.parametrize("procal_flag", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_vlcalibration_and_runner_end_to_end(case, procal_flag, with_dac):
    """VLCalibration(bin_based, multi_isotonic_regression).fit(); predict(...) and runner.test(...) see the same (conf, pred) bit for
    bit; against the as-run reference outputs of the fixture the accuracy is equal, and ECE and mean confidence differ by no more than
    the fixture's own float32-vs-float64 pair does plus one test row's share (1 / N_test: a fit on x values a few ulp away may reorder
    one 0 and one 1, which moves single rows across an ECE bin edge; profiles/isotonic_parity.txt has the measured figures)."""
    from clip_calibration_amd import runner
    from clip_calibration_amd.calibrator import VLCalibration
    from clip_calibration_amd.dac import DistanseAwareCalibration
    vl, tl, tp = g(case, "val_logits"), g(case, "test_logits"), g(case, "test_prox")
    n_val, C = vl.shape
    E = 64
    rng = np.random.default_rng(11)
    feats = lambda n: (lambda f: f / np.linalg.norm(f, axis=1, keepdims=True))(rng.normal(size=(n, E))).astype(np.float32)
    vf, tf = feats(n_val), feats(tl.shape[0])
    val = {"val_logits": vl, "val_labels": g(case, "val_labels"), "val_image_features": vf,
           "val_image_knn_dists": -np.log(g(case, "val_prox").astype(np.float64))[:, None]}
    cal = VLCalibration(val, None, dac_flag=False, base_calibration_mode="bin_based", procal_flag=procal_flag,
                        base_bin_calibrator_name="multi_isotonic_regression")
    cal.fit()
    assert type(cal.base_calibrator) is (iso.BinMeanShift if procal_flag else iso.MultiIsotonicRegression)
    if with_dac:   # the fixture's per-class factor, installed as a fitted DAC calibrator
        cal.dac_calibrator = DistanseAwareCalibration()
        cal.dac_calibrator.class_confidence = g(case, "dac").astype(np.float64)
    sfx = "_dac" if with_dac else ""
    name = "bms" if procal_flag else "plain"
    if procal_flag:
        np.testing.assert_allclose(cal.base_calibrator.bin_edges, g(case, "bin_edges"), rtol=1e-12)
        assert np.array_equal(cal.base_calibrator.bin_index(tp), ref.bin_index(g(case, "bin_edges"), tp))

    # against the fixture: the reference as run (float32) and the float64 fit on the same x
    labels = g(case, "test_labels")
    out = cal.predict(tl, tp if procal_flag else None)
    assert out.dtype == np.float32 and out.shape == tl.shape
    r32 = g(case, f"ref32_{name}_test{sfx}")
    x = g(case, "x_test" + sfx)
    r64 = (ref.calibrate_bins(g(case, "bin_edges"), fixture_tables(case), x, tp) if procal_flag
           else ref.calibrate(g(case, "X64"), g(case, "y64"), x))
    m_dev, m32, m64 = _metrics(out, labels), _metrics(r32, labels), _metrics(r64, labels)
    print(f"{case} {name} dac={with_dac}: (accuracy, ECE, mean conf) device {m_dev}, ref32 {m32}, ref64 {m64}; "
          f"mean |device - ref32| {np.abs(out.astype(np.float64) - r32).mean():.3e}, top-1 differs in "
          f"{np.mean(out.argmax(1) != r32.argmax(1)):.4f} of the rows")
    assert m_dev[0] == m32[0]
    for i in (1, 2):
        assert abs(m_dev[i] - m32[i]) <= abs(m32[i] - m64[i]) + 1.0 / tl.shape[0]

    # runner.test on the same logits: an image is (its row number, its feature vector); the proximity is the runner's own
    t_lg = cuda(tl)
    dac_d = cal.class_confidence_device("cuda")
    assert (dac_d is not None) == with_dac

    def infer(image, dac_conf=None, want_conf_pred=False):
        lg = t_lg[image[:, 0].long()].contiguous()
        conf = pred = None
        if dac_conf is not None or want_conf_pred:
            conf = torch.empty(lg.shape[0], dtype=torch.float32, device=lg.device)
            pred = torch.empty(lg.shape[0], dtype=torch.int32, device=lg.device)
            ops.check(ops.lib.clipmi_calibrate_rows(lg.data_ptr(), None if dac_conf is None else dac_conf.data_ptr(), conf.data_ptr(),
                                                    pred.data_ptr(), lg.shape[0], lg.shape[1], ops._stream()), "clipmi_calibrate_rows")
        return lg, image[:, 1:].contiguous(), None, conf, pred

    images = np.concatenate([np.arange(tl.shape[0], dtype=np.float32)[:, None], tf], axis=1)
    loader = [(torch.from_numpy(images[i:i + 96]), torch.from_numpy(labels[i:i + 96])) for i in range(0, len(images), 96)]
    res = runner.test(infer, loader, val_dict=val, calibrator=cal, image_k=3)
    assert res["total"] == tl.shape[0]
    prox_d = torch.exp(-knn_dists_device(cuda(tf), cuda(vf), 3).mean(dim=1))
    scaled = torch.cat([infer(x.cuda(), dac_d, True)[0] for x, _ in loader])
    _, conf_r, pred_r = cal.base_calibrator.predict_device(scaled, prox_d)      # what runner.test hands the evaluator
    out_p = cal.predict(tl, prox_d.cpu().numpy() if procal_flag else None)
    conf_p, pred_p = ref.conf_pred(out_p)
    np.testing.assert_array_equal(pred_r.cpu().numpy(), pred_p)
    np.testing.assert_array_equal(conf_r.cpu().numpy(), conf_p)
    assert res["accuracy"] == pytest.approx(100.0 * np.mean(pred_p == labels), abs=1e-9)
    assert res["ece"] == pytest.approx(100.0 * _metrics(out_p, labels)[1], abs=1e-4)
    if procal_flag:
        with pytest.raises(AssertionError):
            cal.predict(tl, None)
        with pytest.raises(ValueError, match="val_dict"):
            runner.test(infer, loader, val_dict=None, calibrator=cal)


def test_numpy_interface_of_the_reference():
    """fit_transform / transform on probabilities, numpy in and out, as the reference's classes: the val rows calibrated by the fit
    that has just been made, outputs in the original row order."""
    case = "c50"
    pv, pt = ref.softmax32(g(case, "val_logits")), ref.softmax32(g(case, "test_logits"))
    plain = iso.MultiIsotonicRegression()
    out_v = plain.fit_transform(pv, g(case, "val_labels"))
    x = device_x(pv, from_probs=True)
    same_table((plain.X_thresholds_, plain.y_thresholds_), ref.fit_plain(x, g(case, "val_labels")))
    np.testing.assert_allclose(out_v, ref.calibrate(plain.X_thresholds_, plain.y_thresholds_, x), atol=1e-6)
    assert plain.transform(pt).shape == pt.shape
    bms = iso.BinMeanShift(BINS)
    out_v = bms.fit_transform(pv, g(case, "val_prox"), g(case, "val_labels"))
    np.testing.assert_allclose(out_v, ref.calibrate_bins(bms.bin_edges, bms._tables, x, g(case, "val_prox")), atol=1e-6)
    out_t = bms.transform(pt, g(case, "test_prox"))
    assert np.abs(out_t - g(case, "ref32_bms_test")).mean() <= 2 * g(case, "ref32_vs_ref64_mean")[1]


def test_edge_cases():
    rng = np.random.default_rng(3)
    lg = cuda(rng.normal(0, 2, (64, 7)).astype(np.float32))
    labels = rng.integers(0, 7, 64)
    # an empty val bin: every proximity equal puts all rows in the last bin
    with pytest.raises(ValueError, match="hold no val rows"):
        iso.BinMeanShift(BINS).fit_device(lg, labels, np.full(64, 0.4, np.float32))
    # non-finite val logits, a label outside the classes
    bad = lg.clone()
    bad[3, 2] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        iso.MultiIsotonicRegression().fit_device(bad, labels)
    with pytest.raises(ValueError, match="labels outside"):
        iso.MultiIsotonicRegression().fit_device(lg, np.full(64, 7))
    # an empty test bin and N = 0
    prox = np.linspace(0.2, 0.6, 64).astype(np.float32)
    bms = iso.BinMeanShift(BINS)
    bms.fit_device(lg, labels, prox)
    probs, conf, pred = bms.predict_device(lg[:5], torch.full((5,), 0.9).cuda(), want_probs=True)   # all in the last bin
    X, Y = bms._tables[-1]
    np.testing.assert_allclose(probs.cpu().numpy(), ref.calibrate(X, Y, device_x(lg[:5].cpu().numpy())), atol=1e-6)
    probs, conf, pred = bms.predict_device(lg[:0], torch.zeros(0).cuda(), want_probs=True)
    assert probs.shape == (0, 7) and conf.shape == (0,) and pred.shape == (0,)
    with pytest.raises(AssertionError):
        bms.predict_device(lg, None)
    # every positive key equal: identical rows, one label
    same = cuda(np.tile(rng.normal(0, 2, (1, 7)).astype(np.float32), (32, 1)))
    cal = iso.MultiIsotonicRegression()
    cal.fit_device(same, np.full(32, 4))
    same_table((cal.X_thresholds_, cal.y_thresholds_), ref.fit_plain(device_x(same.cpu().numpy()), np.full(32, 4)))
    # a single class: x = 1 everywhere, one threshold
    one = iso.MultiIsotonicRegression()
    one.fit_device(lg[:, :1].contiguous(), np.zeros(64, np.int64))
    assert one.X_thresholds_.tolist() == [1.0] and one.y_thresholds_.tolist() == [1.0]
    _, conf, pred = one.predict_device(lg[:, :1].contiguous())
    assert pred.cpu().tolist() == [0] * 64 and torch.all(conf == 1.0)


def test_repeatable():
    """Integer counts and min / max are order-independent: two fits give the same bits; so do two predict launches."""
    case = "c131"
    lg, labels = cuda(g(case, "val_logits")), g(case, "val_labels")
    a, b = iso.MultiIsotonicRegression(), iso.MultiIsotonicRegression()
    a.fit_device(lg, labels)
    b.fit_device(lg, labels)
    np.testing.assert_array_equal(a.X_thresholds_, b.X_thresholds_)
    np.testing.assert_array_equal(a.y_thresholds_, b.y_thresholds_)
    p1 = a.predict_device(lg, want_probs=True)
    p2 = a.predict_device(lg, want_probs=True)
    for u, v in zip(p1, p2):
        assert torch.equal(u, v)
