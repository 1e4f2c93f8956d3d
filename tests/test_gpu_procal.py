"""ProCal on the GPU (csrc/procal.hip through clip_calibration_amd.procal) against the float64 oracle of tests/procal_ref.py:
the KDE launch on identical fp32 inputs, the row launch from logits (with and without DAC), repeatability, and runner.test end to end."""
import numpy as np
import pytest
import torch

import procal_ref as ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import ops  # noqa: E402
from clip_calibration_amd.procal import DensityRatioCalibration  # noqa: E402
from clip_calibration_amd.proximity import knn_dists_device  # noqa: E402


def _fit_sets(n_true, n_false, seed):
    """A fitted calibrator whose correct / incorrect (conf, proximity) clouds overlap partly; every coordinate is an fp32 value."""
    rng = np.random.default_rng(seed)
    n = n_true + n_false
    conf = np.concatenate([rng.beta(6, 2, n_true), rng.beta(2, 2, n_false) * 0.8 + 0.1]).astype(np.float32).astype(np.float64)
    prox = np.concatenate([rng.normal(0.55, 0.05, n_true), rng.normal(0.45, 0.06, n_false)]).astype(np.float32).astype(np.float64)
    C = 101                              # max prob = conf as long as conf > (1 - conf) / 100
    conf = np.maximum(conf, 0.02)
    probs = np.repeat(((1 - conf) / (C - 1))[:, None], C, axis=1)
    probs[:, 0] = conf
    preds = np.zeros(n, dtype=np.int64)
    true = np.concatenate([np.zeros(n_true, np.int64), np.ones(n_false, np.int64)])
    cal = DensityRatioCalibration()
    cal.fit(probs, preds, true, prox)
    return cal, ref.ProCalRef(probs, preds, true, prox)


def _queries(n, seed):
    """Inside both clouds, on their edges, and far outside (exp underflow in every term; the 1e-10 clamp in force)."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 4, n)
    conf = np.where(kind == 0, rng.uniform(0.2, 1.0, n), np.where(kind == 1, rng.uniform(0.0, 0.15, n), rng.uniform(0, 1, n)))
    prox = np.where(kind == 0, rng.normal(0.5, 0.06, n), np.where(kind == 1, rng.uniform(0.25, 0.32, n), rng.normal(0.5, 0.15, n)))
    far = kind == 3
    prox = np.where(far, rng.choice([-2.0, 3.0], n) + rng.uniform(0, 1, n), prox)
    return conf.astype(np.float32), prox.astype(np.float32)


@pytest.mark.parametrize("n_true,n_false,n_test", [(2, 2, 1), (16000, 40, 37), (300, 16000, 4096), (2000, 2000, 50000)])
def test_kde_matches_oracle(n_true, n_false, n_test):
    cal, orc = _fit_sets(n_true, n_false, seed=n_true + n_false)
    conf, prox = _queries(n_test, seed=n_test)
    got = ops.procal_kde(cal.device_model(), torch.from_numpy(conf).cuda(), torch.from_numpy(prox).cuda()).cpu().numpy()
    want = orc.cstar(conf, prox)
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - want)
    assert err.max() < 2e-6, (err.max(), int(err.argmax()), want[err.argmax()])
    if n_test >= 37:
        assert (want == 0).any()                      # the clamp regime is covered (far queries: every term underflows)
        assert ((want > 0.01) & (want < 0.99)).any()


def _logits(N, C, seed):
    rng = np.random.default_rng(seed)
    lg = (rng.normal(0, 2.5, (N, C)) + rng.normal(0, 2, (N, 1)) * np.eye(C)[rng.integers(0, C, N)]).astype(np.float32)
    lg[0, :] = 1.5                                    # all tied
    lg[1, :] = np.minimum(lg[1], 3.0)
    lg[1, :2] = 4.0                                   # tied top two
    lg[2, :] = -np.inf                                # S == 0: every other probability is exactly 0
    lg[2, C // 2] = 0.25
    lg[3, :] = lg[3, 0] - 200.0                       # the others far below: probs[j] / S must not underflow
    lg[3, 0] += 200.0
    prox = rng.normal(0.5, 0.08, N).astype(np.float32)
    return lg, prox


@pytest.mark.parametrize("C", [2, 10, 1000])
@pytest.mark.parametrize("with_dac", [False, True])
def test_rows_match_oracle(C, with_dac):
    cal, orc = _fit_sets(700, 300, seed=C)
    N = 3000 if C < 1000 else 700
    lg, prox = _logits(N, C, seed=C + with_dac)
    dac = np.random.default_rng(5).uniform(0.5, 1.8, C).astype(np.float32) if with_dac else None
    d_lg = torch.from_numpy(lg).cuda()
    probs, conf, pred, cstar = ops.procal_rows(cal.device_model(), d_lg, torch.from_numpy(prox).cuda(),
                                               None if dac is None else torch.from_numpy(dac).cuda(), want_probs=True, want_cstar=True)
    assert torch.equal(d_lg.cpu(), torch.from_numpy(lg))   # logits untouched
    want, want_c = orc.predict_logits(lg, prox, dac)
    probs, conf, pred, cstar = probs.cpu().numpy(), conf.cpu().numpy(), pred.cpu().numpy(), cstar.cpu().numpy()
    assert np.abs(probs - want).max() < 1e-4
    assert np.abs(cstar - want_c).max() < 1e-4
    w_conf, w_pred = ref.conf_pred(want)
    clear = ref.top_two_gap(want) > 1e-5
    assert clear.sum() > 0.9 * N
    assert np.array_equal(pred[clear], w_pred[clear])
    assert np.abs(conf - w_conf)[clear].max() < 1e-4
    # conf' is the calibrated row's entry at pred' (ties included: numpy's lowest index)
    assert np.array_equal(conf, probs[np.arange(N), pred])
    assert np.array_equal(pred, probs.argmax(1))
    assert pred[0] in (0, 1) and pred[1] in (0, 1, 2)   # all tied: c* or the first of the rest; tied top two
    assert probs[2, C // 2] == cstar[2] and (np.delete(probs[2], C // 2) == 0).all()
    assert probs[3, 1:].sum() > 0 and abs(probs[3].sum() - 1) < 1e-5
    ok = np.isfinite(want).all(axis=1)
    ok[2] = False                                     # the S == 0 row sums to c*
    assert np.abs(probs.sum(1) - 1)[ok].max() < 1e-5


def test_procal_repeatable():
    cal, _ = _fit_sets(1500, 900, seed=11)
    lg, prox = _logits(4096, 100, seed=12)
    d_lg, d_prox = torch.from_numpy(lg).cuda(), torch.from_numpy(prox).cuda()
    dac = torch.linspace(0.7, 1.4, 100, device="cuda")
    a = ops.procal_rows(cal.device_model(), d_lg, d_prox, dac, want_probs=True, want_cstar=True)
    b = ops.procal_rows(cal.device_model(), d_lg, d_prox, dac, want_probs=True, want_cstar=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    k1 = ops.procal_kde(cal.device_model(), d_prox.clamp(0, 1), d_prox)
    k2 = ops.procal_kde(cal.device_model(), d_prox.clamp(0, 1), d_prox)
    assert torch.equal(k1, k2)
    # a row's result does not depend on the rows around it
    c = ops.procal_rows(cal.device_model(), d_lg[77:1000], d_prox[77:1000], dac, want_probs=True, want_cstar=True)
    for x, y in zip(a, c):
        assert torch.equal(x[77:1000], y)


# ---- runner.test end to end ---------------------------------------------------------------------------------------------------
E2E = dict(C=10, E=64, n_val=200, n_test=161, K=3, scale=18.0, seed=5)


def e2e_fixture(C, E, n_val, n_test, K, scale, seed):
    """Host fixture: normalised fp32 image / text features (an image is its feature vector), labels, and the float64 oracle of
    the run: val logits and val proximity, test logits (fp32-rounded), test proximity."""
    rng = np.random.default_rng(seed)
    txt = rng.normal(size=(C, E))
    txt /= np.linalg.norm(txt, axis=1, keepdims=True)
    def images(n):
        cls = rng.integers(0, C, n)
        x = txt[cls] * rng.uniform(0.2, 1.2, (n, 1)) + rng.normal(size=(n, E)) * 0.25
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), cls
    vf, vc = images(n_val)
    tf, tc = images(n_test)
    txt = txt.astype(np.float32)
    def labels(logits, cls):
        return np.where(rng.random(len(cls)) < 0.7, logits.argmax(1), rng.integers(0, C, len(cls)))
    v_lg = scale * (vf.astype(np.float64) @ txt.T.astype(np.float64))
    t_lg = scale * (tf.astype(np.float64) @ txt.T.astype(np.float64))
    vl, tl = labels(v_lg, vc), labels(t_lg, tc)
    def knn(q, r, k):
        d = np.sqrt(((q[:, None, :].astype(np.float64) - r[None, :, :].astype(np.float64)) ** 2).sum(-1))
        return np.sort(d, axis=1)[:, :k]
    v_knn = knn(vf, vf, K + 1)[:, 1:]
    t_prox = np.exp(-knn(tf, vf, K).mean(1))
    tfd = {k: rng.normal(size=(C, E)) for k in ("base_text_features_zs", "current_text_features_zs")}
    tfd["base_text_features_tuned"] = tfd["base_text_features_zs"] + rng.normal(size=(C, E)) * 0.3
    tfd["current_text_features_tuned"] = tfd["current_text_features_zs"] + rng.normal(size=(C, E)) * 0.3
    return dict(vf=vf, vl=vl, tf=tf, tl=tl, txt=txt, v_lg=v_lg, t_lg=t_lg.astype(np.float32), v_knn=v_knn, t_prox=t_prox, tfd=tfd)


def quantile_margin(x, n_bins=10):
    """The smallest gap between the sorted values that sit next to an equal-mass bin edge (percentiles, linear interpolation): no
    sample changes quantile bin under a perturbation below half of it."""
    s = np.sort(np.asarray(x, np.float64))
    pos = (len(s) - 1) * np.arange(1, n_bins) / n_bins
    idx = np.clip(np.floor(pos).astype(int)[:, None] + np.arange(-1, 2)[None, :], 0, len(s) - 2)
    return (s[idx + 1] - s[idx]).min()


def o_fit(fx):
    """vl_calibrator.py:60-69, 112-121: the oracle's density-ratio fit on the val softmax (no DAC) and the val proximity."""
    vp = ref.softmax(fx["v_lg"])
    return ref.ProCalRef(vp, vp.argmax(1), fx["vl"], np.exp(-fx["v_knn"].mean(1)))


def e2e_oracle(fx, dac_conf, K):
    """Oracle metrics of a ProCal run on the fixture and the margins that make them comparable at 1e-3 percentage points."""
    from oracle import clip_oracle as orc
    out, _ = o_fit(fx).predict_logits(fx["t_lg"], fx["t_prox"], dac_conf)
    conf, pred = ref.conf_pred(out)
    gt, prox = fx["tl"], fx["t_prox"]
    margins = {"bin_edge": np.abs(conf[:, None] - np.linspace(0, 1, 11)[None, :]).min(),
               "conf_gap": quantile_margin(conf), "prox_gap": quantile_margin(prox), "top_two": ref.top_two_gap(out).min(),
               "val_top_two": np.diff(np.sort(fx["v_lg"], axis=1)[:, -2:], axis=1).min()}
    metrics = {"accuracy": 100.0 * np.mean(pred == gt), "ece": 100.0 * orc.ece(conf, pred, gt, 10), "mce": 100.0 * orc.mce(conf, pred, gt, 10),
               "ace": 100.0 * orc.ace(conf, pred, gt, 10), "piece": 100.0 * orc.piece(conf, prox, pred, gt, 10, 10)}
    return out, metrics, margins


@pytest.mark.parametrize("with_dac", [False, True])
def test_runner_procal_flow(with_dac):
    """collect_base_val_features -> VLCalibration(scaling_based, procal) .fit -> predict and runner.test, with a trainer-like
    callable on the fused logits kernel (which applies DAC in place), against the oracle's evaluate on oracle-calibrated probs."""
    from clip_calibration_amd import runner
    from clip_calibration_amd.calibrator import VLCalibration
    p = E2E
    fx = e2e_fixture(**p)
    txt_d = torch.from_numpy(fx["txt"]).cuda()

    def infer(image, dac_conf=None, want_conf_pred=False):
        logits, conf, pred = ops.logits_fused(image, txt_d, p["scale"], dac_conf, want_conf_pred)
        return logits, image, txt_d, conf, pred

    loader = lambda x, y, bs: [(torch.from_numpy(x[i:i + bs]), torch.from_numpy(y[i:i + bs])) for i in range(0, len(x), bs)]
    val = runner.collect_base_val_features(infer, loader(fx["vf"], fx["vl"], 64), image_k=p["K"])
    np.testing.assert_allclose(val["val_image_knn_dists"], fx["v_knn"], atol=1e-5)
    cal = VLCalibration(val, fx["tfd"] if with_dac else None, dac_flag=with_dac, base_calibration_mode="scaling_based", procal_flag=True)
    cal.fit()
    dac = cal.dac_calibrator.class_confidence.astype(np.float32) if with_dac else None
    # the oracle fits on the val dict the device produced and calibrates the test logits and proximity the runner sees (the fused
    # kernel's output is bit-identical for any batch composition): DAC-scaled already, so the oracle applies no DAC to them
    fx["v_lg"], fx["v_knn"] = val["val_logits"].astype(np.float64), val["val_image_knn_dists"].astype(np.float64)
    dac_d = cal.class_confidence_device("cuda")
    t_lg = torch.cat([infer(x.cuda(), dac_d, True)[0] for x, _ in loader(fx["tf"], fx["tl"], 96)])
    t_prox = torch.exp(-knn_dists_device(torch.from_numpy(fx["tf"]).cuda(), torch.from_numpy(fx["vf"]).cuda(), p["K"]).mean(dim=1))
    fx["t_lg"], fx["t_prox"] = t_lg.cpu().numpy(), t_prox.cpu().numpy().astype(np.float64)
    out, want, margins = e2e_oracle(fx, None, p["K"])
    assert margins["bin_edge"] > 1e-4 and margins["conf_gap"] > 1e-5, margins
    assert margins["top_two"] > 1e-4 and margins["val_top_two"] > 1e-3, margins

    # VLCalibration.predict takes raw logits: DAC -> softmax -> ProCal
    raw = torch.cat([infer(x.cuda(), None, True)[0] for x, _ in loader(fx["tf"], fx["tl"], 96)]).cpu().numpy()
    probs = cal.predict(raw, fx["t_prox"])
    assert np.abs(probs - ref.ProCalRef.predict_logits(o_fit(fx), raw, fx["t_prox"], dac)[0]).max() < 1e-4

    res = runner.test(infer, loader(fx["tf"], fx["tl"], 96), val_dict=val, calibrator=cal, image_k=p["K"])
    assert res["total"] == p["n_test"]
    for key in ("accuracy", "ece", "mce", "ace", "piece"):
        assert abs(res[key] - want[key]) < 1e-3, (key, res[key], want[key])
    with pytest.raises(AssertionError):
        cal.predict(raw, None)
    # ProCal changed what the evaluator saw: the plain run differs
    plain = VLCalibration(val, fx["tfd"] if with_dac else None, dac_flag=with_dac)
    plain.fit()
    res0 = runner.test(infer, loader(fx["tf"], fx["tl"], 96), val_dict=val, calibrator=plain, image_k=p["K"])
    assert abs(res0["ece"] - res["ece"]) > 1e-3
