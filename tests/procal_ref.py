"""float64 numpy restatement of ProCal (the density-ratio calibrator) and of what the evaluator then sees -- the oracle of
tests/test_procal_cpu.py and tests/test_gpu_procal.py.  Sources:

* reference trainers/calibration/vl_calibrator.py:60-68 (val softmax, no DAC on val), :71-79, :83-109 (DAC -> softmax -> ProCal),
  :112-121 (the branch that builds DensityRatioCalibration);
* reference trainers/calibration/density_ratio_calibration.py:28-117 (fit: split by correctness, one KDE per set, |F| / |T|;
  predict: c* = T / max(T + ratio F, 1e-10), the rest of the row rescaled to 1 - c*);
* statsmodels 0.12.2 nonparametric/_kernel_base.py:250-265 (_normal_reference: 1.06 std n^(-1/(4+d))), :456-518 (gpke: product of
  the per-dimension kernels / prod(bw), summed), kernels.py:125 (gaussian: exp(-u^2/2) / sqrt(2 pi)), kernel_density.py:162-196
  (pdf: gpke / nobs, per data_predict row);
* reference evaluators/vl_evaluator.py:68, 83 (argmax of the calibrated rows, conf = its value).
"""
from __future__ import annotations

import numpy as np


def softmax(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def bandwidth(points):
    """_kernel_base.py:250-265 with d = 2: np.std's default ddof=0."""
    points = np.asarray(points, dtype=np.float64)
    return 1.06 * np.std(points, axis=0) * points.shape[0] ** (-1.0 / 6.0)


def kde_pdf(data, bw, queries):
    """kernel_density.py:162-196 + gpke: (1 / n) sum_i prod_d phi((q_d - x_id) / h_d) / h_d, phi the standard normal density."""
    data, queries = np.asarray(data, np.float64), np.asarray(queries, np.float64)
    out = np.empty(queries.shape[0])
    for a in range(0, queries.shape[0], 512):
        q = queries[a:a + 512]
        u = (q[:, None, :] - data[None, :, :]) / bw
        k = np.exp(-0.5 * u * u) / np.sqrt(2 * np.pi)
        out[a:a + 512] = (k.prod(axis=2) / np.prod(bw)).sum(axis=1) / data.shape[0]
    return out


class ProCalRef:
    def __init__(self, probs, preds, true, proximity):
        """density_ratio_calibration.py:34-79."""
        conf = np.asarray(probs, np.float64).max(axis=-1)
        correct = np.asarray(preds) == np.asarray(true)
        pts = np.stack([conf, np.asarray(proximity, np.float64)], axis=1)
        self.data_true, self.data_false = pts[correct], pts[~correct]
        for s in (self.data_true, self.data_false):
            if s.shape[0] < 2:
                raise ValueError("fewer than 2 points")
        self.bw_true, self.bw_false = bandwidth(self.data_true), bandwidth(self.data_false)
        if not (np.all(self.bw_true > 0) and np.all(self.bw_false > 0)):
            raise ValueError("no spread")
        self.ratio = (~correct).sum() / correct.sum()

    def cstar(self, conf, proximity):
        """density_ratio_calibration.py:97-105."""
        q = np.stack([np.asarray(conf, np.float64), np.asarray(proximity, np.float64)], axis=1)
        t = kde_pdf(self.data_true, self.bw_true, q)
        f = kde_pdf(self.data_false, self.bw_false, q)
        return t / np.maximum(t + f * self.ratio, 1e-10)

    def predict_logits(self, logits, proximity, dac_conf=None):
        """vl_calibrator.py:83-109 + density_ratio_calibration.py:97-117 from logits.  Returns (calibrated probs, c*, top-two data).
        probs[j] / S is formed from the logits, exp(y_j - y_i2) / sum_{k != i1} exp(y_k - y_i2): the same number as the reference's
        probs[j] / probs.sum() wherever that sum is a normal float, and never 0 / 0 where the other probabilities underflow.  A row
        whose other probabilities are exactly 0 (every other logit -inf) keeps them at 0 (the reference: NaN)."""
        y = np.asarray(logits, np.float32).astype(np.float64)
        if dac_conf is not None:   # distanse_aware_calibration.py:49-58, in fp32 as the reference
            lg32 = np.asarray(logits, np.float32)
            y = (lg32 * np.asarray(dac_conf, np.float32)[lg32.argmax(axis=1)][:, None]).astype(np.float64)
        probs = softmax(y)
        n = y.shape[0]
        i1 = probs.argmax(axis=1)
        c = self.cstar(probs[np.arange(n), i1], proximity)
        others = y.copy()
        others[np.arange(n), i1] = -np.inf
        y2 = others.max(axis=1)
        out = np.zeros_like(probs)
        finite = np.isfinite(y2)
        with np.errstate(invalid="ignore", over="ignore"):
            e = np.exp(others[finite] - y2[finite, None])
        out[finite] = e / e.sum(axis=1, keepdims=True) * (1.0 - c[finite])[:, None]
        out[np.arange(n), i1] = c
        return out, c


def conf_pred(calibrated):
    """vl_evaluator.py:68, 83: numpy argmax (first index on ties) of the calibrated rows and its value."""
    pred = calibrated.argmax(axis=1)
    return calibrated[np.arange(calibrated.shape[0]), pred], pred


def top_two_gap(calibrated):
    """Distance between the largest and the second largest entry of every calibrated row (0 on ties)."""
    s = np.sort(calibrated, axis=1)
    return s[:, -1] - s[:, -2] if calibrated.shape[1] > 1 else np.full(calibrated.shape[0], np.inf)
