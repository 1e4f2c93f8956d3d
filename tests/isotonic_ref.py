"""numpy restatement of multi-class isotonic calibration and Bin-Mean-Shift, and of what the evaluator then sees -- the oracle of
tests/test_isotonic_cpu.py and tests/test_gpu_isotonic.py.  Sources:

* reference trainers/calibration/vl_calibrator.py:60 (val softmax, no DAC on val), :83-109 (DAC -> softmax -> calibrator), :121-147
  (the branch that builds MultiIsotonicRegression / BinMeanShift with 5 quantile bins);
* reference trainers/calibration/multi_isotonic_regression.py (x = exp(p) / sum exp(p) of the PROBABILITIES, one isotonic fit on the
  flattened (x, onehot) pairs, g(x) + 1e-9 x, no renormalisation);
* reference trainers/calibration/multi_proximity_isotonic.py:130-247 (np.percentile edges, searchsorted(edges[1:-1], side="right"));
* sklearn isotonic.py (_build_y: equal x merged into one weighted point, pool-adjacent-violators, then only the first and last point of
  every constant stretch are kept as thresholds; predict: linear interpolation, clipped) and _isotonic.pyx (the pooling loop: a block
  absorbs its successor unless its mean is strictly below);
* reference evaluators/vl_evaluator.py:68, 83 (argmax of the calibrated rows, conf = its value).

The fit here is the sort-based one, in float64 throughout: the exact solution on whatever x it is given.  It shares nothing with the
product's gap-statistics route (clip_calibration_amd/isotonic.py) except ``gap_statistics`` below, a numpy statement of what the device
accumulates, which exists so that the product's host pooling can be checked without a GPU.
"""
from __future__ import annotations

import numpy as np


def softmax32(logits, dac_conf=None):
    """vl_calibrator.py:88-91 in float32: the DAC factor of the raw argmax (distanse_aware_calibration.py:49-58), then softmax."""
    y = np.asarray(logits, np.float32)
    if dac_conf is not None:
        y = y * np.asarray(dac_conf, np.float32)[y.argmax(axis=1)][:, None]
    e = np.exp(y - y.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def second_softmax(p):
    """multi_isotonic_regression.py:26, 33 on float32 probabilities."""
    p = np.asarray(p, np.float32)
    return np.exp(p) / np.sum(np.exp(p), 1)[:, None]


def onehot(labels, n_classes):
    out = np.zeros((len(labels), n_classes))
    out[np.arange(len(labels)), np.asarray(labels)] = 1
    return out


def fit_thresholds(x, targets):
    """sklearn's IsotonicRegression(out_of_bounds='clip').fit(x, targets) for float64 input, returning (X_thresholds_, y_thresholds_):
    sort, merge equal x (weight = multiplicity, y = mean), pool adjacent violators, keep each block's end points."""
    x = np.asarray(x, np.float64).ravel()
    t = np.asarray(targets, np.float64).ravel()
    if x.size == 0:
        raise ValueError("empty fit")
    order = np.argsort(x, kind="stable")
    x, t = x[order], t[order]
    ux, start = np.unique(x, return_index=True)
    w = np.diff(np.append(start, x.size)).astype(np.float64)
    y = np.add.reduceat(t, start) / w
    blocks = []   # [sum_w, sum_wy, first unique-x index, last unique-x index]
    for i in range(ux.size):
        blocks.append([w[i], w[i] * y[i], i, i])
        while len(blocks) > 1 and blocks[-2][1] / blocks[-2][0] >= blocks[-1][1] / blocks[-1][0]:
            b = blocks.pop()
            blocks[-1][0] += b[0]
            blocks[-1][1] += b[1]
            blocks[-1][3] = b[3]
    X, Y = [], []
    for sw, swy, a, b in blocks:
        X.append(ux[a])
        Y.append(swy / sw)
        if b != a:
            X.append(ux[b])
            Y.append(swy / sw)
    return np.asarray(X), np.asarray(Y)


def calibrate(X, Y, x):
    """IsotonicRegression.predict (np.interp clips like out_of_bounds='clip') in float64 on float32 x, rounded to float32, then the
    reference's `+ 1e-9 * p` in float32."""
    x = np.asarray(x, np.float32)
    g = np.interp(x.astype(np.float64), X, Y) if len(X) > 1 else np.full(x.shape, Y[0])
    return g.astype(np.float32) + np.float32(1e-9) * x


def bin_edges(proximity, bins=5):
    return np.asarray(np.percentile(proximity, np.linspace(0, 100, bins + 1)))


def bin_index(edges, proximity):
    return np.searchsorted(np.asarray(edges)[1:-1], proximity, side="right")


def fit_plain(x_val, labels):
    return fit_thresholds(x_val, onehot(labels, x_val.shape[1]))


def fit_bins(x_val, labels, proximity, bins=5):
    edges = bin_edges(proximity, bins)
    no = bin_index(edges, proximity)
    tables = []
    for b in range(bins):
        if not np.any(no == b):
            raise ValueError(f"bin {b} holds no val rows")
        tables.append(fit_plain(x_val[no == b], np.asarray(labels)[no == b]))
    return edges, tables


def calibrate_bins(edges, tables, x, proximity):
    no = bin_index(edges, proximity)
    out = np.empty(x.shape, np.float32)
    for b, (X, Y) in enumerate(tables):
        out[no == b] = calibrate(X, Y, x[no == b])
    return out


def conf_pred(calibrated):
    """vl_evaluator.py:68, 83: numpy argmax (first index on ties) of the calibrated rows and its value."""
    pred = calibrated.argmax(axis=1)
    return calibrated[np.arange(calibrated.shape[0]), pred], pred


def gap_statistics(x, labels):
    """What clipmi_isotonic_gap_stats accumulates for one bin, in numpy: (keys, positives, zeros_equal, gap_count, gap_min, gap_max) with
    keys the sorted distinct x at the labels and gap g the zeros strictly between key g-1 and key g."""
    x = np.asarray(x, np.float32)
    n, C = x.shape
    pos_mask = np.zeros((n, C), bool)
    pos_mask[np.arange(n), np.asarray(labels)] = True
    keys, positives = np.unique(x[pos_mask], return_counts=True)
    zeros = x[~pos_mask]
    g = np.searchsorted(keys, zeros, side="left")
    eq = (g < keys.size) & (keys[np.minimum(g, keys.size - 1)] == zeros)
    zeros_equal = np.bincount(g[eq], minlength=keys.size)
    gap_count = np.bincount(g[~eq], minlength=keys.size + 1)
    gap_min = np.full(keys.size + 1, np.inf, np.float32)
    gap_max = np.zeros(keys.size + 1, np.float32)
    np.minimum.at(gap_min, g[~eq], zeros[~eq])
    np.maximum.at(gap_max, g[~eq], zeros[~eq])
    return keys, positives, zeros_equal, gap_count, gap_min, gap_max


def interp_tolerance(X, Y, x):
    """The error an fp32 evaluation of the table may make against float64 np.interp on the same x: one rounding of the result and of the
    1e-9 x term (2^-22 max|y| covers both), plus the steepest slope times one ulp of x."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    slope = float(np.max(np.diff(Y) / np.diff(X))) if len(X) > 1 else 0.0
    ulp = float(np.spacing(np.float32(np.max(x)))) if np.size(x) else 0.0
    return 2.0 ** -22 * float(np.max(np.abs(Y))) + slope * ulp
