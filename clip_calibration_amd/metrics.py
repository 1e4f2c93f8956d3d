"""Expected Calibration Error, host side (reference tools/metrics.py:90-130).

The per-sample work (softmax top-1, binning, per-bin sums) runs on the GPU (``clipmi_logits`` +
``clipmi_ece_accumulate``); this module only turns the 3*(n_bins+1) accumulated numbers into the scalar, reproducing
the reference's digitize/histogram edge quirk.  ``ECE`` keeps the reference's name and signature for callers that
already hold (conf, pred, gt) arrays on the host.
"""
from __future__ import annotations

import numpy as np


def digitize_bins(conf: np.ndarray, n_bins: int) -> np.ndarray:
    """np.digitize(conf, linspace(0,1,n_bins+1)) - 1 (tools/metrics.py:104-105): bin n_bins holds conf == 1.0."""
    edges = np.linspace(0, 1, n_bins + 1)
    return np.searchsorted(edges, np.asarray(conf), side="right") - 1


def bin_statistics(conf, pred, gt, n_bins: int = 10) -> np.ndarray:
    """float64 [3, n_bins+1] = (count, sum_conf, sum_correct) per digitize bin -- what the device kernel accumulates."""
    conf = np.asarray(conf, dtype=np.float64)
    which = digitize_bins(conf, n_bins)
    out = np.zeros((3, n_bins + 1))
    np.add.at(out[0], which, 1.0)
    np.add.at(out[1], which, conf)
    np.add.at(out[2], which, (np.asarray(pred) == np.asarray(gt)).astype(np.float64))
    return out


def ece_from_bins(bins: np.ndarray, n_bins: int = 10) -> float:
    """Scalar ECE from accumulated (count, sum_conf, sum_correct).  Per-bin means come from the digitize bins
    0..n_bins-1; the weights follow np.histogram, whose closed last edge puts conf == 1.0 into bin n_bins-1
    (tools/metrics.py:108-128)."""
    b = np.asarray(bins, dtype=np.float64).reshape(3, n_bins + 1)
    count, s_conf, s_corr = b[0, :n_bins], b[1, :n_bins], b[2, :n_bins]
    total = b[0].sum()
    if total == 0:
        return float("nan")
    nz = count > 0
    acc = np.where(nz, s_corr / np.where(nz, count, 1), 0.0)
    avg = np.where(nz, s_conf / np.where(nz, count, 1), 0.0)
    weights = count.copy()
    weights[n_bins - 1] += b[0, n_bins]
    return float(np.sum(weights / total * np.abs(avg - acc)))


def ECE(conf, pred, gt, conf_bin_num: int = 10) -> float:
    return ece_from_bins(bin_statistics(conf, pred, gt, conf_bin_num), conf_bin_num)


def mce_from_bins(bins: np.ndarray, n_bins: int = 10) -> float:
    """The reference's "MCE" (tools/metrics.py:181-208): bins from digitize(conf, linspace(0,1,n+1)[1:-1]) -- so conf == 1.0
    belongs to the last bin and DOES enter its means -- and the per-bin gap weighted by the bin's share:
    max_b |mean acc_b - mean conf_b| * count_b / N  =  max_b |sum_correct_b - sum_conf_b| / N."""
    b = np.asarray(bins, dtype=np.float64).reshape(3, n_bins + 1).copy()
    b[:, n_bins - 1] += b[:, n_bins]
    b = b[:, :n_bins]
    total = b[0].sum()
    if total == 0:
        return float("nan")
    nz = b[0] > 0
    return float(np.max(np.abs(b[2][nz] - b[1][nz])) / total)


def MCE(conf, pred, gt, conf_bin_num: int = 10) -> float:
    return mce_from_bins(bin_statistics(conf, pred, gt, conf_bin_num), conf_bin_num)


# ---- metrics that need the samples themselves (quantile bins, per-class counts): evaluated once per test() on the host
# from the (conf, pred, gt[, proximity]) vectors the device evaluator kept -- 12-16 B per sample ------------------------

def quantile_bin_index(x, n_bins: int) -> np.ndarray:
    """Ordinal equal-frequency bin of every value: edges = percentiles 0, 100/n, ..., 100 (linear interpolation), edges
    closer than 1e-8 to their left neighbour dropped, index = number of inner edges <= x.  This is what the reference
    obtains from sklearn's KBinsDiscretizer(encode='ordinal', strategy='quantile') at tools/metrics.py:152,228; a
    constant input collapses to a single bin."""
    col = np.asarray(x)
    if col.dtype not in (np.float32, np.float64):
        col = col.astype(np.float64)
    if col.size == 0:
        return np.zeros(0, dtype=np.int64)
    if col.min() == col.max():
        return np.zeros(col.shape[0], dtype=np.int64)
    edges = np.asarray(np.percentile(col, np.linspace(0, 100, n_bins + 1)), dtype=np.float64)
    edges = edges[np.ediff1d(edges, to_begin=np.inf) > 1e-8]
    return np.searchsorted(edges[1:-1], col, side="right").astype(np.int64)


def _grouped_gap(group: np.ndarray, conf: np.ndarray, correct: np.ndarray) -> float:
    """sum over groups of |mean correct - mean conf| * count / N  =  sum_g |sum correct_g - sum conf_g| / N."""
    _, inv = np.unique(group, return_inverse=True)
    diff = np.bincount(inv, weights=correct) - np.bincount(inv, weights=conf)
    return float(np.abs(diff).sum() / conf.shape[0])


def AdaptiveECE(conf, pred, gt, conf_bin_num: int = 10) -> float:
    """Equal-mass-bin calibration error (tools/metrics.py:212-236)."""
    conf = np.asarray(conf)
    correct = (np.asarray(pred) == np.asarray(gt)).astype(np.float64)
    return _grouped_gap(quantile_bin_index(conf, conf_bin_num), conf.astype(np.float64), correct)


def PIECE(conf, knndist, pred, gt, dist_bin_num: int = 10, conf_bin_num: int = 10) -> float:
    """Proximity-informed ECE (tools/metrics.py:132-178, knn_strategy='quantile'): groups are (quantile bin of the
    proximity value, uniform confidence bin with conf == 1.0 kept in the last bin)."""
    conf = np.asarray(conf)
    correct = (np.asarray(pred) == np.asarray(gt)).astype(np.float64)
    knn_bin = quantile_bin_index(np.asarray(knndist), dist_bin_num)
    conf_bin = np.searchsorted(np.linspace(0, 1, conf_bin_num + 1)[1:-1], conf, side="right")
    return _grouped_gap(knn_bin * (conf_bin_num + 1) + conf_bin, conf.astype(np.float64), correct)


def macro_f1(pred, gt) -> float:
    """Unweighted mean of per-class F1 over the classes PRESENT in gt (vl_evaluator.py:77-82: sklearn f1_score with
    average='macro', labels=np.unique(labels)); a class never predicted scores 0."""
    pred, gt = np.asarray(pred).astype(np.int64), np.asarray(gt).astype(np.int64)
    classes = np.unique(gt)
    n = int(max(pred.max(), gt.max())) + 1
    tp = np.bincount(gt[pred == gt], minlength=n).astype(np.float64)
    n_pred = np.bincount(pred, minlength=n).astype(np.float64)
    n_gt = np.bincount(gt, minlength=n).astype(np.float64)
    denom = (n_pred + n_gt)[classes]                      # 2 tp + fp + fn
    f1 = np.where(denom > 0, 2 * tp[classes] / np.where(denom > 0, denom, 1), 0.0)
    return float(f1.mean())


# ---- the same three metrics from what the device kernels return (csrc/sample_metrics.hip): a few order statistics, the per-group
# sums and the per-class counts -- no per-sample vector reaches the host ------------------------------------------------------------

def _virtual_indexes(n: int, n_bins: int) -> np.ndarray:
    """The float64 positions in the sorted array that np.percentile(x, linspace(0, 100, n_bins + 1), method="linear") interpolates
    at for n values: numpy's own expression for the method, (n - 1) * (q / 100), operation for operation."""
    return (n - 1) * np.true_divide(np.linspace(0, 100, n_bins + 1), 100)


def quantile_ranks(n: int, n_bins: int) -> np.ndarray:
    """int32 [2 * (n_bins + 1)]: the n_bins + 1 floor indexes, then the n_bins + 1 (clipped) ceil indexes, of the sorted-array
    elements np.percentile reads for the edges of ``quantile_bin_index`` -- numpy's _get_indexes: a position at or beyond n - 1
    reads the last element twice, one below 0 the first."""
    if n < 1 or n_bins < 1:
        raise ValueError(f"quantile_ranks: n={n}, n_bins={n_bins} (both >= 1)")
    v = _virtual_indexes(n, n_bins)
    lo = np.floor(v)
    hi = lo + 1
    above, below = v >= n - 1, v < 0
    lo[above] = hi[above] = n - 1
    lo[below] = hi[below] = 0
    return np.concatenate([lo, hi]).astype(np.int32)


def percentiles_from_order_stats(stats, n: int, n_bins: int) -> np.ndarray:
    """np.percentile(x, linspace(0, 100, n_bins + 1)) from ``stats = np.sort(x)[quantile_ranks(n, n_bins)]``, bit for bit: numpy's
    _get_gamma and _lerp restated (a + (b - a) t, and b - (b - a)(1 - t) from t = 0.5 on; the difference in the dtype of x, the
    rest in float64), with the weight taken against the index numpy takes it against (-1 at the upper bound)."""
    stats = np.asarray(stats)
    if stats.shape != (2 * (n_bins + 1),):
        raise ValueError(f"percentiles_from_order_stats: stats {stats.shape} for {n_bins} bins")
    a, b = stats[:n_bins + 1], stats[n_bins + 1:]
    v = _virtual_indexes(n, n_bins)
    prev = np.floor(v)
    prev[v >= n - 1] = -1
    prev[v < 0] = 0
    t = v - prev
    with np.errstate(invalid="ignore"):   # inf - inf: numpy's own lerp answers NaN there, with the same warning silenced here
        diff = np.subtract(b, a)
        out = np.asanyarray(np.add(a, diff * t))
        np.subtract(b, diff * (1 - t), out=out, where=t >= 0.5, casting="unsafe", dtype=type(out.dtype))
    return out


def quantile_edges_from_order_stats(stats, n: int, n_bins: int, nan_count: int = 0) -> np.ndarray:
    """The inner bin edges of ``quantile_bin_index(x, n_bins)`` as float64, from the order statistics of x at
    ``quantile_ranks(n, n_bins)``: bin index = np.searchsorted(edges, x, side="right").  Empty -- every sample in bin 0, as
    quantile_bin_index answers -- when x holds a NaN (``nan_count``, or a NaN among the statistics: NaNs sort last and the last
    element is always read) or when all values are equal."""
    stats = np.asarray(stats)
    if stats.dtype not in (np.float32, np.float64):
        stats = stats.astype(np.float64)
    none = np.zeros(0, dtype=np.float64)
    if stats.shape != (2 * (n_bins + 1),):
        raise ValueError(f"quantile_edges_from_order_stats: stats {stats.shape} for {n_bins} bins")
    if nan_count or np.isnan(stats).any() or stats[0] == stats[-1]:   # stats[0] = min (rank 0), stats[-1] = max (rank n - 1)
        return none
    edges = np.asarray(percentiles_from_order_stats(stats, n, n_bins), dtype=np.float64)
    edges = edges[np.ediff1d(edges, to_begin=np.inf) > 1e-8]
    return edges[1:-1]


def gap_from_groups(groups) -> float:
    """``_grouped_gap`` from float64 [3, G] = (count, sum_conf, sum_correct) per group: sum_g |sum_correct_g - sum_conf_g| / N
    (an empty group adds nothing)."""
    g = np.asarray(groups, dtype=np.float64)
    g = g.reshape(3, -1)
    return float(np.abs(g[2] - g[1]).sum() / g[0].sum())


def macro_f1_from_counts(counts) -> float:
    """``macro_f1`` from int [3 C + 1] = true positives | predicted | labelled per class (| samples outside the classes, not used
    here): the mean F1 over the classes with a label count."""
    c = np.asarray(counts)
    C = (c.shape[0] - 1) // 3
    if c.ndim != 1 or c.shape[0] != 3 * C + 1 or C < 1:
        raise ValueError(f"macro_f1_from_counts: counts {c.shape} is not [3 C + 1]")
    tp, n_pred, n_gt = (c[i * C:(i + 1) * C].astype(np.float64) for i in range(3))
    classes = n_gt > 0
    denom = (n_pred + n_gt)[classes]                      # 2 tp + fp + fn
    f1 = np.where(denom > 0, 2 * tp[classes] / np.where(denom > 0, denom, 1), 0.0)
    return float(f1.mean())


# ---- proper scores of whole probability rows and the class-wise calibration error (csrc/row_scores.hip): the float64 host path, and the
# restatement the device kernels are held to.  The reference has none of them. ------------------------------------------------------------

CONF_FIXED_ONE = 2.0 ** 32    # the device's conf_sum is 32.32 fixed point


def row_probabilities(rows, from_probs: bool = False) -> np.ndarray:
    """float64 [N, C]: the rows themselves (``from_probs``; they need not sum to 1) or their softmax."""
    z = np.asarray(rows, dtype=np.float64)
    if z.ndim != 2 or z.shape[1] < 1:
        raise ValueError(f"rows {z.shape} must be [N, C >= 1]")
    if from_probs:
        return z
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(z - z.max(axis=1, keepdims=True)) if z.shape[0] else z
        return e / e.sum(axis=1, keepdims=True) if z.shape[0] else z


def unscorable_rows(rows, from_probs: bool = False) -> np.ndarray:
    """bool [N]: rows without a softmax -- a NaN, a +inf or nothing but -inf among the logits; any non-finite probability."""
    z = np.asarray(rows, dtype=np.float64)
    if from_probs:
        return ~np.isfinite(z).all(axis=1)
    return np.isnan(z).any(axis=1) | np.isinf(z.max(axis=1, initial=-np.inf))


def row_scores(rows, gt, from_probs: bool = False):
    """(nll float64 [N], brier float64 [N]): nll_i = logsumexp(z_i) - z_iy, or -log(max(p_iy, FLT_MIN)) for probabilities;
    brier_i = sum_c (p_ic - [c == y_i])^2.  NaN for a row without a softmax and for a label outside [0, C) (clipmi_val_score's rule)."""
    z = np.asarray(rows, dtype=np.float64)
    p = row_probabilities(z, from_probs)
    gt = np.asarray(gt).astype(np.int64).reshape(-1)
    N, C = p.shape
    if gt.shape[0] != N:
        raise ValueError(f"{N} rows need {N} labels, got {gt.shape[0]}")
    ok = (gt >= 0) & (gt < C) & ~unscorable_rows(z, from_probs)
    y = np.where(ok, gt, 0)
    idx = np.arange(N)
    nll, brier = np.full(N, np.nan), np.full(N, np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if from_probs:
            val = -np.log(np.maximum(p[idx, y], float(np.finfo(np.float32).tiny)))
        else:
            m = z.max(axis=1)
            val = np.log(np.exp(z - m[:, None]).sum(axis=1)) - (z[idx, y] - m)
        onehot = np.zeros_like(p)
        onehot[idx, y] = 1.0
        b = ((p - onehot) ** 2).sum(axis=1)
    nll[ok], brier[ok] = val[ok], b[ok]
    return nll, brier


def NLL(rows, gt, from_probs: bool = False) -> float:
    """Mean negative log-likelihood of the labels under the rows (logits, or probabilities with ``from_probs``)."""
    nll = row_scores(rows, gt, from_probs)[0]
    return float(nll.mean()) if nll.size else float("nan")


def Brier(rows, gt, from_probs: bool = False) -> float:
    """Mean multi-class Brier score: sum_c (p_c - [c == y])^2 per row (Brier 1950, the unnormalised sum over the classes)."""
    b = row_scores(rows, gt, from_probs)[1]
    return float(b.mean()) if b.size else float("nan")


def classwise_bin_statistics(probs, gt, n_bins: int = 10, unscorable=None) -> np.ndarray:
    """float64 [3, C, n_bins + 1] = (count, sum_conf, hits): element (i, c) counts in bin ``digitize_bins(p_ic)`` of class c -- below 0
    in bin 0, as the device's rule clamps --, adds p_ic clamped to [0, 1] to sum_conf and, when c == y_i, 1 to hits.  The elements of
    an ``unscorable`` row (bool [N]) count in bin n_bins, hit nothing and add nothing, as on the device."""
    p = np.asarray(probs, dtype=np.float64)
    gt = np.asarray(gt).astype(np.int64).reshape(-1)
    N, C = p.shape
    bad = np.zeros(N, bool) if unscorable is None else np.asarray(unscorable, bool)
    which = np.maximum(digitize_bins(p, n_bins), 0)
    which[bad] = n_bins
    cls = np.broadcast_to(np.arange(C), (N, C))
    out = np.zeros((3, C, n_bins + 1))
    np.add.at(out[0], (cls, which), 1.0)
    np.add.at(out[1], (cls, which), np.where(bad[:, None], 0.0, np.clip(np.nan_to_num(p), 0.0, 1.0)))
    hit = (gt >= 0) & (gt < C) & ~bad
    rows = np.nonzero(hit)[0]
    np.add.at(out[2], (gt[rows], which[rows, gt[rows]]), 1.0)
    return out


def classwise_fixed_point(probs, gt, n_bins: int = 10, unscorable=None) -> np.ndarray:
    """int64 [3, C, n_bins + 1]: ``classwise_bin_statistics`` as the device accumulates it -- every element adds
    round-half-even(clip(p, 0, 1) * 2^32) to sum_conf; integer sums, so exact and independent of the order."""
    p = np.asarray(probs, dtype=np.float64)
    N, C = p.shape
    bad = np.zeros(N, bool) if unscorable is None else np.asarray(unscorable, bool)
    st = classwise_bin_statistics(p, gt, n_bins, bad)
    which = np.maximum(digitize_bins(p, n_bins), 0)
    which[bad] = n_bins
    fx = np.rint(np.clip(np.nan_to_num(p), 0.0, 1.0) * CONF_FIXED_ONE).astype(np.int64)
    fx[bad] = 0
    out = np.zeros((3, C, n_bins + 1), dtype=np.int64)
    out[0], out[2] = st[0].astype(np.int64), st[2].astype(np.int64)
    np.add.at(out[1], (np.broadcast_to(np.arange(C), (N, C)), which), fx)
    return out


def classwise_from_bins(acc, n: int) -> float:
    """Class-wise ECE from [3, C, n_bins + 1] = (count, sum_conf, hits) over ``n`` rows:
    (1 / C) sum_c sum_b (n_cb / n) |hits_cb / n_cb - conf_cb / n_cb| = sum_cb |hits_cb - conf_cb| / (n C) over the n_bins intervals, with
    bin n_bins (p == 1.0) counted into the last one, as ``mce_from_bins`` does.  An integer ``acc`` is the device's block, whose sum_conf
    is 32.32 fixed point."""
    a = np.asarray(acc)
    if a.ndim != 3 or a.shape[0] != 3 or a.shape[2] < 2:
        raise ValueError(f"classwise_from_bins: acc {a.shape} is not [3, C, n_bins + 1]")
    conf = a[1].astype(np.float64) / CONF_FIXED_ONE if np.issubdtype(a.dtype, np.integer) else a[1].astype(np.float64)
    hits = a[2].astype(np.float64)
    conf = np.concatenate([conf[:, :-2], conf[:, -2:].sum(axis=1, keepdims=True)], axis=1)
    hits = np.concatenate([hits[:, :-2], hits[:, -2:].sum(axis=1, keepdims=True)], axis=1)
    if n < 1:
        return float("nan")
    return float(np.abs(hits - conf).sum(axis=1).sum() / n / a.shape[1])


def ClasswiseECE(probs, gt, n_bins: int = 10) -> float:
    """Class-wise expected calibration error of probability rows (Kull et al. 2019; Nixon et al.'s static calibration error): every
    class's probabilities are binned on their own and the classes' gaps averaged."""
    p = np.asarray(probs, dtype=np.float64)
    return classwise_from_bins(classwise_bin_statistics(p, gt, n_bins, unscorable_rows(p, True)), p.shape[0])
