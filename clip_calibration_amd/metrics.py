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
