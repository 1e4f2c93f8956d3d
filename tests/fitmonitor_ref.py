"""The fit monitor (csrc/fit_monitor.hip) restated in numpy float64: the row scoring, the epoch record, the selection rule and the ECE
from a record.  tests/test_fitmonitor_cpu.py holds it to torch and to clip_calibration_amd.metrics; the GPU tests hold the kernels to it.

The record as a dict: ``n``, ``correct``, ``nll_sum`` and, per bin of ``metrics.digitize_bins`` (n_bins + 1 of them, the last holding
conf == 1.0), ``count``, ``hits`` and ``conf_sum``.  The two defined outcomes: a label outside [0, C) counts as wrong with a NaN nll; a
row that holds a NaN counts as wrong with a NaN nll and a NaN confidence (which digitize sorts into the last bin)."""
import numpy as np

from clip_calibration_amd import metrics

EDGE_GUARD = 2.0 ** -20      # no confidence of a test input may lie this close (relative) to a bin edge without lying on it
FLOOR = 2.0 ** -22           # the relative floor of the fp32 sums' bound (the project's other fp32 fits use it)


def score_rows(logits, labels):
    """(hit bool [N], nll float64 [N], conf float64 [N]) of the fp32 ``logits`` [N, C] taken to float64."""
    z = np.asarray(logits).astype(np.float64)
    y = np.asarray(labels).astype(np.int64)
    N, C = z.shape
    with np.errstate(all="ignore"):
        has_nan = np.isnan(z).any(axis=1)
        safe = np.where(np.isnan(z), -np.inf, z)
        arg = np.argmax(safe, axis=1)                       # the first index of the maximum: the tie rule
        m = safe[np.arange(N), arg]
        s = np.exp(z - m[:, None]).sum(axis=1)
        lse = m + np.log(s)
        in_range = (y >= 0) & (y < C)
        zy = z[np.arange(N), np.where(in_range, y, 0)]
        nll = np.where(in_range, np.log(s) - (zy - m), np.nan)   # lse - z[y] with the maximum cancelled first
        conf = 1.0 / s                                      # exp(m - lse)
        del lse
    hit = in_range & (arg == y) & ~has_nan
    nll = np.where(has_nan, np.nan, nll)
    conf = np.where(has_nan, np.nan, conf)
    return hit, nll, conf


def record(logits, labels, n_bins):
    hit, nll, conf = score_rows(logits, labels)
    which = metrics.digitize_bins(conf, n_bins)
    count = np.bincount(which, minlength=n_bins + 1).astype(np.int64)
    hits = np.bincount(which, weights=hit.astype(np.float64), minlength=n_bins + 1).astype(np.int64)
    conf_sum = np.zeros(n_bins + 1)
    np.add.at(conf_sum, which, conf)
    return {"n": int(len(hit)), "correct": int(hit.sum()), "nll_sum": float(nll.sum()), "count": count, "hits": hits, "conf_sum": conf_sum}


def record_bins(rec):
    """float64 [3, n_bins + 1] = (count, sum_conf, sum_correct): what metrics.ece_from_bins takes."""
    return np.stack([rec["count"].astype(np.float64), rec["conf_sum"], rec["hits"].astype(np.float64)])


def ece(rec):
    return metrics.ece_from_bins(record_bins(rec), len(rec["count"]) - 1)


def select(records, criterion):
    """The best block after every epoch of ``records`` (dicts with ``correct`` and ``nll_sum``): a list of (best_epoch, best_correct,
    best_nll_sum, better).  Better iff strictly better; under "nll" a non-finite epoch is never better."""
    best_epoch, best_correct, best_nll = -1, -1, np.inf
    out = []
    for e, r in enumerate(records):
        if criterion == "accuracy":
            better = r["correct"] > best_correct
        else:
            better = bool(np.isfinite(r["nll_sum"]) and r["nll_sum"] < best_nll)
        if better:
            best_epoch, best_correct, best_nll = e, r["correct"], r["nll_sum"]
        out.append((best_epoch, best_correct, best_nll, better))
    return out


def best_epoch(records, criterion):
    return select(records, criterion)[-1][0] if records else -1


# the hand-written selection sequences: (name, [(correct, nll_sum), ...], best epoch under accuracy, best epoch under nll)
NAN = float("nan")
SEQUENCES = [
    ("strict improvement", [(3, 9.0), (5, 7.0), (4, 8.0)], 1, 1),
    ("tie keeps the earlier epoch", [(5, 7.0), (5, 7.0), (5, 7.0)], 0, 0),
    ("a NaN epoch in the middle", [(3, 9.0), (6, NAN), (4, 8.0)], 1, 2),
    ("a first epoch that is NaN", [(2, NAN), (1, 5.0), (1, 6.0)], 0, 1),
    ("every epoch NaN", [(0, NAN), (0, NAN)], 0, -1),
    ("an inf epoch", [(1, float("inf")), (1, 4.0)], 0, 1),
]


def off_the_edges(conf, n_bins):
    """True when no finite confidence lies within EDGE_GUARD (relative; absolute at the edge 0) of an edge of linspace(0, 1, n_bins + 1)
    without lying exactly on it."""
    c = np.asarray(conf, np.float64)
    c = c[np.isfinite(c)]
    edges = np.linspace(0, 1, n_bins + 1)
    d = np.abs(c[:, None] - edges[None, :])
    near = (d <= EDGE_GUARD * np.maximum(edges[None, :], 1.0 / n_bins)) & (d != 0)
    return not bool(near.any())


def clean_logits(N, C, n_bins, seed, scale=100.0):
    """fp32 logits [N, C] = scale * N(0, 1) and labels such that no row's float64 confidence lies near a bin edge without lying on it:
    a row that does is drawn again from a new seed, none is left out.  A confidence of exactly 1.0 lies on the edge and stays."""
    rng = np.random.default_rng(seed)
    z = (scale * rng.standard_normal((N, C))).astype(np.float32)
    labels = rng.integers(0, C, N)
    # half of the rows' labels are their arg-max, so that both outcomes occur
    labels[::2] = np.argmax(z[::2], axis=1)
    for i in range(N):
        tries = 0
        while not off_the_edges(score_rows(z[i:i + 1], labels[i:i + 1])[2], n_bins):
            tries += 1
            assert tries < 1000, "no clean row found"
            z[i] = (scale * np.random.default_rng([seed, i, tries]).standard_normal(C)).astype(np.float32)
            if i % 2 == 0:
                labels[i] = int(np.argmax(z[i]))
    assert off_the_edges(score_rows(z, labels)[2], n_bins)
    return z, labels.astype(np.int64)
