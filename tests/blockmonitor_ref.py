"""The row-chunked validation score (csrc/fit_monitor.hip: clipmi_val_score_rows, clipmi_val_score_finish) restated in numpy float64,
on top of tests/fitmonitor_ref.py: the row result, the finish's order of additions -- 64-row partial records in ascending row order, then
the partials in ascending order -- and the chunkings the tests cut a set into."""
import numpy as np

import fitmonitor_ref as ref
from clip_calibration_amd import metrics

ROWS_PER_PARTIAL = 64     # csrc/fit_monitor.hip VS_ROWS
ROW_DTYPE = np.dtype([("conf", "<f8"), ("nll", "<f8"), ("hit", "<i4"), ("bin", "<i4")])


def row_results(logits, labels, n_bins):
    """One result per row: confidence, nll, hit and the confidence's digitize bin (a NaN sorts into the last)."""
    hit, nll, conf = ref.score_rows(logits, labels)
    out = np.zeros(len(hit), ROW_DTYPE)
    out["conf"], out["nll"], out["hit"], out["bin"] = conf, nll, hit, metrics.digitize_bins(conf, n_bins)
    return out


def _partial(rows, n_bins):
    p = {"n": 0, "correct": 0, "nll_sum": 0.0, "count": np.zeros(n_bins + 1, np.int64), "hits": np.zeros(n_bins + 1, np.int64),
         "conf_sum": np.zeros(n_bins + 1)}
    with np.errstate(all="ignore"):
        for r in rows:              # ascending row order
            p["n"] += 1
            p["correct"] += int(r["hit"])
            p["nll_sum"] += float(r["nll"])
            b = int(r["bin"])
            p["count"][b] += 1
            p["hits"][b] += int(r["hit"])
            p["conf_sum"][b] += float(r["conf"])
    return p


def finish(rows, n_bins):
    """The record of the row results in the kernel's order: one partial per 64 rows, the partials added in ascending order."""
    parts = [_partial(rows[k:k + ROWS_PER_PARTIAL], n_bins) for k in range(0, len(rows), ROWS_PER_PARTIAL)]
    out = _partial(rows[:0], n_bins)
    with np.errstate(all="ignore"):
        for p in parts:
            for k in out:
                out[k] = out[k] + p[k]
    out["nll_sum"] = float(out["nll_sum"])
    return out


def chunkings(N):
    """name -> chunk sizes that sum to N: one chunk; chunks of 1; (5, 59, 1, rest), a seam on row 64; (64, 64, ...); (63, 2, rest),
    a chunk that straddles the seam.  A prescribed head that does not fit into N is cut off at N."""
    def cut(head):
        out, left = [], N
        for h in head:
            if left <= 0:
                break
            out.append(min(h, left))
            left -= out[-1]
        if left > 0:
            out.append(left)
        return out
    return {"one": [N], "ones": [1] * N, "seam": cut([5, 59, 1]), "partials": cut([64] * (N // 64)), "straddle": cut([63, 2])}


def chunked_record(logits, labels, n_bins, sizes):
    """The record of the set scored chunk by chunk."""
    assert sum(sizes) == len(labels)
    parts, lo = [], 0
    for s in sizes:
        parts.append(row_results(logits[lo:lo + s], labels[lo:lo + s], n_bins))
        lo += s
    return finish(np.concatenate(parts), n_bins)


def sum_bound(terms):
    """Two float64 sums of the same ``terms`` in different orders differ by at most (n - 1) 2^-52 sum |terms| (each of the n - 1 additions
    of either order rounds by at most 2^-53 of a partial sum no larger than sum |terms|)."""
    t = np.asarray(terms, np.float64)
    return max(len(t) - 1, 0) * 2.0 ** -52 * float(np.abs(t).sum())
