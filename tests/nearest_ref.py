"""float64 numpy restatement of clipmi_nearest_rows (include/clipmi.h): distances in difference form from the fp32 inputs, a stable
argsort (ties to the lower index), NaN treated as +inf.  Small shapes form the whole matrix; large ones go query by query."""
import numpy as np


def sq_dists(q, refs):
    """sum_e (q_e - r_e)^2 in float64, [Nq, Nr]; NaN -> +inf."""
    q64, r64 = np.asarray(q, dtype=np.float64), np.asarray(refs, dtype=np.float64)
    out = np.empty((q64.shape[0], r64.shape[0]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(q64.shape[0]):
            diff = r64 - q64[i]
            out[i] = np.einsum("re,re->r", diff, diff)
    out[np.isnan(out)] = np.inf
    return out


def nearest_rows(q, refs, k):
    """(dist float64 [Nq, k] -- the distance, not its square --, idx int64 [Nq, k], sq float64 [Nq, Nr])."""
    sq = sq_dists(q, refs)
    idx = np.argsort(sq, axis=1, kind="stable")[:, :k]
    return np.sqrt(np.take_along_axis(sq, idx, axis=1)), idx, sq
