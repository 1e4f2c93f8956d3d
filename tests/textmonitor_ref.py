"""The inference expressions the CoCoOp and ProDA fit monitors score, restated in float64 from the reference's eval forwards
(cocoop.py:186-199; proda.py:316-331 set_classifier, 304-313 forward).  Both start from the text tower's raw outputs, which the GPU tests
take from the trainers' own inference path: the tower itself is held to its oracle elsewhere (tests/test_gpu_text_ops.py).

Error bounds (u = 2^-24, fp32's unit roundoff; first order, times tail_ref.MARGIN):

* ``cocoop_logit_bound``: the device forms ``scale * dot * inv`` with ``dot = sum_e t_e f_e`` and ``ss = sum_e t_e^2`` added lane-strided
  and by a butterfly -- any order of E additions errs by at most (E - 1) u sum |terms| --, ``inv = 1 / sqrt(ss)`` (ss carries E u
  relative, the root halves it, root and reciprocal add 2 u) and two products (2 u): |dz| <= (E + E / 2 + 4) u |scale| S / |t| with
  S = sum |t_e f_e| <= |t| |f| and |f| = 1 up to its own normalisation, (E / 2 + 2) u relative.  Together below (2 E + 8) u |scale|.
* ``mean_bound``: with m = max_p |u_{p,e}| over a class's unit rows u_p = t_p / |t_p|, an element of a unit row carries (E / 2 + 3) u
  relative (its norm, the root, the reciprocal, the product).  The P elements are added one by one from zero: the k-th partial sum is at
  most k m and rounds by at most u k m, u m P (P + 1) / 2 over the P additions, u m (P + 1) / 2 after the division by P, which rounds once
  more: at most (P + 1) u m for the accumulation -- "P fp32 roundings" -- beside the rows' own (E / 2 + 3) u m.
"""
import numpy as np

import fitmonitor_ref as ref
from tail_ref import MARGIN, U


def unit(x):
    x = np.asarray(x, np.float64)
    return x / np.sqrt((x * x).sum(axis=-1, keepdims=True))


def cocoop_logits(features, txt, scale):
    """cocoop.py:186-199: ``features`` raw image features [N, E], ``txt`` the N images' own raw text features [N, C, E] ->
    float64 logits [N, C] = scale * <x_n, t_{n,c} / |t_{n,c}|>."""
    return float(np.float32(scale)) * np.einsum("ne,nce->nc", unit(features), unit(txt))


def cocoop_logit_bound(E, scale):
    return (2 * E + 8) * U * abs(float(np.float32(scale))) * MARGIN


def proda_mean(text, P):
    """proda.py:324-331: raw text features [C P, E], a class's P rows together -> the per-class mean of the unit rows, NOT renormalised."""
    u = unit(text)
    return u.reshape(-1, P, u.shape[-1]).mean(axis=1)


def mean_bound(text, P):
    """Per element [C, E]: the bound of the module docstring on a device mean of these rows."""
    u = np.abs(unit(text)).reshape(-1, P, np.asarray(text).shape[-1])
    E = u.shape[-1]
    return ((P + 1) + (E / 2 + 3)) * U * u.max(axis=1) * MARGIN


def proda_logits(features, text, P, scale):
    """proda.py:304-313 on set_classifier's means: float64 logits [N, C] = scale * x_n . mean_c."""
    return float(np.float32(scale)) * unit(features) @ proda_mean(text, P).T


def record(logits64, labels, n_bins):
    """The epoch record of float64 logits (tests/fitmonitor_ref.py's rules)."""
    return ref.record(np.asarray(logits64, np.float64), labels, n_bins)


def worse(later, earlier):
    """``later`` is strictly worse than ``earlier`` under both criteria: fewer correct rows, and an nll_sum that is larger or not finite."""
    nll_worse = (not np.isfinite(later["nll_sum"])) or later["nll_sum"] > earlier["nll_sum"]
    return later["correct"] < earlier["correct"] and nll_worse and np.isfinite(earlier["nll_sum"])
