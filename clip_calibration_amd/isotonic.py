"""Multi-class isotonic calibration and Bin-Mean-Shift (reference trainers/calibration/multi_isotonic_regression.py and
multi_proximity_isotonic.py:130-247), the base calibrators VLCalibration builds on ``base_calibration_mode="bin_based"`` with
``base_bin_calibrator_name="multi_isotonic_regression"`` (vl_calibrator.py:121-147; ``procal_flag`` picks Bin-Mean-Shift).

What the reference computes: the calibrator is handed p = softmax(logits) and softmaxes it AGAIN, x = exp(p) / sum_j exp(p_j) per row
(float32); one sklearn ``IsotonicRegression(out_of_bounds="clip")`` is fitted on the N * C pairs (x_ij, onehot_ij); a row is calibrated
as g(x) + 1e-9 x, g being linear interpolation through the fitted thresholds, clipped outside them.  Rows are not renormalised.
Bin-Mean-Shift cuts the val proximities at their quantiles (``np.percentile(proximity, linspace(0, 100, bins + 1))``), files a sample
under ``searchsorted(edges[1:-1], proximity, side="right")`` and keeps one such calibrator per bin.

The fit here (csrc/isotonic.hip): a constant block of an isotonic fit to 0/1 targets can only start at a point followed
by a 1, so the solution is determined by the N positive keys (x at the label) and per-gap statistics of the zeros.  One small launch
writes the positive keys, the host sorts and de-duplicates them, a second launch accumulates, per gap between consecutive keys, the
count, smallest and largest zero, and per key the zeros and positives equal to it.  ``pool_gap_statistics`` pools those <= 2 m + 1
weighted points with the stack algorithm in float64: the EXACT isotonic solution on the float32 x values.  The reference as run lets
sklearn pool in float32 (block weights up to 10^6) and merges x values closer than 1e-6; its function differs from the exact one by up
to 0.2 at isolated points, which is the noise level the tests hold this module to.

Defined where the reference is not:
* a proximity bin without val rows (sklearn raises on the empty input) -> ValueError from the fit;
* a proximity bin without test rows is no special case (the reference concatenates an empty prediction);
* non-finite val logits, or a label outside the classes -> ValueError from the fit.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops


def pool_gap_statistics(keys, positives, zeros_equal, gap_count, gap_min, gap_max) -> Tuple[np.ndarray, np.ndarray]:
    """The isotonic fit from gap statistics: ``keys`` [m] the sorted distinct positive keys, ``positives`` / ``zeros_equal`` [m] how many
    ones / zeros sit at each key, ``gap_count`` / ``gap_min`` / ``gap_max`` [m + 1] the zeros strictly between key g-1 and key g.
    Pool-adjacent-violators over the weighted points in ascending x (a pooled block whose mean is not below its successor's absorbs it),
    block sums in float64 (integers: exact).  Returns sklearn's (X_thresholds_, y_thresholds_): per block its smallest and largest x
    (one point if they coincide) with the block mean."""
    keys = np.asarray(keys, dtype=np.float64)
    m = keys.shape[0]
    pts = []   # (weight, sum of targets, smallest x, largest x)
    for g in range(m + 1):
        if gap_count[g] > 0:
            pts.append((float(gap_count[g]), 0.0, float(gap_min[g]), float(gap_max[g])))
        if g < m:
            pts.append((float(positives[g]) + float(zeros_equal[g]), float(positives[g]), keys[g], keys[g]))
    blocks: List[list] = []
    for w, s, lo, hi in pts:
        blocks.append([w, s, lo, hi])
        while len(blocks) > 1 and blocks[-2][1] / blocks[-2][0] >= blocks[-1][1] / blocks[-1][0]:
            w2, s2, _, hi2 = blocks.pop()
            blocks[-1][0] += w2
            blocks[-1][1] += s2
            blocks[-1][3] = hi2
    X, Y = [], []
    for w, s, lo, hi in blocks:
        X.append(lo)
        Y.append(s / w)
        if hi != lo:
            X.append(hi)
            Y.append(s / w)
    return np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)


def split_gap_statistics(stats: np.ndarray, key_offset: Sequence[int], b: int):
    """Bin b's slices of the device statistics (include/clipmi.h, clipmi_isotonic_gap_stats): (positives, zeros_equal, gap_count,
    gap_min, gap_max), the extrema as float32 values."""
    m = key_offset[b + 1] - key_offset[b]
    base = 3 * key_offset[b] + b
    cnt = stats[0]
    as_f32 = lambda plane: np.ascontiguousarray(plane[base:base + m + 1]).view(np.float32)
    return (cnt[base + 2 * m + 1:base + 3 * m + 1], cnt[base + m + 1:base + 2 * m + 1], cnt[base:base + m + 1],
            as_f32(stats[1]), as_f32(stats[2]))


def fit_tables_device(logits: torch.Tensor, labels: torch.Tensor, bin_index: Optional[np.ndarray] = None, n_bins: int = 1,
                      from_probs: bool = False) -> List[Tuple[np.ndarray, np.ndarray]]:
    """One (X_thresholds_, y_thresholds_) pair per bin from device logits [N, C] fp32 and labels [N] int64: the two launches of
    csrc/isotonic.hip around the host's sort of the positive keys, then the float64 pooling."""
    N = logits.shape[0]
    bins = np.zeros(N, dtype=np.int64) if bin_index is None else np.asarray(bin_index, dtype=np.int64)
    if bins.shape != (N,):
        raise ValueError(f"isotonic fit: {N} rows but bin index of shape {bins.shape}")
    counts = np.bincount(bins, minlength=n_bins)
    if counts.shape[0] != n_bins or np.any(counts == 0):
        empty = [int(b) for b in np.nonzero(counts[:n_bins] == 0)[0]]
        raise ValueError(f"isotonic fit: proximity bin(s) {empty} hold no val rows ({n_bins} bins over {N} rows)")
    keys = ops.isotonic_keys(logits, labels, from_probs=from_probs).cpu().numpy()
    if not np.all(np.isfinite(keys)):
        raise ValueError("isotonic fit: non-finite val logits, or a label outside the classes")
    per_bin = [np.unique(keys[bins == b]) for b in range(n_bins)]
    key_offset = [0] + [int(v) for v in np.cumsum([k.shape[0] for k in per_bin])]
    keys_d = torch.from_numpy(np.concatenate(per_bin)).to(logits.device)
    bin_d = None if n_bins == 1 else torch.from_numpy(bins.astype(np.int32)).to(logits.device)
    stats, status = ops.isotonic_gap_stats(logits, labels, keys_d, key_offset, bin_d, from_probs=from_probs)
    stats, status = stats.cpu().numpy(), int(status.item())
    if status & 2:
        raise ValueError("isotonic fit: non-finite val logits")
    if status:
        raise RuntimeError(f"isotonic fit: the device statistics are inconsistent (status {status})")
    return [pool_gap_statistics(per_bin[b], *split_gap_statistics(stats, key_offset, b)) for b in range(n_bins)]


def pack_tables(tables: Sequence[Tuple[np.ndarray, np.ndarray]]) -> np.ndarray:
    """clipmi_isotonic_pack: the tables checked (finite, X strictly ascending) and laid out as the kernel reads them."""
    x = np.ascontiguousarray(np.concatenate([np.asarray(t[0], dtype=np.float64) for t in tables]))
    y = np.ascontiguousarray(np.concatenate([np.asarray(t[1], dtype=np.float64) for t in tables]))
    for X, Y in tables:
        if np.shape(X) != np.shape(Y) or np.ndim(X) != 1:
            raise ValueError("isotonic tables: X and y must be equal 1-d arrays")
    counts = (ctypes.c_int32 * len(tables))(*[len(t[0]) for t in tables])
    packed = np.empty(3 * x.shape[0], dtype=np.float64)
    _lib.check(_lib.lib.clipmi_isotonic_pack(x.ctypes.data, y.ctypes.data, counts, len(tables), packed.ctypes.data), "clipmi_isotonic_pack")
    return packed


class _Tables:
    """Fitted state shared by the two calibrators: plain numpy tables, uploaded once per device."""

    def __init__(self):
        self._tables: Optional[List[Tuple[np.ndarray, np.ndarray]]] = None
        self._inner_edges: np.ndarray = np.zeros(0)
        self._dev = None   # (device, IsotonicModel, table tensor kept alive)

    def _set(self, tables, inner_edges=()):
        self._tables = [(np.asarray(X, np.float64), np.asarray(Y, np.float64)) for X, Y in tables]
        self._inner_edges = np.asarray(inner_edges, dtype=np.float64)
        self._dev = None

    def device_model(self, device="cuda") -> "_lib.IsotonicModel":
        if self._tables is None:
            raise RuntimeError(f"{type(self).__name__}: fit first")
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._dev is not None and self._dev[0] == device:
            return self._dev[1]
        if len(self._tables) > _lib.ISOTONIC_MAX_TABLES:
            raise ValueError(f"isotonic: {len(self._tables)} tables (at most {_lib.ISOTONIC_MAX_TABLES})")
        t = torch.from_numpy(pack_tables(self._tables)).to(device)
        m = _lib.IsotonicModel()
        m.table, m.n_tables = t.data_ptr(), len(self._tables)
        off = 0
        for i, (X, _) in enumerate(self._tables):
            off += X.shape[0]
            m.offset[i + 1] = off
        for i, e in enumerate(self._inner_edges):
            m.edges[i] = float(e)
        self._dev = (device, m, t)
        return m

    def predict_device(self, logits: torch.Tensor, proximity=None, dac_conf: Optional[torch.Tensor] = None, want_probs: bool = False,
                       from_probs: bool = False):
        """softmax(DAC(logits)) -> the calibrator on device tensors, then the evaluator's top-1 of the calibrated rows: returns
        (calibrated rows fp32 [N,C] or None, conf fp32 [N], pred int32 [N]).  One launch, no host synchronisation."""
        model = self.device_model(logits.device)
        prox = None
        if model.n_tables > 1:
            if proximity is None:
                raise AssertionError("Bin-Mean-Shift needs the proximity of every row")
            prox = torch.as_tensor(proximity, device=logits.device).float()
        probs, conf, pred, _ = ops.isotonic_rows(model, logits, prox, dac_conf, want_probs=want_probs, from_probs=from_probs)
        return probs, conf, pred

    def _transform(self, probs, proximity=None) -> np.ndarray:
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(probs, dtype=np.float32))).cuda()
        prox = None if proximity is None else torch.from_numpy(np.asarray(proximity, dtype=np.float32)).to(p.device)
        return self.predict_device(p, prox, want_probs=True, from_probs=True)[0].cpu().numpy()


def _labels_1d(label, n_classes: int) -> np.ndarray:
    """The reference takes class indices or one-hot rows; one-hot rows are read back as indices."""
    label = np.asarray(label)
    if label.ndim == 2:
        if label.shape[1] != n_classes or not np.all(label.sum(axis=1) == 1):
            raise ValueError("isotonic fit: 2-d labels must be one-hot rows")
        label = label.argmax(axis=1)
    label = label.astype(np.int64).reshape(-1)
    if label.size and (label.min() < 0 or label.max() >= n_classes):
        raise ValueError(f"isotonic fit: labels outside [0, {n_classes})")
    return label


class MultiIsotonicRegression(_Tables):
    """multi_isotonic_regression.py: one isotonic function for every class.  Fitted state: ``X_thresholds_``, ``y_thresholds_``."""

    @property
    def X_thresholds_(self) -> np.ndarray:
        return self._tables[0][0]

    @property
    def y_thresholds_(self) -> np.ndarray:
        return self._tables[0][1]

    def set_thresholds(self, X, y) -> None:
        """Install a given table (tests; restoring a saved calibrator)."""
        self._set([(X, y)])

    def fit_device(self, logits: torch.Tensor, labels, from_probs: bool = False) -> None:
        labels = _labels_1d(labels.cpu().numpy() if isinstance(labels, torch.Tensor) else labels, logits.shape[1])
        if logits.shape[0] == 0:
            raise ValueError("isotonic fit: no val rows")
        self._set(fit_tables_device(logits.float(), torch.from_numpy(labels).to(logits.device), from_probs=from_probs))

    def fit_transform(self, logit, label) -> np.ndarray:
        """The reference's signature: ``logit`` holds probabilities [N, C] (vl_calibrator.py:147 passes the val softmax)."""
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(logit, dtype=np.float32))).cuda()
        self.fit_device(p, label, from_probs=True)
        return self.predict_device(p, want_probs=True, from_probs=True)[0].cpu().numpy()

    def transform(self, logit) -> np.ndarray:
        return self._transform(logit)


class BinMeanShift(_Tables):
    """multi_proximity_isotonic.py:130-247 with method 'multi_isotonic_regression', bin_strategy 'quantile', normalize_conf False.
    Fitted state: ``bin_edges`` [proximity_bin + 1] and one ``MultiIsotonicRegression`` per bin in ``calibrators``."""

    def __init__(self, proximity_bin: int = 5):
        super().__init__()
        if not 1 <= proximity_bin <= _lib.ISOTONIC_MAX_TABLES:
            raise ValueError(f"proximity_bin={proximity_bin} (1 .. {_lib.ISOTONIC_MAX_TABLES})")
        self.proximity_bin = proximity_bin
        self.bin_edges: Optional[np.ndarray] = None
        self.calibrators: List[MultiIsotonicRegression] = []

    def bin_index(self, proximity) -> np.ndarray:
        return np.searchsorted(self.bin_edges[1:-1], np.asarray(proximity), side="right")

    def set_thresholds(self, bin_edges, tables) -> None:
        self.bin_edges = np.asarray(bin_edges, dtype=np.float64)
        if self.bin_edges.shape != (self.proximity_bin + 1,) or len(tables) != self.proximity_bin:
            raise ValueError("BinMeanShift: one table per bin and proximity_bin + 1 edges")
        self._set(tables, self.bin_edges[1:-1])
        self.calibrators = []
        for X, Y in self._tables:
            c = MultiIsotonicRegression()
            c.set_thresholds(X, Y)
            self.calibrators.append(c)

    def fit_device(self, logits: torch.Tensor, labels, proximity, from_probs: bool = False) -> None:
        labels = _labels_1d(labels.cpu().numpy() if isinstance(labels, torch.Tensor) else labels, logits.shape[1])
        proximity = np.asarray(proximity)
        if proximity.shape != (logits.shape[0],):
            raise ValueError(f"BinMeanShift fit: {logits.shape[0]} rows but proximity of shape {proximity.shape}")
        if logits.shape[0] == 0:
            raise ValueError("isotonic fit: no val rows")
        self.bin_edges = np.asarray(np.percentile(proximity, np.linspace(0, 100, self.proximity_bin + 1)))
        tables = fit_tables_device(logits.float(), torch.from_numpy(labels).to(logits.device), self.bin_index(proximity),
                                   self.proximity_bin, from_probs=from_probs)
        self.set_thresholds(self.bin_edges, tables)

    def fit_transform(self, logit, proximity, label) -> np.ndarray:
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(logit, dtype=np.float32))).cuda()
        self.fit_device(p, label, proximity, from_probs=True)
        return self._transform(logit, proximity)

    def transform(self, logit, proximity) -> np.ndarray:
        return self._transform(logit, proximity)
