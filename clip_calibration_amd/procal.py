"""ProCal, the proximity-informed density-ratio calibrator (reference trainers/calibration/density_ratio_calibration.py:28-117), the
base calibrator VLCalibration builds on ``base_calibration_mode="scaling_based"`` with ``procal_flag`` (vl_calibrator.py:112-121).

``fit`` stays on the host in float64: it is O(N_val) and reproduces statsmodels' ``KDEMultivariate(var_type='cc',
bw='normal_reference')`` bandwidths exactly (h = 1.06 * std(x, ddof=0) * n^(-1/6) per set and dimension, _kernel_base.py:250-265).
The two point sets are uploaded once per device, pre-scaled for the kernel (csrc/procal.hip).  The evaluation -- the reference's
Python loop of one float64 numpy pass over the val samples per test sample -- is one HIP launch (``clipmi_procal_rows``).

Defined where the reference is not:
* ``fit`` raises ValueError when the correct or the incorrect set has fewer than 2 points or no spread in a dimension (the reference
  divides by a zero bandwidth);
* the rest of a row is rescaled as ``probs[j] * (1 - c*) / S`` with the ratio probs[j] / S formed from the logits, so it never
  underflows; a row whose other probabilities are exactly 0 (a single class, or every other logit -inf) keeps them at 0 -- the
  reference computes 0 / 0 = NaN there.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib, ops

# 2^(-(x k)^2) = exp(-x^2 / (2 h^2)) for k = sqrt(log2(e) / 2) / h
_EXP2_SCALE = math.sqrt(math.log2(math.e) / 2.0)


def normal_reference_bandwidth(points: np.ndarray) -> np.ndarray:
    """statsmodels _kernel_base.py:250-265 (``_normal_reference``): 1.06 * std(ddof=0) * n^(-1/(4 + d)), d = 2 here."""
    points = np.asarray(points, dtype=np.float64)
    n, d = points.shape
    return 1.06 * np.std(points, axis=0) * n ** (-1.0 / (4 + d))


class DensityRatioCalibration:
    def __init__(self):
        self.data_true: Optional[np.ndarray] = None    # float64 [n_T, 2]: (conf, proximity) of the correctly classified val samples
        self.data_false: Optional[np.ndarray] = None
        self.bw_true: Optional[np.ndarray] = None      # (h_conf, h_proximity)
        self.bw_false: Optional[np.ndarray] = None
        self.false_true_ratio: Optional[float] = None
        self._dev = None                               # (device, ProcalModel, point tensors kept alive)

    def fit(self, probs, preds, true, proximity) -> None:
        """density_ratio_calibration.py:34-79: split the val samples into correct / incorrect, fit a 2-D Gaussian KDE on
        (max prob, proximity) of each, and keep |F| / |T|."""
        probs = np.asarray(probs, dtype=np.float64)
        if not (np.all(probs >= 0) and np.all(probs <= 1)):
            raise AssertionError("All elements in 'probs' should be in the range [0, 1].")
        conf = probs.max(axis=-1)
        correct = np.asarray(preds) == np.asarray(true)
        prox = np.asarray(proximity, dtype=np.float64)
        if prox.shape != conf.shape or correct.shape != conf.shape:
            raise ValueError(f"fit: probs {probs.shape}, preds / true {correct.shape} and proximity {prox.shape} disagree")
        pts = np.stack([conf, prox], axis=1)
        sets = {}
        for name, mask in (("correct", correct), ("incorrect", ~correct)):
            s = pts[mask]
            if s.shape[0] < 2:
                raise ValueError(f"ProCal fit: the {name} val samples number {s.shape[0]}; the density needs at least 2")
            bw = normal_reference_bandwidth(s)
            if not np.all(bw > 0):
                raise ValueError(f"ProCal fit: the {name} val samples have no spread in "
                                 f"{'confidence' if bw[0] <= 0 else 'proximity'}; the density is undefined")
            sets[name] = (s, bw)
        (self.data_true, self.bw_true), (self.data_false, self.bw_false) = sets["correct"], sets["incorrect"]
        self.false_true_ratio = float(self.data_false.shape[0]) / float(self.data_true.shape[0])
        self._dev = None

    def device_model(self, device="cuda") -> "_lib.ProcalModel":
        """The fitted sets as csrc/procal.hip takes them, uploaded once per device: point (c, p) of a set becomes (c k_c, p k_p) in
        fp64, k = sqrt(log2 e / 2) / h (the kernel scales the query by the same k)."""
        if self.data_true is None:
            raise RuntimeError("DensityRatioCalibration: call fit() first")
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._dev is not None and self._dev[0] == device:
            return self._dev[1]
        m = _lib.ProcalModel()
        keep = []
        for k, (data, bw) in enumerate(((self.data_true, self.bw_true), (self.data_false, self.bw_false))):
            scale = _EXP2_SCALE / bw
            t = torch.from_numpy(np.ascontiguousarray(data * scale)).to(device)
            keep.append(t)
            for d in range(2):
                m.scale[k][d] = float(scale[d])
            m.norm[k] = 1.0 / (data.shape[0] * bw[0] * bw[1] * 2.0 * math.pi)
        m.points_true, m.points_false = keep[0].data_ptr(), keep[1].data_ptr()
        m.n_true, m.n_false = self.data_true.shape[0], self.data_false.shape[0]
        m.ratio = self.false_true_ratio
        self._dev = (device, m, keep)
        return m

    def predict_device(self, logits: torch.Tensor, proximity: torch.Tensor, dac_conf: Optional[torch.Tensor] = None,
                       want_probs: bool = False):
        """softmax(DAC(logits)) -> ProCal on device tensors, then the evaluator's top-1 of the calibrated rows: returns
        (calibrated probs fp32 [N,C] or None, conf' fp32 [N], pred' int32 [N]).  No host synchronisation."""
        prox = torch.as_tensor(proximity, device=logits.device).float()
        probs, conf, pred, _ = ops.procal_rows(self.device_model(logits.device), logits, prox, dac_conf, want_probs=want_probs)
        return probs, conf, pred

    def predict(self, probs, proximities) -> np.ndarray:
        """density_ratio_calibration.py:82-117 on numpy probability rows (each summing to 1): rows are handed to the device as
        log-probabilities, whose softmax is the row itself up to fp32 rounding; returns the calibrated rows (float32)."""
        probs = np.asarray(probs, dtype=np.float64)
        if not (np.all(probs >= 0) and np.all(probs <= 1)):
            raise AssertionError("All elements in 'probs' should be in the range [0, 1].")
        with np.errstate(divide="ignore"):
            lg = np.log(probs).astype(np.float32)
        lg_d = torch.from_numpy(lg).cuda()
        prox = torch.from_numpy(np.asarray(proximities, dtype=np.float32)).to(lg_d.device)
        out, _, _ = self.predict_device(lg_d, prox, want_probs=True)
        return out.cpu().numpy()
