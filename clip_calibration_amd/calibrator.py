"""VLCalibration (reference trainers/calibration/vl_calibrator.py:27-121, 170-200): optional Distance-Aware Calibration of the
logits, softmax, then optionally ProCal, the proximity-informed density-ratio calibrator (procal.py):

| base_calibration_mode | procal_flag | base calibrator                                       |
| "scaling_based"       | True        | DensityRatioCalibration                               |
| "scaling_based"       | False       | none (DAC -> softmax)                                 |
| None                  | either      | none (DAC -> softmax)                                 |
| "bin_based"           | either      | refused: its calibrators need netcal (NotImplementedError) |

Any other mode is refused as well rather than silently skipped."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import ops
from .dac import DistanseAwareCalibration
from .procal import DensityRatioCalibration

TEXT_FEATURE_KEYS = ("base_text_features_zs", "current_text_features_zs", "base_text_features_tuned",
                     "current_text_features_tuned")


class VLCalibration:
    def __init__(self, val_dict: Dict[str, np.ndarray], text_feature_dict: Optional[Dict[str, np.ndarray]] = None,
                 dac_flag: bool = False, k_dac: int = 5, base_calibration_mode: Optional[str] = None, procal_flag: bool = False):
        if base_calibration_mode not in (None, "scaling_based"):
            raise NotImplementedError(f"base_calibration_mode={base_calibration_mode!r}: only None and 'scaling_based' are built "
                                      "(the bin_based calibrators need netcal)")
        self.base_calibration_mode, self.procal_flag = base_calibration_mode, bool(procal_flag)
        self.dac_flag, self.k_dac = dac_flag, k_dac
        self.text_feature_dict = text_feature_dict
        self.val_logits = np.asarray(val_dict["val_logits"])
        self.val_labels = np.asarray(val_dict["val_labels"])
        self.val_image_features = np.asarray(val_dict["val_image_features"])
        self.val_image_knn_dists = np.asarray(val_dict["val_image_knn_dists"])
        self.val_image_proximity = np.exp(-np.mean(self.val_image_knn_dists, axis=-1))     # vl_calibrator.py:69
        self.dac_calibrator: Optional[DistanseAwareCalibration] = None
        self.base_calibrator: Optional[DensityRatioCalibration] = None

    @property
    def procal_active(self) -> bool:
        """vl_calibrator.py:114-117: the density-ratio calibrator is built on 'scaling_based' with procal_flag only."""
        return self.base_calibration_mode == "scaling_based" and self.procal_flag

    def fit(self) -> None:
        """vl_calibrator.py:72-80 + build_dac_calibrator :170-200 + build_base_calibrator :112-121."""
        self.dac_calibrator = None
        self.base_calibrator = None
        if self.dac_flag:
            t = self.text_feature_dict
            if t is None or any(k not in t for k in TEXT_FEATURE_KEYS):
                raise KeyError(f"DAC needs text_feature_dict with {TEXT_FEATURE_KEYS}")
            self.dac_calibrator = DistanseAwareCalibration()
            self.dac_calibrator.fit(t["base_text_features_zs"], t["current_text_features_zs"],
                                    t["base_text_features_tuned"], t["current_text_features_tuned"], k=self.k_dac)
        if self.procal_active:   # vl_calibrator.py:60-62: softmax of the val logits, NO DAC on val
            lg = self.val_logits.astype(np.float64)
            e = np.exp(lg - lg.max(axis=1, keepdims=True))
            val_probs = e / e.sum(axis=1, keepdims=True)
            self.base_calibrator = DensityRatioCalibration()
            self.base_calibrator.fit(val_probs, val_probs.argmax(axis=1), self.val_labels, self.val_image_proximity)

    def class_confidence_device(self, device="cuda") -> Optional[torch.Tensor]:
        """The per-class DAC factor as the fused logits kernel takes it (None when DAC is off)."""
        return None if self.dac_calibrator is None else self.dac_calibrator.class_confidence_device(device)

    def procal_device(self) -> Optional[DensityRatioCalibration]:
        """The fitted ProCal calibrator when ProCal is on (None otherwise); raises if it is on but fit() has not run."""
        if not self.procal_active:
            return None
        if self.base_calibrator is None:
            raise RuntimeError("VLCalibration: ProCal is on; call fit() first")
        return self.base_calibrator

    def predict(self, logits, test_proximity=None) -> np.ndarray:
        """vl_calibrator.py:83-109: numpy [N,C] logits -> calibrated probabilities (float32: the DAC step already rounds to fp32
        in the reference, and the row softmax runs in fp32 on the device).  With ProCal: DAC -> softmax -> ProCal in one launch,
        and ``test_proximity`` (one entry per row) is required."""
        logits = np.asarray(logits)
        procal = self.procal_device()
        if procal is not None and test_proximity is None:
            raise AssertionError("ProCal needs test_proximity")
        if test_proximity is not None and logits.shape[0] != np.asarray(test_proximity).shape[0]:
            raise AssertionError(f"Shape mismatch: logits shape {logits.shape[0]} != test_proximity shape {np.asarray(test_proximity).shape[0]}")
        lg = torch.from_numpy(logits).float().cuda()
        if procal is not None:
            prox = torch.from_numpy(np.asarray(test_proximity, dtype=np.float32)).to(lg.device)
            return procal.predict_device(lg, prox, self.class_confidence_device(lg.device), want_probs=True)[0].cpu().numpy()
        return ops.softmax_rows(lg, self.class_confidence_device(lg.device)).cpu().numpy()
