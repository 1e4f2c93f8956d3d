"""VLCalibration (reference trainers/calibration/vl_calibrator.py:27-121, 170-200): optional Distance-Aware Calibration of the
logits, softmax, then optionally a base calibrator: ProCal, the proximity-informed density-ratio calibrator (procal.py), or
multi-class isotonic regression, plain or proximity-binned (isotonic.py):

| base_calibration_mode | base_bin_calibrator_name    | procal_flag | base calibrator                                  |
| "scaling_based"       | ignored                     | True        | DensityRatioCalibration                          |
| "scaling_based"       | ignored                     | False       | none (DAC -> softmax)                            |
| None                  | ignored                     | either      | none (DAC -> softmax)                            |
| "bin_based"           | "multi_isotonic_regression" | False       | MultiIsotonicRegression                          |
| "bin_based"           | "multi_isotonic_regression" | True        | BinMeanShift (5 quantile bins of the proximity)  |
| "bin_based"           | "histogram_binning"         | either      | refused: a netcal class (NotImplementedError)    |
| "bin_based"           | "isotonic_regression"       | either      | refused: a netcal class (NotImplementedError)    |
| "bin_based"           | None / anything else        | either      | refused (NotImplementedError)                    |

Any other mode is refused as well rather than silently skipped."""
from __future__ import annotations

from typing import Dict, Optional, Union

import numpy as np
import torch

from . import ops
from .dac import DistanseAwareCalibration
from .isotonic import BinMeanShift, MultiIsotonicRegression
from .procal import DensityRatioCalibration

PROXIMITY_BINS = 5   # vl_calibrator.py:122

TEXT_FEATURE_KEYS = ("base_text_features_zs", "current_text_features_zs", "base_text_features_tuned",
                     "current_text_features_tuned")


class VLCalibration:
    def __init__(self, val_dict: Dict[str, np.ndarray], text_feature_dict: Optional[Dict[str, np.ndarray]] = None,
                 dac_flag: bool = False, k_dac: int = 5, base_calibration_mode: Optional[str] = None, procal_flag: bool = False,
                 base_bin_calibrator_name: Optional[str] = None):
        if base_calibration_mode == "bin_based":
            if base_bin_calibrator_name in ("histogram_binning", "isotonic_regression"):
                raise NotImplementedError(f"base_bin_calibrator_name={base_bin_calibrator_name!r} is a netcal class and netcal is not "
                                          "a dependency; of the bin_based calibrators only 'multi_isotonic_regression' is built")
            if base_bin_calibrator_name != "multi_isotonic_regression":
                raise NotImplementedError(f"base_calibration_mode='bin_based' with base_bin_calibrator_name={base_bin_calibrator_name!r}: "
                                          "only 'multi_isotonic_regression' is built")
        elif base_calibration_mode not in (None, "scaling_based"):
            raise NotImplementedError(f"base_calibration_mode={base_calibration_mode!r}: only None, 'scaling_based' and 'bin_based' "
                                      "(with 'multi_isotonic_regression') are built")
        self.base_calibration_mode, self.procal_flag = base_calibration_mode, bool(procal_flag)
        self.base_bin_calibrator_name = base_bin_calibrator_name
        self.dac_flag, self.k_dac = dac_flag, k_dac
        self.text_feature_dict = text_feature_dict
        self.val_logits = np.asarray(val_dict["val_logits"])
        self.val_labels = np.asarray(val_dict["val_labels"])
        self.val_image_features = np.asarray(val_dict["val_image_features"])
        self.val_image_knn_dists = np.asarray(val_dict["val_image_knn_dists"])
        self.val_image_proximity = np.exp(-np.mean(self.val_image_knn_dists, axis=-1))     # vl_calibrator.py:69
        self.dac_calibrator: Optional[DistanseAwareCalibration] = None
        self.base_calibrator: Union[None, DensityRatioCalibration, MultiIsotonicRegression, BinMeanShift] = None

    @property
    def bin_based_active(self) -> bool:
        """vl_calibrator.py:121-147: a bin-based calibrator is built whatever procal_flag says (it picks the class)."""
        return self.base_calibration_mode == "bin_based"

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
        if self.bin_based_active:   # vl_calibrator.py:121-147 on the val softmax, NO DAC on val; the first softmax runs on the device too
            lg = torch.from_numpy(np.ascontiguousarray(self.val_logits, dtype=np.float32)).cuda()
            if self.procal_flag:
                cal = BinMeanShift(PROXIMITY_BINS)
                cal.fit_device(lg, self.val_labels, self.val_image_proximity)
            else:
                cal = MultiIsotonicRegression()
                cal.fit_device(lg, self.val_labels)
            self.base_calibrator = cal

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

    def row_calibrator_device(self):
        """The fitted calibrator that turns the (DAC-scaled) logits of a split into the evaluator's (conf, pred) in one launch -- ProCal
        or a bin-based one -- with a flag saying whether it needs the proximity of every row; (None, False) when neither is on.
        Raises if one is on but fit() has not run."""
        if self.bin_based_active:
            if self.base_calibrator is None:
                raise RuntimeError("VLCalibration: a bin_based calibrator is on; call fit() first")
            return self.base_calibrator, self.procal_flag
        return self.procal_device(), self.procal_active

    def predict(self, logits, test_proximity=None) -> np.ndarray:
        """vl_calibrator.py:83-109: numpy [N,C] logits -> calibrated probabilities (float32: the DAC step already rounds to fp32
        in the reference, and the row softmax runs in fp32 on the device).  With ProCal or a bin-based calibrator: DAC -> softmax ->
        calibrator in one launch; ``test_proximity`` (one entry per row) is required where the calibrator uses it (ProCal,
        Bin-Mean-Shift)."""
        logits = np.asarray(logits)
        procal, needs_proximity = self.row_calibrator_device()
        if needs_proximity and test_proximity is None:
            raise AssertionError("ProCal needs test_proximity")
        if test_proximity is not None and logits.shape[0] != np.asarray(test_proximity).shape[0]:
            raise AssertionError(f"Shape mismatch: logits shape {logits.shape[0]} != test_proximity shape {np.asarray(test_proximity).shape[0]}")
        lg = torch.from_numpy(logits).float().cuda()
        if procal is not None:
            prox = None if test_proximity is None else torch.from_numpy(np.asarray(test_proximity, dtype=np.float32)).to(lg.device)
            return procal.predict_device(lg, prox, self.class_confidence_device(lg.device), want_probs=True)[0].cpu().numpy()
        return ops.softmax_rows(lg, self.class_confidence_device(lg.device)).cpu().numpy()
