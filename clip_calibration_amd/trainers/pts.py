"""Parameterized temperature scaling as a trainer (the reference's ``CALIBRATION.SCALING.MODE = 'ParameterizedTempScaling'`` with its
``CALIBRATION.P_TS`` block, train.py:238-247, for which it ships no trainer class): the frozen base model's scaled logits go through a
small MLP on their ``top_k`` largest values that gives every row its own temperature (clip_calibration_amd/ptsfit.py, csrc/pts.hip).

Modelled on ``CustomCLIPCalibration`` (tempscaling.py): ``logits_encoder`` is a base model that emits cosine logits; where TempScaling
multiplies them by its learnt scalar, this class multiplies them by the fixed ``base_scale`` (``exp(CALIBRATION.SCALING.INIT_TEMP)``)
and divides each row by its temperature."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .. import ops, ptsfit
from .._lib import check, lib


class CustomCLIPParameterizedCalibration(nn.Module):
    def __init__(self, base_model, base_scale: float = math.exp(4.6052), n_layers: int = 2, n_nodes: int = 5, top_k: int = 10, generator=None):
        super().__init__()
        self.logits_encoder = base_model
        self.dtype = getattr(base_model, "dtype", torch.float32)
        self.base_scale = float(base_scale)
        self.n_layers, self.n_nodes, self.top_k = ptsfit._check_net("CustomCLIPParameterizedCalibration", n_layers, n_nodes, top_k)
        self.pts_params = nn.Parameter(ptsfit.init_params(self.n_layers, self.n_nodes, self.top_k, generator), requires_grad=False)

    @torch.no_grad()
    def scaled_logits(self, image):
        """What the PTS net reads: (``base_scale`` x cosine logits fp32 [B, C], image_features, text_features), the towers run once."""
        _, image_features, text_features = self.logits_encoder(image)[:3]
        logits, _, _ = ops.logits_fused(image_features, text_features, self.base_scale, None, False)
        return logits, image_features, text_features

    def fit_pts(self, loader, **fit_args):
        """One pass of ``loader`` (an iterable of (image, label) batches) through ``scaled_logits``, the logits kept on the device, then
        ``ptsfit.fit_pts(logits, labels, **fit_args)`` starting from the current parameters unless ``params`` says otherwise.  The fitted
        block is written into ``pts_params``; returns what ``ptsfit.fit_pts`` returns."""
        from ..runner import fit_pts
        fit_args.setdefault("params", self.pts_params.detach())
        fitted = fit_pts(self.scaled_logits, loader, n_layers=self.n_layers, n_nodes=self.n_nodes, top_k=self.top_k, **fit_args)
        block = fitted[0] if isinstance(fitted, tuple) else fitted
        with torch.no_grad():
            if self.pts_params.device != block.device:
                self.pts_params.data = self.pts_params.data.to(block.device)
            self.pts_params.copy_(block)
        return fitted

    def calibrator(self) -> ptsfit.PTSCalibrator:
        return ptsfit.PTSCalibrator(self.pts_params.detach(), self.n_layers, self.n_nodes, self.top_k)

    @torch.no_grad()
    def forward(self, image, label=None, dac_conf=None, want_conf_pred: bool = False):
        """(logits / T, image_features, text_features[, conf, pred]).  DAC's class factor is applied after the temperature, as it is after
        TempScaling's scale; conf and pred are the softmax top-1 of the returned rows."""
        logits, image_features, text_features = self.scaled_logits(image)
        if self.pts_params.device != logits.device:
            self.pts_params.data = self.pts_params.data.to(logits.device)
        ops.pts_apply(logits, self.pts_params.detach(), self.n_layers, self.n_nodes, self.top_k, out=logits)
        B, C = logits.shape
        dac_conf, pd = ops._dac(dac_conf, C, "CustomCLIPParameterizedCalibration")
        conf, pred, pc, pp = ops._conf_pred(want_conf_pred, B, logits.device)
        if pd is not None or want_conf_pred:
            check(lib.clipmi_calibrate_rows(logits.data_ptr(), pd, pc, pp, B, C, ops._stream()), "clipmi_calibrate_rows")
        if want_conf_pred:
            return logits, image_features, text_features, conf, pred
        return logits, image_features, text_features
