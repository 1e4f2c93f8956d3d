"""TempScaling (reference trainers/calibration/tempscaling.py:31-59) -- the forward, and the 1-parameter SGD fit both ways:

* ``fit_scale`` runs the loader through the frozen base model ONCE, keeps the cosine logits on the device and fits the scalar there
  (clip_calibration_amd/tempfit.py, csrc/tempscale.hip): every epoch of the reference's loop (tempscaling.py:146-169) sees the same
  cosine matrix, so the 20 epochs need the towers once, not 20 times;
* ``forward_train`` keeps the step under torch autograd for a caller who drives the loop: it returns
  ``scale_learner() * cosine_logits`` with the cosine logits from the HIP path as a constant and the scalar as the only leaf, so
  ``F.cross_entropy(logits, label).backward()`` is exactly the reference's step (tempscaling.py:146-158)."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops


class ScaleLearner(nn.Module):
    """tempscaling.py:31-41: one scalar ``logit_scale`` initialised to 4.6052 (= ln 100)."""

    def __init__(self, dtype=torch.float32, init: float = 4.6052, device=None):
        super().__init__()
        self.logit_scale = nn.Parameter(torch.tensor(init, dtype=dtype, device=device))

    def forward(self):
        return self.logit_scale.exp()


class CustomCLIPCalibration(nn.Module):
    """tempscaling.py:44-59: ``logits_encoder`` is a base model that emits cosine logits (logit_scale = 1.0); the learnt
    scale multiplies the normalised image features before the text matmul."""

    def __init__(self, base_model, init: float = 4.6052):
        super().__init__()
        self.logits_encoder = base_model
        self.dtype = getattr(base_model, "dtype", torch.float32)
        self.scale_learner = ScaleLearner(torch.float32, init)

    def forward_train(self, image, label=None):
        """tempscaling.py:53-56 under autograd: ``logit_scale * image_features @ text_features.t()``.  The towers and the
        [B, C] cosine matmul run on the HIP path (no graph: every tower weight is frozen there, tempscaling.py:93-106);
        the product with the learnt scalar is the one differentiable operation, so d loss / d logit_scale is the
        reference's.  Returns (logits, image_features, text_features) like ``forward``."""
        with torch.no_grad():
            _, image_features, text_features = self.logits_encoder(image)[:3]
            cosine, _, _ = ops.logits_fused(image_features, text_features, 1.0, None, False)
        return self.scale_learner() * cosine, image_features, text_features

    @torch.no_grad()
    def cosine_logits(self, image):
        """The constant of ``forward_train``, formed the same way: (cosine logits fp32 [B, C], image_features, text_features)."""
        _, image_features, text_features = self.logits_encoder(image)[:3]
        cosine, _, _ = ops.logits_fused(image_features, text_features, 1.0, None, False)
        return cosine, image_features, text_features

    def fit_scale(self, loader, **fit_args) -> float:
        """The reference's training run (tempscaling.py:146-169) with the towers run once: one pass of ``loader`` (an iterable of
        (image, label) batches) through ``logits_encoder``, the cosine logits kept on the device, then
        ``tempfit.fit_logit_scale(cosine, labels, **fit_args)`` starting from the current ``logit_scale`` unless ``init`` says otherwise.
        The fitted scalar is written into ``scale_learner.logit_scale`` and returned."""
        from ..runner import fit_temperature
        fit_args.setdefault("init", float(self.scale_learner.logit_scale.detach()))
        fitted = fit_temperature(self.cosine_logits, loader, **fit_args)
        theta = fitted[0] if isinstance(fitted, tuple) else fitted
        with torch.no_grad():
            self.scale_learner.logit_scale.fill_(theta)
        return fitted

    @torch.no_grad()
    def forward(self, image, label=None, dac_conf=None, want_conf_pred: bool = False):
        _, image_features, text_features = self.logits_encoder(image)[:3]
        scale = float(self.scale_learner().detach())
        logits, conf, pred = ops.logits_fused(image_features, text_features, scale, dac_conf, want_conf_pred)
        if want_conf_pred:
            return logits, image_features, text_features, conf, pred
        return logits, image_features, text_features
