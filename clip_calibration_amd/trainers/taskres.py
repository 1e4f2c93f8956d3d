"""TaskRes (reference trainers/classification/taskres.py:96-210): the inference forward, and the training of the residuals on the GPU
(``CustomCLIP.fit_residuals``; clip_calibration_amd/taskresfit.py, csrc/taskres_train.hip) from cached image features or, with a
``TrainPreprocess``, under the reference's random train transform (clip_calibration_amd/augment.py, csrc/augment.hip).

The classifier is ``base_text_features + alpha * text_feature_residuals`` (taskres.py:105-106), where the base features are
the text-encoder outputs of the hand-written templates averaged per class (taskres.py:109-135, NOT normalised before the
mean) and the residual is the only learned tensor.  ``forward`` normalises both sides and multiplies (taskres.py:191-210;
the reference returns the logits alone, the mirror the trainer-level 3-tuple)."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from ..model import CLIP
from . import _fit


class TaskResLearner(nn.Module):
    def __init__(self, base_text_features: torch.Tensor, alpha: float = 0.5):
        super().__init__()
        self.alpha = alpha
        self.register_buffer("base_text_features", base_text_features)
        self.text_feature_residuals = nn.Parameter(torch.zeros_like(base_text_features))

    def forward(self) -> torch.Tensor:
        return ops.scale_add(self.base_text_features, self.text_feature_residuals, self.alpha)


class CustomCLIP(nn.Module):
    def __init__(self, clip_model: CLIP, tokenized_templates: torch.Tensor, alpha: float = 0.5, logit_scale: Optional[float] = None):
        """``tokenized_templates``: [C, T, 77] token ids of T hand-written templates per class (T = 1 for every dataset but
        ImageNet); the base feature of a class is the plain mean of its T text-encoder outputs."""
        super().__init__()
        if tokenized_templates.dim() == 2:
            tokenized_templates = tokenized_templates.unsqueeze(1)
        C, T, L = tokenized_templates.shape
        with torch.no_grad():
            feats = clip_model.text_features_f32(tokenized_templates.reshape(C * T, L).to(clip_model.device))
            base = ops.group_mean(feats, T)
        self.prompt_learner = TaskResLearner(base, alpha)
        self.logit_scale = clip_model.logit_scale
        self.dtype = clip_model.dtype
        object.__setattr__(self, "clip_model", clip_model)
        self._fixed_scale = logit_scale

    @property
    def scale(self) -> float:
        return float(self._fixed_scale) if self._fixed_scale is not None else float(self.logit_scale.detach().exp())

    @torch.no_grad()
    def forward(self, image: torch.Tensor, label=None, dac_conf: Optional[torch.Tensor] = None, want_conf_pred: bool = False):
        text_features = ops.l2_normalize(self.prompt_learner())
        logits, image_features, conf, pred = ops.fused_tail(self.clip_model.image_features_f32(image), text_features, self.scale,
                                                            dac_conf, want_conf_pred)
        if want_conf_pred:
            return logits, image_features, text_features, conf, pred
        return logits, image_features, text_features

    def fit_residuals(self, loader, transform=None, **fit_args):
        """Train the residuals on the GPU, starting from the module's residuals, with ``alpha`` and ``logit_scale`` taken from this model
        unless ``fit_args`` say otherwise.  The fitted matrix is copied into ``prompt_learner.text_feature_residuals`` in the parameter's
        dtype (the fit itself keeps fp32 master values) and returned as ``taskresfit.fit_residuals`` returns it.

        ``transform=None``: one pass of ``loader`` (an iterable of (image, label) batches of preprocessed images) through the frozen
        image tower (``image_features_f32``), the raw features and the labels kept on the device, then ``taskresfit.fit_residuals(
        features, labels, base_text_features, residuals, **fit_args)``.  Caching the features equals the reference's loop only for a
        DETERMINISTIC train transform; the reference's config trains with ``random_resized_crop`` + ``random_flip``, which give every
        epoch other features.

        ``transform=TrainPreprocess(...)`` is that regime: ``loader`` yields (decoded uint8 images, labels) and is iterated once per
        epoch, every batch going transform -> image tower -> ``TaskResFitState.step`` with nothing synchronising until the end
        (``augment.fit_with_transform``).  ``fit_args``: ``epochs`` (200), ``lr`` (2e-4), ``lr_per_epoch``, ``optimizer`` and its settings,
        ``views`` (explicit boxes and flips per batch) and ``return_history``; the batch size and the order are the loader's.

        Validation, on either route: ``val_loader=`` (an iterable of (image, label) batches of test-transformed images, run through the
        image tower once before the first epoch) or ``val=(val_features, val_labels)``, with ``val_bins``, ``final_model`` ("last_step"
        or "best_val", the reference's TEST.FINAL_MODEL), ``val_criterion`` and ``return_monitor`` as ``taskresfit.fit_residuals`` takes
        them.  The cached route validates inside its one library call; with a ``transform`` ``TaskResFitState.validate`` runs behind
        every epoch.  ``final_model="best_val"`` installs the best epoch's residuals into the module."""
        _fit.validation_set("fit_residuals", self.clip_model, fit_args)
        fit_args.setdefault("alpha", self.prompt_learner.alpha)
        fit_args.setdefault("logit_scale", math.log(self.scale))
        res = self.prompt_learner.text_feature_residuals
        base = self.prompt_learner.base_text_features.float()
        if transform is not None:
            from ..taskresfit import TaskResFitState
            run, epochs, lr = _fit.split_fit_args(fit_args, 200, 2e-4)
            watch = _fit.split_monitor_args("fit_residuals", fit_args, base.shape[0], base.shape[1])
            state = TaskResFitState(base, res.detach().float(), **fit_args)
            losses, monitor = _fit.run_with_transform("fit_residuals", state, self.clip_model, base.shape[0], base.shape[1], loader, transform,
                                                      epochs, lr, run, watch)
            fitted = _fit.pack(state.best_residuals() if watch["final_model"] == "best_val" else state.residuals, losses)
            if monitor is not None:
                fitted = fitted + (monitor,) if isinstance(fitted, tuple) else (fitted, monitor)
        else:
            from ..taskresfit import fit_residuals
            feats, labels = _fit.cached_features("fit_residuals", self.clip_model, loader)
            fitted = fit_residuals(feats, labels, base, res.detach().float(), **fit_args)
        with torch.no_grad():
            res.copy_(fitted[0] if isinstance(fitted, tuple) else fitted)
        return fitted
