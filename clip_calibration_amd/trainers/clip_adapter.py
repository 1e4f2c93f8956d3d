"""CLIP-Adapter (reference trainers/classification/clip_adapter.py:138-187): the inference forward, and the training of the bottleneck
on the GPU (``CustomCLIP.fit_adapter``; clip_calibration_amd/adapterfit.py, csrc/adapter_train.hip) from cached image features or, with a
``TrainPreprocess``, under the reference's random train transform (clip_calibration_amd/augment.py, csrc/augment.hip).

A two-layer bias-free bottleneck (E -> E/4 -> E, ReLU after each) on the un-normalised image features, blended with them
by ``ratio`` (clip_adapter.py:170-172); the text side is CoOp's prompt splice through the text tower (clip_adapter.py:174-176;
with the shipped config the context is the frozen hand-written template)."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from . import _fit
from .coop import CustomCLIP as _CoOpCLIP


class Adapter(nn.Module):
    def __init__(self, c_in: int, reduction: int = 4):
        super().__init__()
        self.fc = nn.Sequential(nn.Linear(c_in, c_in // reduction, bias=False), nn.ReLU(inplace=True),
                                nn.Linear(c_in // reduction, c_in, bias=False), nn.ReLU(inplace=True))


class CustomCLIP(_CoOpCLIP):
    def __init__(self, clip_model, tokenized_prompts, n_ctx: int = 16, ratio: float = 0.2, **kw):
        super().__init__(clip_model, tokenized_prompts, n_ctx=n_ctx, **kw)
        self.adapter = Adapter(clip_model.visual.output_dim, 4).to(clip_model.device, clip_model.dtype)
        self.ratio = ratio

    def _image_features(self, image: torch.Tensor) -> torch.Tensor:
        f = self.clip_model.image_features_f32(image)
        return ops.adapter_blend(f, self.adapter.fc[0].weight.float(), self.adapter.fc[2].weight.float(), self.ratio)

    def fit_adapter(self, loader, transform=None, **fit_args):
        """Train the bottleneck on the GPU, starting from the module's weights, with ``ratio`` and ``logit_scale`` taken from this model
        unless ``fit_args`` say otherwise.  The fitted matrices are copied into ``adapter.fc[0].weight`` and ``adapter.fc[2].weight`` in
        the module's dtype (the fit itself keeps fp32 master weights) and returned as ``adapterfit.fit_adapter`` returns them.

        ``transform=None``: one pass of ``loader`` (an iterable of (image, label) batches of preprocessed images) through the frozen
        image tower (``image_features_f32``), the raw features and the labels kept on the device, then ``adapterfit.fit_adapter(features,
        labels, self.text_features(), w1, w2, **fit_args)``.  Caching the features equals the reference's loop only for a DETERMINISTIC
        train transform; the reference's config trains with ``random_resized_crop`` + ``random_flip``, which give every epoch other
        features.

        ``transform=TrainPreprocess(...)`` is that regime: ``loader`` yields (decoded uint8 images, labels) and is iterated once per
        epoch, every batch going transform -> image tower -> ``AdapterFitState.step`` with nothing synchronising until the end
        (``augment.fit_with_transform``).  ``fit_args``: ``epochs`` (200), ``lr`` (0.002), ``lr_per_epoch``, the optimiser's ``momentum``,
        ``dampening``, ``weight_decay``, ``nesterov``, ``views`` (explicit boxes and flips per batch) and ``return_history``; the batch size
        and the order are the loader's.

        Validation, on either route: ``val_loader=`` (an iterable of (image, label) batches of test-transformed images, run through the
        image tower once before the first epoch) or ``val=(val_features, val_labels)``, with ``val_bins``, ``final_model`` ("last_step"
        or "best_val", the reference's TEST.FINAL_MODEL), ``val_criterion`` and ``return_monitor`` as ``adapterfit.fit_adapter`` takes
        them.  The cached route validates inside its one library call; with a ``transform`` ``AdapterFitState.validate`` runs behind
        every epoch.  ``final_model="best_val"`` installs the best epoch's weights into the module."""
        _fit.validation_set("fit_adapter", self.clip_model, fit_args)
        fit_args.setdefault("ratio", self.ratio)
        fit_args.setdefault("logit_scale", math.log(self.scale))
        fc1, fc2 = self.adapter.fc[0].weight, self.adapter.fc[2].weight
        with torch.no_grad():
            text = self.text_features()
        if transform is not None:
            from ..adapterfit import AdapterFitState
            run, epochs, lr = _fit.split_fit_args(fit_args, 200, 0.002)
            watch = _fit.split_monitor_args("fit_adapter", fit_args, text.shape[0], text.shape[1])
            state = AdapterFitState(text, fc1.detach().float(), fc2.detach().float(), **fit_args)
            losses, monitor = _fit.run_with_transform("fit_adapter", state, self.clip_model, text.shape[0], text.shape[1], loader, transform,
                                                      epochs, lr, run, watch)
            fitted = _fit.pack(state.best_weights() if watch["final_model"] == "best_val" else (state.w1, state.w2), losses)
            fitted = fitted + (monitor,) if monitor is not None else fitted
        else:
            from ..adapterfit import fit_adapter
            feats, labels = _fit.cached_features("fit_adapter", self.clip_model, loader)
            fitted = fit_adapter(feats, labels, text, fc1.detach().float(), fc2.detach().float(), **fit_args)
        with torch.no_grad():
            fc1.copy_(fitted[0])
            fc2.copy_(fitted[1])
        return fitted
