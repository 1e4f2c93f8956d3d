"""CLIP-Adapter (reference trainers/classification/clip_adapter.py:138-187): the inference forward, and the training of the bottleneck
on the GPU from cached image features (``CustomCLIP.fit_adapter``; clip_calibration_amd/adapterfit.py, csrc/adapter_train.hip).

A two-layer bias-free bottleneck (E -> E/4 -> E, ReLU after each) on the un-normalised image features, blended with them
by ``ratio`` (clip_adapter.py:170-172); the text side is CoOp's prompt splice through the text tower (clip_adapter.py:174-176;
with the shipped config the context is the frozen hand-written template)."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from .. import ops
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

    def fit_adapter(self, loader, **fit_args):
        """Train the bottleneck on the GPU: one pass of ``loader`` (an iterable of (image, label) batches) through the frozen image tower
        (``image_features_f32``), the raw features and the labels kept on the device, then ``adapterfit.fit_adapter(features, labels,
        self.text_features(), w1, w2, **fit_args)`` starting from the module's weights, with ``ratio`` and ``logit_scale`` taken from this
        model unless ``fit_args`` say otherwise.  The fitted matrices are copied into ``adapter.fc[0].weight`` and ``adapter.fc[2].weight``
        in the module's dtype (the fit itself keeps fp32 master weights) and returned as ``fit_adapter`` returns them.

        Caching the features equals the reference's loop only for a DETERMINISTIC train transform: the reference's config trains with
        ``random_resized_crop`` + ``random_flip``, which give every epoch other features.  For such a transform run the tower on every
        batch and hand its features to ``adapterfit.AdapterFitState.step``."""
        from ..adapterfit import fit_adapter
        feats, labels = [], []
        with torch.no_grad():
            for image, label in loader:
                f = self.clip_model.image_features_f32(image)
                feats.append(f)
                labels.append(torch.as_tensor(label).to(device=f.device, dtype=torch.int64))
            text = self.text_features()
        if not feats:
            raise ValueError("fit_adapter: the loader gave no batch")
        fit_args.setdefault("ratio", self.ratio)
        fit_args.setdefault("logit_scale", math.log(self.scale))
        fc1, fc2 = self.adapter.fc[0].weight, self.adapter.fc[2].weight
        fitted = fit_adapter(torch.cat(feats), torch.cat(labels), text, fc1.detach().float(), fc2.detach().float(), **fit_args)
        with torch.no_grad():
            fc1.copy_(fitted[0])
            fc2.copy_(fitted[1])
        return fitted
