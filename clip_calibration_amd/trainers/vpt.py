"""VPT (reference trainers/classification/vpt.py:70-116): the inference forward, and ``fit_prompts``, the reference's training of the visual
prompts on the GPU (``vptfit``).

Vision-side prompting: the CLIP is built with design_details trainer='VPT' (prompt tokens inside the image tower,
clip/model.py:361-424), the text side is the fixed hand-written prompts "a photo of a {name}." encoded once
(``FixedEmbeddings``, vpt.py:70-92).  The reference's eval ``forward`` returns the logits alone (vpt.py:105-116); the
mirror returns the trainer-level 3-tuple every other trainer returns (base_learner.py:86), logits first."""
from __future__ import annotations

import torch

from . import _fit
from .zsclip import ZeroshotCLIP


class CustomCLIP(ZeroshotCLIP):
    def __init__(self, clip_model, tokenized_prompts: torch.Tensor, logit_scale: float | None = None):
        if clip_model.design_details.get("trainer") != "VPT" or int(clip_model.design_details.get("vision_depth", 0)) < 1:
            raise ValueError("VPT needs a CLIP built with design_details trainer='VPT' and vision_depth >= 1 (vpt.py:39)")
        super().__init__(clip_model, tokenized_prompts, logit_scale)

    @property
    def fixed_embeddings(self) -> torch.Tensor:
        return self.text_features

    def fit_prompts(self, train_loader, transform=None, **fit_args):
        """Train ``visual.VPT`` and ``visual.transformer.resblocks.{i}.VPT_shallow`` on the GPU, starting from the parameters' values,
        against this model's fixed text features and ``logit_scale`` unless ``fit_args`` say otherwise (vpt.py with both towers' weights
        frozen).  The fitted prompts are copied into the parameters in place, in their dtype (the fit keeps an fp32 master block) -- that
        moves their versions, so the next inference forward uses them -- and returned as ``vptfit.fit_prompts`` returns them:
        fp32 [depth, n_ctx, Dv], slot 0 ``visual.VPT``.  The image tower runs on every step: no features are cached.

        ``transform=None``: ``train_loader`` is a sized iterable of (preprocessed images, labels) batches, iterated once per epoch.
        ``transform=TrainPreprocess.for_model(model)``: it yields (decoded uint8 images, labels) and every batch goes transform ->
        ``VPTFitState.step`` with nothing synchronising until the end (``augment.fit_with_transform``).  ``fit_args``: ``epochs`` (5),
        ``lr`` (0.0025), ``lr_per_epoch``, the optimiser's ``momentum``, ``dampening``, ``weight_decay``, ``nesterov``, ``grad_scale``,
        ``views`` (with a transform) and ``return_history``; the batch size and the order are the loader's.  The defaults restate the
        reference's VPT config (SGD, lr 0.0025, 5 epochs).  ``grad_scale="dynamic"`` with ``scaler=dict(init_scale, growth_factor,
        backoff_factor, growth_interval)``: the device-side loss scale (``vptfit``'s module docstring).

        Validation, on either route: ``val_loader=`` (a sized iterable of (test-transformed images, labels) batches on the GPU, iterated
        once per epoch) or ``val=(val_images_or_loader, val_labels)``, with ``val_batch_size``, ``val_bins``, ``final_model``
        ("last_step" or "best_val", the reference's TEST.FINAL_MODEL), ``val_criterion`` and ``return_monitor`` as
        ``vptfit.fit_prompts`` takes them.  Validation images go through the test transform, never through ``transform``.
        ``final_model="best_val"`` installs the best epoch's prompts into the parameters."""
        import math
        from .. import vptfit
        shard = _fit.checked_shard("fit_prompts", fit_args, "block")
        _fit.validation_set("fit_prompts", None, fit_args)
        fit_args.setdefault("logit_scale", math.log(self.scale))
        text = self.text_features.float()
        if transform is not None:
            from ..augment import fit_with_transform
            from ..coopfit import shard_states
            run, epochs, lr = _fit.split_fit_args(fit_args, 5, 0.0025)
            watch = _fit.split_monitor_args("fit_prompts", fit_args)
            state = shard_states(lambda sh: vptfit.VPTFitState(self.clip_model, text, **dict(fit_args, shard=sh)), shard)
            end, monitored = _fit.image_end_epoch(state, watch, epochs, len(train_loader))
            losses = fit_with_transform(state, lambda x: x, text.shape[0], train_loader, transform, epochs, lr, end_epoch=end, **run)
            best = monitored and watch["final_model"] == "best_val"
            fitted = _fit.pack_monitored(state, state.best_prompts() if best else state.prompts, losses, watch, monitored)
        else:
            fitted = vptfit.fit_prompts(train_loader, None, self.clip_model, text, **fit_args)
        block = fitted[0] if isinstance(fitted, tuple) else fitted
        shallow, deep = self.clip_model.ivlp_vision_prompts()
        with torch.no_grad():
            for p, v in zip([shallow] + list(deep), block):
                p.copy_(v)
        return fitted
