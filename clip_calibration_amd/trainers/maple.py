"""MaPLe (reference trainers/classification/maple.py:51-216): the inference forward, and ``CustomCLIP.fit_prompt_learner``, the prompt
learner's training on the GPU through both towers (clip_calibration_amd/maplefit.py)."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..model import CLIP
from . import _fit
from .coop import CustomCLIP as _CoOpCLIP, TextEncoder  # noqa: F401


class MultiModalPromptLearner(nn.Module):
    """maple.py:77-187: shallow text ctx [n_ctx,Dt], its Linear(Dt->Dv) image-side projection, and
    (PROMPT_DEPTH-1) deep text prompts each with its own Linear(Dt->Dv).  The few [n_ctx, D] x [D, Dv] projections are
    tiny host-controlled ops (2 x 512 x 768) kept in torch, as in the reference; ``forward`` returns the same 4-tuple
    (prompts, shared_ctx, deep text prompts, deep visual prompts)."""

    def __init__(self, clip_model: CLIP, tokenized_prompts: torch.Tensor, n_ctx: int = 2, prompt_depth: int = 9, seed: int = 0):
        super().__init__()
        assert prompt_depth >= 1, "For MaPLe, PROMPT_DEPTH should be >= 1"
        dev, dtype = clip_model.device, clip_model.dtype
        dt = clip_model.ln_final.weight.shape[0]
        dv = clip_model.visual.conv1.weight.shape[0]
        g = torch.Generator().manual_seed(seed)
        self.ctx = nn.Parameter((0.02 * torch.randn(n_ctx, dt, generator=g)).to(dev, dtype))
        self.proj = nn.Linear(dt, dv).to(dev).half()
        self.compound_prompts_text = nn.ParameterList(
            [nn.Parameter((0.02 * torch.randn(n_ctx, dt, generator=g)).to(dev)) for _ in range(prompt_depth - 1)])
        self.compound_prompt_projections = nn.ModuleList([nn.Linear(dt, dv).to(dev) for _ in range(prompt_depth - 1)])
        tokenized_prompts = tokenized_prompts.to(dev)
        with torch.no_grad():
            embedding = clip_model.token_embedding(tokenized_prompts).type(dtype)
        self.register_buffer("token_prefix", embedding[:, :1, :])
        self.register_buffer("token_suffix", embedding[:, 1 + n_ctx:, :])
        self.n_cls, self.n_ctx = tokenized_prompts.shape[0], n_ctx
        self.tokenized_prompts = tokenized_prompts

    def forward(self):
        ctx = self.ctx.unsqueeze(0).expand(self.n_cls, -1, -1)
        prompts = torch.cat([self.token_prefix, ctx.to(self.token_prefix.dtype), self.token_suffix], dim=1)
        visual_deep = [layer(p) for layer, p in zip(self.compound_prompt_projections, self.compound_prompts_text)]
        return prompts, self.proj(self.ctx.to(self.proj.weight.dtype)), list(self.compound_prompts_text), visual_deep


class CustomCLIP(_CoOpCLIP):
    """maple.py:190-216: text tower with deep text prompts, image tower with shared_ctx + deep visual prompts."""

    def __init__(self, clip_model: CLIP, tokenized_prompts: torch.Tensor, n_ctx: int = 2, prompt_depth: int = 9,
                 logit_scale=None, cache_text_features: bool = True, seed: int = 0):
        nn.Module.__init__(self)
        self.prompt_learner = MultiModalPromptLearner(clip_model, tokenized_prompts, n_ctx, prompt_depth, seed)
        self.tokenized_prompts = self.prompt_learner.tokenized_prompts
        self.image_encoder = clip_model.visual
        self.text_encoder = TextEncoder(clip_model)
        self.logit_scale = clip_model.logit_scale
        self.dtype = clip_model.dtype
        object.__setattr__(self, "clip_model", clip_model)
        self._fixed_scale = logit_scale
        self.cache_text_features = cache_text_features
        self._cache_key = None
        self._cache = None

    def _text_inputs(self):
        prompts, _, deep_t, _ = self.prompt_learner()
        return prompts, deep_t, self.prompt_learner.n_ctx

    def _image_features(self, image: torch.Tensor) -> torch.Tensor:
        _, shared_ctx, _, deep_v = self.prompt_learner()
        return self.clip_model.image_features_f32(image, shared_ctx, deep_v)

    def learner_params(self):
        """The prompt learner's trained parameters under their ``state_dict`` names (the buffers left out)."""
        return {k: v for k, v in self.prompt_learner.named_parameters()}

    def fit_prompt_learner(self, train_loader, transform=None, **fit_args):
        """Train the prompt learner -- ``ctx``, ``compound_prompts_text``, ``proj`` and ``compound_prompt_projections`` -- on the GPU,
        starting from the parameters' values, with ``logit_scale`` taken from this model unless ``fit_args`` say otherwise (maple.py:279-300
        with both towers frozen).  The fitted block is copied into the parameters in place, each in its own dtype (the fit keeps fp32
        masters; ``proj`` is a half Linear) -- that moves their versions, so the cached text features retire on their own; the cache is
        dropped as well -- and returned as ``maplefit.fit_prompt_learner`` returns it.  Both towers run on every step: nothing is cached.

        ``transform=None``: ``train_loader`` is a sized iterable of (preprocessed images, labels) batches, iterated once per epoch.
        ``transform=TrainPreprocess.for_model(model)``: it yields (decoded uint8 images, labels) and every batch goes transform ->
        ``MaPLeFitState.step`` with nothing synchronising until the end (``augment.fit_with_transform``).  ``fit_args``: ``epochs`` (5),
        ``lr`` (0.0035), ``lr_per_epoch``, the optimiser's ``momentum``, ``dampening``, ``weight_decay``, ``nesterov``, ``grad_scale``,
        ``seq_rows``, ``views`` (with a transform) and ``return_history``; the batch size and the order are the loader's.
        ``grad_scale="dynamic"`` with ``scaler=dict(init_scale, growth_factor, backoff_factor, growth_interval)``: the device-side loss
        scale (``maplefit``'s module docstring).

        Validation, on either route: ``val_loader=`` (a sized iterable of (test-transformed images, labels) batches on the GPU, iterated
        once per epoch) or ``val=(val_images_or_loader, val_labels)``, with ``val_batch_size``, ``val_bins``, ``final_model``
        ("last_step" or "best_val", the reference's TEST.FINAL_MODEL), ``val_criterion`` and ``return_monitor`` as
        ``maplefit.fit_prompt_learner`` takes them.  Validation images go through the test transform, never through ``transform``.
        ``final_model="best_val"`` installs the best epoch's parameters."""
        import math
        from .. import maplefit
        shard = _fit.checked_shard("fit_prompt_learner", fit_args, "block")
        _fit.validation_set("fit_prompt_learner", None, fit_args)
        fit_args.setdefault("logit_scale", math.log(self.scale))
        fit_args.setdefault("class_token_position", getattr(self.prompt_learner, "class_token_position", "end"))
        ids, params = self.prompt_learner.tokenized_prompts, self.learner_params()
        if transform is not None:
            from ..augment import fit_with_transform
            run, epochs, lr = _fit.split_fit_args(fit_args, 5, 0.0035)
            watch = _fit.split_monitor_args("fit_prompt_learner", fit_args)
            from ..coopfit import shard_states
            state = shard_states(lambda sh: maplefit.MaPLeFitState(self.clip_model, ids, params, **dict(fit_args, shard=sh)), shard)
            end, monitored = _fit.image_end_epoch(state, watch, epochs, len(train_loader))
            losses = fit_with_transform(state, lambda x: x, ids.shape[0], train_loader, transform, epochs, lr, end_epoch=end, **run)
            best = monitored and watch["final_model"] == "best_val"
            fitted = _fit.pack_monitored(state, state.best_params() if best else state.params(), losses, watch, monitored)
        else:
            fitted = maplefit.fit_prompt_learner(train_loader, None, self.clip_model, ids, params, **fit_args)
        block = fitted[0] if isinstance(fitted, tuple) else fitted
        with torch.no_grad():
            for name, p in params.items():
                p.copy_(block[name])
        self._cache_key = self._cache = None
        return fitted
