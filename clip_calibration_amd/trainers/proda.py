"""ProDA (reference trainers/classification/proda.py:76-333): the inference forward, and ``fit_context`` for training the contexts.

A collection of ``n_prompt`` learned contexts; at test time ``set_classifier`` (proda.py:316-333) runs ALL
n_cls * n_prompt prompts through the text tower once, L2-normalises each feature, and keeps the per-class MEAN (not
re-normalised) as the classifier; ``forward`` (proda.py:309-313) is then image tower -> normalise -> scaled matmul.
Context position varies over the collection (proda.py:110-114): the first quarter of the prompts put the class name in
front of the context, the second quarter in the middle, the rest at the end.

Index plumbing (which embedding row goes where) is torch indexing; the tower, normalisation, ensemble mean and logits
are device kernels.  ``CustomCLIP.fit_context`` trains ``prompt_learner.ctx`` on the GPU (clip_calibration_amd/prodafit.py,
csrc/proda_train.hip); the next ``set_classifier`` / ``forward`` then uses the fitted contexts."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from ..model import CLIP
from . import _fit
from .coop import TextEncoder


class PromptLearner(nn.Module):
    def __init__(self, clip_model: CLIP, tokenized_prompts: torch.Tensor, n_ctx: int = 16, n_prompt: int = 32, seed: int = 0):
        super().__init__()
        dtype, dev = clip_model.dtype, clip_model.device
        ctx_dim = clip_model.ln_final.weight.shape[0]
        tokenized_prompts = tokenized_prompts.to(dev)
        g = torch.Generator().manual_seed(seed)
        self.ctx = nn.Parameter((0.02 * torch.randn(n_prompt, n_ctx, ctx_dim, generator=g)).to(dev, dtype))
        if n_prompt > 1:    # proda.py:110-114
            pos = [0] * (n_prompt // 4) + [1] * (n_prompt // 4) + [2] * (n_prompt // 2)
        else:
            pos = [2]
        self.register_buffer("pos", torch.tensor(pos, device=dev), persistent=False)
        with torch.no_grad():
            embedding = clip_model.token_embedding(tokenized_prompts).type(dtype)
        self.register_buffer("token_prefix", embedding[:, :1, :])
        self.register_buffer("token_suffix", embedding[:, 1 + n_ctx:, :])
        # tokens of "X X .. X name ." are [SOT, X*n_ctx, name.., '.', EOT]: the name length follows from the EOT position
        self.name_lens = (tokenized_prompts.argmax(dim=-1) - n_ctx - 2).tolist()
        self.n_cls, self.n_ctx, self.n_prompt = tokenized_prompts.shape[0], n_ctx, n_prompt
        self.tokenized_prompts = tokenized_prompts

    def forward(self, infer: bool = True):
        """proda.py:146-222 with infer=True: prompts [n_cls * n_prompt, 77, D] ordered class-major, and inside a class
        [end-position prompts | middle | front] -- the order the reference's final ``torch.cat(..., dim=1)`` produces."""
        ctx, pos = self.ctx, self.pos
        P, n_cls, half = ctx.shape[0], self.n_cls, self.n_ctx // 2
        tokenized = self.tokenized_prompts.unsqueeze(1).repeat(1, P, 1).view(n_cls * P, -1)
        pre, suf = self.token_prefix, self.token_suffix
        ctx_end, ctx_mid, ctx_front = ctx[pos == 2], ctx[pos == 1], ctx[pos == 0]

        def rep(t, n):      # [1, len, D] -> [1, n, len, D]
            return t.unsqueeze(1).expand(-1, n, -1, -1)
        end = torch.cat([rep(pre, ctx_end.shape[0]), ctx_end.unsqueeze(0).expand(n_cls, -1, -1, -1), rep(suf, ctx_end.shape[0])], dim=2)
        mids, fronts = [], []
        for i, nl in enumerate(self.name_lens):
            p_i, cls_i, suf_i = pre[i:i + 1], suf[i:i + 1, :nl], suf[i:i + 1, nl:]
            nm, nf = ctx_mid.shape[0], ctx_front.shape[0]
            mids.append(torch.cat([rep(p_i, nm), ctx_mid[:, :half].unsqueeze(0), rep(cls_i, nm), ctx_mid[:, half:].unsqueeze(0),
                                   rep(suf_i, nm)], dim=2))
            fronts.append(torch.cat([rep(p_i, nf), rep(cls_i, nf), ctx_front.unsqueeze(0), rep(suf_i, nf)], dim=2))
        prompts = torch.cat([end, torch.cat(mids, dim=0), torch.cat(fronts, dim=0)], dim=1)
        return prompts.reshape(n_cls * P, -1, ctx.shape[-1]), tokenized


class CustomCLIP(nn.Module):
    def __init__(self, clip_model: CLIP, tokenized_prompts: torch.Tensor, n_ctx: int = 16, n_prompt: int = 32,
                 logit_scale: Optional[float] = None, prompts_per_call: int = 4096, **kw):
        super().__init__()
        self.n_class, self.n_prompt = tokenized_prompts.shape[0], n_prompt
        self.text_encoder = TextEncoder(clip_model)
        self.prompt_learner = PromptLearner(clip_model, tokenized_prompts, n_ctx, n_prompt, **kw)
        self.image_encoder = clip_model.visual
        self.logit_scale = clip_model.logit_scale
        self.dtype = clip_model.dtype
        object.__setattr__(self, "clip_model", clip_model)
        self._fixed_scale = logit_scale
        self.prompts_per_call = prompts_per_call
        self.text_features: Optional[torch.Tensor] = None

    @property
    def scale(self) -> float:
        return float(self._fixed_scale) if self._fixed_scale is not None else float(self.logit_scale.detach().exp())

    @torch.no_grad()
    def set_classifier(self) -> None:
        """proda.py:316-333 (called by VLBaseLearner.test before the loop, base_learner.py:65-67)."""
        prompts, tokenized = self.prompt_learner(infer=True)
        feats = []
        for lo in range(0, prompts.shape[0], self.prompts_per_call):
            feats.append(self.text_encoder(prompts[lo:lo + self.prompts_per_call].contiguous(), tokenized[lo:lo + self.prompts_per_call]))
        tf = ops.l2_normalize(torch.cat(feats))
        self.text_features = ops.group_mean(tf, self.n_prompt)

    def fit_context(self, train_loader, transform=None, **fit_args):
        """Train ``prompt_learner.ctx`` on the GPU, starting from the parameter's values, with ``logit_scale`` taken from this model
        unless ``fit_args`` say otherwise (proda.py:258-304 with both towers frozen).  The fitted contexts are copied into
        ``prompt_learner.ctx`` in the parameter's dtype (the fit keeps an fp32 master) and the cached classifier is cleared, so the
        next ``forward`` / ``set_classifier`` uses them; returned as ``prodafit.fit_context`` returns them.  ``grad_scale="dynamic"`` with
        ``scaler=dict(...)`` in ``fit_args`` is the reference's ``prec == "amp"`` branch (proda.py:370, 388-394) on either route.

        ``transform=None``: one pass of ``train_loader`` (an iterable of (image, label) batches of preprocessed images) through the
        frozen image tower, then ``prodafit.fit_context(features, labels, clip_model, tokenized_prompts, ctx, **fit_args)`` -- equal to
        the reference's loop only for a deterministic train transform.  ``transform=TrainPreprocess(...)``: ``train_loader`` yields
        (decoded uint8 images, labels) and is iterated once per epoch, every batch going transform -> image tower ->
        ``ProDAFitState.step`` (``augment.fit_with_transform``); ``fit_args`` are then ``epochs``, ``lr``, ``lr_per_epoch``, ``views``,
        ``return_history`` and ``ProDAFitState``'s own.

        Validation, on either route: ``val_loader=`` (an iterable of (image, label) batches of test-transformed images, run through the
        frozen image tower once before the first epoch) or ``val=(val_features, val_labels)``, with ``val_class_chunk`` (classes per
        tower call), ``val_bins``, ``final_model`` ("last_step" or "best_val", the reference's TEST.FINAL_MODEL), ``val_criterion`` and
        ``return_monitor`` as ``prodafit.fit_context`` takes them; ``ProDAFitState.validate`` runs behind every epoch and scores what
        ``set_classifier`` + ``forward`` would compute.  ``final_model="best_val"`` installs the best epoch's contexts.

        ``shard=coopfit.Shard(world, rank, gather)`` on either route: the class-sharded fit in the place of the reference's
        ``nn.DataParallel`` over the text encoder, one process per GPU, every rank making this call on the same data with a like-seeded
        ``generator`` (``prodafit``'s module docstring).  What ``shard`` refuses -- validation by ``val_loader=`` included -- is refused
        here, before either tower runs.  With a ``LocalGather`` the one call makes and steps all the ranks' states, on either route."""
        import math
        who = "fit_context"
        shard = _fit.checked_shard(who, fit_args, n_cls=self.prompt_learner.tokenized_prompts.shape[0], n_prompt=self.prompt_learner.ctx.shape[0])
        _fit.validation_set(who, self.clip_model, fit_args)
        fit_args.setdefault("logit_scale", math.log(self.scale))
        dynamic = fit_args.get("grad_scale") == "dynamic"
        self._scaler_state = None
        ctx = self.prompt_learner.ctx
        ids = self.prompt_learner.tokenized_prompts
        if transform is not None:
            from ..prodafit import ProDAFitState
            run, epochs, lr = _fit.split_fit_args(fit_args, 200, 0.002)
            E = int(self.clip_model.geometry.embed_dim)
            watch = _fit.split_monitor_args(who, fit_args, ids.shape[0], E)
            val_class_chunk = fit_args.pop("val_class_chunk", None)
            from ..coopfit import shard_states
            state = shard_states(lambda sh: ProDAFitState(self.clip_model, ids, ctx.detach(), **dict(fit_args, shard=sh)), shard)
            state.val_class_chunk = val_class_chunk
            losses, monitor = _fit.run_with_transform(who, state, self.clip_model, ids.shape[0], E, train_loader, transform, epochs, lr, run, watch)
            fitted = _fit.pack(state.best_params() if watch["final_model"] == "best_val" else state.ctx, losses)
            if monitor is not None:
                fitted = fitted + (monitor,) if isinstance(fitted, tuple) else (fitted, monitor)
            if dynamic:
                self._scaler_state = state.scaler_state()
        else:
            from ..prodafit import fit_context
            feats, labels = _fit.cached_features(who, self.clip_model, train_loader)
            fitted = fit_context(feats, labels, self.clip_model, ids, ctx.detach(), return_scaler_state=dynamic, **fit_args)
            if dynamic:      # the scaler's state sits behind the history and in front of the monitor's dict
                fitted = list(fitted)
                self._scaler_state = fitted.pop(1 + int(bool(fit_args.get("return_history"))))
                fitted = tuple(fitted) if len(fitted) > 1 else fitted[0]
        with torch.no_grad():
            ctx.copy_(fitted[0] if isinstance(fitted, tuple) else fitted)
        self.text_features = None
        return fitted

    def scaler_state(self) -> dict:
        """``ProDAFitState.scaler_state()`` of the last ``fit_context(..., grad_scale="dynamic")``, as read after its last step: ``dict(scale,
        growth_tracker, skipped_steps, applied_steps, found_inf)``."""
        if getattr(self, "_scaler_state", None) is None:
            raise ValueError("ProDA CustomCLIP.scaler_state: no fit_context under grad_scale='dynamic' has run")
        return dict(self._scaler_state)

    @torch.no_grad()
    def forward(self, image: torch.Tensor, label=None, dac_conf: Optional[torch.Tensor] = None, want_conf_pred: bool = False):
        if self.text_features is None:
            self.set_classifier()
        logits, image_features, conf, pred = ops.fused_tail(self.clip_model.image_features_f32(image), self.text_features, self.scale,
                                                            dac_conf, want_conf_pred)
        if want_conf_pred:
            return logits, image_features, self.text_features, conf, pred
        return logits, image_features, self.text_features
