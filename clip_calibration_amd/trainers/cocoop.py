"""CoCoOp (reference trainers/classification/cocoop.py:71-199): the inference forward, and ``CustomCLIP.fit_prompt_learner``, which trains
``ctx`` and ``meta_net`` on the GPU through ``cocoopfit`` (cocoop.py:186-202, 259-278 with both towers frozen).

Every image gets its own context: ``ctx + meta_net(image_features)`` (cocoop.py:154-161), hence its own C prompts and its
own pass through the text tower -- B*C prompts per batch, which makes the TEXT tower the dominant cost (5.96 GFLOP per
prompt against 35 GFLOP per image).  The reference loops over the images in Python and runs the tower on C prompts at
a time (cocoop.py:193-198); here the prompts of several images form one text-encoder call (``prompts_per_call``), the
meta-net, the prompt splice and the per-image normalise + dot product are HIP kernels, and nothing returns to the host.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from ..model import CLIP
from . import _fit
from .coop import TextEncoder


class PromptLearner(nn.Module):
    """cocoop.py:71-171: ``ctx`` [n_ctx, D] plus ``meta_net`` = Linear(E, E//16) - ReLU - Linear(E//16, D).  ``forward``
    returns the shifted contexts [B, n_ctx, D]; the [B, C, 77, D] prompt tensor the reference stacks is never built whole."""

    def __init__(self, clip_model: CLIP, tokenized_prompts: torch.Tensor, n_ctx: int = 4,
                 ctx_init_ids: Optional[torch.Tensor] = None, seed: int = 0):
        super().__init__()
        dtype, dev = clip_model.dtype, clip_model.device
        ctx_dim = clip_model.ln_final.weight.shape[0]
        vis_dim = clip_model.visual.output_dim
        tokenized_prompts = tokenized_prompts.to(dev)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            if ctx_init_ids is not None:      # CTX_INIT "a photo of a" (cocoop.py:85-93)
                emb = clip_model.token_embedding(ctx_init_ids.to(dev)).type(dtype)
                n_ctx = n_ctx_from_init_ids(ctx_init_ids, tokenized_prompts.shape[-1])
                ctx_vectors = emb[0, 1:1 + n_ctx, :].clone()
            else:
                ctx_vectors = (0.02 * torch.randn(n_ctx, ctx_dim, generator=g)).to(dev, dtype)
            embedding = clip_model.token_embedding(tokenized_prompts).type(dtype)
        self.ctx = nn.Parameter(ctx_vectors)
        self.meta_net = nn.Sequential(OrderedDict([("linear1", nn.Linear(vis_dim, vis_dim // 16)), ("relu", nn.ReLU(inplace=True)),
                                                   ("linear2", nn.Linear(vis_dim // 16, ctx_dim))])).to(dev, dtype)
        self.register_buffer("token_prefix", embedding[:, :1, :])
        self.register_buffer("token_suffix", embedding[:, 1 + n_ctx:, :])
        self.register_buffer("_base", embedding, persistent=False)     # [C,77,D]: rows 1..n_ctx are overwritten per image
        self.n_cls, self.n_ctx = tokenized_prompts.shape[0], n_ctx
        self.tokenized_prompts = tokenized_prompts

    def base_embedding(self) -> torch.Tensor:
        return self._base

    def forward(self, im_features: torch.Tensor) -> torch.Tensor:
        m = self.meta_net
        return ops.cocoop_ctx(im_features.float(), m.linear1.weight.float(), m.linear1.bias.float(), m.linear2.weight.float(),
                              m.linear2.bias.float(), self.ctx.float())


class CustomCLIP(nn.Module):
    """cocoop.py:174-199.  eval ``forward(image) -> (logits [B,C], image_features [B,E], text_features [C,E])`` where, as in
    the reference, ``text_features`` are those of the LAST image of the batch."""

    def __init__(self, clip_model: CLIP, tokenized_prompts: torch.Tensor, n_ctx: int = 4, logit_scale: Optional[float] = None,
                 prompts_per_call: int = 4096, text_stream_f16: bool = True, **kw):
        super().__init__()
        # Here the TEXT tower is the hot path (B * C prompts per batch, cocoop.py:186-197).  text_stream_f16: run it on the fp16
        # residual stream like the image tower (the reference's own GPU precision: clip/model.py:186-187 adds in fp16) -- +20 %
        # prompts/s (profiles/r02_text_tower_f16_stream.txt).  The library default keeps the text tower's stream in fp32 because
        # zero-shot / CoOp text features are computed once and feed every logit.  It is a PER-CALL flag of the tower call
        # (CLIPMI_CALL_STREAM_F16): no library state is touched, the same model handle keeps serving fp32-stream text features;
        # a model (or process) set to residual_f16 = 0 or ln_fold = 0 keeps the fp32 stream here too.
        self.text_stream_f16 = text_stream_f16
        self.prompt_learner = PromptLearner(clip_model, tokenized_prompts, n_ctx, **kw)
        self.tokenized_prompts = self.prompt_learner.tokenized_prompts
        self.image_encoder = clip_model.visual
        self.text_encoder = TextEncoder(clip_model)
        self.logit_scale = clip_model.logit_scale
        self.dtype = clip_model.dtype
        object.__setattr__(self, "clip_model", clip_model)
        self._fixed_scale = logit_scale
        self.prompts_per_call = prompts_per_call

    @property
    def scale(self) -> float:
        return float(self._fixed_scale) if self._fixed_scale is not None else float(self.logit_scale.detach().exp())

    @torch.no_grad()
    def per_image_text_features(self, image_features: torch.Tensor) -> torch.Tensor:
        """Un-normalised text-encoder outputs [B, C, E] for the given L2-normalised image features."""
        pl = self.prompt_learner
        B, Cn = image_features.shape[0], pl.n_cls
        ctx_shifted = pl(image_features)
        out = torch.empty(B, Cn, self.clip_model.geometry.embed_dim, dtype=torch.float32, device=image_features.device)
        step = max(1, self.prompts_per_call // Cn)
        from .. import _lib
        m = self.clip_model
        f16 = self.text_stream_f16 and m.get_option("residual_f16") == 2 and m.get_option("ln_fold") == 1   # 2 = image tower only (the default)
        flags = _lib.CALL_STREAM_F16 if f16 else _lib.CALL_DEFAULT
        rows = m.live_rows(self.tokenized_prompts)      # of the class list (kept with it: no per-batch read-back); every image repeats it
        for lo in range(0, B, step):
            nb = min(step, B - lo)
            prompts = ops.cocoop_prompts(pl.base_embedding(), ctx_shifted[lo:lo + nb])
            ids = self.tokenized_prompts.repeat(nb, 1)                       # EOT index plumbing
            out[lo:lo + nb] = self.text_encoder(prompts, ids, flags=flags, seq_rows=rows).view(nb, Cn, -1)
        return out

    def fit_prompt_learner(self, train_loader, transform=None, **fit_args):
        """Train ``prompt_learner.ctx`` and ``prompt_learner.meta_net`` on the GPU, starting from the module's values, with ``logit_scale``
        taken from this model unless ``fit_args`` say otherwise.  The fitted tensors are copied into the module in its dtype (the fit
        keeps one fp32 master block), so the next ``forward`` uses them; returned as ``cocoopfit.fit_prompt_learner`` returns them.

        ``transform=None``: one pass of ``train_loader`` (an iterable of (image, label) batches of preprocessed images) through the
        frozen image tower, then ``cocoopfit.fit_prompt_learner(features, labels, clip_model, tokenized_prompts, params, **fit_args)`` --
        equal to the reference's loop only for a deterministic train transform.  ``transform=TrainPreprocess(...)``: ``train_loader``
        yields (decoded uint8 images, labels) and is iterated once per epoch, every batch going transform -> image tower ->
        ``CoCoOpFitState.step`` (``augment.fit_with_transform``); ``fit_args`` are then ``epochs``, ``lr``, ``lr_per_epoch``, ``views``,
        ``return_history`` and ``CoCoOpFitState``'s own.  ``grad_scale="dynamic"`` with ``scaler=dict(init_scale, growth_factor,
        backoff_factor, growth_interval)`` on either route: the device-side loss scale (``cocoopfit``'s module docstring).

        Validation, on either route: ``val_loader=`` (an iterable of (image, label) batches of test-transformed images, run through the
        frozen image tower once before the first epoch) or ``val=(val_features, val_labels)``, with ``val_batch_size`` (images per
        validation chunk), ``val_bins``, ``final_model`` ("last_step" or "best_val", the reference's TEST.FINAL_MODEL),
        ``val_criterion`` and ``return_monitor`` as ``cocoopfit.fit_prompt_learner`` takes them; ``CoCoOpFitState.validate`` runs behind
        every epoch and scores what this module's ``forward`` would compute.  ``final_model="best_val"`` installs the best epoch's
        tensors into the module.

        ``shard=coopfit.Shard(world, rank, gather)`` on either route: the class-sharded fit in the place of the reference's
        ``nn.DataParallel`` over the text encoder, one process per GPU, every rank making this call on the same data (``cocoopfit``'s
        module docstring).  Both loss scales and all three optimisers work under it.  What ``shard`` refuses -- validation by
        ``val_loader=`` included -- is refused here, before either tower runs.  With a ``LocalGather`` the one call makes and steps all
        the ranks' states, on either route."""
        import math
        from ..cocoopfit import NAMES
        who = "fit_prompt_learner"
        shard = _fit.checked_shard(who, fit_args, n_cls=self.prompt_learner.tokenized_prompts.shape[0])
        _fit.validation_set(who, self.clip_model, fit_args)
        fit_args.setdefault("logit_scale", math.log(self.scale))
        pl = self.prompt_learner
        params = {k: v.detach() for k, v in pl.state_dict().items() if k in NAMES}
        ids = pl.tokenized_prompts
        if transform is not None:
            from ..cocoopfit import CoCoOpFitState
            run, epochs, lr = _fit.split_fit_args(fit_args, 10, 0.002)
            E = int(self.clip_model.geometry.embed_dim)
            watch = _fit.split_monitor_args(who, fit_args, ids.shape[0], E)
            val_batch_size = fit_args.pop("val_batch_size", None)
            if watch["val"] is not None and val_batch_size is not None:
                from ..fitmonitor import _batch_size
                _batch_size(who, val_batch_size)
            from ..coopfit import shard_states
            state = shard_states(lambda sh: CoCoOpFitState(self.clip_model, ids, params, **dict(fit_args, shard=sh)), shard)
            state.val_stream_f16, state.val_batch_size = self.text_stream_f16, val_batch_size
            losses, monitor = _fit.run_with_transform(who, state, self.clip_model, ids.shape[0], E, train_loader, transform, epochs, lr, run, watch)
            fitted = _fit.pack(state.best_params() if watch["final_model"] == "best_val" else state.params(), losses)
            if monitor is not None:
                fitted = fitted + (monitor,) if isinstance(fitted, tuple) else (fitted, monitor)
        else:
            from ..cocoopfit import fit_prompt_learner
            feats, labels = _fit.cached_features(who, self.clip_model, train_loader)
            fit_args.setdefault("val_stream_f16", self.text_stream_f16)
            fitted = fit_prompt_learner(feats, labels, self.clip_model, ids, params, **fit_args)
        values = fitted[0] if isinstance(fitted, tuple) else fitted
        target = dict(pl.named_parameters())
        with torch.no_grad():
            for k in NAMES:
                target[k].copy_(values[k])
        return fitted

    @torch.no_grad()
    def forward(self, image: torch.Tensor, label=None, dac_conf: Optional[torch.Tensor] = None, want_conf_pred: bool = False):
        image_features = ops.l2_normalize(self.clip_model.image_features_f32(image))
        txt = self.per_image_text_features(image_features)
        logits, conf, pred, text_features = ops.logits_per_image(image_features, txt, self.scale, dac_conf, want_conf_pred)
        if want_conf_pred:
            return logits, image_features, text_features, conf, pred
        return logits, image_features, text_features
