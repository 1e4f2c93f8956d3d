"""CoOp (reference trainers/classification/coop.py:47-222): the inference forward, and the context's training on the GPU
(``CustomCLIP.fit_context``, clip_calibration_amd/coopfit.py)."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from ..model import CLIP
from . import _fit


class TextEncoder(nn.Module):
    """coop.py:47-67.  ``forward(prompts, tokenized_prompts)``: the reference adds the positional embedding, runs
    ``clip_model.transformer``, ``ln_final``, gathers the EOT row and multiplies by ``text_projection``; here the same
    chain is one fused device call (clipmi_text_encoder)."""

    def __init__(self, clip_model: CLIP):
        super().__init__()
        object.__setattr__(self, "clip_model", clip_model)
        self.dtype = clip_model.dtype

    def forward(self, prompts: torch.Tensor, tokenized_prompts: torch.Tensor, compound_prompts_deeper_text=None,
                n_ctx: int = 0, flags: int = 0, seq_rows: Optional[int] = None) -> torch.Tensor:
        return self.clip_model.text_encoder_f32(prompts, tokenized_prompts, compound_prompts_deeper_text, n_ctx, flags=flags, seq_rows=seq_rows)


def n_ctx_from_init_ids(ctx_init_ids: torch.Tensor, context_length: int) -> int:
    """Number of context words of a CTX_INIT prompt from its token ids ``[1, L]`` = ``[SOT, w1..wn, EOT, 0...]``: the
    reference counts ``len(ctx_init.split(" "))`` (coop.py:82-84); here it is the EOT position (the largest id, as in
    ``clip.tokenize``) minus one, so both the zero-padded ``[1, 77]`` tensor ``tokenize`` returns and an unpadded
    ``[1, n+2]`` slice give n.  (For the templates the configs ship -- "a photo of a" -- every word is one token.)"""
    ids = ctx_init_ids.reshape(-1, ctx_init_ids.shape[-1])[0]
    n_ctx = int(ids.argmax()) - 1
    if not (1 <= n_ctx and 1 + n_ctx < context_length):
        raise ValueError(f"CTX_INIT ids give n_ctx={n_ctx}: expected [SOT, words.., EOT, padding] with 1 <= n_ctx < {context_length - 1}")
    return n_ctx


class PromptLearner(nn.Module):
    """coop.py:70-192.  ``tokenized_prompts`` are the ids of ``"X X ... X {classname}."`` (coop.py:107-112).

    ``class_token_position`` (TRAINER.COOP.CLASS_TOKEN_POSITION): "end" (the shipped configs), prompts = [SOS | ctx | class tokens, EOS,
    pad]; "middle", [SOS | ctx[:h] | name | ctx[h:] | '.', EOS, pad] with h = n_ctx // 2; "front", [SOS | name | ctx | '.', EOS, pad]
    (coop.py:146-190).  ``name_lens``: every class's name length in tokens (the reference's ``self.name_lens``); None derives
    ``eot - n_ctx - 2`` from the ids.  With the context on the GPU "middle" and "front" are assembled by one launch
    (``ops.prompt_place``) into fp32 prompts, which the text tower takes as it takes the fp16 ones -- not by a Python loop over the
    classes, which the reference runs on every batch."""

    def __init__(self, clip_model: CLIP, tokenized_prompts: torch.Tensor, n_ctx: int = 16, csc: bool = False,
                 ctx_init_ids: Optional[torch.Tensor] = None, seed: int = 0, class_token_position: str = "end", name_lens=None):
        super().__init__()
        dtype = clip_model.dtype
        dev = clip_model.device
        ctx_dim = clip_model.ln_final.weight.shape[0]
        n_cls = tokenized_prompts.shape[0]
        tokenized_prompts = tokenized_prompts.to(dev)
        with torch.no_grad():
            if ctx_init_ids is not None:  # CTX_INIT: embedding of the given words (coop.py:82-90)
                emb = clip_model.token_embedding(ctx_init_ids.to(dev)).type(dtype)
                n_ctx = n_ctx_from_init_ids(ctx_init_ids, tokenized_prompts.shape[-1])
                ctx_vectors = emb[0, 1:1 + n_ctx, :].clone()
            else:
                g = torch.Generator().manual_seed(seed)
                shape = (n_cls, n_ctx, ctx_dim) if csc else (n_ctx, ctx_dim)
                ctx_vectors = (0.02 * torch.randn(*shape, generator=g)).to(dev, dtype)
            embedding = clip_model.token_embedding(tokenized_prompts).type(dtype)
        if not 1 + n_ctx < tokenized_prompts.shape[-1]:
            raise ValueError(f"n_ctx={n_ctx} does not fit a context of {tokenized_prompts.shape[-1]} tokens")
        self.ctx = nn.Parameter(ctx_vectors)
        self.register_buffer("token_prefix", embedding[:, :1, :])            # SOS
        self.register_buffer("token_suffix", embedding[:, 1 + n_ctx:, :])    # class tokens, EOS, padding
        self.n_cls, self.n_ctx = n_cls, n_ctx
        self.tokenized_prompts = tokenized_prompts
        from ..coopfit import _placement
        placement = _placement("PromptLearner", tokenized_prompts, n_ctx, class_token_position, name_lens)
        self.class_token_position = class_token_position
        self.name_lens = None if name_lens is None else [int(n) for n in name_lens]   # as given: what fit_context hands to coopfit
        if placement is not None:   # what ops.prompt_place reads; neither is part of the state dict
            self.register_buffer("token_base", embedding.contiguous(), persistent=False)
            self.register_buffer("name_lens_i32", torch.from_numpy(placement[1]).to(dev), persistent=False)

    def forward(self) -> torch.Tensor:
        ctx = self.ctx
        if self.class_token_position != "end" and ctx.is_cuda:
            return ops.prompt_place(self.token_base, ctx.detach().float(), self.class_token_position, self.name_lens_i32)
        if ctx.dim() == 2:
            ctx = ctx.unsqueeze(0).expand(self.n_cls, -1, -1)
        ctx = ctx.to(self.token_prefix.dtype)
        if self.class_token_position == "end":
            return torch.cat([self.token_prefix, ctx, self.token_suffix], dim=1)  # layout only
        # a model on the CPU: the reference's loop (coop.py:146-190), layout only
        h = self.n_ctx // 2 if self.class_token_position == "middle" else 0
        rows = []
        for c, nl in enumerate(self.name_lens_i32.tolist()):
            name, rest = self.token_suffix[c:c + 1, :nl], self.token_suffix[c:c + 1, nl:]
            rows.append(torch.cat([self.token_prefix[c:c + 1], ctx[c:c + 1, :h], name, ctx[c:c + 1, h:], rest], dim=1))
        return torch.cat(rows, dim=0)


class CustomCLIP(nn.Module):
    """coop.py:192-222.  eval ``forward(image) -> (logits, image_features, text_features)``.

    The reference re-runs the 12-layer text tower on every batch although ``ctx`` is frozen at test time; the text
    features are cached here and recomputed only when ``ctx`` changes (same outputs; precedent in the reference:
    ProDA's set_classifier, proda.py:315-333).  ``logit_scale=1.0`` gives the cosine-logit base model of
    trainers/calibration/base_model/coop.py:222-224.

    ``cache_text_features=False`` is the reference's own schedule (coop.py:208-210: prompt learner + text tower on every
    batch).  The text tower is then per-batch work, and ``text_stream_f16`` (None = "when not cached") runs it on the fp16
    residual stream -- the reference's own GPU precision, clip/model.py:186-187 -- through the per-call flag
    CLIPMI_CALL_STREAM_F16, as the CoCoOp mirror does: -17 % per text tower call at 500 classes
    (profiles/r03_bench_coop_dac.json).  Cached features keep the fp32 stream: they are computed once and feed every logit."""

    text_stream_f16: Optional[bool] = None   # class default for mirrors that build themselves (MaPLe)

    def __init__(self, clip_model: CLIP, tokenized_prompts: torch.Tensor, n_ctx: int = 16, csc: bool = False,
                 logit_scale: Optional[float] = None, cache_text_features: bool = True,
                 text_stream_f16: Optional[bool] = None, **kw):
        super().__init__()
        self.text_stream_f16 = text_stream_f16
        self.prompt_learner = PromptLearner(clip_model, tokenized_prompts, n_ctx, csc, **kw)
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

    @property
    def scale(self) -> float:
        return float(self._fixed_scale) if self._fixed_scale is not None else float(self.logit_scale.detach().exp())

    def _text_inputs(self):
        return self.prompt_learner(), None, 0

    def _text_flags(self) -> int:
        from .. import _lib
        want = (not self.cache_text_features) if self.text_stream_f16 is None else self.text_stream_f16
        m = self.clip_model
        # a model (or process) set to residual_f16 != 2 or ln_fold = 0 has chosen its streams explicitly: no per-call override
        if want and m.get_option("residual_f16") == 2 and m.get_option("ln_fold") == 1:
            return _lib.CALL_STREAM_F16
        return _lib.CALL_DEFAULT

    def _cache_params(self):
        """Everything the cached text features depend on (besides the frozen tower weights)."""
        return list(self.prompt_learner.parameters())

    @torch.no_grad()
    def text_features(self) -> torch.Tensor:
        key = tuple((p.data_ptr(), p._version) for p in self._cache_params())
        if self.cache_text_features and key == self._cache_key and self._cache is not None:
            return self._cache
        prompts, deep, n_ctx = self._text_inputs()
        # the live token rows of the class list, from the OWNER's copy of the ids and the owner's table (one read-back per prompt set, ever): under
        # nn.DataParallel a replica's buffers are re-broadcast -- new tensors -- on every forward, and a per-forward bound would sync every device
        m = self.clip_model
        rows = m._home().live_rows(self.prompt_learner.tokenized_prompts, n_ctx if deep else 0) if hasattr(m, "_home") else None
        tf = ops.l2_normalize(self.text_encoder(prompts, self.tokenized_prompts, deep, n_ctx, flags=self._text_flags(), seq_rows=rows))
        self._cache_key, self._cache = key, tf
        return tf

    def _image_features(self, image: torch.Tensor) -> torch.Tensor:
        return self.clip_model.image_features_f32(image)

    def fit_context(self, train_loader, transform=None, **fit_args):
        """Train ``prompt_learner.ctx`` on the GPU, starting from the parameter's values, with ``logit_scale`` taken from this model
        unless ``fit_args`` say otherwise (coop.py:282-309 with both towers frozen).  The fitted context is copied into
        ``prompt_learner.ctx`` in the parameter's dtype (the fit itself keeps an fp32 master copy) -- that moves the parameter's
        version, so the cached text features retire on their own -- and returned as ``coopfit.fit_context`` returns it.

        ``transform=None``: one pass of ``train_loader`` (an iterable of (image, label) batches of preprocessed images) through the
        frozen image tower, the raw features and the labels kept on the device, then ``coopfit.fit_context(features, labels, clip_model,
        tokenized_prompts, ctx, **fit_args)``.  Caching the features equals the reference's loop only for a DETERMINISTIC train
        transform; the reference's config trains with ``random_resized_crop`` + ``random_flip``.

        ``transform=TrainPreprocess(...)`` is that regime: ``train_loader`` yields (decoded uint8 images, labels) and is iterated once
        per epoch, every batch going transform -> image tower -> ``CoOpFitState.step`` with nothing synchronising until the end
        (``augment.fit_with_transform``).  ``fit_args``: ``epochs`` (200), ``lr`` (0.002), ``lr_per_epoch``, the optimiser's
        ``momentum``, ``dampening``, ``weight_decay``, ``nesterov``, ``grad_scale``, ``seq_rows``, ``views`` and ``return_history``;
        the batch size and the order are the loader's.  ``grad_scale="dynamic"`` with ``scaler=dict(init_scale, growth_factor,
        backoff_factor, growth_interval)`` is the reference's ``amp`` branch on either route (``coopfit``'s module docstring): a step
        that overflows fp16 is skipped on the device and the scale adapts, with no read-back per step.  The prompt learner's
        ``class_token_position`` and ``name_lens`` go to ``coopfit`` with it.

        Validation (the cached route): ``val_loader=`` (an iterable of (image, label) batches, run through the image tower once before the
        first epoch, as the train features are) or ``val=(val_features, val_labels)``, with ``val_bins``, ``final_model`` ("last_step" or
        "best_val", the reference's TEST.FINAL_MODEL), ``val_criterion`` and ``return_monitor`` as ``coopfit.fit_context`` takes them.
        ``final_model="best_val"`` installs the best epoch's context into the prompt learner.

        ``shard=coopfit.Shard(world, rank, gather)`` on either route: the class-sharded fit, one process per GPU, every rank making
        this call on the same data (``coopfit``'s module docstring; KgCoOp's and ProGrad's ``fit_context`` pass it on).  What ``shard``
        refuses -- validation by ``val_loader=`` included -- is refused here, before either tower runs.  With a ``LocalGather`` the one
        call makes and steps all the ranks' states, on either route."""
        import math
        shard = _fit.checked_shard("fit_context", fit_args, "coop", n_cls=self.prompt_learner.tokenized_prompts.shape[0], grad_scale=fit_args.get("grad_scale"),
                                   class_token_position=fit_args.get("class_token_position", getattr(self.prompt_learner, "class_token_position", "end")))
        val_loader = fit_args.pop("val_loader", None)
        if val_loader is not None and fit_args.get("val") is not None:
            raise ValueError("fit_context: val_loader and val are two ways to give one validation set")
        monitored = val_loader is not None or any(k in fit_args for k in ("val", "val_bins", "final_model", "val_criterion", "return_monitor"))
        if transform is not None and monitored:
            raise ValueError("fit_context: validation and final_model belong to the cached route (transform=None)")
        if val_loader is not None:
            fit_args["val"] = _fit.cached_features("fit_context", self.clip_model, val_loader)
        fit_args.setdefault("logit_scale", math.log(self.scale))
        ctx = self.prompt_learner.ctx
        ids = self.prompt_learner.tokenized_prompts
        fit_args.setdefault("class_token_position", getattr(self.prompt_learner, "class_token_position", "end"))
        fit_args.setdefault("name_lens", getattr(self.prompt_learner, "name_lens", None))
        if transform is not None:
            from ..augment import fit_with_transform
            from ..coopfit import CoOpFitState, shard_states
            run, epochs, lr = _fit.split_fit_args(fit_args, 200, 0.002)
            state = shard_states(lambda sh: CoOpFitState(self.clip_model, ids, ctx.detach(), **dict(fit_args, shard=sh)), shard)
            losses = fit_with_transform(state, self.clip_model.image_features_f32, ids.shape[0], train_loader, transform, epochs, lr, **run)
            fitted = _fit.pack(state.gathered_context(), losses)   # state.ctx, but for a class-specific context under shard=
        else:
            from ..coopfit import fit_context
            feats, labels = _fit.cached_features("fit_context", self.clip_model, train_loader)
            fitted = fit_context(feats, labels, self.clip_model, ids, ctx.detach(), **fit_args)
        with torch.no_grad():
            ctx.copy_(fitted[0] if isinstance(fitted, tuple) else fitted)
        return fitted

    overlap_towers: bool = True   # per-batch text tower (cache_text_features=False): run it on a side stream beside the image tower

    @torch.no_grad()
    def towers(self, image: torch.Tensor):
        """(image features fp32 un-normalised, text features fp32 normalised) of one batch.  With the reference's per-batch schedule
        (coop.py:208-210: prompt learner + text tower on every batch) the two towers are independent until the logits, so the text tower
        is issued on a side stream and the image tower on the caller's; the caller's stream then waits for the side stream.  They use
        separate workspaces (the model's "text" and "vision" buffers)."""
        if self.cache_text_features or not self.overlap_towers or not image.is_cuda:
            text_features = self.text_features()
            return self._image_features(image), text_features
        # Weight binding is lazy and packs BOTH towers with torch ops on whatever stream is current: do it here, on the caller's stream,
        # so that the side stream (which waits for this point) and the caller's stream both see finished operands.
        self.clip_model._resident(image.device)._ensure_bound()
        cur = torch.cuda.current_stream(image.device)
        side = getattr(self, "_side_stream", None)
        if side is None or side.device != image.device:
            side = torch.cuda.Stream(device=image.device)
            object.__setattr__(self, "_side_stream", side)
        side.wait_stream(cur)                       # the prompt learner's parameters may have been written on the caller's stream
        with torch.cuda.stream(side):
            text_features = self.text_features()
        image_features = self._image_features(image)
        cur.wait_stream(side)
        text_features.record_stream(cur)
        return image_features, text_features

    @torch.no_grad()
    def forward(self, image: torch.Tensor, label=None, dac_conf: Optional[torch.Tensor] = None, want_conf_pred: bool = False):
        image_features_raw, text_features = self.towers(image)
        logits, image_features, conf, pred = ops.fused_tail(image_features_raw, text_features, self.scale, dac_conf,
                                                            want_conf_pred)
        if want_conf_pred:
            return logits, image_features, text_features, conf, pred
        return logits, image_features, text_features
