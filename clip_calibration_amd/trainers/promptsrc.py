"""PromptSRC / IVLP (reference trainers/classification/promptsrc.py:73-317): the inference forward and training on the GPU.

At test time PromptSRC is CoOp's prompt splice (``[SOS | ctx | class tokens]``, promptsrc.py:141-171) run through a CLIP
built with the IVLP design, whose blocks carry their own per-layer prompt tokens on both towers (clip/model.py:191-256).
Those tokens live in the model (``build_model(..., {"trainer": "IVLP", ...})``), so the forward is CoOp's; the only
addition is that the text-feature cache also watches the model's text-side tokens.

Training (``fit_prompts``) reads the frozen teacher branch of the loss (promptsrc.py:197-210): ``teacher_text_features`` is the
reference's ``fixed_embeddings`` (``teacher_features`` computes it from the caller's own templates), and the frozen image tower
(``ZS_image_encoder``) is this model's own tower run without its prompt tokens -- ``promptsrcfit`` has the step."""
from __future__ import annotations

import torch

from . import _fit
from .coop import CustomCLIP as _CoOpCLIP


def teacher_features(clip_model, tokenized_templates: torch.Tensor) -> torch.Tensor:
    """The frozen text features of hand-written templates averaged per class, fp32 [C, E], NOT normalised (the loss head normalises):
    ``tokenized_templates`` [C, T, context_length] (or [C, context_length] for one template per class).  A prompt-free pass: the
    model's own text-side prompt tokens are not spliced in, as the reference computes ``fixed_embeddings`` on a plain CLIP
    (promptsrc.py:110-135).  The reference's template list is not restated here: the caller passes its own."""
    import ctypes as C
    from .. import _lib, ops
    from .._lib import check, lib
    if tokenized_templates.dim() == 2:
        tokenized_templates = tokenized_templates.unsqueeze(1)
    Cn, T, L = tokenized_templates.shape
    m = clip_model
    m._ensure_bound()
    ids = ops._dev(tokenized_templates.reshape(Cn * T, L).to(m.device), "tokenized_templates", (torch.int64,))
    if L != m.geometry.context_length:
        raise ValueError(f"teacher_features: expected ids [C, T, {m.geometry.context_length}], got {tuple(tokenized_templates.shape)}")
    out = torch.empty(Cn * T, m.geometry.embed_dim, dtype=torch.float32, device=ids.device)
    rows = m.live_rows(ids)
    with m._launch_lock:
        ws = m._workspace("text", lib.clipmi_text_workspace_bytes(m._handle, Cn * T, rows))
        check(lib.clipmi_encode_text(m._handle, ids.data_ptr(), Cn * T, rows, out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.CALL_DEFAULT,
                                     ops._stream()), "clipmi_encode_text")
    return ops.group_mean(out, T)


class CustomCLIP(_CoOpCLIP):
    def __init__(self, clip_model, tokenized_prompts, n_ctx: int = 4, **kw):
        if clip_model.design_details.get("trainer") != "IVLP" or int(clip_model.design_details.get("language_depth", 0)) < 1:
            raise ValueError("PromptSRC needs a CLIP built with design_details trainer='IVLP' and language_depth >= 1 "
                             "(promptsrc.py:77-80)")
        super().__init__(clip_model, tokenized_prompts, n_ctx=n_ctx, **kw)

    def _cache_params(self):
        deep, _ = self.clip_model.ivlp_text_prompts()
        return list(self.prompt_learner.parameters()) + list(deep or [])

    def prompt_params(self):
        """``prompt_learner.ctx`` and the model's own ``VPT`` / ``VPT_shallow`` parameters under ``promptsrcfit``'s names."""
        from .. import promptsrcfit
        return promptsrcfit.model_params(self.clip_model, self.prompt_learner.ctx)

    def fit_prompts(self, train_loader, teacher_text_features, transform=None, **fit_args):
        """Train ``prompt_learner.ctx`` and the model's ``visual.VPT`` and ``VPT_shallow`` tokens on the GPU with PromptSRC's
        self-regularising losses (or, with ``method="ivlp"``, plain cross-entropy), starting from the parameters' values, with
        ``logit_scale`` taken from this model unless ``fit_args`` say otherwise (promptsrc.py:186-210, 298-341 with both towers frozen).
        ``teacher_text_features`` [C, E] is the caller's ``fixed_embeddings`` (``teacher_features``).  The fitted block -- after the
        Gaussian-weighted aggregation over the epochs unless ``gpa=None`` -- is copied into the parameters in place, each in its own
        dtype (the fit keeps fp32 masters); that moves their versions, so the cached text features retire on their own, and the cache
        is dropped as well; a following ``encode_image`` reads the new tokens.  Returned as ``promptsrcfit.fit_prompts`` returns it.

        ``transform=None``: ``train_loader`` is a sized iterable of (preprocessed images, labels) batches, iterated once per epoch.
        ``transform=TrainPreprocess.for_model(model)``: it yields (decoded uint8 images, labels) and every batch goes transform ->
        ``PromptSRCFitState.step`` with nothing synchronising until the end (``augment.fit_with_transform``).  ``fit_args``: ``epochs``
        (50), ``lr`` (0.0025), ``lr_per_epoch``, ``method``, ``w_text``, ``w_image``, ``w_logit``, ``gpa``, the optimiser's ``momentum``,
        ``dampening``, ``weight_decay``, ``nesterov``, ``grad_scale``, ``seq_rows``, ``views`` (with a transform) and
        ``return_history`` and ``one_call``; the batch size and the order are the loader's (``batch_size`` / ``drop_last`` are refused).
        ``grad_scale="dynamic"`` with ``scaler=dict(init_scale, growth_factor, backoff_factor, growth_interval)``, for ``method="ivlp"``
        as well: the device-side loss scale (``promptsrcfit``'s module docstring).

        Validation, on either route: ``val_loader=`` (a sized iterable of (test-transformed images, labels) batches on the GPU, iterated
        once per epoch) or ``val=(val_images_or_loader, val_labels)``, with ``val_batch_size``, ``val_bins``, ``final_model``
        ("last_step" or "best_val", the reference's TEST.FINAL_MODEL), ``val_criterion`` and ``return_monitor`` as
        ``promptsrcfit.fit_prompts`` takes them: the GPA work of an epoch comes before its validation, so the last epoch scores the
        aggregate.  Validation images go through the test transform, never through ``transform``.  ``final_model="best_val"`` installs
        the best epoch's parameters."""
        import math
        from .. import promptsrcfit
        shard = _fit.checked_shard("fit_prompts", fit_args, "block")
        _fit.validation_set("fit_prompts", None, fit_args)
        fit_args.setdefault("logit_scale", math.log(self.scale))
        fit_args.setdefault("class_token_position", getattr(self.prompt_learner, "class_token_position", "end"))
        ids, params = self.prompt_learner.tokenized_prompts, self.prompt_params()
        if transform is not None:
            from ..augment import fit_with_transform
            for k in ("batch_size", "drop_last"):
                if k in fit_args:
                    raise ValueError(f"fit_prompts: {k} belongs to a tensor of images; with a transform the batches are the loader's")
            one_call = bool(fit_args.pop("one_call", False))
            run, epochs, lr = _fit.split_fit_args(fit_args, 50, 0.0025)
            epochs = int(epochs)
            gpa = fit_args.pop("gpa", (30.0, 30.0))
            watch = _fit.split_monitor_args("fit_prompts", fit_args)
            from ..coopfit import shard_states
            state = shard_states(lambda sh: promptsrcfit.PromptSRCFitState(self.clip_model, ids, params, teacher_text_features, **dict(fit_args, shard=sh)),
                                 shard)
            weights = None if fit_args.get("method", "promptsrc") == "ivlp" else promptsrcfit._gpa_for("fit_prompts", gpa, epochs)

            def aggregate(e: int) -> None:
                state.end_epoch(float(weights[e]))
                if e == epochs - 1:
                    state.apply_gpa()

            end, monitored = _fit.image_end_epoch(state, watch, epochs, len(train_loader), None if weights is None else aggregate)
            stepper = state if not one_call else type("OneCall", (), {"step": staticmethod(
                lambda x, y, r, want_loss=False: state.step(x, y, r, want_loss=want_loss, one_call=True))})()
            losses = fit_with_transform(stepper, lambda x: x, ids.shape[0], train_loader, transform, epochs, lr, end_epoch=end, **run)
            best = monitored and watch["final_model"] == "best_val"
            fitted = _fit.pack_monitored(state, state.best_params() if best else state.params(), losses, watch, monitored)
        else:
            fitted = promptsrcfit.fit_prompts(train_loader, None, self.clip_model, ids, teacher_text_features, params, **fit_args)
        block = fitted[0] if isinstance(fitted, tuple) else fitted
        with torch.no_grad():
            for name, p in params.items():
                p.copy_(block[name])
        self._cache_key = self._cache = None
        return fitted
