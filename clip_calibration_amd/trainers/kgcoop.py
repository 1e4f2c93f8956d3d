"""KgCoOp (reference trainers/classification/kgcoop.py:90-271): the inference forward, and the context's training on the GPU
(``CustomCLIP.fit_context``, clip_calibration_amd/coopfit.py with ``method="kgcoop"``).

At test time KgCoOp is CoOp with ``ctx`` initialised from the embedding of "a photo of a" (n_ctx = 4,
kgcoop.py:102-112) plus a stored zero-shot text embedding ``ori_embedding`` (kgcoop.py:151-165).  ``forward``
(kgcoop.py:246-259) returns the same 3-tuple as CoOp.  In training the loss is CoOp's cross-entropy plus
``w (1 - mean_c cos(text_c, ori_embedding_c))`` (kgcoop.py:261-269, W = 8.0): one backward per step, as CoOp.  The
optimiser's defaults are CoOp's restatements of Dassl's and as unverified as there (coopfit.py)."""
from __future__ import annotations

import torch

from .. import ops
from .coop import CustomCLIP as _CoOpCLIP


class CustomCLIP(_CoOpCLIP):
    def __init__(self, clip_model, tokenized_prompts, zeroshot_tokenized_prompts=None, ctx_init_ids=None, n_ctx: int = 4,
                 w: float = 8.0, **kw):
        super().__init__(clip_model, tokenized_prompts, n_ctx=n_ctx, ctx_init_ids=ctx_init_ids, **kw)
        self.w = w
        self.ori_embedding = None
        if zeroshot_tokenized_prompts is not None:
            with torch.no_grad():  # kgcoop.py:160-165: encode_text of the hand-written prompts, L2-normalised
                self.ori_embedding = ops.l2_normalize(clip_model.text_features_f32(zeroshot_tokenized_prompts.to(clip_model.device)))

    def fit_context(self, train_loader, transform=None, **fit_args):
        """``coop.CustomCLIP.fit_context`` with KgCoOp's loss: ``method="kgcoop"``, ``teacher=self.ori_embedding`` and ``w=self.w``
        unless ``fit_args`` say otherwise.  Needs the ``zeroshot_tokenized_prompts`` the model was built with.  ``grad_scale="dynamic"``
        and ``scaler`` (the reference's ``amp`` branch, kgcoop.py) pass through on both routes as they do for CoOp."""
        if fit_args.get("teacher", self.ori_embedding) is None:
            raise ValueError("kgcoop.CustomCLIP.fit_context: no ori_embedding -- build the model with zeroshot_tokenized_prompts")
        fit_args.setdefault("method", "kgcoop")
        fit_args.setdefault("teacher", self.ori_embedding)
        fit_args.setdefault("w", self.w)
        return super().fit_context(train_loader, transform, **fit_args)
