"""ProGrad (reference trainers/classification/prograd.py:230-450): the inference forward, and the context's training on the GPU
(``CustomCLIP.fit_context``, clip_calibration_amd/coopfit.py with ``method="prograd"``).

At test time ProGrad IS CoOp: ``CustomCLIP.forward`` (prograd.py:272-289) runs the prompt learner's ``[SOS | ctx | class]``
splice through the text tower and returns the same 3-tuple.  What distinguishes the method lives in the training loop
(prograd.py:291-306, 371-409): two losses of one forward, the cross-entropy and the distillation loss against the logits of the
frozen zero-shot teacher ``CLIP`` (prograd.py:230-259, ``ZeroshotCLIP`` with the hand-written templates), two backward passes, and
the cross-entropy's gradient applied without its component along the other one where the two conflict.  ``T`` = 1.0 and ``lam`` =
1.0 are what every shipped config sets.  Not mirrored and unverified: the reference's ``amp`` branch (prograd.py:415-424), which
hands ``GradScaler.scale`` a tuple; Dassl's optimiser defaults are CoOp's restatements (coopfit.py)."""
from __future__ import annotations

import torch

from .. import ops
from .coop import CustomCLIP as _CoOpCLIP
from .zsclip import ZeroshotCLIP as CLIP  # noqa: F401


class CustomCLIP(_CoOpCLIP):
    """prograd.py:262-289, the same forward and the same cache as CoOp.  ``zeroshot_tokenized_prompts``: the ids of the hand-written
    prompts; their L2-normalised text features, the reference's ``CLIP.text_features`` (prograd.py:242-247), are computed once."""

    def __init__(self, clip_model, tokenized_prompts, zeroshot_tokenized_prompts=None, T: float = 1.0, lam: float = 1.0, **kw):
        super().__init__(clip_model, tokenized_prompts, **kw)
        self.T, self.lam = T, lam
        self.zs_text_features = None
        if zeroshot_tokenized_prompts is not None:
            with torch.no_grad():
                self.zs_text_features = ops.l2_normalize(clip_model.text_features_f32(zeroshot_tokenized_prompts.to(clip_model.device)))

    def fit_context(self, train_loader, transform=None, **fit_args):
        """``coop.CustomCLIP.fit_context`` with ProGrad's step: ``method="prograd"``, ``teacher=self.zs_text_features``, ``T=self.T``
        and ``lam=self.lam`` unless ``fit_args`` say otherwise.  Needs the ``zeroshot_tokenized_prompts`` the model was built with.
        With ``return_history`` the losses are the cross-entropy's."""
        if fit_args.get("teacher", self.zs_text_features) is None:
            raise ValueError("prograd.CustomCLIP.fit_context: no zero-shot text features -- build the model with zeroshot_tokenized_prompts")
        fit_args.setdefault("method", "prograd")
        fit_args.setdefault("teacher", self.zs_text_features)
        fit_args.setdefault("T", self.T)
        fit_args.setdefault("lam", self.lam)
        return super().fit_context(train_loader, transform, **fit_args)
