"""TempScaling's one-parameter fit on the GPU (reference trainers/calibration/tempscaling.py:146-169) from cosine logits computed once.

The reference trains ``logit_scale`` with Dassl's epoch loop over ``dm.val_loader`` (tempscaling.py:143): every step runs both frozen
towers, forms ``exp(logit_scale) * cosine``, takes ``F.cross_entropy`` and one ``torch.optim.SGD`` step.  The base model is frozen and the
loader is sequential, so every epoch sees the same [N, C] cosine matrix: the fit is a function of that matrix, the labels and the
optimiser settings.  ``fit_logit_scale`` hands those to csrc/tempscale.hip, which enqueues every step of every epoch on the current stream
with no host synchronisation in between; the host reads the scalar back once at the end.

Dassl is not part of this repository's environment.  The defaults below -- SGD with momentum 0.9 and weight decay 5e-4, no dampening, no
Nesterov; a constant warm-up epoch that hands over to a cosine schedule; batches of 100 in the loader's sequential order, the last one
short -- restate Dassl's public defaults as the reference's configs select them (configs/trainers/CoOp/vit_b16_c16_ep200_batch32.yaml:15-22
with LR and MAX_EPOCH overridden at train.py:272-274, DATALOADER.TEST.BATCH_SIZE 100) and are UNVERIFIED here; that is why each of them is
an argument.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import fitloop, ops
from .fitloop import cosine_warmup_schedule, steps_per_epoch   # re-exported: tools and tests reach both through this module


def fit_logit_scale(cosine_logits: torch.Tensor, labels, init: float = 4.6052, epochs: int = 20, lr: float = 0.05, batch_size: int = 100,
                    momentum: float = 0.9, dampening: float = 0.0, weight_decay: float = 5e-4, nesterov: bool = False,
                    lr_per_epoch: Optional[Sequence[float]] = None, order=None, drop_last: bool = False, return_history: bool = False):
    """Fit TempScaling's ``logit_scale`` to ``cosine_logits`` fp32 [N, C] (on the GPU; the rows may be a column slice of a wider matrix)
    and ``labels`` [N]: ``epochs`` passes of ``torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov)`` on
    ``F.cross_entropy(exp(logit_scale) * cosine_logits[batch], labels[batch])``, starting from ``init``, in fp32 like ``ScaleLearner``.

    ``lr_per_epoch`` gives every epoch's rate; None takes ``cosine_warmup_schedule(lr, epochs)``.  ``order`` is an integer [epochs, N]
    array of sample indices, batch k of epoch e being ``order[e, k * batch_size : (k + 1) * batch_size]``; None is 0 .. N-1 in every
    epoch, the reference's sequential loader.  The last batch of an epoch is short unless ``drop_last`` drops it.

    Labels (and ``order``) are checked against their ranges on the host before anything is launched.  Returns the fitted scalar, or
    (scalar, per-step batch losses as a float32 numpy array) with ``return_history``.  The defaults are unverified restatements of
    Dassl's (module docstring)."""
    who = "fit_logit_scale"
    if not isinstance(cosine_logits, torch.Tensor) or cosine_logits.dim() != 2:
        raise ValueError(f"{who}: cosine_logits must be a [N, C] tensor")
    N, C = cosine_logits.shape
    if N < 1 or C < 2:
        raise ValueError(f"{who}: cosine_logits {(N, C)} need at least one row and two classes")
    epochs, batch_size = fitloop.check_run(who, epochs, batch_size)
    fitloop.check_sgd(who, momentum, dampening, weight_decay, nesterov)
    lab = fitloop._labels(who, labels, N, C)
    order = fitloop.check_order(who, order, epochs, N)
    per_epoch = steps_per_epoch(N, batch_size, drop_last)
    dev = cosine_logits.device
    _, lr_steps = fitloop.schedule(who, lr, epochs, lr_per_epoch, per_epoch, dev)
    fitloop._need_gpu(cosine_logits, "cosine_logits")
    if epochs * per_epoch == 0:
        return (float(np.float32(init)), np.zeros(0, np.float32)) if return_history else float(np.float32(init))
    state = torch.tensor([float(init), 0.0, 0.0, 0.0], dtype=torch.float32).to(dev)
    losses = ops.tempscale_fit(cosine_logits, fitloop.labels_on(labels, lab, dev), state, lr_steps, batch_size, epochs, momentum, dampening,
                               weight_decay, nesterov, fitloop.order_on(order, np.int32, dev), drop_last, want_losses=return_history)
    theta = float(state[0].item())   # the run's one synchronisation
    return (theta, losses.cpu().numpy()) if return_history else theta
