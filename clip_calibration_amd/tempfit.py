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

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import ops


def cosine_warmup_schedule(lr: float, epochs: int, warmup_epochs: int = 1, warmup_lr: float = 1e-5) -> List[float]:
    """The learning rate of every epoch under OPTIM.LR_SCHEDULER "cosine" with WARMUP_TYPE "constant": ``warmup_lr`` for the first
    ``warmup_epochs`` epochs, then ``torch.optim.lr_scheduler.CosineAnnealingLR(T_max=epochs)``.  The hand-over rule (Dassl's
    ConstantWarmupScheduler as publicly documented, unverified here): the cosine scheduler is not stepped while the warm-up lasts and is
    stepped once at the end of every epoch from the last warm-up epoch on, so epoch ``e >= warmup_epochs`` runs at the cosine value of
    index ``e - warmup_epochs + 1``: ``lr * (1 + cos(pi * (e - warmup_epochs + 1) / epochs)) / 2``.  Without a warm-up epoch ``e`` runs at
    index ``e``."""
    epochs, warmup_epochs = int(epochs), int(warmup_epochs)
    if epochs < 0 or warmup_epochs < 0:
        raise ValueError(f"cosine_warmup_schedule: epochs={epochs}, warmup_epochs={warmup_epochs} (both >= 0)")
    out = []
    for e in range(epochs):
        if e < warmup_epochs:
            out.append(float(warmup_lr))
        else:
            t = e - warmup_epochs + 1 if warmup_epochs > 0 else e
            out.append(float(lr) * (1.0 + math.cos(math.pi * t / epochs)) / 2.0)
    return out


def steps_per_epoch(n: int, batch_size: int, drop_last: bool = False) -> int:
    return n // batch_size if drop_last else -(-n // batch_size)


def _host_int_array(x, name: str) -> np.ndarray:
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.dtype.kind not in "iu":
        raise TypeError(f"fit_logit_scale: {name} must be integers, got {a.dtype}")
    return a


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
    if not isinstance(cosine_logits, torch.Tensor) or cosine_logits.dim() != 2:
        raise ValueError("fit_logit_scale: cosine_logits must be a [N, C] tensor")
    N, C = cosine_logits.shape
    epochs, batch_size = int(epochs), int(batch_size)
    if N < 1 or C < 2:
        raise ValueError(f"fit_logit_scale: cosine_logits {(N, C)} need at least one row and two classes")
    if epochs < 0 or batch_size < 1:
        raise ValueError(f"fit_logit_scale: epochs={epochs} (>= 0), batch_size={batch_size} (>= 1)")
    if not (0.0 <= momentum < 1.0 and 0.0 <= dampening < 1.0 and weight_decay >= 0.0):
        raise ValueError(f"fit_logit_scale: momentum={momentum}, dampening={dampening} (both in [0, 1)), weight_decay={weight_decay} (>= 0)")
    if nesterov and (momentum <= 0.0 or dampening != 0.0):
        raise ValueError("fit_logit_scale: Nesterov momentum requires a momentum and zero dampening")
    lab = _host_int_array(labels, "labels")
    if lab.shape != (N,):
        raise ValueError(f"fit_logit_scale: {N} rows need {N} labels, got {lab.shape}")
    if lab.min() < 0 or lab.max() >= C:
        raise ValueError(f"fit_logit_scale: labels span [{int(lab.min())}, {int(lab.max())}], outside the {C} classes [0, {C})")
    if order is not None:
        order = _host_int_array(order, "order")
        if order.shape != (epochs, N):
            raise ValueError(f"fit_logit_scale: order {order.shape} must be [epochs, N] = [{epochs}, {N}]")
        if order.size and (order.min() < 0 or order.max() >= N):
            raise ValueError(f"fit_logit_scale: order holds sample indices outside [0, {N})")
    rates = cosine_warmup_schedule(lr, epochs) if lr_per_epoch is None else [float(r) for r in lr_per_epoch]
    if len(rates) != epochs:
        raise ValueError(f"fit_logit_scale: {len(rates)} learning rates for {epochs} epochs")
    per_epoch = steps_per_epoch(N, batch_size, drop_last)
    if not cosine_logits.is_cuda:
        raise RuntimeError(f"clipmi: `cosine_logits` must be a tensor on the GPU (got {cosine_logits.device}); the HIP path has no CPU fallback")
    dev = cosine_logits.device
    if epochs * per_epoch == 0:
        return (float(np.float32(init)), np.zeros(0, np.float32)) if return_history else float(np.float32(init))
    state = torch.tensor([float(init), 0.0, 0.0, 0.0], dtype=torch.float32).to(dev)
    lr_steps = torch.from_numpy(np.repeat(np.asarray(rates, np.float64), per_epoch).astype(np.float32)).to(dev)
    labels_d = torch.from_numpy(lab.astype(np.int64)).to(dev) if not (isinstance(labels, torch.Tensor) and labels.is_cuda
                                                                      and labels.dtype == torch.int64) else labels
    order_d = None if order is None else torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(dev)
    losses = ops.tempscale_fit(cosine_logits, labels_d, state, lr_steps, batch_size, epochs, momentum, dampening, weight_decay, nesterov,
                               order_d, drop_last, want_losses=return_history)
    theta = float(state[0].item())   # the run's one synchronisation
    return (theta, losses.cpu().numpy()) if return_history else theta
