"""TaskRes' text residuals trained on the GPU (reference trainers/classification/taskres.py:96-210).

The reference trains one tensor, the residual matrix ``text_feature_residuals`` [C, E] of the classifier ``base_text_features + alpha *
residuals``, with Dassl's epoch loop: every step runs the frozen image tower, normalises both sides, takes ``F.cross_entropy`` of
``exp(logit_scale)`` times the cosine and one optimiser step on the residuals.  Both towers and ``logit_scale`` are frozen and the base
text features are computed once: a step is a function of the image features, the labels, the base text features, ``alpha`` and the
optimiser state.  csrc/taskres_train.hip computes forward, backward and the optimiser's step (``torch.optim.Adam``'s rule, or
``torch.optim.SGD``'s) in three launches per step, all in fp32 as the reference's ``model.float()`` has it, with no autograd graph.

Two ways in.  ``fit_residuals`` trains from a cached [N, E] feature matrix and enqueues every step of every epoch on the current stream
with no synchronisation between the steps and one at the end (labels that arrive on the GPU are copied to the host once, before the first
launch, for their range check): that equals the reference's loop only when the train transform is deterministic, since the reference's
``random_resized_crop`` + ``random_flip`` change the features every epoch.  ``TaskResFitState.step`` takes one batch of features at a
time, for callers that run the image tower on every step: ``TaskResCLIP.fit_residuals(loader, transform=TrainPreprocess(...))`` is that
caller, with the reference's train transform computed on the device (clip_calibration_amd/augment.py).

Dassl is not part of this repository's environment.  The defaults below -- Adam at 2e-4 with betas (0.9, 0.999), eps 1e-8 and weight
decay 5e-4 (for SGD: momentum 0.9, no dampening, no Nesterov); 200 epochs in batches of 256, the last short batch dropped; a constant
warm-up epoch at 1e-5 that hands over to a cosine schedule -- restate configs/trainers/TaskRes/vit_b16_c16_ep200_batch256.yaml and
Dassl's public defaults and are UNVERIFIED here; that is why each of them is an argument.  ``alpha`` defaults to the mirror trainer's
0.5 (the reference's train.py sets RESIDUAL_SCALE 1.0; ``CustomCLIP.fit_residuals`` passes the model's own).  Dassl's random sampler is
the caller's ``order``.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import fitloop, fitmonitor, ops
from .fitloop import _need_gpu, steps_per_epoch


def _check_optimiser(who: str, optimizer: str, betas, eps: float, weight_decay: float, momentum: float, dampening: float, nesterov: bool) -> None:
    if optimizer not in ("adam", "sgd"):
        raise ValueError(f"{who}: optimizer {optimizer!r} must be 'adam' or 'sgd'")
    if optimizer == "adam":
        if not weight_decay >= 0.0 or not math.isfinite(weight_decay):
            raise ValueError(f"{who}: weight_decay={weight_decay} (finite, >= 0)")
        if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
            raise ValueError(f"{who}: betas={tuple(betas)} (two values in [0, 1))")
        if not eps >= 0.0 or not math.isfinite(eps):
            raise ValueError(f"{who}: eps={eps} (finite, >= 0)")
        return
    fitloop.check_sgd(who, momentum, dampening, weight_decay, nesterov)


def _check_shapes(who: str, features, base, residuals) -> Tuple[int, int, int]:
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] < 1:
        raise ValueError(f"{who}: features must be a [N >= 1, E] tensor")
    N, E = features.shape
    if not isinstance(base, torch.Tensor) or base.dim() != 2 or base.shape[1] != E or base.shape[0] < 2:
        raise ValueError(f"{who}: base text features {tuple(getattr(base, 'shape', ()))} must be [C >= 2, E = {E}]")
    if residuals is not None and (not isinstance(residuals, torch.Tensor) or residuals.shape != base.shape):
        raise ValueError(f"{who}: residuals {tuple(getattr(residuals, 'shape', ()))} must have the base text features' shape {tuple(base.shape)}")
    return N, E, base.shape[0]


def _master(base: torch.Tensor, residuals: Optional[torch.Tensor], dev) -> torch.Tensor:
    """A fresh contiguous fp32 copy on the device (zeros without ``residuals``): the master values the kernels update in place."""
    if residuals is None:
        return torch.zeros(tuple(base.shape), dtype=torch.float32, device=dev)
    return fitloop.master(residuals, dev)


def _state(r: torch.Tensor, optimizer: str, momentum: float):
    if optimizer == "adam":
        return torch.zeros_like(r), torch.zeros_like(r)
    return (torch.zeros_like(r) if momentum != 0.0 else None), None


def fit_residuals(features: torch.Tensor, labels, base_text_features: torch.Tensor, residuals: Optional[torch.Tensor] = None, alpha: float = 0.5,
                  logit_scale: float = 4.6052, optimizer: str = "adam", lr: float = 2e-4, epochs: int = 200, batch_size: int = 256,
                  betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 5e-4, momentum: float = 0.9,
                  dampening: float = 0.0, nesterov: bool = False, lr_per_epoch: Optional[Sequence[float]] = None, order=None,
                  drop_last: bool = True, return_history: bool = False, val=None, val_bins: int = 10, final_model: str = "last_step",
                  val_criterion: str = "accuracy", return_monitor: bool = False):
    """Train TaskRes' residuals on cached ``features`` fp32 [N, E] (raw, un-normalised image features on the GPU; the rows may be a
    column slice of a wider matrix), ``labels`` [N] and the frozen ``base_text_features`` fp32 [C, E] (not normalised), starting from
    ``residuals`` [C, E] (not modified; None = zeros, the reference's initialisation): ``epochs`` passes of ``torch.optim.Adam(lr, betas,
    eps, weight_decay)`` -- or, with ``optimizer="sgd"``, ``torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov)`` -- on
    ``F.cross_entropy(exp(logit_scale) * normalise(f) @ normalise(base + alpha * residuals).T, labels)`` over batches of ``batch_size``,
    all in fp32.

    ``lr_per_epoch`` gives every epoch's rate; None takes ``cosine_warmup_schedule(lr, epochs)``.  ``order`` is an integer [epochs, N]
    array of sample indices, batch k of epoch e being ``order[e, k * batch_size : (k + 1) * batch_size]``; None is 0 .. N-1 in every
    epoch.  The last batch of an epoch is short unless ``drop_last`` drops it.

    Labels (and ``order``) are checked against their ranges on the host before anything is launched -- a label tensor on the GPU is
    copied to the host for that, which waits for whatever produced it; from the first launch on nothing synchronises until the one wait
    at the end.  Returns the fitted fp32 residuals on the device, or ``(residuals, per-step batch losses as a float32 numpy array)`` with
    ``return_history``.  The defaults are unverified restatements of the reference's config and Dassl's (module docstring).

    ``val=(val_features, val_labels)`` (raw image features [N_val, E] on the GPU and their labels): behind the last step of every epoch
    the run scores the residuals against them on the device, into ``val_bins`` confidence bins (clipmi_taskres_fit_monitored: the
    training step's logits kernel on the validation rows, ``clipmi_val_score``, ``clipmi_best_select``) -- the fitted residuals are bit
    for bit those of the same call without ``val``, and the run is still one library call and one wait.  ``final_model``: "last_step"
    returns the last epoch's residuals; "best_val" (the reference's TEST.FINAL_MODEL, base_learner.py:41-47) those of the epoch that was
    strictly better than every earlier one under ``val_criterion`` -- "accuracy" (Dassl's rule) or "nll", where an epoch with a
    non-finite nll is never taken; the starting residuals when no epoch was taken.  "best_val" without ``val`` is refused.
    ``return_monitor`` adds a dict behind everything else, read once after the run's one wait: per-epoch ``accuracy``, ``nll`` and
    ``ece``, the raw ``bins``, ``records`` and ``best_epoch`` (``TaskResFitState.monitor``); empty without ``val`` or without steps."""
    who = "fit_residuals"
    fitmonitor.check_args(who, val, val_bins, final_model, val_criterion)
    N, E, C = _check_shapes(who, features, base_text_features, residuals)
    epochs, batch_size = fitloop.check_run(who, epochs, batch_size)
    _check_optimiser(who, optimizer, betas, eps, weight_decay, momentum, dampening, nesterov)
    if not (math.isfinite(alpha) and math.isfinite(logit_scale)):
        raise ValueError(f"{who}: alpha={alpha}, logit_scale={logit_scale} (both finite)")
    lab = fitloop._labels(who, labels, N, C)
    order = fitloop.check_order(who, order, epochs, N)
    per_epoch = steps_per_epoch(N, batch_size, drop_last)
    dev = features.device
    _, lr_steps = fitloop.schedule(who, lr, epochs, lr_per_epoch, per_epoch, dev)
    if val is not None:
        vf, vl = fitmonitor.check_val(who, val, E, C)
    _need_gpu(features, "features")
    r = _master(base_text_features, residuals, dev)
    if epochs * per_epoch == 0:
        return fitmonitor.pack(r, np.zeros(0, np.float32), fitmonitor.empty_monitor(val_bins), return_history, return_monitor)
    s1, s2 = _state(r, optimizer, momentum)
    mon = monitor = None
    if val is not None:
        _need_gpu(vf, "val_features")
        mon = fitmonitor.Monitor(who, epochs, val_bins, val_criterion, r if final_model == "best_val" else None, dev)
        mon.seen = epochs
        monitor = ops.fit_monitor(fitmonitor._fp32(vf), vl.to(dev), mon.bins, mon.records, val_criterion, mon.block,
                                  mon.best)
    losses = ops.taskres_fit(features, fitloop.labels_on(labels, lab, dev), base_text_features, r, s1, s2, lr_steps, alpha,
                             float(np.float32(math.exp(logit_scale))), batch_size, epochs, optimizer, weight_decay, momentum, dampening, nesterov,
                             betas, eps, fitloop.order_on(order, np.int32, dev), drop_last, steps_done=0, want_losses=return_history,
                             monitor=monitor)
    torch.cuda.current_stream().synchronize()   # the run's one synchronisation
    return fitmonitor.pack(mon.best if final_model == "best_val" else r, losses.cpu().numpy() if return_history else None,
                           fitmonitor.returned_monitor(mon, mon is not None, val_bins, return_monitor),
                           return_history, return_monitor)


class TaskResFitState(fitmonitor.Monitored):
    """The training state of TaskRes' residuals for callers that produce the image features step by step (a random train transform: the
    image tower runs on every batch): the fp32 master ``residuals`` [C, E], the optimiser's state (``state1``: Adam's first moment or
    SGD's momentum buffer, ``state2``: Adam's second moment) and the number of steps taken.  ``step`` enqueues one forward, backward and
    optimiser update and does not synchronise.  ``validate`` scores cached validation features on the device (``start_monitor``,
    ``monitor``, ``best_residuals``, ``val_logits``: ``fitmonitor.Monitored`` on a ``fitmonitor.Monitor``; the optimiser's state is not
    selected)."""
    _who, _unseen_summary = "TaskResFitState", True

    def __init__(self, base_text_features: torch.Tensor, residuals: Optional[torch.Tensor] = None, alpha: float = 0.5,
                 logit_scale: float = 4.6052, optimizer: str = "adam", betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 5e-4, momentum: float = 0.9, dampening: float = 0.0, nesterov: bool = False):
        _check_optimiser("TaskResFitState", optimizer, betas, eps, weight_decay, momentum, dampening, nesterov)
        if not isinstance(base_text_features, torch.Tensor) or base_text_features.dim() != 2 or base_text_features.shape[0] < 2:
            raise ValueError("TaskResFitState: base text features must be a [C >= 2, E] tensor")
        _check_shapes("TaskResFitState", base_text_features[:1], base_text_features, residuals)
        if not (math.isfinite(alpha) and math.isfinite(logit_scale)):
            raise ValueError(f"TaskResFitState: alpha={alpha}, logit_scale={logit_scale} (both finite)")
        _need_gpu(base_text_features, "base_text_features")
        self.base_text_features = base_text_features
        self.residuals = _master(base_text_features, residuals, base_text_features.device)
        self.state1, self.state2 = _state(self.residuals, optimizer, momentum)
        self.alpha, self.scale = float(alpha), float(np.float32(math.exp(logit_scale)))
        self.optimizer, self.betas, self.eps, self.weight_decay = optimizer, (float(betas[0]), float(betas[1])), eps, weight_decay
        self.momentum, self.dampening, self.nesterov = momentum, dampening, nesterov
        self.steps = 0

    # ---- per-epoch validation and best-epoch selection on the device (DESIGN.md "Fit monitor")

    def _master(self) -> torch.Tensor:
        return self.residuals

    def validate(self, val_features: torch.Tensor, val_labels, epoch: int) -> None:
        """Enqueue one validation of the current master residuals into slot ``epoch`` of the device history; no host read.
        ``clipmi_taskres_val_logits`` runs the training step's logits kernel on ``val_features`` (raw image features [N_val, E] on the
        GPU) into fp32 [N_val, C] logits the state owns (4 N_val C bytes, kept for the next epoch); ``clipmi_val_score`` scores them into
        the record and, when the monitor selects, ``clipmi_best_select`` compares the record with the best block and copies the
        residuals into the best slot.  ``val_labels`` [N_val]: an int64 tensor on the GPU is taken as it is (a label outside [0, C) then
        counts as wrong with a NaN nll), anything else is range-checked on the host, once per set.  Without ``start_monitor`` the history
        starts with ``epoch + 1`` slots of 10 bins and no selection; it grows when ``epoch`` lies behind its end."""
        who = "TaskResFitState.validate"
        mon = self._monitor_for(epoch)
        epoch = mon.slot(who, epoch)
        C, E = self.base_text_features.shape
        feats, labels_d = mon.operands(who, val_features, val_labels, E, C)
        ops.taskres_val_logits(feats, self.base_text_features, self.residuals, self.alpha, self.scale, out=mon.logits)
        mon.score(epoch, labels_d, self.residuals)

    def best_residuals(self) -> torch.Tensor:
        """The best slot on the device: the residuals of the best epoch so far, or those ``start_monitor`` saw while no epoch has been
        taken.  No read-back."""
        return self._best_block("best_residuals")

    def step(self, features: torch.Tensor, labels, lr, want_loss: bool = False) -> Optional[torch.Tensor]:
        """One optimiser step on the batch ``features`` fp32 [B, E] (raw image features on the GPU) and ``labels`` [B] at the rate
        ``lr``: an fp32 tensor of one element on the device is read where it lies (slice a per-step rate array filled once:
        ``rates[k:k + 1]``); a Python number is uploaded on every call, a host-to-device copy the per-step path is better off without.
        A label tensor on the GPU is taken as it is -- a label outside [0, C) then makes the residuals NaN, it is never used as an
        address; host labels are range-checked.  Returns the batch loss, fp32 [1] on the device, when ``want_loss``."""
        N, _, C = _check_shapes("TaskResFitState.step", features, self.base_text_features, None)
        _need_gpu(features, "features")
        labels_d = fitloop.step_labels("TaskResFitState.step", labels, N, C, features.device)
        loss = ops.taskres_train_step(features, labels_d, self.base_text_features, self.residuals, self.state1, self.state2,
                                      fitloop.lr_operand(lr, features.device), self.alpha, self.scale, self.steps, self.optimizer, self.weight_decay, self.momentum, self.dampening, self.nesterov,
                                      self.betas, self.eps, want_loss=want_loss)
        self.steps += 1
        return loss
