"""CLIP-Adapter's bottleneck trained on the GPU (reference trainers/classification/clip_adapter.py:138-187).

The reference trains the bias-free bottleneck E -> E/4 -> E with Dassl's epoch loop: every step runs both frozen towers, blends the
adapter's output with the raw image features by ``ratio``, normalises, takes ``F.cross_entropy`` of ``exp(logit_scale)`` times the cosine
against the frozen text features and one ``torch.optim.SGD`` step on the two matrices.  The towers are frozen and, with the shipped
config, so is the context: a step is a function of the image features, the labels, the text features and the optimiser settings.
csrc/adapter_train.hip computes forward, backward and the SGD step in two launches per step, with no autograd graph.

Two ways in.  ``fit_adapter`` trains from a cached [N, E] feature matrix and enqueues every step of every epoch on the current stream with
no synchronisation between the steps and one at the end (labels that arrive on the GPU are copied to the host once, before the first
launch, for their range check): that equals the reference's loop only when the train transform is deterministic, since the reference's
``random_resized_crop`` + ``random_flip`` change the features every epoch.  ``AdapterFitState.step`` takes one batch of features at a time,
for callers that run the image tower on every step: ``CLIPAdapterCLIP.fit_adapter(loader, transform=TrainPreprocess(...))`` is that
caller, with the reference's train transform computed on the device (clip_calibration_amd/augment.py).

Dassl is not part of this repository's environment.  The defaults below -- SGD at 0.002 with momentum 0.9 and weight decay 5e-4, no
dampening, no Nesterov; 200 epochs in batches of 32, the last short batch dropped; a constant warm-up epoch that hands over to a cosine
schedule; ratio 0.2 -- restate configs/trainers/CLIP_Adapter/vit_b16_c4_ep200_batch32.yaml and Dassl's public defaults and are UNVERIFIED
here; that is why each of them is an argument.  Dassl's random sampler is the caller's ``order``.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import fitloop, fitmonitor, ops
from .fitloop import _need_gpu, steps_per_epoch


def _check_shapes(who: str, features, text_features, w1, w2):
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] < 1:
        raise ValueError(f"{who}: features must be a [N >= 1, E] tensor")
    N, E = features.shape
    if not isinstance(text_features, torch.Tensor) or text_features.dim() != 2 or text_features.shape[1] != E or text_features.shape[0] < 2:
        raise ValueError(f"{who}: text features {tuple(getattr(text_features, 'shape', ()))} must be [C >= 2, E = {E}]")
    if (not isinstance(w1, torch.Tensor) or not isinstance(w2, torch.Tensor) or w1.dim() != 2 or w1.shape[0] < 1 or w1.shape[1] != E
            or tuple(w2.shape) != (E, w1.shape[0])):
        raise ValueError(f"{who}: adapter shapes do not chain (E = {E}, w1 {tuple(getattr(w1, 'shape', ()))}, w2 {tuple(getattr(w2, 'shape', ()))})")
    return N, E, w1.shape[0], text_features.shape[0]


def fit_adapter(features: torch.Tensor, labels, text_features: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, ratio: float = 0.2,
                logit_scale: float = 4.6052, epochs: int = 200, lr: float = 0.002, batch_size: int = 32, momentum: float = 0.9,
                dampening: float = 0.0, weight_decay: float = 5e-4, nesterov: bool = False, lr_per_epoch: Optional[Sequence[float]] = None,
                order=None, drop_last: bool = True, return_history: bool = False, val=None, val_bins: int = 10,
                final_model: str = "last_step", val_criterion: str = "accuracy", return_monitor: bool = False):
    """Train CLIP-Adapter's bottleneck on cached ``features`` fp32 [N, E] (raw, un-normalised image features on the GPU; the rows may be a
    column slice of a wider matrix), ``labels`` [N] and the frozen L2-normalised ``text_features`` fp32 [C, E], starting from ``w1``
    [H, E] and ``w2`` [E, H] (not modified): ``epochs`` passes of ``torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov)`` on
    ``F.cross_entropy(exp(logit_scale) * normalise(ratio * adapter(f) + (1 - ratio) * f) @ text_features.T, labels)`` over batches of
    ``batch_size``, all in fp32.

    ``lr_per_epoch`` gives every epoch's rate; None takes ``cosine_warmup_schedule(lr, epochs)``.  ``order`` is an integer [epochs, N]
    array of sample indices, batch k of epoch e being ``order[e, k * batch_size : (k + 1) * batch_size]``; None is 0 .. N-1 in every
    epoch.  The last batch of an epoch is short unless ``drop_last`` drops it.

    Labels (and ``order``) are checked against their ranges on the host before anything is launched -- a label tensor on the GPU is
    copied to the host for that, which waits for whatever produced it; from the first launch on nothing synchronises until the one wait
    at the end.  Returns the fitted fp32 ``(w1, w2)`` on the device, or ``(w1, w2, per-step batch losses as a float32 numpy array)`` with
    ``return_history``.  The defaults are unverified restatements of the reference's config and Dassl's (module docstring).

    ``val=(val_features, val_labels)`` (raw image features [N_val, E] on the GPU and their labels): behind the last step of every epoch
    the run scores the weights against them on the device, into ``val_bins`` confidence bins (clipmi_adapter_fit_monitored: the training
    forward on the validation rows, ``clipmi_val_score``, ``clipmi_best_select``) -- the fitted weights are bit for bit those of the same
    call without ``val``, and the run is still one library call and one wait.  ``final_model``: "last_step" returns the last epoch's
    weights; "best_val" (the reference's TEST.FINAL_MODEL, base_learner.py:41-47) those of the epoch that was strictly better than every
    earlier one under ``val_criterion`` -- "accuracy" (Dassl's rule) or "nll", where an epoch with a non-finite nll is never taken; the
    starting weights when no epoch was taken.  "best_val" without ``val`` is refused.  ``return_monitor`` adds a dict behind everything
    else, read once after the run's one wait: per-epoch ``accuracy``, ``nll`` and ``ece``, the raw ``bins``, ``records`` and
    ``best_epoch`` (``AdapterFitState.monitor``); empty without ``val`` or without steps."""
    who = "fit_adapter"
    fitmonitor.check_args(who, val, val_bins, final_model, val_criterion)
    N, E, H, C = _check_shapes(who, features, text_features, w1, w2)
    epochs, batch_size = fitloop.check_run(who, epochs, batch_size)
    fitloop.check_sgd(who, momentum, dampening, weight_decay, nesterov)
    if not (math.isfinite(ratio) and math.isfinite(logit_scale)):
        raise ValueError(f"{who}: ratio={ratio}, logit_scale={logit_scale} (both finite)")
    lab = fitloop._labels(who, labels, N, C)
    order = fitloop.check_order(who, order, epochs, N)
    per_epoch = steps_per_epoch(N, batch_size, drop_last)
    dev = features.device
    _, lr_steps = fitloop.schedule(who, lr, epochs, lr_per_epoch, per_epoch, dev)
    if val is not None:
        vf, vl = fitmonitor.check_val(who, val, E, C)
    _need_gpu(features, "features")
    if val is not None:
        block, w1, w2 = ops.adapter_master_block(w1, w2, dev)      # one block [w1 | w2]: what the selection copies
    else:
        w1, w2 = fitloop.master(w1, dev), fitloop.master(w2, dev)
    if epochs * per_epoch == 0:
        return fitmonitor.pack((w1, w2), np.zeros(0, np.float32), fitmonitor.empty_monitor(val_bins), return_history, return_monitor)
    m1, m2 = (torch.zeros_like(w1), torch.zeros_like(w2)) if momentum != 0.0 else (None, None)
    mon = monitor = None
    if val is not None:
        _need_gpu(vf, "val_features")
        mon = fitmonitor.Monitor(who, epochs, val_bins, val_criterion, block if final_model == "best_val" else None, dev)
        mon.seen = epochs
        monitor = ops.fit_monitor(fitmonitor._fp32(vf), vl.to(dev), mon.bins, mon.records, val_criterion, mon.block,
                                  mon.best)
    losses = ops.adapter_fit(features, fitloop.labels_on(labels, lab, dev), text_features, w1, w2, m1, m2, lr_steps, ratio,
                             float(np.float32(math.exp(logit_scale))), batch_size, epochs, momentum, dampening, weight_decay, nesterov,
                             fitloop.order_on(order, np.int32, dev), drop_last, first_step=True, want_losses=return_history, monitor=monitor)
    torch.cuda.current_stream().synchronize()   # the run's one synchronisation
    if final_model == "best_val":
        w1, w2 = mon.best[:w1.numel()].view(w1.shape), mon.best[w1.numel():].view(w2.shape)
    return fitmonitor.pack((w1, w2), losses.cpu().numpy() if return_history else None,
                           fitmonitor.returned_monitor(mon, mon is not None, val_bins, return_monitor),
                           return_history, return_monitor)


class AdapterFitState(fitmonitor.Monitored):
    """The training state of CLIP-Adapter's bottleneck for callers that produce the image features step by step (a random train
    transform: the image tower runs on every batch): fp32 master weights ``w1`` [H, E], ``w2`` [E, H], their momentum buffers and the
    number of steps taken.  ``step`` enqueues one forward, backward and SGD update and does not synchronise.  ``validate`` scores cached
    validation features on the device (``start_monitor``, ``monitor``, ``best_weights``, ``val_logits``: ``fitmonitor.Monitored`` on a
    ``fitmonitor.Monitor``)."""
    _who, _unseen_summary = "AdapterFitState", True

    def __init__(self, text_features: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, ratio: float = 0.2, logit_scale: float = 4.6052,
                 momentum: float = 0.9, dampening: float = 0.0, weight_decay: float = 5e-4, nesterov: bool = False):
        fitloop.check_sgd("AdapterFitState", momentum, dampening, weight_decay, nesterov)
        if not isinstance(text_features, torch.Tensor) or text_features.dim() != 2 or text_features.shape[0] < 2:
            raise ValueError("AdapterFitState: text features must be a [C >= 2, E] tensor")
        _need_gpu(text_features, "text_features")
        dev = text_features.device
        self.text_features = text_features
        if not isinstance(w1, torch.Tensor) or not isinstance(w2, torch.Tensor):
            raise ValueError("AdapterFitState: w1 and w2 must be tensors")
        self._block, self.w1, self.w2 = ops.adapter_master_block(w1, w2, dev)     # one block [w1 | w2]: what the monitor's selection copies
        _check_shapes("AdapterFitState", text_features[:1], text_features, self.w1, self.w2)
        self.m1, self.m2 = (torch.zeros_like(self.w1), torch.zeros_like(self.w2)) if momentum != 0.0 else (None, None)
        self.ratio, self.scale = float(ratio), float(np.float32(math.exp(logit_scale)))
        self.momentum, self.dampening, self.weight_decay, self.nesterov = momentum, dampening, weight_decay, nesterov
        self.steps = 0

    # ---- per-epoch validation and best-epoch selection on the device (DESIGN.md "Fit monitor")

    def _master(self) -> torch.Tensor:
        return self._block      # [w1 | w2]

    def validate(self, val_features: torch.Tensor, val_labels, epoch: int) -> None:
        """Enqueue one validation of the current master weights into slot ``epoch`` of the device history; no host read.
        ``clipmi_adapter_val_logits`` runs the training step's forward on ``val_features`` (raw image features [N_val, E] on the GPU)
        into fp32 [N_val, C] logits the state owns (4 N_val C bytes, kept for the next epoch); ``clipmi_val_score`` scores them into the
        record and, when the monitor selects, ``clipmi_best_select`` compares the record with the best block and copies [w1 | w2] into
        the best slot.  ``val_labels`` [N_val]: an int64 tensor on the GPU is taken as it is (a label outside [0, C) then counts as wrong
        with a NaN nll), anything else is range-checked on the host, once per set.  Without ``start_monitor`` the history starts with
        ``epoch + 1`` slots of 10 bins and no selection; it grows when ``epoch`` lies behind its end."""
        who = "AdapterFitState.validate"
        mon = self._monitor_for(epoch)
        epoch = mon.slot(who, epoch)
        feats, labels_d = mon.operands(who, val_features, val_labels, self.w1.shape[1], self.text_features.shape[0])
        ops.adapter_val_logits(feats, self.text_features, self.w1, self.w2, self.ratio, self.scale, out=mon.logits)
        mon.score(epoch, labels_d, self._block)

    def best_weights(self):
        """``(w1, w2)`` of the best slot on the device: the weights of the best epoch so far, or those ``start_monitor`` saw while no
        epoch has been taken.  No read-back."""
        best, k = self._best_block("best_weights"), self.w1.numel()
        return best[:k].view(self.w1.shape), best[k:].view(self.w2.shape)

    def step(self, features: torch.Tensor, labels, lr, want_loss: bool = False) -> Optional[torch.Tensor]:
        """One SGD step on the batch ``features`` fp32 [B, E] (raw image features on the GPU) and ``labels`` [B] at the rate ``lr``: an fp32
        tensor of one element on the device is read where it lies (slice a per-step rate array filled once: ``rates[k:k + 1]``); a Python
        number is uploaded on every call, a host-to-device copy the per-step path is better off without.  A label tensor on the GPU is taken as it is -- a label
        outside [0, C) then makes the weights NaN, it is never used as an address; host labels are range-checked.  Returns the batch
        loss, fp32 [1] on the device, when ``want_loss``."""
        N, _, _, C = _check_shapes("AdapterFitState.step", features, self.text_features, self.w1, self.w2)
        _need_gpu(features, "features")
        labels_d = fitloop.step_labels("AdapterFitState.step", labels, N, C, features.device)
        loss = ops.adapter_train_step(features, labels_d, self.text_features, self.w1, self.w2, self.m1, self.m2,
                                      fitloop.lr_operand(lr, features.device), self.ratio, self.scale,
                                      self.steps == 0, self.momentum, self.dampening, self.weight_decay, self.nesterov, want_loss=want_loss)
        self.steps += 1
        return loss
