"""What every GPU fit driver shares: the host-side argument checks, the learning-rate schedule and the two epoch loops.

A fit is ``epochs`` passes over batches, one optimiser step per batch at its epoch's rate, every step enqueued with no synchronisation
until one wait at the end.  ``tempfit``, ``adapterfit`` and ``taskresfit`` hand the whole schedule to one library call and use the checks
and ``schedule``; ``coopfit``, ``prodafit`` and ``cocoopfit`` step through a cached feature matrix with ``run_cached``; ``vptfit``,
``maplefit``, ``promptsrcfit`` and ``augment.fit_with_transform`` step through a sized iterable of batches with ``run_batches``.  Every
check takes ``who``, the name of the function the caller called, for its message.  Nothing here touches the library: numpy and torch only.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch


def _host_int_array(who: str, x, name: str) -> np.ndarray:
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{who}: {name} must be integers, got {a.dtype}")
    return a


def _need_gpu(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"clipmi: `{name}` must be a tensor on the GPU (got {t.device}); the HIP path has no CPU fallback")


def _labels(who: str, labels, N: int, C: int, rows: str = "rows") -> np.ndarray:
    """``labels`` on the host after the type, shape and range checks (a tensor on the GPU is copied over: one wait)."""
    lab = _host_int_array(who, labels, "labels")
    if lab.shape != (N,):
        raise ValueError(f"{who}: {N} {rows} need {N} labels, got {lab.shape}")
    if lab.min() < 0 or lab.max() >= C:
        raise ValueError(f"{who}: labels span [{int(lab.min())}, {int(lab.max())}], outside the {C} classes [0, {C})")
    return lab


def _on_gpu_as_is(labels) -> bool:
    return isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.int64


def labels_on(labels, lab: np.ndarray, dev) -> torch.Tensor:
    """The checked host labels ``lab`` of ``labels`` as int64 on ``dev``: ``labels`` itself when it already is that."""
    return labels if _on_gpu_as_is(labels) else torch.from_numpy(lab.astype(np.int64)).to(dev)


def step_labels(who: str, labels, N: int, C: int, dev, rows: str = "rows") -> torch.Tensor:
    """A step's labels as int64 on ``dev``: an int64 tensor on the GPU is taken as it is after the shape check, with no read-back (a label
    outside [0, C) then poisons the parameters with NaN, it is never used as an address); anything else is checked on the host."""
    if _on_gpu_as_is(labels):
        if labels.shape != (N,):
            raise ValueError(f"{who}: {N} {rows} need {N} labels, got {tuple(labels.shape)}")
        return labels
    return torch.from_numpy(_labels(who, labels, N, C, rows).astype(np.int64)).to(dev)


def check_sgd(who: str, momentum: float, dampening: float, weight_decay: float, nesterov: bool) -> None:
    """torch.optim.SGD's argument checks."""
    if not (0.0 <= momentum < 1.0 and 0.0 <= dampening < 1.0):
        raise ValueError(f"{who}: momentum={momentum}, dampening={dampening} (both in [0, 1))")
    if not weight_decay >= 0.0 or not math.isfinite(weight_decay):
        raise ValueError(f"{who}: weight_decay={weight_decay} (finite, >= 0)")
    if nesterov and (momentum <= 0.0 or dampening != 0.0):
        raise ValueError(f"{who}: Nesterov momentum requires a momentum and zero dampening")


OPTIMIZERS = ("sgd", "adam", "adamw")     # the reference's OPTIM.NAME values the prompt fits take
SGD_DEFAULTS = (0.9, 0.0, False)          # momentum, dampening, nesterov of every prompt fit when the caller names none


def check_adam(who: str, betas, eps: float, weight_decay: float) -> Tuple[float, float]:
    """torch.optim.Adam's argument checks (no amsgrad); returns the betas as a pair of floats."""
    try:
        b1, b2 = (float(b) for b in betas)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: betas={betas!r} must be a pair of numbers") from None
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"{who}: betas={betas!r} (both in [0, 1))")
    if not (math.isfinite(eps) and eps > 0.0):
        raise ValueError(f"{who}: eps={eps} (finite, > 0)")
    if not weight_decay >= 0.0 or not math.isfinite(weight_decay):
        raise ValueError(f"{who}: weight_decay={weight_decay} (finite, >= 0)")
    return b1, b2


def adam_bias_table(betas, steps: int) -> np.ndarray:
    """float64 [steps, 2]: row t - 1 holds ``1 - beta1 ** t`` and ``math.sqrt(1 - beta2 ** t)`` for Adam's step number t = 1 .. steps,
    formed in Python doubles exactly as torch's single-tensor Adam forms them.  The step kernels index it (no pow on the device)."""
    b1, b2 = (float(b) for b in betas)
    if int(steps) < 1:
        raise ValueError(f"adam_bias_table: steps={steps} (>= 1)")
    return np.array([[1 - b1 ** t, math.sqrt(1 - b2 ** t)] for t in range(1, int(steps) + 1)], dtype=np.float64)


def refuse_one_call(who: str, optimizer: str) -> None:
    """The one-call steps stay SGD: ``check_optimizer(one_call=True)`` and every state's ``step(one_call=True)`` under Adam end here."""
    raise ValueError(f"{who}: one_call=True with optimizer={optimizer!r}: the one-call steps stay SGD")


def check_optimizer(who: str, optimizer, momentum, dampening, nesterov, weight_decay: float, betas=(0.9, 0.999), eps: float = 1e-8,
                    one_call: bool = False, shard=None, sgd_defaults=SGD_DEFAULTS):
    """The optimiser arguments of a prompt fit after their checks, before any device call: ``(optimizer, momentum, dampening, nesterov,
    betas)``.  ``"sgd"``: torch.optim.SGD's checks, the arguments as they are, ``betas`` None.  ``"adam"`` / ``"adamw"``: ``momentum``,
    ``dampening`` and ``nesterov`` belong to SGD -- a value other than the fit's own default (``sgd_defaults``; a signature cannot tell a
    default from the same value passed on purpose) is refused --; torch.optim.Adam's checks; the one-call steps and the class-sharded fit
    stay SGD and are refused.  The three come back as 0, 0, False there, which is what the fits' gradient-only calls take."""
    if not isinstance(optimizer, str) or optimizer not in OPTIMIZERS:
        raise ValueError(f"{who}: optimizer={optimizer!r} must be one of {OPTIMIZERS}")
    if optimizer == "sgd":
        check_sgd(who, momentum, dampening, weight_decay, nesterov)
        return optimizer, momentum, dampening, nesterov, None
    for name, v, d in zip(("momentum", "dampening", "nesterov"), (momentum, dampening, nesterov), sgd_defaults):
        if v is not None and v != d:
            raise ValueError(f"{who}: {name}={v!r} is an argument of optimizer='sgd'; optimizer={optimizer!r} takes betas and eps")
    betas = check_adam(who, betas, eps, weight_decay)
    if one_call:
        refuse_one_call(who, optimizer)
    if shard is not None:
        raise ValueError(f"{who}: shard with optimizer={optimizer!r}: the class-sharded fit stays SGD")
    return optimizer, 0.0, 0.0, False, betas


def check_run(who: str, epochs, batch_size) -> Tuple[int, int]:
    epochs, batch_size = int(epochs), int(batch_size)
    if epochs < 0 or batch_size < 1:
        raise ValueError(f"{who}: epochs={epochs} (>= 0), batch_size={batch_size} (>= 1)")
    return epochs, batch_size


def check_order(who: str, order, epochs: int, N: int) -> Optional[np.ndarray]:
    """``order`` (None: every epoch runs 0 .. N-1) as a host integer array [epochs, N] of sample indices in [0, N)."""
    if order is None:
        return None
    order = _host_int_array(who, order, "order")
    if order.shape != (epochs, N):
        raise ValueError(f"{who}: order {order.shape} must be [epochs, N] = [{epochs}, {N}]")
    if order.size and (order.min() < 0 or order.max() >= N):
        raise ValueError(f"{who}: order holds sample indices outside [0, {N})")
    return order


def order_on(order: Optional[np.ndarray], dtype, dev) -> Optional[torch.Tensor]:
    """The checked ``order`` on ``dev``: int32 for the library's whole-run calls, int64 for ``run_cached`` (``index_select``)."""
    return None if order is None else torch.from_numpy(np.ascontiguousarray(order, dtype=dtype)).to(dev)


def exp_logit_scale(who: str, logit_scale: float) -> float:
    """exp(logit_scale) as the fp32 value the heads multiply by; a non-finite logit_scale is refused."""
    if not math.isfinite(logit_scale):
        raise ValueError(f"{who}: logit_scale={logit_scale} (finite)")
    return float(np.float32(math.exp(logit_scale)))


def master(t: torch.Tensor, dev) -> torch.Tensor:
    """A fresh contiguous fp32 copy on the device: the master values the kernels update in place."""
    return t.detach().to(device=dev, dtype=torch.float32, copy=True).contiguous()


def lr_operand(lr, dev) -> torch.Tensor:
    """A step's rate as the kernels read it: an fp32 tensor of one element is used where it lies (slice a per-step array filled once:
    ``rates[k:k + 1]``); a Python number is uploaded, a host-to-device copy the per-step path is better off without."""
    return lr if isinstance(lr, torch.Tensor) else torch.tensor([float(lr)], dtype=torch.float32).to(dev)


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


def schedule(who: str, lr: float, epochs: int, lr_per_epoch: Optional[Sequence[float]], per_epoch: int, dev) -> Tuple[List[float], torch.Tensor]:
    """``(rates, lr_steps)``: every epoch's rate -- ``lr_per_epoch``, or ``cosine_warmup_schedule(lr, epochs)`` without one -- and the
    rate of every step as fp32 [epochs * per_epoch] on ``dev``, filled once so that no step uploads anything."""
    rates = cosine_warmup_schedule(lr, epochs) if lr_per_epoch is None else [float(r) for r in lr_per_epoch]
    if len(rates) != epochs:
        raise ValueError(f"{who}: {len(rates)} learning rates for {epochs} epochs")
    return rates, torch.from_numpy(np.repeat(np.asarray(rates, np.float64), per_epoch).astype(np.float32)).to(device=dev)


def cut_batches(who: str, images_or_loader, labels, n_classes: int, batch_size, drop_last: bool, dev):
    """The sized iterable of (images, labels) batches ``run_batches`` takes: a tensor of images with ``labels`` [N] is cut into batches of
    ``batch_size`` in order (the last one short unless ``drop_last``); anything else is the caller's own batches."""
    if not isinstance(images_or_loader, torch.Tensor):
        return images_or_loader
    N, bs = images_or_loader.shape[0], int(batch_size)
    if bs < 1:
        raise ValueError(f"{who}: batch_size={batch_size} (>= 1)")
    lab = step_labels(who, labels, N, n_classes, dev, "images")
    return [(images_or_loader[k * bs:min((k + 1) * bs, N)], lab[k * bs:min((k + 1) * bs, N)]) for k in range(steps_per_epoch(N, bs, drop_last))]


def _no_steps(return_history: bool) -> Optional[np.ndarray]:
    return np.zeros(0, np.float32) if return_history else None


def _finish(losses: list, return_history: bool, dev) -> Optional[np.ndarray]:
    """The run's one synchronisation and, with ``return_history``, its one read-back."""
    if dev.type == "cuda":
        torch.cuda.current_stream(dev).synchronize()
    return torch.cat(losses).cpu().numpy() if return_history else None


def run_cached(step: Callable, features: torch.Tensor, labels_d: torch.Tensor, order_d: Optional[torch.Tensor], batch_size: int, per_epoch: int,
               epochs: int, lr_steps: torch.Tensor, return_history: bool = False,
               end_epoch: Optional[Callable[[int], None]] = None) -> Optional[np.ndarray]:
    """``epochs`` passes over the cached ``features`` [N, E] and ``labels_d`` [N] in ``per_epoch`` batches of ``batch_size``: batch k of
    epoch e is the rows ``order_d[e, k * batch_size : (k + 1) * batch_size]`` (int64 [epochs, N] on the features' device), or that range
    itself without an order.  Every batch goes to ``step(f, y, lr_steps[s:s + 1], want_loss)``.  ``end_epoch(e)``, when given, is called
    behind the last step of every epoch and must not synchronise.  Returns the per-step losses as a float32 numpy array with
    ``return_history``.  Nothing synchronises before the one wait at the end (none at all off the GPU or without steps)."""
    if epochs * per_epoch == 0:
        return _no_steps(return_history)
    N = features.shape[0]
    losses = []
    s = 0
    for e in range(epochs):
        for k in range(per_epoch):
            lo, hi = k * batch_size, min((k + 1) * batch_size, N)
            if order_d is None:
                f, y = features[lo:hi], labels_d[lo:hi]
            else:
                idx = order_d[e, lo:hi]
                f, y = features.index_select(0, idx), labels_d.index_select(0, idx)   # index plumbing
            loss = step(f, y, lr_steps[s:s + 1], return_history)
            if return_history:
                losses.append(loss)
            s += 1
        if end_epoch is not None:
            end_epoch(e)
    return _finish(losses, return_history, features.device)


def run_batches(step: Callable, batches, epochs: int, lr_steps: torch.Tensor, return_history: bool = False,
                end_epoch: Optional[Callable[[int], None]] = None) -> Optional[np.ndarray]:
    """``epochs`` passes over ``batches``, a sized iterable iterated once per epoch: batch k of epoch e goes to
    ``step(e, k, batch, lr_steps[s:s + 1], want_loss)`` with ``s = e * len(batches) + k``.  ``end_epoch(e)``, when given, is called behind
    the last step of every epoch and must not synchronise.  An iterable that gives another number of batches than its length is refused.
    Returns the per-step losses as a float32 numpy array with ``return_history``.  Nothing synchronises before the one wait at the end, on
    ``lr_steps``' device (none at all off the GPU or without steps)."""
    per_epoch = len(batches)
    if epochs * per_epoch == 0:
        return _no_steps(return_history)
    losses = []
    for e in range(epochs):
        k = -1
        for k, batch in enumerate(batches):
            if k >= per_epoch:
                raise RuntimeError(f"the loader gave more than its length of {per_epoch} batches")
            s = e * per_epoch + k
            loss = step(e, k, batch, lr_steps[s:s + 1], return_history)
            if return_history:
                losses.append(loss)
        if k + 1 != per_epoch:
            raise RuntimeError(f"the loader gave {k + 1} batches in epoch {e}, its length says {per_epoch}")
        if end_epoch is not None:
            end_epoch(e)
    return _finish(losses, return_history, lr_steps.device)
