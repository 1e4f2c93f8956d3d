"""Parameterized temperature scaling (PTS; Tomani, Cremers, Buettner, ECCV 2022) on the GPU: the fit and the per-row apply.

The reference names the mode -- ``CALIBRATION.SCALING.MODE = 'ParameterizedTempScaling'`` with ``CALIBRATION.P_TS.N_LAYERS 2``,
``N_NODES 5``, ``TOP_K_LOGITS 10`` (train.py:238-247), selected by run/calibration/fewshot_scaling.sh:68-70 with 50 epochs at lr 5e-2 --
and ships no trainer for it.  This module restates the published method; it is not a port.  For a row ``z`` of C logits:

    f = the top_k largest values of z, descending;  h_0 = f;  h_l = relu(W_l h_{l-1} + b_l), l = 1 .. n_layers, each n_nodes wide;
    t = w_out . h_last + b_out;  T = clamp(|t|, 1e-12, 1e12);  calibrated logits z / T;
    loss = (1 / C) sum_c (softmax(z / T)_c - [c == y])^2, averaged over the batch (the paper's mean-squared error).

The base model is frozen and the validation loader sequential, so the whole fit is a function of one cached [N, C] logits matrix, the
labels and the optimiser settings: ``fit_pts`` hands them to csrc/pts.hip, which computes the features once and enqueues two launches per
step on the current stream with no host synchronisation in between; the host waits once at the end.

The parameters live in one flat fp32 block ``[W_1 | b_1 | ... | W_n | b_n | w_out | b_out]``, every W row-major [out, in]
(``nn.Linear``'s layout).  The batch size, the SGD settings and the schedule default to what ``tempfit.fit_logit_scale`` takes: the same
UNVERIFIED restatement of Dassl's public defaults (tempfit's module docstring), which is why each of them is an argument.  The paper
trains with Adam; ``optimizer="adam"`` is ``torch.optim.Adam``'s rule.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, fitloop, ops

MAX_LAYERS, MAX_NODES, MAX_TOP_K = 4, 32, 32
_OPTIMIZERS = {"sgd": _lib.OPTIM_SGD, "adam": _lib.OPTIM_ADAM}


def _check_net(who: str, n_layers, n_nodes, top_k) -> Tuple[int, int, int]:
    n_layers, n_nodes, top_k = int(n_layers), int(n_nodes), int(top_k)
    if not (0 <= n_layers <= MAX_LAYERS and 1 <= n_nodes <= MAX_NODES and 1 <= top_k <= MAX_TOP_K):
        raise ValueError(f"{who}: n_layers={n_layers} (0 .. {MAX_LAYERS}), n_nodes={n_nodes} (1 .. {MAX_NODES}), top_k={top_k} (1 .. {MAX_TOP_K})")
    return n_layers, n_nodes, top_k


def _shapes(n_layers: int, n_nodes: int, top_k: int):
    """(name, shape) of every tensor of the block, in the block's order."""
    out, n_in = [], top_k
    for l in range(1, n_layers + 1):
        out += [(f"W{l}", (n_nodes, n_in)), (f"b{l}", (n_nodes,))]
        n_in = n_nodes
    return out + [("w_out", (n_in,)), ("b_out", (1,))]


def param_count(n_layers: int = 2, n_nodes: int = 5, top_k: int = 10) -> int:
    n_layers, n_nodes, top_k = _check_net("param_count", n_layers, n_nodes, top_k)
    return sum(int(np.prod(s)) for _, s in _shapes(n_layers, n_nodes, top_k))


def split_params(block: torch.Tensor, n_layers: int = 2, n_nodes: int = 5, top_k: int = 10) -> Dict[str, torch.Tensor]:
    """Named views into the flat block: ``W1 [n_nodes, top_k]``, ``b1``, ..., ``w_out``, ``b_out [1]``."""
    n_layers, n_nodes, top_k = _check_net("split_params", n_layers, n_nodes, top_k)
    P = param_count(n_layers, n_nodes, top_k)
    if block.dim() != 1 or block.numel() != P:
        raise ValueError(f"split_params: a block of {tuple(block.shape)}, the net has {P} parameters")
    out, at = {}, 0
    for name, shape in _shapes(n_layers, n_nodes, top_k):
        n = int(np.prod(shape))
        out[name] = block[at:at + n].view(shape)
        at += n
    return out


def init_params(n_layers: int = 2, n_nodes: int = 5, top_k: int = 10, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """A fresh block, fp32 on the CPU, with ``nn.Linear``'s default initialisation: weights and biases uniform in
    +-1 / sqrt(fan_in), drawn from ``generator`` (torch's global CPU generator without one) in the block's order.  This is our choice: the
    paper's code initialises with Keras' defaults, and neither its distribution nor its random stream is restated here."""
    n_layers, n_nodes, top_k = _check_net("init_params", n_layers, n_nodes, top_k)
    parts = []
    for name, shape in _shapes(n_layers, n_nodes, top_k):
        if name[0] in "Ww":
            fan_in = shape[-1]
        bound = 1.0 / math.sqrt(fan_in)      # a bias takes its layer's fan_in
        parts.append(((torch.rand(shape, generator=generator, dtype=torch.float32) * 2.0 - 1.0) * bound).reshape(-1))
    return torch.cat(parts)


def fit_pts(logits: torch.Tensor, labels, params: Optional[torch.Tensor] = None, epochs: int = 50, lr: float = 0.05, batch_size: int = 100,
            optimizer: str = "sgd", momentum: float = 0.9, dampening: float = 0.0, weight_decay: float = 5e-4, nesterov: bool = False,
            betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, lr_per_epoch: Optional[Sequence[float]] = None, order=None,
            drop_last: bool = False, return_history: bool = False, n_layers: int = 2, n_nodes: int = 5, top_k: int = 10):
    """Fit the PTS net to ``logits`` fp32 [N, C] (on the GPU; the rows may be a column slice of a wider matrix) and ``labels`` [N]:
    ``epochs`` passes of ``torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov)`` or, with ``optimizer="adam"``,
    ``torch.optim.Adam(lr, betas, eps, weight_decay)`` on the batch mean of the loss above, in fp32, starting from ``params`` (a flat block;
    None draws ``init_params``).  ``logits`` are the base model's SCALED logits, ``exp(logit_scale) * cosine``.

    ``lr_per_epoch``, ``order`` and ``drop_last`` are ``tempfit.fit_logit_scale``'s: every epoch's rate (None takes
    ``cosine_warmup_schedule(lr, epochs)``), an integer [epochs, N] array of sample indices (None is 0 .. N-1 in every epoch), and whether
    a short last batch is dropped.  These defaults, like the batch size and the SGD settings, are unverified restatements of Dassl's
    (module docstring).

    Non-finite logits, labels and ``order`` outside their ranges are refused on the host before anything is launched.  Returns the fitted
    block fp32 [P] on the logits' device, or (block, per-step batch losses as a float32 numpy array) with ``return_history``."""
    who = "fit_pts"
    n_layers, n_nodes, top_k = _check_net(who, n_layers, n_nodes, top_k)
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2:
        raise ValueError(f"{who}: logits must be a [N, C] tensor")
    N, C = logits.shape
    if N < 1 or C < 2 or C < top_k:
        raise ValueError(f"{who}: logits {(N, C)} need at least one row, two classes and top_k={top_k} classes")
    if optimizer not in _OPTIMIZERS:
        raise ValueError(f"{who}: optimizer={optimizer!r} (one of {sorted(_OPTIMIZERS)})")
    epochs, batch_size = fitloop.check_run(who, epochs, batch_size)
    if optimizer == "sgd":
        fitloop.check_sgd(who, momentum, dampening, weight_decay, nesterov)
    elif not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and eps >= 0.0 and math.isfinite(eps) and weight_decay >= 0.0
              and math.isfinite(weight_decay)):
        raise ValueError(f"{who}: betas={tuple(betas)} (both in [0, 1)), eps={eps}, weight_decay={weight_decay} (finite, >= 0)")
    P = param_count(n_layers, n_nodes, top_k)
    if params is None:
        params = init_params(n_layers, n_nodes, top_k)
    if not isinstance(params, torch.Tensor) or params.shape != (P,):
        raise ValueError(f"{who}: params must be a flat block of {P} values")
    lab = fitloop._labels(who, labels, N, C)
    order = fitloop.check_order(who, order, epochs, N)
    per_epoch = fitloop.steps_per_epoch(N, batch_size, drop_last)
    dev = logits.device
    _, lr_steps = fitloop.schedule(who, lr, epochs, lr_per_epoch, per_epoch, dev)
    if not bool(torch.isfinite(logits).all()):
        raise ValueError(f"{who}: the logits hold a NaN or an infinity")
    fitloop._need_gpu(logits, "logits")
    state = torch.zeros(3 * P + 2, dtype=torch.float32, device=dev)
    state[:P] = params.detach().to(device=dev, dtype=torch.float32)
    if epochs * per_epoch == 0:
        return (state[:P].clone(), np.zeros(0, np.float32)) if return_history else state[:P].clone()
    losses = ops.pts_fit(logits, fitloop.labels_on(labels, lab, dev), state, n_layers, n_nodes, top_k, lr_steps, batch_size, epochs,
                         _OPTIMIZERS[optimizer], momentum, dampening, weight_decay, nesterov, betas, eps, fitloop.order_on(order, np.int32, dev),
                         drop_last, want_losses=return_history)
    fitted = state[:P].clone()
    torch.cuda.current_stream(dev).synchronize()   # the run's one synchronisation
    return (fitted, losses.cpu().numpy()) if return_history else fitted


class PTSCalibrator:
    """A fitted PTS net: ``apply(logits)`` is ``logits / T`` with every row's own temperature, in one launch."""

    def __init__(self, params: torch.Tensor, n_layers: int = 2, n_nodes: int = 5, top_k: int = 10):
        self.n_layers, self.n_nodes, self.top_k = _check_net("PTSCalibrator", n_layers, n_nodes, top_k)
        P = param_count(self.n_layers, self.n_nodes, self.top_k)
        if not isinstance(params, torch.Tensor) or params.shape != (P,):
            raise ValueError(f"PTSCalibrator: params must be a flat block of {P} values")
        self.params = params.detach().to(torch.float32)

    def apply(self, logits: torch.Tensor, return_temperature: bool = False):
        """fp32 [N, C] calibrated logits (softmax them for probabilities), or (logits, T fp32 [N]) with ``return_temperature``."""
        fitloop._need_gpu(logits, "logits")
        if self.params.device != logits.device:
            self.params = self.params.to(logits.device)
        return ops.pts_apply(logits, self.params, self.n_layers, self.n_nodes, self.top_k, want_temperature=return_temperature)
