"""What the prompt fits' states share on the optimiser's side: the loss scale's argument rules, the dynamic scale's device block
(``_BlockScaler``), Adam's moments (``_AdamBlock``) and ``Optimised``, the mix-in the seven fit states take them through
(``coopfit.CoOpFitState``, ``prodafit.ProDAFitState``, ``cocoopfit.CoCoOpFitState`` and ``vptfit._BlockFitState`` for VPT, MaPLe and
PromptSRC), as ``fitmonitor.Monitored`` is their monitor's.  DESIGN.md "Fit optimiser: shared plumbing" says what stays with each fit.
"""
from __future__ import annotations

import math
from typing import Callable, Optional

import torch

from . import fitloop, ops
from ._lib import lib


def _check_grad_scale(who: str, grad_scale: float) -> float:
    g = float(grad_scale)
    if not (math.isfinite(g) and g > 0.0 and math.frexp(g)[0] == 0.5):
        raise ValueError(f"{who}: grad_scale={grad_scale} must be a power of two (the scaling has to be exact)")
    return g


DYNAMIC = "dynamic"


def _is_dynamic(who: str, grad_scale) -> bool:
    """True for ``grad_scale="dynamic"``; any other string is refused, a number is the static path's."""
    if isinstance(grad_scale, str):
        if grad_scale != DYNAMIC:
            raise ValueError(f"{who}: grad_scale={grad_scale!r} must be a power of two or {DYNAMIC!r}")
        return True
    return False


def _check_scaler(who: str, scaler) -> dict:
    """torch.cuda.amp.GradScaler's arguments with its defaults filled in; the scale and both factors must be powers of two."""
    if scaler is not None and not isinstance(scaler, dict):
        raise ValueError(f"{who}: scaler must be a dict of {sorted(ops.SCALER_DEFAULTS)} or None")
    cfg = dict(ops.SCALER_DEFAULTS)
    for k, v in (scaler or {}).items():
        if k not in cfg:
            raise ValueError(f"{who}: scaler has no option {k!r} (one of {sorted(cfg)})")
        cfg[k] = v
    for k in ("init_scale", "growth_factor", "backoff_factor"):
        g = float(cfg[k])
        if not (math.isfinite(g) and 2.0 ** -126 <= g <= 2.0 ** 127 and math.frexp(g)[0] == 0.5):
            raise ValueError(f"{who}: scaler[{k!r}]={cfg[k]} must be a finite, positive power of two of fp32's range (the scaling has to be exact)")
        cfg[k] = g
    if cfg["growth_factor"] < 1.0 or cfg["backoff_factor"] > 1.0:
        raise ValueError(f"{who}: scaler growth_factor={cfg['growth_factor']} (>= 1), backoff_factor={cfg['backoff_factor']} (<= 1)")
    gi = cfg["growth_interval"]
    if isinstance(gi, bool) or int(gi) != gi or not 1 <= int(gi) < 2 ** 31:
        raise ValueError(f"{who}: scaler growth_interval={gi} must be an integer >= 1")
    cfg["growth_interval"] = int(gi)
    return cfg


def _scale_args(who: str, grad_scale, scaler):
    """``(dynamic, grad_scale, scaler)`` after the checks every fit makes of the pair: a number with no ``scaler`` (the static path; the
    dict is then None), or ``"dynamic"`` with the scaler's dict filled in (the number is then None)."""
    if _is_dynamic(who, grad_scale):
        return True, None, _check_scaler(who, scaler)
    if scaler is not None:
        raise ValueError(f"{who}: scaler is an argument of grad_scale={DYNAMIC!r}")
    return False, _check_grad_scale(who, grad_scale), None


def static_grad_scale(who: str, grad_scale, state_name: str, fit_name: str) -> float:
    """A gradient entry point's ``grad_scale``: a power of two; the dynamic scale is a fit's and is refused by the fit's names."""
    if _is_dynamic(who, grad_scale):
        raise ValueError(f"{who}: grad_scale={DYNAMIC!r} belongs to a fit ({state_name}, {fit_name}); one gradient needs a number")
    return _check_grad_scale(who, grad_scale)


def check_fit(who: str, optimizer, momentum, dampening, nesterov, weight_decay, betas, eps, grad_scale, scaler, one_call: bool = False, shard=None,
              between: Optional[Callable[[], None]] = None):
    """A fit driver's refusals of the optimiser and the loss scale before anything is loaded, in the drivers' order:
    ``fitloop.check_optimizer``, then ``between()`` (CoOp's ProGrad rule), then ``_scale_args``, whose triple is returned."""
    fitloop.check_optimizer(who, optimizer, momentum, dampening, nesterov, weight_decay, betas, eps, one_call=one_call, shard=shard)
    if between is not None:
        between()
    return _scale_args(who, grad_scale, scaler)


class _BlockScaler:
    """The dynamic loss scale of a fit: the device block (clipmi_scaler_state; only the kernels touch it once it is made), the scaler's
    arguments and the scaled step's workspace.  ``step`` is for the fits whose parameters are one fp32 master block (CoCoOp, VPT, MaPLe,
    PromptSRC); CoOp's and ProDA's scaled steps are their own (``Optimised._apply_block``)."""

    def __init__(self, cfg: dict, dev):
        self.cfg = cfg
        self.block = ops.new_scaler_state(cfg["init_scale"], dev)
        self.ws = None

    def args(self):
        """The three arguments every ``_scaled`` call takes behind the state block."""
        return self.cfg["growth_factor"], self.cfg["backoff_factor"], self.cfg["growth_interval"]

    def step(self, grad: torch.Tensor, params: torch.Tensor, buf: Optional[torch.Tensor], lr_d: torch.Tensor, momentum: float, dampening: float,
             weight_decay: float, nesterov: bool) -> None:
        """``ops.block_step_scaled`` on ``grad`` = scale * gradient: unscale, decide on the device, apply when clean."""
        if self.ws is None:
            self.ws = torch.empty(max(lib.clipmi_block_step_scaled_workspace_bytes(params.numel()), 256), dtype=torch.uint8, device=params.device)
        ops.block_step_scaled(grad, self.block, params, buf, lr_d, *self.args(), momentum, dampening, weight_decay, nesterov, want_grad=False,
                              workspace=self.ws)

    def state(self) -> dict:
        return ops.scaler_state_dict(self.block)


class _AdamBlock:
    """torch.optim.Adam's or AdamW's state beside a fit's fp32 master block (DESIGN.md "Adam steps for the prompt fits"): the two
    moments, the bias-correction table on the device and the number of steps enqueued.  ``step`` applies a gradient block that the fit's
    own launches formed without applying it; under a ``_BlockScaler`` the device decides whether the step counts, and ``steps_taken``
    is then an upper bound of the applied steps, which is all the table's length has to cover."""
    TABLE_STEPS = 1024     # the table's first length; it doubles when the steps reach it

    def __init__(self, optimizer: str, betas, eps: float, weight_decay: float, master: torch.Tensor):
        self.decoupled = optimizer == "adamw"
        self.betas, self.eps, self.weight_decay = betas, float(eps), float(weight_decay)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(master), torch.zeros_like(master)
        self.steps_taken = 0
        self.table = None
        self.ws = None

    def _table(self, dev) -> torch.Tensor:
        """The table with a row for step ``steps_taken + 1``; a longer one is uploaded (in stream order) when it has none."""
        need = self.steps_taken + 1
        if self.table is None or self.table.shape[0] < need:
            self.table = torch.from_numpy(fitloop.adam_bias_table(self.betas, max(self.TABLE_STEPS, 2 * need))).to(dev)
        return self.table

    def step(self, grad: torch.Tensor, params: torch.Tensor, lr_d: torch.Tensor, grad_scale: float = 1.0, scaler: Optional[_BlockScaler] = None) -> None:
        """``ops.block_step_adam`` on ``grad`` = ``grad_scale`` * gradient, or, with ``scaler``, ``ops.block_step_adam_scaled`` on
        ``grad`` = the scaler's scale * gradient."""
        table = self._table(params.device)
        rule = dict(betas=self.betas, eps=self.eps, weight_decay=self.weight_decay, decoupled=self.decoupled, want_grad=False)
        if scaler is None:
            ops.block_step_adam(grad, params, self.exp_avg, self.exp_avg_sq, lr_d, self.steps_taken + 1, table, grad_scale, **rule)
        else:
            if self.ws is None:
                need = lib.clipmi_block_step_adam_scaled_workspace_bytes(params.numel())
                self.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=params.device)
            ops.block_step_adam_scaled(grad, scaler.block, params, self.exp_avg, self.exp_avg_sq, lr_d, table, *scaler.args(), workspace=self.ws, **rule)
        self.steps_taken += 1


class Optimised:
    """The optimiser's and the loss scale's side of a fit state.  The state calls ``_init_optimiser`` where its constructor has always
    made these refusals and ``_init_moments`` once its master block exists, and defines ``_who`` and ``_master()`` (as
    ``fitmonitor.Monitored`` asks of it too).  A step then takes the head's scale from ``_head_scale``, multiplies the head's output
    gradients with ``_scale_rows`` and hands the finished gradient block to ``_apply_block``.  Per fit stay: the static-SGD step entry
    (passed in), CoOp's and ProDA's own scaled steps (they override ``_apply_scaled``) and the ``grad_scale`` Adam is told of."""

    def _init_optimiser(self, who: str, logit_scale: float, momentum, dampening, nesterov, weight_decay: float, grad_scale, scaler,
                        optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8, sgd_shard=None) -> None:
        """The refusals that need no model, in the order every state has made them: the loss scale's, the optimiser's, the logit
        scale's.  ``optimizer``: "sgd" (``momentum``, ``dampening``, ``nesterov``), "adam" or "adamw" (``betas``, ``eps``;
        ``weight_decay`` keeps the fit's own default -- torch's AdamW default of 1e-2 is NOT taken over).  ``sgd_shard``: the shard of a
        fit whose sharded step stays SGD (CoOp, ProDA), refused together with an Adam optimiser."""
        self.dynamic, self.grad_scale, self.scaler = _scale_args(who, grad_scale, scaler)
        self.optimizer, self.momentum, self.dampening, self.nesterov, self._betas = fitloop.check_optimizer(
            who, optimizer, momentum, dampening, nesterov, weight_decay, betas, eps, shard=sgd_shard)
        self._eps, self.weight_decay = eps, weight_decay
        self.scale = fitloop.exp_logit_scale(who, logit_scale)

    def _init_moments(self, master: torch.Tensor) -> None:
        """What the steps keep beside ``master``: SGD's momentum buffer, the step count, the scaler's device block, Adam's moments."""
        self.buf = torch.zeros_like(master) if self.momentum != 0.0 else None
        self.steps = 0
        self._scaler = _BlockScaler(self.scaler, master.device) if self.dynamic else None
        self._adam = _AdamBlock(self.optimizer, self._betas, self._eps, self.weight_decay, master) if self.optimizer != "sgd" else None

    def scaler_state(self) -> dict:
        """The dynamic scale's block as ``dict(scale, growth_tracker, skipped_steps, applied_steps, found_inf)`` (``found_inf``: of the
        last step).  It waits for the steps enqueued so far: one synchronisation, the only read-back of the dynamic path."""
        if not self.dynamic:
            raise ValueError(f"{self._who}.scaler_state: the state was made with a static grad_scale={self.grad_scale}")
        return self._scaler.state()

    def _no_one_call_adam(self, who: str, one_call: bool) -> None:
        if one_call and self._adam is not None:
            fitloop.refuse_one_call(who, self.optimizer)

    @property
    def _head_scale(self) -> float:
        """What the loss head multiplies by: 1 under the dynamic scale (``_scale_rows`` brings the block's scale in behind it)."""
        return 1.0 if self.dynamic else self.grad_scale

    def _scale_rows(self, *d_outs: torch.Tensor) -> None:
        """Under the dynamic scale: the head's output gradients times the scale of the device block, in place."""
        if self.dynamic:
            for d in d_outs:
                ops.grad_scale_rows(d, self._scaler.block)

    @property
    def _sgd(self):
        """``(momentum, dampening, weight_decay, nesterov)`` as every step entry takes them."""
        return float(self.momentum), float(self.dampening), float(self.weight_decay), int(bool(self.nesterov))

    def _apply_scaled(self, grad: torch.Tensor, lr_d: torch.Tensor) -> None:
        """SGD under the dynamic scale on ``grad`` = scale * gradient of the whole master block."""
        self._scaler.step(grad, self._master(), self.buf, lr_d, *self._sgd)

    def _apply_block(self, grad, lr_d: torch.Tensor, static_step: Optional[Callable[[], None]], adam_grad_scale: float = 1.0) -> None:
        """One optimiser step from a finished gradient.  Under Adam ``grad`` is ``adam_grad_scale`` times the master block's gradient
        (the scaler's scale times it under the dynamic scale); under SGD with the dynamic scale ``_apply_scaled`` takes it; else
        ``static_step()``, the fit's own static-SGD entry, forms and applies it (None where the caller has taken that route itself)."""
        if self._adam is not None:
            self._adam.step(grad, self._master(), lr_d, adam_grad_scale, self._scaler)
        elif self.dynamic:
            self._apply_scaled(grad, lr_d)
        else:
            static_step()
