"""ProDA's collection of contexts trained on the GPU (reference trainers/classification/proda.py:76-228, 258-304).

ProDA learns ``n_prompt`` contexts ``ctx`` [P, n_ctx, D].  Context p puts the class name in front of its vectors (p < P // 4), in their
middle (P // 4 <= p < 2 (P // 4)) or behind them (the rest).  A training step draws ``prompt_bs`` = Pb of them, runs the frozen text
tower on the C Pb class prompts -- class-major, a class's prompts ordered end | middle | front -- and on the P no-class prompts
``[SOS | ctx_p | '.' EOT]``, and takes one ``torch.optim.SGD`` step on the whole ``ctx`` for

    loss = CE(s x_b . m_c + 0.5 s^2 sigma[b, c], y) + alpha mean_{p != q} |n_p . n_q|

with m_c the mean of a class's normalised features, sigma the image-weighted variance of the difference to the label's class around
those means, and n_p the normalised no-class features (include/clipmi.h and DESIGN.md "ProDA fit" have the formulas).  csrc/proda_train.hip
has the prompt assembly, that head with its backward and the gather-reduce of the tower's input gradient back into ``ctx`` with the
optimiser's rule; between them runs the frozen-tower forward and backward of csrc/text_backward.hip that CoOp trains on, once, over
N = C Pb + P prompts.  The contexts outside a step's selection still receive the no-class term's gradient, weight decay and momentum.

The entry points mirror ``coopfit``'s: ``context_gradient`` (one batch's loss parts and gradient; the tests' diagnostic entry),
``ProDAFitState.step`` (one batch of image features at a time) and ``fit_context`` (cached features, every step enqueued, one
synchronisation at the end).  The selection schedule is the reference's, drawn on the HOST from a ``torch.Generator``: a fresh
``randperm(P)`` every P / Pb steps, consumed in slices of Pb (the reference draws on the device from the global generator; the stream
of numbers differs, the scheme does not).

Refused: ``n_prompt`` that is no multiple of 4 (the reference's position list then has fewer than ``n_prompt`` entries and indexing it
fails; with one prompt the no-class loss is the mean of nothing), ``n_prompt`` that is no multiple of ``prompt_bs``, models with deep
prompts, more than 80 live token rows (the backward's limit).

UNVERIFIED, as for CoOp: Dassl is not part of this environment, so the defaults -- SGD at 0.002 with momentum 0.9 and weight decay 5e-4,
batches of 32, 32 prompts in slices of 4, 16 context vectors from N(0, 0.02^2), alpha = 0.1 -- restate the reference's configs and
Dassl's public defaults without a run of the reference behind them; each is an argument.

``shard=coopfit.Shard(world, rank, gather)`` on ``ProDAFitState``, ``fit_context`` and ``context_gradient`` is the class-sharded fit, in
the place of the reference's ``nn.DataParallel`` over the text encoder (proda.py:374-378): one process per GPU, rank r of G running the
tower over the contiguous classes ``parallel.shard_bounds(C, r, G)`` with all ``prompt_bs`` prompts of each and over the no-class
prompts of the contexts ``shard_bounds(P, r, G)`` -- dealt out, not replicated: the tower's kernel choice follows a call's row count,
and replicated rows could differ in their bits from rank to rank.  Two all-gathers per step move the raw text features and the ranks'
partial gradients (clipmi_proda_ctx_partial); the head runs replicated, and clipmi_proda_ctx_step_gathered adds the partials in rank
order, so every rank holds the same contexts bit for bit with no all-reduce and no float atomic.  Every rank is given the same batch
and the whole collection.  ``grad_scale="dynamic"`` works under the shard (clipmi_proda_ctx_reduce_gathered_scaled): every rank reduces
the same gathered bytes, takes the same skip-or-apply decision and holds the same scaler block.  The selection schedule is drawn on the
host: under a ``LocalGather`` only the driving state -- the first that steps -- draws, and stepping another is refused; under RCCL
EVERY RANK MUST BE BUILT WITH THE SAME GENERATOR SEED (the default is one), or be given the same ``selections`` / ``sel``.  With one
rank the sharded step gives the unsharded step's bits.  Refused under ``shard``, by name and before any device call: ``C < G``,
``P < G``, ``optimizer="adam" | "adamw"``, ``one_call=True``, ``val=`` / ``final_model="best_val"`` / ``validate``, and
``context_gradient``'s operand statistics.  DESIGN.md "Class-sharded ProDA fit".

``grad_scale="dynamic"`` with ``scaler=dict(init_scale, growth_factor, backoff_factor, growth_interval)`` is the reference's ``prec ==
"amp"`` branch (proda.py:370, 388-394, ``torch.cuda.amp.GradScaler``) with the scale in a device block, as ``coopfit``'s: the head runs at
``grad_scale = 1``, its fp32 ``d_text`` is multiplied by the block's scale before the backward rounds it to fp16, and
clipmi_proda_ctx_step_scaled forms the unscaled gradient of all P contexts, skips the step when any element -- a selected context's
class rows or any context's no-class row -- is an inf or a NaN, and updates the scale by torch's rule.  The selection schedule
advances on a skipped step as on an applied one (the reference draws it in the forward, before ``GradScaler.step`` decides).  No step
reads anything back; ``ProDAFitState.scaler_state()`` does, once.  With a scale that never changes the dynamic path gives the static
path's bits.  DESIGN.md "Dynamic loss scale for ProDA".

Validation: ``fit_context(val=(val_features, val_labels), val_class_chunk=, val_bins=, final_model="last_step" | "best_val",
val_criterion=, return_monitor=)`` scores the contexts behind every epoch on the device and keeps the contexts of the best epoch in a
device slot, with no read-back before the run's one wait (``ProDAFitState.validate`` / ``start_monitor`` / ``monitor`` / ``best_params``).
It scores the test-time classifier (proda.py:316-331; ``trainers.proda.CustomCLIP.set_classifier``): the mean over ALL ``n_prompt``
contexts at their three positions, of which a training step only ever runs ``prompt_bs`` -- one call, clipmi_proda_val_logits, which
runs the inference text tower ``val_class_chunk`` classes at a time.  It draws no random number: the selection schedule is the one of
the fit without ``val``.  DESIGN.md "Fit monitor", "CoCoOp and ProDA".
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, fitloop, fitmonitor, fitoptim, ops
from . import shard as sharding
from ._lib import check, lib
from .coopfit import DEFAULT_GRAD_SCALE, MAX_LIVE_ROWS, _DT, _Tower, _check_batch, _live_rows, operand_stats_dict
from .fitloop import _host_int_array, _need_gpu, steps_per_epoch
from .parallel import shard_bounds
from .shard import Shard, shard_states


def positions(n_prompt: int) -> np.ndarray:
    """proda.py:110-114: 0 (front) for the first quarter, 1 (middle) for the second, 2 (end) for the rest."""
    q = n_prompt // 4
    return np.array([0] * q + [1] * q + [2] * (n_prompt - 2 * q), np.int32)


def reference_order(sel, pos: np.ndarray) -> np.ndarray:
    """``sel`` as the reference's forward orders a class's prompts: the end-position contexts, then the middle, then the front ones, the
    order inside a group kept (proda.py:167-213)."""
    sel = np.asarray(sel, np.int64)
    return np.concatenate([sel[pos[sel] == k] for k in (2, 1, 0)]).astype(np.int32)


def draw_selections(n_prompt: int, prompt_bs: int, steps: int, generator: torch.Generator) -> np.ndarray:
    """The reference's schedule (proda.py:148-157) for ``steps`` steps, int32 [steps, prompt_bs]: a ``randperm(n_prompt)`` from
    ``generator`` every n_prompt / prompt_bs steps, consumed in slices of ``prompt_bs``, each slice in ``reference_order``.  With
    ``prompt_bs == n_prompt`` nothing is drawn: every step uses all contexts in their natural order."""
    pos, n_iter = positions(n_prompt), n_prompt // prompt_bs
    out = np.empty((steps, prompt_bs), np.int32)
    perm = None
    for k in range(steps):
        if n_iter == 1:
            batch = np.arange(n_prompt)
        else:
            if k % n_iter == 0:
                perm = torch.randperm(n_prompt, generator=generator).numpy()
            batch = perm[(k % n_iter) * prompt_bs:(k % n_iter + 1) * prompt_bs]
        out[k] = reference_order(batch, pos)
    return out


def _check_collection(who: str, n_prompt: int, prompt_bs: int) -> None:
    if n_prompt < 4 or n_prompt % 4:
        raise ValueError(f"{who}: n_prompt={n_prompt} must be a positive multiple of 4: the reference's position list [front] * (n // 4) + [middle] * (n // 4) "
                         "+ [end] * (n // 2) has fewer than n_prompt entries otherwise, and with one prompt the no-class loss is the mean of nothing")
    if prompt_bs < 1 or n_prompt % prompt_bs:
        raise ValueError(f"{who}: prompt_bs={prompt_bs} must divide n_prompt={n_prompt}")


def _check_alpha(who: str, alpha: float) -> float:
    if not (math.isfinite(alpha) and alpha >= 0.0):
        raise ValueError(f"{who}: alpha={alpha} (finite, >= 0)")
    return float(alpha)


def _check_sel(who: str, sel, P: int, pos: np.ndarray, name: str = "sel") -> np.ndarray:
    """One selection [Pb] or a schedule [steps, Pb] in the reference's order, after the range and repeat checks."""
    a = _host_int_array(who, sel, name)
    if a.ndim not in (1, 2) or a.shape[-1] < 1 or P % a.shape[-1]:
        raise ValueError(f"{who}: {name} {a.shape} must hold prompt_bs indices (a divisor of n_prompt={P}) per step")
    if a.size and (a.min() < 0 or a.max() >= P):
        raise ValueError(f"{who}: {name} holds indices outside the {P} contexts [0, {P})")
    rows = a.reshape(-1, a.shape[-1])
    if any(len(set(r.tolist())) != len(r) for r in rows):
        raise ValueError(f"{who}: {name} names a context twice in one step")
    out = np.stack([reference_order(r, pos) for r in rows]) if len(rows) else np.zeros((0, a.shape[-1]), np.int32)
    return out[0] if a.ndim == 1 else out


def _check_prompts(who: str, clip_model, tokenized_prompts, ctx, name_lens, seq_rows):
    """(ids with the no-class prompt appended [C + 1, Lc], C, P, n_ctx, name_lens int32 [C], last EOT) after the host-side checks."""
    L, D = int(clip_model.context_length), int(clip_model.ln_final.weight.shape[0])
    if getattr(clip_model, "ivlp_text_prompts", None) is not None and clip_model.ivlp_text_prompts()[0]:
        raise ValueError(f"{who}: the model's text tower carries deep prompts; the training forward does not support them")
    ids = _host_int_array(who, tokenized_prompts, "tokenized_prompts")
    if ids.ndim != 2 or ids.shape[1] != L or ids.shape[0] < 2:
        raise ValueError(f"{who}: tokenized_prompts {ids.shape} must be [C >= 2, {L}]")
    if not isinstance(ctx, torch.Tensor) or ctx.dim() != 3 or ctx.shape[-1] != D or not ctx.dtype.is_floating_point:
        raise ValueError(f"{who}: ctx {tuple(getattr(ctx, 'shape', ()))} must be [n_prompt, n_ctx, {D}]")
    P, n_ctx = int(ctx.shape[0]), int(ctx.shape[1])
    eot = ids.argmax(axis=1)
    if n_ctx < 1 or int(eot.min()) < n_ctx + 2:
        raise ValueError(f"{who}: n_ctx={n_ctx} does not fit the prompts (first EOT at {int(eot.min())}): the layout is [SOS | X * n_ctx | name | '.' | EOT]")
    own = eot - n_ctx - 2
    if name_lens is None:
        nl = own
    else:
        nl = _host_int_array(who, name_lens, "name_lens")
        if nl.shape != (ids.shape[0],):
            raise ValueError(f"{who}: name_lens {nl.shape} must hold one length per class ({ids.shape[0]})")
        if nl.min() < 0:
            raise ValueError(f"{who}: name_lens holds a negative length")
        if (nl > own).any():
            c = int(np.argmax(nl > own))
            raise ValueError(f"{who}: name_lens[{c}]={int(nl[c])} pushes a context row past the live rows of its prompt (EOT at {int(eot[c])}, n_ctx={n_ctx}: at "
                             f"most {int(own[c])})")
    last = int(eot.max())
    if seq_rows is not None and int(seq_rows) and int(seq_rows) <= last:
        raise ValueError(f"{who}: seq_rows={int(seq_rows)} cuts the EOT row {last}")
    live = _live_rows(clip_model, last, seq_rows) or L
    if live > MAX_LIVE_ROWS:
        raise ValueError(f"{who}: seq_rows gives {live} live token rows per prompt; the backward holds at most {MAX_LIVE_ROWS}")
    # the no-class prompt "X .. X ." from a class prompt with its name taken out: [SOS, X * n_ctx, '.', EOT, 0 ..]
    c0 = int(np.argmin(own))
    nc = np.zeros((1, L), ids.dtype)
    nc[0, :1 + n_ctx] = ids[c0, :1 + n_ctx]
    nc[0, 1 + n_ctx:L - int(own[c0])] = ids[c0, 1 + n_ctx + int(own[c0]):]
    return np.concatenate([ids, nc]), ids.shape[0], P, n_ctx, nl.astype(np.int32), last


class _ProDATower(_Tower):
    """``coopfit._Tower`` over ProDA's N = C Pb + P assembled prompts: ``base`` holds the C class embeddings and, last, the no-class one.
    ``nc=(lo, hi)``: a rank of the class-sharded fit -- ``ids_all``, ``n_cls`` and ``name_lens`` are its own classes' and of the P
    no-class prompts it runs those of the contexts lo .. hi - 1: N = C_r Pb + (hi - lo)."""

    def __init__(self, who, clip_model, ids_all, n_cls, P, Pb, n_ctx, name_lens, last_eot, seq_rows, nc=None):
        super().__init__(who, clip_model, ids_all, n_cls * Pb + (P if nc is None else nc[1] - nc[0]), n_ctx, False, last_eot, seq_rows)
        dev = clip_model.device
        self.n_cls, self.P, self.Pb, self.nc = n_cls, P, Pb, nc
        self.N = self.C                       # _Tower sizes workspace, stash, text and d_embed by the number of prompts
        self.cls_base, self.nc_base = self.base[:n_cls], self.base[n_cls:]
        self.cls_eot = self.eot[:n_cls].contiguous()      # of the ids: every prompt of a class keeps its class's EOT row
        self.pos = torch.from_numpy(positions(P)).to(dev)
        self.name_lens = torch.from_numpy(name_lens).to(dev)
        self.prompts = torch.empty(self.N, self.Lc, self.D, dtype=torch.float32, device=dev)
        self.eot = torch.empty(self.N, dtype=torch.int32, device=dev)

    def forward(self, ctx: torch.Tensor, sel: torch.Tensor) -> torch.Tensor:
        m = self.model
        if self.nc is None:
            ops.proda_embed(self.cls_base, self.nc_base, ctx, sel, self.pos, self.name_lens, self.cls_eot, self.rows, self.prompts, self.eot)
        else:
            ops.proda_embed_shard(self.cls_base, self.nc_base, ctx, sel, self.pos, self.name_lens, self.cls_eot, *self.nc, self.rows, self.prompts, self.eot)
        with m._launch_lock:
            check(lib.clipmi_text_encoder_train(m._handle, self.prompts.data_ptr(), _lib.F32, None, 0, 0, self.eot.data_ptr(), self.N, self.rows, None,
                                                self.text.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self.stash.data_ptr(), self.stash.numel(),
                                                _lib.CALL_DEFAULT, ops._stream()), "clipmi_text_encoder_train")
        return self.text

    def one_call_workspace(self, B: int, scaled: bool = False) -> torch.Tensor:
        if scaled:
            need = lib.clipmi_proda_train_step_scaled_bytes(self.model._handle, self.n_cls, self.Pb, self.P, self.rows, B, self.n_ctx)
        else:
            need = lib.clipmi_proda_train_step_bytes(self.model._handle, self.n_cls, self.Pb, self.P, self.rows, B)
        if self.step_ws is None or self.step_ws.numel() < need:
            self.step_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.ws.device)
        return self.step_ws


def context_gradient(clip_model, tokenized_prompts, ctx: torch.Tensor, features: torch.Tensor, labels, sel=None, name_lens=None, alpha: float = 0.1,
                     logit_scale: float = 4.6052, grad_scale: float = DEFAULT_GRAD_SCALE, seq_rows: Optional[int] = None, return_parts: bool = False,
                     return_operand_stats: bool = False, shard: Optional[Shard] = None):
    """``(loss, grad)`` of ProDA's training loss (module docstring) with respect to ``ctx`` [P, n_ctx, D] on the GPU: loss fp32 [1], grad
    fp32 [P, n_ctx, D].  ``tokenized_prompts`` [C, context_length]: the ids of ``"X .. X name."``; ``features`` fp32 [B, E] raw image
    features (the rows may be a column slice).  ``sel``: the contexts this step uses (None: all of them; any order -- it is put into the
    reference's end | middle | front order); ``name_lens``: the classes' name lengths in tokens (None: EOT - n_ctx - 2, as the inference
    mirror derives them; a shorter one moves fewer tokens in front of or between the context vectors, as in the reference, and the
    EOT row stays the prompt's own).  ``return_parts`` adds a dict: ``upper``, ``m`` (fp32 [1] each), ``text`` (the raw text features fp32
    [C Pb + P, E], class prompts first) and ``sel`` (int32, as used).  ``return_operand_stats`` adds, last, ``coopfit.context_gradient``'s
    dict over every fp16 dgrad-GEMM operand element of the backward.

    ``shard``: the gradient the class-sharded step would apply (module docstring), reduced over the ranks in rank order -- the same bits
    on every rank; ``text`` is then the gathered, compacted matrix.  The operand statistics are per rank and are refused."""
    who = "context_gradient"
    ids_all, Cn, P, n_ctx, nl, last = _check_prompts(who, clip_model, tokenized_prompts, ctx, name_lens, seq_rows)
    if shard is not None:
        sharding.check(who, shard, n_cls=Cn, n_prompt=P, return_operand_stats=return_operand_stats)
    pos = positions(P)
    sel_h = _check_sel(who, np.arange(P) if sel is None else sel, P, pos)
    if sel_h.ndim != 1:
        raise ValueError(f"{who}: sel {sel_h.shape} must be one selection [prompt_bs]")
    _check_collection(who, P, len(sel_h))
    alpha = _check_alpha(who, alpha)
    gs = fitoptim.static_grad_scale(who, grad_scale, "ProDAFitState", "fit_context")
    scale = fitloop.exp_logit_scale(who, logit_scale)
    E = int(clip_model.geometry.embed_dim)
    labels_d = _check_batch(who, features, labels, Cn, E)
    _need_gpu(features, "features")
    dev = features.device
    if shard is not None:     # the sharded step's phases with a report in the step's place
        make = lambda sh: ProDAFitState(clip_model, tokenized_prompts, ctx, len(sel_h), alpha, logit_scale, 0.0, 0.0, False, 0.0, gs, seq_rows, name_lens,
                                        shard=sh)
        state = shard_states(make, shard)
        sel_d = torch.from_numpy(sel_h).to(dev)

        def phases(s, report):
            report["losses"] = torch.empty(3, dtype=torch.float32, device=dev)
            return s._shard_phases(features, labels_d, sel_d, None, report["losses"], True, report)
        report = sharding.report_all(shard, state, who, phases)
        losses, grad, text = report["losses"], report["grad"], report["text"]
    else:
        tower = _ProDATower(who, clip_model, ids_all, Cn, P, len(sel_h), n_ctx, nl, last, seq_rows)
        sel_d = torch.from_numpy(sel_h).to(dev)
        text = tower.forward(fitloop.master(ctx, dev), sel_d)
        stats = torch.zeros(4, dtype=torch.int64, device=dev) if return_operand_stats else None
        losses, d_text = ops.proda_head(features, labels_d, text, Cn, len(sel_h), scale, gs, alpha)
        d_embed = tower.backward(d_text, stats)
        grad = ops.proda_ctx_step(d_embed, sel_d, tower.pos, tower.name_lens, n_ctx, gs)
    out = (losses[0:1], grad)
    if return_parts:
        out += ({"upper": losses[1:2], "m": losses[2:3], "text": text.clone(), "sel": sel_d},)
    return out + ((operand_stats_dict(stats),) if return_operand_stats else ())


def _aligned_fp32(features: torch.Tensor) -> torch.Tensor:
    """What clipmi_proda_val_logits reads: fp32, contiguous, on a 16-byte boundary."""
    feats = features.detach().to(torch.float32).contiguous()
    return feats.clone() if feats.data_ptr() % 16 else feats


class ProDAFitState(fitmonitor.Monitored, fitoptim.Optimised):
    """The training state of ProDA's contexts: the fp32 master ``ctx`` [P, n_ctx, D], SGD's momentum buffer, the tower's stash, the
    selection schedule's generator and the number of steps taken.  ``step`` enqueues one forward, backward and update and does not
    synchronise.  ``validate`` scores cached validation features through the inference mirror (``start_monitor``, ``monitor``,
    ``best_params``, ``val_logits``: ``fitmonitor.Monitored`` on a plain ``fitmonitor.History``; the logits live in a workspace of the
    state's own, scored inside the one library call).  The loss scale, the optimiser's arguments and moments and ``scaler_state`` are
    ``fitoptim.Optimised``'s."""
    _who, _history = "ProDAFitState", fitmonitor.History

    def __init__(self, clip_model, tokenized_prompts, ctx: torch.Tensor, prompt_bs: int = 4, alpha: float = 0.1, logit_scale: float = 4.6052,
                 momentum: float = 0.9, dampening: float = 0.0, nesterov: bool = False, weight_decay: float = 5e-4,
                 grad_scale: float = DEFAULT_GRAD_SCALE, seq_rows: Optional[int] = None, name_lens=None,
                 optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8,
                 shard: Optional[Shard] = None, generator: Optional[torch.Generator] = None, scaler: Optional[dict] = None):
        """``optimizer``: "sgd" (``momentum``, ``dampening``, ``nesterov``), "adam" or "adamw" (``betas``, ``eps``;
        ``weight_decay`` keeps the fit's default of 5e-4 under all three -- torch's AdamW default of 1e-2 is NOT taken over).
        ``shard``: this state is one rank of the class-sharded fit (module docstring).  It holds the whole ``ctx`` and runs the tower
        over its own classes and no-class prompts; ``generator`` must be seeded alike on every rank of an RCCL run (the default is)."""
        who = "ProDAFitState"
        ids_all, self.C, self.P, self.n_ctx, nl, last = _check_prompts(who, clip_model, tokenized_prompts, ctx, name_lens, seq_rows)
        self.Pb = int(prompt_bs)
        _check_collection(who, self.P, self.Pb)
        self.shard = shard
        if shard is not None:
            sharding.check(who, shard, n_cls=self.C, n_prompt=self.P)
        self.alpha = _check_alpha(who, alpha)
        self._init_optimiser(who, logit_scale, momentum, dampening, nesterov, weight_decay, grad_scale, scaler, optimizer, betas, eps, sgd_shard=shard)
        dev = clip_model.device
        if shard is None:
            self.tower = _ProDATower(who, clip_model, ids_all, self.C, self.P, self.Pb, self.n_ctx, nl, last, seq_rows)
        else:   # the tower over the rank's own classes and no-class prompts; the live-row cut is the full prompt set's
            self.lo, self.hi = shard_bounds(self.C, shard.rank, shard.world)
            self.nc_lo, self.nc_hi = shard_bounds(self.P, shard.rank, shard.world)
            own = np.concatenate([ids_all[self.lo:self.hi], ids_all[self.C:]])
            self.tower = _ProDATower(who, clip_model, own, self.hi - self.lo, self.P, self.Pb, self.n_ctx, nl[self.lo:self.hi], last, seq_rows,
                                     nc=(self.nc_lo, self.nc_hi))
            self._shard_buffers(dev)
        self.ctx = fitloop.master(ctx, dev)
        self._init_moments(self.ctx)
        self.generator = generator if generator is not None else torch.Generator().manual_seed(0)
        self.pos_host = positions(self.P)
        self._perm = None
        self._ids = ids_all[:self.C]
        self._val = None            # what a validation keeps between epochs: the inference operands and the two workspaces
        self.val_class_chunk = None # validate's classes per tower call when its argument is None (None: 4096 // n_prompt, at least 1)

    # ---- the class-sharded step (csrc/proda_train.hip, DESIGN.md "Class-sharded ProDA fit")

    def _shard_buffers(self, dev) -> None:
        """The send and receive blocks of the step's two gathers, made once.  The tower writes its text features straight into the first
        rows of the padded send block; the padding of either block is moved and never read."""
        sh, t = self.shard, self.tower
        G, rows = sh.world, ops.proda_shard_rows(self.C, self.Pb, self.P, sh.world)
        f32 = dict(dtype=torch.float32, device=dev)
        self._send_text = torch.empty(rows, t.E, **f32)
        t.text = self._send_text[:t.N]
        self._all_text = torch.empty(G, rows, t.E, **f32)
        self._text = torch.empty(self.C * self.Pb + self.P, t.E, **f32)
        self._own_d_text = torch.empty(t.N, t.E, **f32)
        slots = self.Pb + -(-self.P // G)          # the class sums of the Pb selected contexts | the rank's no-class rows, padded
        self._send_part = torch.empty(slots, t.n_ctx, t.D, **f32)
        self._all_part = torch.empty(G, slots * t.n_ctx * t.D, **f32)
        sharding.file_state(sh, self)

    def _shard_phases(self, features, labels_d, sel_d, lr_d, losses, first: bool, report: Optional[dict] = None):
        """One sharded step as phases, a ``yield`` behind every gather.  ``report``: a dict that receives the reduced gradient and the
        compacted text features INSTEAD of a step: neither the contexts nor the momentum buffer nor the scaler block is touched."""
        t, sh, st, gs = self.tower, self.shard, ops._stream(), self._head_scale
        t.forward(self.ctx, sel_d)                                                           # the rank's own prompts
        sh.gather(self._send_text, self._all_text, self._send_text.numel() * 4, st)
        yield
        text = ops.proda_shard_compact(self._all_text, self.C, self.Pb, self.P, self._text)
        _, d_text = ops.proda_head(features, labels_d, text, self.C, self.Pb, self.scale, gs, self.alpha, losses)
        own, n_cls, all_cls = self._own_d_text, (self.hi - self.lo) * self.Pb, self.C * self.Pb
        own[:n_cls].copy_(d_text[self.lo * self.Pb:self.hi * self.Pb])                       # the rank's own rows of the replicated d_text
        own[n_cls:].copy_(d_text[all_cls + self.nc_lo:all_cls + self.nc_hi])
        self._scale_rows(own)
        d_embed = t.backward(own)
        n_own = self.nc_hi - self.nc_lo
        ops.proda_ctx_partial(d_embed, sel_d, t.pos, t.name_lens, n_own, t.n_ctx, self._send_part[:self.Pb + n_own])
        sh.gather(self._send_part, self._all_part, self._send_part.numel() * 4, st)
        yield
        if report is not None:
            report["grad"], report["text"] = ops.proda_ctx_step_gathered(self._all_part, sel_d, self.P, t.n_ctx, t.D, gs), text
            return
        if self.dynamic:
            ops.proda_ctx_reduce_gathered_scaled(self._all_part, sel_d, self.P, t.n_ctx, t.D, self._scaler.block, self.ctx, self.buf, lr_d,
                                                 *self._scaler.args(), *self._sgd, want_grad=False, workspace=self._scaled_ws())
        else:
            ops.proda_ctx_step_gathered(self._all_part, sel_d, self.P, t.n_ctx, t.D, gs, self.ctx, self.buf, lr_d, first, *self._sgd, want_grad=False)

    def _scaled_ws(self) -> torch.Tensor:
        """The workspace of ProDA's scaled steps (one size for the unsharded and the gathered one), made on the first step."""
        sc, t = self._scaler, self.tower
        if sc.ws is None:
            need = lib.clipmi_proda_ctx_step_scaled_workspace_bytes(self.P, t.D, t.n_ctx)
            sc.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.ctx.device)
        return sc.ws

    # ---- per-epoch validation and best-epoch selection on the device (DESIGN.md "Fit monitor", "CoCoOp and ProDA")

    def _master(self) -> torch.Tensor:
        return self.ctx.reshape(-1)

    def _val_operands(self):
        """What the inference mirror (``trainers.proda.CustomCLIP.set_classifier``) works on, made once: the classes' embeddings
        [C, context_length, D] in the model's type, the order of a class's prompts (ALL contexts, end | middle | front) and the live
        token rows of the class list."""
        if self._val is None:
            m = self.tower.model
            m._ensure_bound()
            ids_h = torch.from_numpy(np.ascontiguousarray(self._ids)).long()
            with torch.no_grad():
                base = m.token_embedding(ids_h.to(m.device)).type(m.dtype).contiguous()
            order = torch.from_numpy(reference_order(np.arange(self.P), self.pos_host)).to(m.device)
            self._val = {"base": base, "order": order, "rows": m.live_rows(ids_h), "ws": None, "mon_ws": None}
        return self._val

    def validate(self, val_features: torch.Tensor, val_labels, epoch: int, val_class_chunk: Optional[int] = None) -> None:
        """Enqueue one validation of the current master contexts into slot ``epoch`` of the device history; no host read, and no random
        number is drawn: the selection schedule is not touched.  It scores what ``trainers.proda.CustomCLIP`` would compute with these
        contexts (proda.py:316-331, 304-313): ALL ``n_prompt`` contexts at their positions, rounded to the model's type as loading them into
        the module rounds them, through the INFERENCE text tower ``val_class_chunk`` classes at a time (None: as many as keep a call at or
        below 4096 prompts, ``CustomCLIP``'s ``prompts_per_call``), every feature L2-normalised and a class's ``n_prompt`` features
        averaged (not renormalised), then ``exp(logit_scale)`` times the normalised ``val_features`` (raw image features fp32
        [N_val, E] on the GPU) against the means into the monitor's [N_val, C] workspace (4 N_val C bytes), ``clipmi_val_score`` into
        the record and, when the monitor selects, ``clipmi_best_select`` of ``ctx`` -- one library call, clipmi_proda_val_logits.  The
        record does not depend on ``val_class_chunk`` as long as the tower's kernel choice, which follows the row count of a call, does
        not change (include/clipmi.h).  ``val_labels`` [N_val]: an int64 tensor on the GPU is taken as it is; anything else is
        range-checked on the host.  The contexts, the momentum buffer, the scaler block and the training stash are not touched.  The
        classes' name lengths are the state's (``name_lens``); the inference mirror derives its own from the EOT rows, which is the
        state's default.  Without ``start_monitor`` the history starts with ``epoch + 1`` slots of 10 bins and no selection."""
        who = "ProDAFitState.validate"
        if self.shard is not None:
            raise ValueError(f"{who}: shard has no validation (the sharded fit scores nothing between epochs)")
        mon, t, m = self._monitor_for(epoch), self.tower, self.tower.model
        epoch = mon.slot(who, epoch)
        if val_class_chunk is None:
            val_class_chunk = self.val_class_chunk
        cc = max(1, 4096 // self.P) if val_class_chunk is None else val_class_chunk
        if isinstance(cc, bool) or int(cc) != cc or int(cc) < 1:
            raise ValueError(f"{who}: val_class_chunk={val_class_chunk} must be an integer >= 1")
        cc = min(int(cc), self.C)
        v = self._val_operands()
        feats, labels_d, _ = mon.val_set(who, val_features, val_labels, t.E, self.C, _aligned_fp32)
        N, dev = feats.shape[0], feats.device
        need = lib.clipmi_proda_val_logits_bytes(m._handle, self.C, self.P, v["rows"], cc, N)
        mon_need = lib.clipmi_proda_val_monitor_bytes(N, self.C, mon.bins)
        if need == 0 or mon_need == 0:
            raise ValueError(f"{who}: N_val={N}, C={self.C}, n_prompt={self.P}, val_class_chunk={cc} are more than one validation call takes")
        if v["ws"] is None or v["ws"].numel() < need:
            v["ws"] = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        if v["mon_ws"] is None or v["mon_ws"].numel() < mon_need:
            v["mon_ws"] = torch.empty(max(mon_need, 256), dtype=torch.uint8, device=dev)
        v["n_val"] = N
        select = mon.block is not None
        with m._launch_lock:
            check(lib.clipmi_proda_val_logits(m._handle, v["base"].data_ptr(), _DT[v["base"].dtype], self.ctx.data_ptr(), v["order"].data_ptr(),
                                              t.pos.data_ptr(), t.name_lens.data_ptr(), t.cls_eot.data_ptr(), self.C, self.P, self.n_ctx, v["rows"], cc,
                                              self.scale, _lib.CALL_DEFAULT, epoch, feats.data_ptr(), feats.stride(0), labels_d.data_ptr(), N, mon.bins,
                                              mon.records.data_ptr(), ops.VAL_CRITERIA[mon.criterion], mon.block.data_ptr() if select else None,
                                              mon.best.data_ptr() if select else None, v["mon_ws"].data_ptr(), v["mon_ws"].numel(),
                                              v["ws"].data_ptr(), v["ws"].numel(), ops._stream()), "clipmi_proda_val_logits")
        mon.seen = max(mon.seen, epoch + 1)

    def val_logits(self) -> torch.Tensor:
        """The fp32 [N_val, C] logits of the last ``validate``, where the monitor's workspace keeps them (the next one overwrites them)."""
        if self._val is None or self._val.get("mon_ws") is None:
            raise ValueError("ProDAFitState.val_logits: nothing has been validated")
        N = self._val["n_val"]
        return self._val["mon_ws"][:4 * N * self.C].view(torch.float32).view(N, self.C)

    def best_params(self) -> torch.Tensor:
        """The best slot on the device, fp32 [P, n_ctx, D]: the contexts of the best epoch so far, or the contexts ``start_monitor`` saw
        while no epoch has been taken."""
        return self._best_block("best_params").view_as(self.ctx)

    def next_selection(self) -> np.ndarray:
        """The schedule's next slice (``draw_selections``, one step at a time)."""
        n_iter = self.P // self.Pb
        k = self.steps % n_iter
        if n_iter == 1:
            return reference_order(np.arange(self.P), self.pos_host)
        if k == 0 or self._perm is None:
            self._perm = torch.randperm(self.P, generator=self.generator).numpy()
        return reference_order(self._perm[k * self.Pb:(k + 1) * self.Pb], self.pos_host)

    def step(self, features: torch.Tensor, labels, lr, sel=None, want_loss: bool = False, one_call: bool = False) -> Optional[torch.Tensor]:
        """One optimiser step on the batch ``features`` fp32 [B, E] and ``labels`` [B] at the rate ``lr``, as ``CoOpFitState.step`` takes
        them.  ``sel``: this step's contexts -- None draws the schedule's next slice on the host; an int32 tensor [prompt_bs] on the
        GPU is taken as it is, already in the reference's order (a bad entry then poisons the context with NaN, it is never an
        address); anything else is checked and ordered on the host.  ``one_call``: the same launches through
        clipmi_proda_train_step (clipmi_proda_train_step_scaled under the dynamic scale).  Returns the batch loss, fp32 [1] on the device,
        when ``want_loss``.  Under the dynamic scale a skipped step still counts in ``steps`` -- the selection schedule moves on -- and
        still returns its loss; whether it was applied is in ``scaler_state()``.  Under ``optimizer="adam" | "adamw"`` the gather-reduce
        leaves the contexts' gradient as ``context_gradient`` returns it -- every context has one, its no-class prompt's row -- and
        clipmi_block_step_adam applies it to the whole collection (clipmi_block_step_adam_scaled under the dynamic scale, on the gradient
        formed at ``grad_scale = 1``); ``one_call`` is then refused: the one-call steps stay SGD.  Under ``shard`` every rank makes this
        call with the same batch and, where ``sel`` is None, draws the same selection from its like-seeded generator; under a
        ``LocalGather`` the first state that steps drives all the world's states and draws alone (``one_call`` is refused)."""
        who = "ProDAFitState.step"
        self._no_one_call_adam(who, one_call)
        states = None
        if self.shard is not None:
            # every rank is given the same batch; under a local gather this call steps all the world's states, one phase at a time, and
            # this state alone draws the selection
            sharding.check(who, self.shard, one_call=one_call)
            states = sharding.drive(self.shard, self, who)
        labels_d = _check_batch(who, features, labels, self.C, self.tower.E)
        _need_gpu(features, "features")
        if features.dtype != torch.float32 or features.stride(1) != 1:
            raise TypeError(f"{who}: features must be fp32 with unit column stride")
        dev = features.device
        if isinstance(sel, torch.Tensor) and sel.is_cuda and sel.dtype == torch.int32:
            if sel.shape != (self.Pb,):
                raise ValueError(f"{who}: sel {tuple(sel.shape)} must be [prompt_bs] = [{self.Pb}]")
            sel_d = sel.contiguous()
        else:
            sel_h = self.next_selection() if sel is None else _check_sel(who, sel, self.P, self.pos_host)
            if sel_h.shape != (self.Pb,):
                raise ValueError(f"{who}: sel {sel_h.shape} must be [prompt_bs] = [{self.Pb}]")
            sel_d = torch.from_numpy(sel_h).to(dev)
        lr_d = ops._dev(fitloop.lr_operand(lr, dev), "lr", (torch.float32,))
        t, first = self.tower, self.steps == 0
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        if states is not None:
            sharding.step_all(states, self, lambda s: s._shard_phases(features, labels_d, sel_d, lr_d, losses if s is self else torch.empty_like(losses), first))
        elif one_call:
            self._one_call(features, labels_d, sel_d, lr_d, losses, first)
        else:
            gs = self._head_scale
            text = t.forward(self.ctx, sel_d)
            _, d_text = ops.proda_head(features, labels_d, text, t.n_cls, t.Pb, self.scale, gs, self.alpha, losses)
            self._scale_rows(d_text)
            d_embed = t.backward(d_text)
            step_args = (d_embed, sel_d, t.pos, t.name_lens, t.n_ctx)
            # Adam: the step entry forms the contexts' gradient at the head's scale and applies nothing
            grad = ops.proda_ctx_step(*step_args, gs) if self._adam is not None else (d_embed, sel_d)
            self._apply_block(grad, lr_d, lambda: ops.proda_ctx_step(*step_args, gs, self.ctx, self.buf, lr_d, first, *self._sgd, want_grad=False))
        self.steps += 1
        return losses[0:1] if want_loss else None

    def _apply_scaled(self, grad, lr_d: torch.Tensor) -> None:
        """SGD under the dynamic scale is ProDA's own kernel, not the block's: clipmi_proda_ctx_step_scaled is handed the tower's input
        gradient and the selection (``grad`` is the pair), gathers and reduces the selected contexts' rows itself and decides on the
        device whether the step is applied."""
        t, sc = self.tower, self._scaler
        ops.proda_ctx_step_scaled(*grad, t.pos, t.name_lens, t.n_ctx, sc.block, self.ctx, self.buf, lr_d, *sc.args(), *self._sgd, want_grad=False,
                                  workspace=self._scaled_ws())

    def _one_call(self, features, labels_d, sel_d, lr_d, losses, first: bool) -> None:
        """``step`` through the library's one-call step: one of two symbols (static or scaled) on one run of arguments."""
        t, m, sc = self.tower, self.tower.model, self._scaler
        ws = t.one_call_workspace(features.shape[0], scaled=self.dynamic)
        name = "clipmi_proda_train_step" + ("_scaled" if self.dynamic else "")
        front = (m._handle, C.byref(t.dgrad[0]), t.cls_base.data_ptr(), t.nc_base.data_ptr(), _DT[t.base.dtype], self.ctx.data_ptr(),
                 None if self.buf is None else self.buf.data_ptr(), t.n_ctx, sel_d.data_ptr(), t.pos.data_ptr(), t.name_lens.data_ptr(), t.cls_eot.data_ptr(),
                 t.n_cls, t.Pb, t.P, t.rows, features.data_ptr(), features.stride(0), labels_d.data_ptr(), features.shape[0], self.scale)
        if self.dynamic:
            how = (sc.block.data_ptr(), *sc.args(), self.alpha, lr_d.data_ptr())
        else:
            how = (self.grad_scale, self.alpha, lr_d.data_ptr(), int(first))
        with m._launch_lock:
            check(getattr(lib, name)(*front, *how, *self._sgd, losses.data_ptr(), None, ws.data_ptr(), ws.numel(), t.stash.data_ptr(), t.stash.numel(),
                                     ops._stream()), name)


def init_context(clip_model, n_ctx: int = 16, n_prompt: int = 32, seed: int = 0) -> torch.Tensor:
    """The reference's random initialisation (proda.py:93-94): N(0, 0.02^2), [n_prompt, n_ctx, D]."""
    D = int(clip_model.ln_final.weight.shape[0])
    return 0.02 * torch.randn(n_prompt, n_ctx, D, generator=torch.Generator().manual_seed(seed))


def fit_context(features: torch.Tensor, labels, clip_model, tokenized_prompts, ctx: Optional[torch.Tensor] = None, n_ctx: int = 16, n_prompt: int = 32,
                prompt_bs: int = 4, alpha: float = 0.1, logit_scale: float = 4.6052, lr: float = 0.002, epochs: int = 200, batch_size: int = 32,
                momentum: float = 0.9, dampening: float = 0.0, weight_decay: float = 5e-4, nesterov: bool = False,
                grad_scale: float = DEFAULT_GRAD_SCALE, seq_rows: Optional[int] = None, lr_per_epoch: Optional[Sequence[float]] = None, order=None,
                drop_last: bool = False, name_lens=None, selections=None, generator: Optional[torch.Generator] = None,
                optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8, val=None,
                val_class_chunk: Optional[int] = None, val_bins: int = 10, final_model: str = "last_step", val_criterion: str = "accuracy",
                return_monitor: bool = False, shard: Optional[Shard] = None, return_history: bool = False, scaler: Optional[dict] = None,
                return_scaler_state: bool = False):
    """Train ProDA's contexts on cached ``features`` fp32 [N, E] and ``labels`` [N], starting from ``ctx`` [n_prompt, n_ctx, D] (not
    modified; None = ``init_context(clip_model, n_ctx, n_prompt)``).  The loop and its arguments are ``coopfit.fit_context``'s:
    ``epochs`` passes of ``torch.optim.SGD`` over batches of ``batch_size``, ``lr_per_epoch`` (None: ``cosine_warmup_schedule``),
    ``order`` [epochs, N], ``drop_last``; everything is checked on the host before the first launch and nothing synchronises until the
    one wait at the end.  ``selections``: an int array [steps, prompt_bs] that replaces the schedule drawn from ``generator`` (None: a
    generator seeded with 0).  ``grad_scale="dynamic"`` with ``scaler`` (module docstring): a step that overflows fp16 is skipped on the
    device and the scale adapts; the schedule of rates and selections moves on over a skipped step.  Returns the fitted fp32 contexts on the device, or ``(ctx, per-step total losses)`` with
    ``return_history``; ``return_scaler_state`` (dynamic only) appends ``ProDAFitState.scaler_state()`` as read after the last step.  The defaults are unverified restatements of the reference's config (module docstring).

    ``val=(val_features, val_labels)`` (raw image features [N_val, E] on the GPU and their labels): behind the last step of every epoch
    ``ProDAFitState.validate`` scores the contexts against them on the device as the inference mirror would -- the mean over ALL
    ``n_prompt`` contexts, ``val_class_chunk`` classes per tower call -- into ``val_bins`` confidence bins; it draws no random number, so
    the fitted contexts and the sequence of selections are bit for bit those of the same call without ``val``, and the run still
    synchronises once.  ``final_model``, ``val_criterion`` and ``return_monitor`` as ``coopfit.fit_context`` takes them: "best_val" returns
    the contexts of the epoch that was strictly better than every earlier one (the starting contexts when no epoch was taken) and is
    refused without ``val``; ``return_monitor`` adds ``ProDAFitState.monitor()``'s dict as the last element of the result.  The six
    validation arguments stand in front of ``return_history`` (``scaler`` and ``return_scaler_state`` stay the signature's last two): pass
    them, and the three behind them, by keyword.

    ``optimizer``, ``betas``, ``eps``: "sgd" (the default; ``momentum``, ``dampening``, ``nesterov``), "adam" or
    "adamw", as ``coopfit.fit_context`` takes them; ``weight_decay`` keeps this fit's default of 5e-4 under all three (torch's AdamW
    default of 1e-2 is NOT taken over).  DESIGN.md "Adam steps for the prompt fits".

    ``shard=Shard(world, rank, gather)``: the class-sharded fit (module docstring).  Every rank makes this call with the same arguments
    -- the whole prompt set, the whole collection, all features -- and returns the same contexts.  The schedule of selections is drawn
    here, on the host, once: under RCCL every rank must pass a like-seeded ``generator`` (None is one) or the same ``selections``.  With
    a ``LocalGather`` the one call runs all ``world`` shard states in this process.  Both loss scales work; Adam, validation and
    ``final_model="best_val"`` are refused."""
    who = "fit_context"
    fitmonitor.check_args(who, val, val_bins, final_model, val_criterion)
    if val is not None and val_class_chunk is not None and (isinstance(val_class_chunk, bool) or int(val_class_chunk) != val_class_chunk
                                                            or int(val_class_chunk) < 1):
        raise ValueError(f"{who}: val_class_chunk={val_class_chunk} must be an integer >= 1")
    if ctx is None:
        _check_collection(who, int(n_prompt), int(prompt_bs))
        ctx = init_context(clip_model, n_ctx, n_prompt)
    _, Cn, P, n_ctx, _, _ = _check_prompts(who, clip_model, tokenized_prompts, ctx, name_lens, seq_rows)
    _check_collection(who, P, int(prompt_bs))
    if shard is not None:
        sharding.check(who, shard, n_cls=Cn, n_prompt=P, val=val, final_model=final_model)
    E = int(clip_model.geometry.embed_dim)
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] < 1 or features.shape[1] != E:
        raise ValueError(f"{who}: features must be a [N >= 1, E = {E}] tensor")
    N = features.shape[0]
    epochs, batch_size = fitloop.check_run(who, epochs, batch_size)
    dynamic, _, cfg = fitoptim.check_fit(who, optimizer, momentum, dampening, nesterov, weight_decay, betas, eps, grad_scale, scaler, shard=shard)
    if return_scaler_state and not dynamic:
        raise ValueError(f"{who}: return_scaler_state is an argument of grad_scale={fitoptim.DYNAMIC!r}")
    _check_alpha(who, alpha)
    lab = fitloop._labels(who, labels, N, Cn)
    order = fitloop.check_order(who, order, epochs, N)
    per_epoch = steps_per_epoch(N, batch_size, drop_last)
    dev = features.device
    _, lr_steps = fitloop.schedule(who, lr, epochs, lr_per_epoch, per_epoch, dev)
    steps = epochs * per_epoch
    if selections is None:
        sels = draw_selections(P, int(prompt_bs), steps, generator if generator is not None else torch.Generator().manual_seed(0))
    else:
        sels = _check_sel(who, selections, P, positions(P), "selections")
        if sels.ndim != 2 or sels.shape != (steps, int(prompt_bs)):
            raise ValueError(f"{who}: selections {sels.shape} must be [steps, prompt_bs] = [{steps}, {int(prompt_bs)}]")
    if val is not None:
        vf, vl = fitmonitor.check_val(who, val, E, Cn)
    if steps == 0:
        out = ctx.detach().to(torch.float32).clone()
        out = (out.to(dev) if features.is_cuda else out,) + ((np.zeros(0, np.float32),) if return_history else ())
        if return_scaler_state:
            out += ({"scale": cfg["init_scale"], "growth_tracker": 0, "skipped_steps": 0, "applied_steps": 0, "found_inf": 0},)
        if return_monitor:
            out += (fitmonitor.empty_monitor(val_bins),)
        return out if len(out) > 1 else out[0]
    _need_gpu(features, "features")
    make = lambda sh: ProDAFitState(clip_model, tokenized_prompts, ctx, prompt_bs, alpha, logit_scale, momentum, dampening, nesterov, weight_decay,
                                    grad_scale, seq_rows, name_lens, scaler=scaler, optimizer=optimizer, betas=betas, eps=eps, shard=sh)
    state = shard_states(make, shard)     # under a LocalGather all the world's states live here; a step of one steps them all
    sels_d = torch.from_numpy(np.ascontiguousarray(sels, dtype=np.int32)).to(dev)
    end_epoch = None
    if val is not None:
        _need_gpu(vf, "val_features")
        vl = vl.to(vf.device)
        state.start_monitor(epochs, val_bins, select=final_model == "best_val", val_criterion=val_criterion)
        end_epoch = lambda e: state.validate(vf, vl, e, val_class_chunk)
    history = fitloop.run_cached(lambda f, y, r, want: state.step(f, y, r, sel=sels_d[state.steps], want_loss=want), features,
                                 fitloop.labels_on(labels, lab, dev), fitloop.order_on(order, np.int64, dev), batch_size, per_epoch, epochs, lr_steps,
                                 return_history, end_epoch)
    fitted = state.best_params() if final_model == "best_val" else state.ctx
    out = (fitted, history) if return_history else (fitted,)
    if return_scaler_state:
        out = out + (state.scaler_state(),)
    if return_monitor:
        out = out + (fitmonitor.returned_monitor(state, val is not None, val_bins, True),)
    return out if len(out) > 1 else out[0]
