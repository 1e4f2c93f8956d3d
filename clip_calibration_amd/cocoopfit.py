"""CoCoOp's context and meta-net trained on the GPU (reference trainers/classification/cocoop.py:71-202, 259-278).

CoCoOp learns ``ctx`` [n_ctx, D] and ``meta_net`` = Linear(E, H) - ReLU - Linear(H, D) (H = E // 16 in the reference).  Every image gets
its own context ``ctx + meta_net(x_b)``, x_b its normalised feature, hence its own C prompts: a step runs the frozen text tower on
N = B C prompts, takes the cross-entropy of ``exp(logit_scale) x_b . u_{b,c}`` per image and one ``torch.optim.SGD`` step on the five
tensors, all with one set of hyper-parameters (the reference hands the whole prompt learner to one optimiser: weight decay falls on the
biases too).  The image tower is frozen, and the learned tensors reach the loss only through the text tower's input rows, so the step
stands on the frozen-tower forward and backward of csrc/text_backward.hip that CoOp trains on, once over the N prompts.  Around them,
csrc/cocoop_train.hip: the meta-net's forward with its ReLU output and the unit features kept, the fp32 prompt assembly, the per-pair
loss head, the reduce of the tower's input gradient into the five gradients, and one SGD launch over one contiguous fp32 master block
``[ctx | W1 | b1 | W2 | b2]`` (include/clipmi.h and DESIGN.md "CoCoOp fit" have the formulas).

The entry points mirror ``coopfit``'s and ``prodafit``'s: ``gradients`` (one batch's loss and the five gradients; the tests' diagnostic
entry), ``CoCoOpFitState.step`` (one batch of image features at a time) and ``fit_prompt_learner`` (cached features, every step
enqueued, one synchronisation at the end).  The five tensors travel as a dict under the names of the reference's ``state_dict``:
``ctx`` and ``meta_net.linear{1,2}.{weight,bias}``.

Refused: a class-specific context, models with deep prompts, more than 80 live token rows (the backward's limit), a meta-net whose
shapes do not chain.

UNVERIFIED, as for CoOp: Dassl is not part of this environment, so the defaults -- SGD at 0.002, batches of 1, 10 epochs, 4 context
vectors (``CTX_INIT "a photo of a"`` in the shipped config) -- restate the reference's config and Dassl's public defaults without a run of
the reference behind them; each is an argument.

``grad_scale="dynamic"`` with ``scaler=dict(init_scale, growth_factor, backoff_factor, growth_interval)`` is the reference's ``prec ==
"amp"`` branch (cocoop.py:249, ``torch.cuda.amp.GradScaler``) as ``coopfit`` has it: the scale lives in a block on the device, a step whose
gradient block holds an inf or a NaN changes neither the parameters nor the momentum block, and the scale backs off and grows again.  No
step reads anything back; ``CoCoOpFitState.scaler_state()`` does, once.  DESIGN.md "Dynamic loss scale for the block fits".  The
reference's ``autocast`` casts differ from this path's fixed fp16 operand points (unverified).  Not covered: class-token positions other
than ``end`` (the reference has none).

``shard=coopfit.Shard(world, rank, gather)`` on ``CoCoOpFitState``, ``fit_prompt_learner`` and ``gradients`` is the class-sharded fit, in
the place of the reference's ``nn.DataParallel`` over the text encoder (cocoop.py:252-257): one process per GPU, rank r of G running the
tower over the ``B x C_r`` prompts of its contiguous classes ``coopfit.shard_classes(C, G, r)`` -- the stash and the workspace are sized by
``B x C_r`` (``stash_bytes``).  The meta-net, the head, the meta-net's backward and the optimiser step run replicated on every rank; two
all-gathers per step move the raw text features (``B x ceil(C / G)`` rows per rank) and the ranks' partial sums ``[B, n_ctx, D]``
(clipmi_cocoop_dcs_partial), which clipmi_cocoop_reduce_gathered adds in rank order: every rank then holds the same gradient block bit
for bit, with no all-reduce and no float atomic, and steps its replicated master block with the unsharded state's own step.  So SGD,
``optimizer="adam" | "adamw"`` and ``grad_scale="dynamic"`` all work under the shard, and every rank takes the same skip-or-apply
decision.  Every rank is given the same batch.  With one rank the sharded step gives the unsharded step's bits.  Refused under ``shard``,
by name and before any device call: ``C < G``, ``one_call=True``, ``val=`` / ``val_loader=`` / ``final_model="best_val"`` /
``validate``, and ``gradients``' operand statistics.  DESIGN.md "Class-sharded CoCoOp fit".

Validation: ``fit_prompt_learner(val=(val_features, val_labels), val_batch_size=, val_bins=, final_model="last_step" | "best_val",
val_criterion=, return_monitor=)`` scores the parameters behind every epoch on the device and keeps the block of the best epoch in a
device slot, with no read-back before the run's one wait (``CoCoOpFitState.validate`` / ``start_monitor`` / ``monitor`` / ``best_params``).
It scores what the INFERENCE forward (``trainers.cocoop.CustomCLIP.forward``) computes: every validation image has its own C prompts, so
a chunk of ``val_batch_size`` images runs ``val_batch_size x C`` prompts through the inference text tower (clipmi_cocoop_val_chunk) and a
fused kernel forms an image's C logits in LDS and scores the row -- no [N_val, C] matrix of any kind exists.  DESIGN.md "Fit monitor",
"CoCoOp and ProDA".
"""
from __future__ import annotations

import collections
import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib, fitloop, fitmonitor, fitoptim, ops
from ._lib import check, lib
from . import shard as sharding
from .coopfit import MAX_LIVE_ROWS, _DT, _Tower, _check_batch, _live_rows, operand_stats_dict
from .coopfit import _check_prompts as _check_coop_prompts
from .fitloop import _host_int_array, _need_gpu, steps_per_epoch
from .shard import Shard, shard_classes, shard_states

# 2^10, measured on the ViT-B/16 text geometry with synthetic weights at the reference's batch of 1 (profiles/cocoopfit_parity.txt,
# "grad_scale"): with one image dz is not divided down by a batch, and CoOp's 2^12 leaves the largest fp16 dgrad-GEMM operand only 2^1.9
# below fp16's largest value; 2^10 leaves 2^3.9.  A model whose gradients are much larger overflows fp16 at this scale -- the parameters
# then turn NaN, they do not go wrong silently; pass a smaller power of two.
DEFAULT_GRAD_SCALE = 1024.0

NAMES = ("ctx", "meta_net.linear1.weight", "meta_net.linear1.bias", "meta_net.linear2.weight", "meta_net.linear2.bias")


def _check_params(who: str, clip_model, params) -> int:
    """The hidden width H after the shape checks of the five tensors against the model."""
    if not isinstance(params, dict) or any(k not in params for k in NAMES):
        raise ValueError(f"{who}: params must be a dict with the keys {NAMES}")
    for k in NAMES:
        if not isinstance(params[k], torch.Tensor) or not params[k].dtype.is_floating_point:
            raise ValueError(f"{who}: params[{k!r}] must be a floating-point tensor")
    D, E = int(clip_model.ln_final.weight.shape[0]), int(clip_model.geometry.embed_dim)
    ctx, w1, b1, w2, b2 = (params[k] for k in NAMES)
    if ctx.dim() != 2:
        raise ValueError(f"{who}: ctx {tuple(ctx.shape)} must be [n_ctx, {D}]: CoCoOp has no class-specific context")
    H = int(w1.shape[0]) if w1.dim() == 2 else 0
    if w1.dim() != 2 or w1.shape[1] != E or not 1 <= H <= 4096 or tuple(b1.shape) != (H,) or tuple(w2.shape) != (D, H) or tuple(b2.shape) != (D,):
        raise ValueError(f"{who}: meta_net shapes W1 {tuple(w1.shape)}, b1 {tuple(b1.shape)}, W2 {tuple(w2.shape)}, b2 {tuple(b2.shape)} must be "
                         f"[H, {E}], [H], [{D}, H], [{D}] with 1 <= H <= 4096")
    return H


def _check_prompts(who: str, clip_model, tokenized_prompts, params, seq_rows):
    """(C, n_ctx, H, last EOT) after the host-side checks."""
    H = _check_params(who, clip_model, params)
    Cn, n_ctx, _, last = _check_coop_prompts(who, clip_model, tokenized_prompts, params["ctx"])
    if seq_rows is not None and int(seq_rows) and int(seq_rows) <= last:
        raise ValueError(f"{who}: seq_rows={int(seq_rows)} cuts the EOT row {last}")
    live = _live_rows(clip_model, last, seq_rows) or int(clip_model.context_length)
    if live > MAX_LIVE_ROWS:
        raise ValueError(f"{who}: seq_rows gives {live} live token rows per prompt; the backward holds at most {MAX_LIVE_ROWS}")
    return Cn, n_ctx, H, last


def _master_block(params, n_ctx: int, D: int, E: int, H: int, dev) -> torch.Tensor:
    """The five tensors as one contiguous fp32 block on the device (a copy)."""
    layout, total = ops.cocoop_block_layout(n_ctx, D, E, H)
    block = torch.empty(total, dtype=torch.float32, device=dev)
    for k, (off, shape) in layout.items():
        block[off:off + params[k].numel()].copy_(params[k].detach().reshape(-1))
    return block


class _CoCoOpTower(_Tower):
    """``coopfit._Tower`` over CoCoOp's N = B C assembled prompts of one batch size, with the meta-net's kept outputs.  ``sharded``: a
    rank of the class-sharded fit -- ``tokenized_prompts`` and ``n_cls`` are its own classes' (one is enough), ``last_eot`` the whole
    prompt set's."""

    def __init__(self, who, clip_model, tokenized_prompts, n_cls, B, n_ctx, H, last_eot, seq_rows, sharded=False):
        super().__init__(who, clip_model, tokenized_prompts, n_cls * B, n_ctx, False, last_eot, seq_rows)
        dev = clip_model.device
        self.n_cls, self.B, self.H, self.sharded = n_cls, B, H, sharded
        self.N = self.C                       # _Tower sizes workspace, stash, text and d_embed by the number of prompts
        self.cls_eot = self.eot               # of the ids: every image's prompt of a class keeps the class's EOT row
        self.prompts = torch.empty(self.N, self.Lc, self.D, dtype=torch.float32, device=dev)
        self.eot = torch.empty(self.N, dtype=torch.int32, device=dev)
        self.meta = tuple(torch.empty(B, n, dtype=torch.float32, device=dev) for n in (self.E, H, self.D))     # x_n, hid, pi
        self.grad = torch.empty(lib.clipmi_cocoop_block_floats(n_ctx, self.D, self.E, H), dtype=torch.float32, device=dev)

    def forward(self, views: Dict[str, torch.Tensor], features: torch.Tensor) -> torch.Tensor:
        m = self.model
        ops.cocoop_meta(features, *(views[k] for k in NAMES[1:]), out=self.meta)
        if self.sharded:
            ops.cocoop_embed_classes(self.base, views["ctx"], self.meta[2], self.cls_eot, 0, self.n_cls, self.rows, self.prompts, self.eot)
        else:
            ops.cocoop_embed(self.base, views["ctx"], self.meta[2], self.cls_eot, self.rows, self.prompts, self.eot)
        with m._launch_lock:
            check(lib.clipmi_text_encoder_train(m._handle, self.prompts.data_ptr(), _lib.F32, None, 0, 0, self.eot.data_ptr(), self.N, self.rows, None,
                                                self.text.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self.stash.data_ptr(), self.stash.numel(),
                                                _lib.CALL_DEFAULT, ops._stream()), "clipmi_text_encoder_train")
        return self.text

    def reduce(self, d_embed: torch.Tensor, w2: torch.Tensor, grad_scale: float) -> torch.Tensor:
        return ops.cocoop_reduce(d_embed, self.meta[0], self.meta[1], w2, self.n_cls, self.n_ctx, grad_scale, self.grad)

    def one_call_workspace(self, scaled: bool = False) -> torch.Tensor:
        sizer = lib.clipmi_cocoop_train_step_scaled_bytes if scaled else lib.clipmi_cocoop_train_step_bytes
        need = sizer(self.model._handle, self.n_cls, self.rows, self.B, self.H, self.n_ctx)
        if need == 0:
            raise ValueError(f"cocoopfit: {self.N} prompts are more than the tower takes in one call")
        if self.step_ws is None or self.step_ws.numel() < need:
            self.step_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.ws.device)
        return self.step_ws


def stash_bytes(clip_model, tokenized_prompts, batch: int, seq_rows: Optional[int] = None, world: int = 1, rank: int = 0):
    """``(workspace bytes, stash bytes)`` of the training tower of one step on ``batch`` images, as clipmi_text_train_bytes reports them
    for the ``batch x C_r`` prompts of ``rank`` of ``world`` under the live-row cut of the WHOLE prompt set (``world=1``: the unsharded
    ``batch x C``).  The model must be bound to its GPU; nothing is launched."""
    who = "stash_bytes"
    ids = _host_int_array(who, tokenized_prompts, "tokenized_prompts")
    if isinstance(batch, bool) or int(batch) != batch or batch < 1:
        raise ValueError(f"{who}: batch={batch} must be an integer >= 1")
    lo, hi = shard_classes(int(ids.shape[0]), int(world), int(rank))
    rows = _live_rows(clip_model, int(ids.argmax(axis=-1).max()), seq_rows)
    clip_model._ensure_bound()
    wsb, stb = C.c_size_t(0), C.c_size_t(0)
    check(lib.clipmi_text_train_bytes(clip_model._handle, int(batch) * (hi - lo), rows, C.byref(wsb), C.byref(stb)), "clipmi_text_train_bytes")
    return wsb.value, stb.value


def gradients(clip_model, tokenized_prompts, params, features: torch.Tensor, labels, logit_scale: float = 4.6052,
              grad_scale: float = DEFAULT_GRAD_SCALE, seq_rows: Optional[int] = None, return_parts: bool = False, return_operand_stats: bool = False,
              shard: Optional[Shard] = None):
    """``(loss, grads)`` of CoCoOp's training loss (module docstring) on the GPU: loss fp32 [1], grads a dict of the five fp32 gradients
    under the names of ``params`` (the reference's ``state_dict`` names).  ``tokenized_prompts`` [C, context_length]: the ids of
    ``"X .. X name."``; ``features`` fp32 [B, E] raw image features (the rows may be a column slice).  ``return_parts`` adds a dict:
    ``text`` (raw text features fp32 [B C, E]), ``x_n``, ``hid``, ``pi`` and the row losses ``rows``; ``return_operand_stats`` the
    dict ``coopfit.context_gradient`` returns.

    ``shard``: the gradient block the class-sharded step would apply (module docstring), reduced over the ranks in rank order -- the same
    bits on every rank; ``text`` is then the gathered, compacted matrix.  Under a ``LocalGather`` the call runs all ranks.  The operand
    statistics are per rank and are refused."""
    who = "gradients"
    Cn, n_ctx, H, last = _check_prompts(who, clip_model, tokenized_prompts, params, seq_rows)
    if shard is not None:
        sharding.check(who, shard, n_cls=Cn, return_operand_stats=return_operand_stats)
    gs = fitoptim.static_grad_scale(who, grad_scale, "CoCoOpFitState", "fit_prompt_learner")
    scale = fitloop.exp_logit_scale(who, logit_scale)
    E = int(clip_model.geometry.embed_dim)
    labels_d = _check_batch(who, features, labels, Cn, E)
    _need_gpu(features, "features")
    if features.dtype != torch.float32 or features.stride(1) != 1:
        raise TypeError(f"{who}: features must be fp32 with unit column stride")
    if shard is not None:     # the sharded step's phases with a report in the step's place
        make = lambda sh: CoCoOpFitState(clip_model, tokenized_prompts, params, logit_scale, 0.0, 0.0, 0.0, False, gs, seq_rows, shard=sh)
        state = shard_states(make, shard)
        phases = lambda s, r: s._shard_phases(features, labels_d, None, torch.empty(1, dtype=torch.float32, device=features.device), True, r)
        report = sharding.report_all(shard, state, who, phases)
        grads = {k: v.clone() for k, v in ops.cocoop_block_views(report["grad"], n_ctx, state.D, E, H).items()}
        return (report["loss"], grads) + (({k: report[k] for k in ("text", "x_n", "hid", "pi", "rows")},) if return_parts else ())
    tower = _CoCoOpTower(who, clip_model, tokenized_prompts, Cn, features.shape[0], n_ctx, H, last, seq_rows)
    dev = features.device
    views = ops.cocoop_block_views(_master_block(params, n_ctx, tower.D, E, H, dev), n_ctx, tower.D, E, H)
    text = tower.forward(views, features)
    loss, d_text, rows = ops.cocoop_head(features, labels_d, text, scale, gs, want_rows=True)
    stats = torch.zeros(4, dtype=torch.int64, device=dev) if return_operand_stats else None
    d_embed = tower.backward(d_text, stats)
    grads = {k: v.clone() for k, v in ops.cocoop_block_views(tower.reduce(d_embed, views[NAMES[3]], gs), n_ctx, tower.D, E, H).items()}
    out = (loss, grads)
    if return_parts:
        out += ({"text": text.clone(), "x_n": tower.meta[0].clone(), "hid": tower.meta[1].clone(), "pi": tower.meta[2].clone(), "rows": rows},)
    if return_operand_stats:
        out += (operand_stats_dict(stats),)
    return out


class CoCoOpFitState(fitmonitor.Monitored, fitoptim.Optimised):
    """The training state of CoCoOp's prompt learner: the fp32 master block ``[ctx | W1 | b1 | W2 | b2]``, SGD's momentum block, the
    tower's stash (one per batch size seen) and the number of steps taken.  ``step`` enqueues one forward, backward and update and does
    not synchronise.  ``validate`` scores cached validation features through the inference forward (``start_monitor``, ``monitor``,
    ``best_params``, ``val_row_results``: ``fitmonitor.Monitored`` on a ``fitmonitor.ImageMonitor``, whose row results it fills).  The
    loss scale, the optimiser's arguments and moments and ``scaler_state`` are ``fitoptim.Optimised``'s."""
    _who, _history = "CoCoOpFitState", fitmonitor.ImageMonitor

    def __init__(self, clip_model, tokenized_prompts, params, logit_scale: float = 4.6052, momentum: float = 0.9,
                 dampening: float = 0.0, weight_decay: float = 5e-4, nesterov: bool = False, grad_scale: float = DEFAULT_GRAD_SCALE,
                 seq_rows: Optional[int] = None, scaler: Optional[dict] = None, optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8,
                 shard: Optional[Shard] = None):
        """``optimizer``: "sgd" (``momentum``, ``dampening``, ``nesterov``), "adam" or "adamw" (``betas``, ``eps``;
        ``weight_decay`` keeps the fit's default of 5e-4 under all three -- torch's AdamW default of 1e-2 is NOT taken over).
        ``shard``: this state is one rank of the class-sharded fit (module docstring).  It holds the whole master block and runs the
        tower over its own classes; both loss scales and all three optimisers work under it."""
        who = "CoCoOpFitState"
        self.C, self.n_ctx, self.H, self._last = _check_prompts(who, clip_model, tokenized_prompts, params, seq_rows)
        self.shard = shard
        if shard is not None:
            sharding.check(who, shard, n_cls=self.C)
        self._init_optimiser(who, logit_scale, momentum, dampening, nesterov, weight_decay, grad_scale, scaler, optimizer, betas, eps)
        dev = clip_model.device
        if dev.type != "cuda":
            raise RuntimeError(f"clipmi: {who} needs the model on a ROCm GPU (model.to('cuda')); the HIP path has no CPU fallback")
        self.model, self.ids, self.seq_rows = clip_model, tokenized_prompts, seq_rows
        self.D, self.E = int(clip_model.ln_final.weight.shape[0]), int(clip_model.geometry.embed_dim)
        self.block = _master_block(params, self.n_ctx, self.D, self.E, self.H, dev)
        self._init_moments(self.block)
        self._views = ops.cocoop_block_views(self.block, self.n_ctx, self.D, self.E, self.H)
        self._towers: Dict[int, _CoCoOpTower] = {}
        self._val = None            # what a validation keeps between epochs: the inference operands and one workspace per chunk size
        self.val_stream_f16 = True  # trainers.cocoop.CustomCLIP's text_stream_f16: validation runs the tower as that forward does
        self.val_batch_size = None  # validate's chunk when its argument is None (None: the largest training batch seen)
        if shard is not None:       # the tower over the rank's own classes; the live-row cut is the full prompt set's
            self.lo, self.hi = shard_classes(self.C, shard.world, shard.rank)
            self._own_ids = _host_int_array(who, tokenized_prompts, "tokenized_prompts")[self.lo:self.hi]
            sharding.file_state(shard, self)

    # ---- per-epoch validation and best-epoch selection on the device (DESIGN.md "Fit monitor", "CoCoOp and ProDA")

    def _master(self) -> torch.Tensor:
        return self.block

    def _val_operands(self):
        """What the inference forward (``trainers.cocoop.CustomCLIP``) works on, made once: the classes' embeddings [C, context_length, D]
        in the model's type, their EOT rows, the live token rows of the class list and the tower call's flags."""
        if self._val is None:
            m = self.model
            m._ensure_bound()
            ids_h = torch.from_numpy(np.ascontiguousarray(fitloop._host_int_array("CoCoOpFitState.validate", self.ids, "tokenized_prompts"))).long()
            with torch.no_grad():
                base = m.token_embedding(ids_h.to(m.device)).type(m.dtype).contiguous()
            f16 = self.val_stream_f16 and m.get_option("residual_f16") == 2 and m.get_option("ln_fold") == 1
            self._val = {"base": base, "eot": ids_h.argmax(dim=-1).to(torch.int32), "rows": m.live_rows(ids_h),
                         "flags": _lib.CALL_STREAM_F16 if f16 else _lib.CALL_DEFAULT, "chunks": {}}
        return self._val

    def _val_chunk(self, v: dict, B: int):
        """(the classes' EOT rows repeated for ``B`` images, clipmi_cocoop_val_chunk's workspace), one pair per chunk size."""
        if B not in v["chunks"]:
            dev = self.block.device
            need = lib.clipmi_cocoop_val_chunk_bytes(self.model._handle, self.C, v["rows"], B, self.n_ctx)
            if need == 0:
                raise ValueError(f"CoCoOpFitState.validate: {B} x {self.C} prompts are more than the tower takes in one call; pass a smaller val_batch_size")
            v["chunks"][B] = (v["eot"].repeat(B).to(dev), torch.empty(max(need, 256), dtype=torch.uint8, device=dev))
        return v["chunks"][B]

    def validate(self, val_features: torch.Tensor, val_labels, epoch: int, val_batch_size: Optional[int] = None) -> None:
        """Enqueue one validation of the current master block into slot ``epoch`` of the device history; no host read.  It scores what
        ``trainers.cocoop.CustomCLIP.forward`` would compute with these parameters once they are loaded into the module (rounded through the
        model's type, as ``CustomCLIP.fit_prompt_learner`` stores them): ``val_features`` (raw image features fp32 or fp16
        [N_val, E] on the GPU) are L2-normalised once per set; every chunk of ``val_batch_size`` images (None: the state's
        ``val_batch_size`` attribute, else the largest training batch seen, at least 1) goes through clipmi_cocoop_val_chunk -- the meta-net and the context shift, the prompt assembly, the INFERENCE
        text tower over ``val_batch_size x C`` prompts and the fused per-pair tail and row score --, ``ops.val_score_finish`` folds the
        16 N_val bytes of row results into the record, byte for byte ``ops.val_score``'s on the inference logits, and
        ``clipmi_best_select`` keeps the block of the best epoch when the monitor selects.  Neither the [N_val, C] logits nor an
        [N_val, C, E] text matrix exists at any time; the footprint is one chunk's operands.  The record does not depend on
        ``val_batch_size`` as long as the tower's kernel choice, which follows the row count of a call, does not change (include/clipmi.h).
        ``val_labels`` [N_val]: an int64 tensor on the GPU is taken as it is; anything else is range-checked on the host.  The fitted
        parameters, the momentum block, the scaler block and the training stash are not touched.  Without ``start_monitor`` the history
        starts with ``epoch + 1`` slots of 10 bins and no selection."""
        who = "CoCoOpFitState.validate"
        if self.shard is not None:
            raise ValueError(f"{who}: shard has no validation (the sharded fit scores nothing between epochs)")
        mon, m = self._monitor_for(epoch), self.model
        epoch = mon.slot(who, epoch)
        if val_batch_size is None:
            val_batch_size = max(self._towers, default=1) if self.val_batch_size is None else self.val_batch_size
        bs = fitmonitor._batch_size(who, val_batch_size)
        v = self._val_operands()
        img_n, labels_d, _ = mon.val_set(who, val_features, val_labels, self.E, self.C, ops.l2_normalize)
        N, dev = img_n.shape[0], img_n.device
        if mon.n_val and N != mon.n_val and mon.seen:
            raise ValueError(f"{who}: the validation set has {N} rows, the history's earlier epochs {mon.n_val}")
        rows = mon.room(N, N, dev)
        # what the module would hold after ``fit_prompt_learner`` copied the masters into it: the block rounded through the model's type
        # (index-level plumbing on a few ten thousand values, once per validation; the fp32 masters themselves are what is selected)
        block = self.block if m.dtype == torch.float32 else self.block.to(m.dtype).to(torch.float32)
        for lo in range(0, N, bs):
            B = min(bs, N - lo)
            eot, ws = self._val_chunk(v, B)
            pr = ops._row_results(who, rows, B, lo)
            with m._launch_lock:
                check(lib.clipmi_cocoop_val_chunk(m._handle, v["base"].data_ptr(), _DT[v["base"].dtype], block.data_ptr(), self.n_ctx, self.H,
                                                  eot.data_ptr(), self.C, v["rows"], img_n[lo:lo + B].data_ptr(), B, self.scale,
                                                  labels_d[lo:lo + B].data_ptr(), mon.bins, pr, v["flags"], ws.data_ptr(), ws.numel(), ops._stream()),
                      "clipmi_cocoop_val_chunk")
        mon.n_val = N
        need = lib.clipmi_val_score_finish_workspace_bytes(N, mon.bins)
        if mon.finish_ws is None or mon.finish_ws.numel() < need:
            mon.finish_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        ops.val_score_finish(rows[:N], mon.bins, mon.records[epoch], mon.finish_ws)
        mon.select(epoch, self.block)

    def best_params(self) -> Dict[str, torch.Tensor]:
        """The best slot on the device as the five tensors (views of one block): the parameters of the best epoch so far, or those
        ``start_monitor`` saw while no epoch has been taken."""
        return collections.OrderedDict(ops.cocoop_block_views(self._best_block("best_params"), self.n_ctx, self.D, self.E, self.H))

    def params(self) -> Dict[str, torch.Tensor]:
        """The five tensors as views of the master block (fp32, on the device), under the reference's ``state_dict`` names."""
        return collections.OrderedDict(self._views)

    def tower(self, B: int) -> _CoCoOpTower:
        if B not in self._towers and self.shard is None:
            self._towers[B] = _CoCoOpTower("CoCoOpFitState.step", self.model, self.ids, self.C, B, self.n_ctx, self.H, self._last, self.seq_rows)
        elif B not in self._towers:
            self._towers[B] = self._shard_tower(B)
        return self._towers[B]

    # ---- the class-sharded step (csrc/cocoop_train.hip, DESIGN.md "Class-sharded CoCoOp fit")

    def _shard_tower(self, B: int) -> _CoCoOpTower:
        """The rank's tower for batches of ``B`` with the send and receive blocks of the step's two gathers, made once per batch size.
        The tower writes its text features straight into the first rows of the padded send block; the padding is moved and never read."""
        G, Cr = self.shard.world, self.hi - self.lo
        t = _CoCoOpTower("CoCoOpFitState.step", self.model, self._own_ids, Cr, B, self.n_ctx, self.H, self._last, self.seq_rows, sharded=True)
        f32 = dict(dtype=torch.float32, device=self.block.device)
        rows = B * ops.cocoop_shard_pad(self.C, G)
        t.send_text = torch.empty(rows, t.E, **f32)
        t.text = t.send_text[:t.N]
        t.all_text = torch.empty(G, rows * t.E, **f32)
        t.full_text = torch.empty(B * self.C, t.E, **f32)
        t.own_d_text = torch.empty(t.N, t.E, **f32)
        t.send_part = torch.empty(B, t.n_ctx, t.D, **f32)
        t.all_part = torch.empty(G, B * t.n_ctx * t.D, **f32)
        return t

    def _shard_phases(self, features, labels_d, lr_d, loss, first: bool, report: Optional[dict] = None):
        """One sharded step as phases, a ``yield`` behind every gather.  ``report``: a dict that receives the reduced gradient block,
        the loss and the parts ``gradients`` returns INSTEAD of a step: no block of the state is touched."""
        B, sh, st = int(features.shape[0]), self.shard, ops._stream()
        t, gs = self.tower(B), self._head_scale
        t.forward(self._views, features)                                   # the meta-net over all B rows, then the rank's own B C_r prompts
        sh.gather(t.send_text, t.all_text, t.send_text.numel() * 4, st)
        yield
        text = ops.cocoop_shard_compact(t.all_text, B, self.C, t.E, t.full_text)
        head = ops.cocoop_head(features, labels_d, text, self.scale, gs, loss, want_rows=report is not None)
        own = ops.cocoop_shard_rows(head[1], B, self.lo, self.hi, t.own_d_text)   # the rank's own rows of the replicated d_text
        self._scale_rows(own)
        ops.cocoop_dcs_partial(t.backward(own), B, t.n_cls, t.n_ctx, t.send_part)
        sh.gather(t.send_part, t.all_part, t.send_part.numel() * 4, st)
        yield
        grad = ops.cocoop_reduce_gathered(t.all_part, t.meta[0], t.meta[1], self._views[NAMES[3]], t.n_ctx, gs, t.grad)
        if report is not None:
            report.update(grad=grad.clone(), loss=loss, text=text.clone(), x_n=t.meta[0].clone(), hid=t.meta[1].clone(), pi=t.meta[2].clone(),
                          rows=head[2])
            return
        self._apply_block(grad, lr_d, lambda: self._static_step(grad, lr_d, first))

    def _static_step(self, grad: torch.Tensor, lr_d: torch.Tensor, first: bool) -> None:
        ops.cocoop_step(grad, self.block, self.buf, lr_d, self.n_ctx, self.D, self.E, self.H, first, *self._sgd)

    def step(self, features: torch.Tensor, labels, lr, want_loss: bool = False, one_call: bool = False) -> Optional[torch.Tensor]:
        """One optimiser step on the batch ``features`` fp32 [B, E] and ``labels`` [B] at the rate ``lr``, as ``CoOpFitState.step`` takes
        them (a device scalar is read where it lies; a label tensor on the GPU is taken as it is -- a label outside [0, C) then makes
        the parameters NaN, it is never used as an address).  ``one_call``: the same launches through clipmi_cocoop_train_step.
        Returns the batch loss, fp32 [1] on the device, when ``want_loss``.  Under ``grad_scale="dynamic"`` the head and the reduce run at
        ``grad_scale = 1``, ``d_text`` is multiplied by the device block's scale in between and clipmi_block_step_scaled decides on the
        device whether the step is applied (one call: clipmi_cocoop_train_step_scaled); a skipped step still counts in ``steps`` and still
        returns its loss; whether it was applied is in ``scaler_state()``.  Under ``optimizer="adam" | "adamw"`` the reduce leaves the
        block's gradient as ``gradients`` returns it and clipmi_block_step_adam applies it (clipmi_block_step_adam_scaled under the dynamic
        scale); ``one_call`` is then refused: the one-call steps stay SGD.  Under ``shard`` every rank makes this call with the same
        batch; under a ``LocalGather`` the first state that steps drives all the world's states (``one_call`` is refused)."""
        who = "CoCoOpFitState.step"
        if self.shard is not None:
            sharding.check(who, self.shard, one_call=one_call)
        self._no_one_call_adam(who, one_call)
        states = sharding.drive(self.shard, self, who) if self.shard is not None else None
        labels_d = _check_batch(who, features, labels, self.C, self.E)
        _need_gpu(features, "features")
        if features.dtype != torch.float32 or features.stride(1) != 1:
            raise TypeError(f"{who}: features must be fp32 with unit column stride")
        dev = features.device
        lr_d = ops._dev(fitloop.lr_operand(lr, dev), "lr", (torch.float32,))
        first = self.steps == 0
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        if states is not None:
            sharding.step_all(states, self, lambda s: s._shard_phases(features, labels_d, lr_d, loss if s is self else torch.empty_like(loss), first))
            self.steps += 1
            return loss if want_loss else None
        t, m, sc = self.tower(int(features.shape[0])), self.model, self._scaler
        if one_call:        # one of two symbols (static or scaled) on one run of arguments
            ws = t.one_call_workspace(scaled=self.dynamic)
            name = "clipmi_cocoop_train_step" + ("_scaled" if self.dynamic else "")
            front = (m._handle, C.byref(t.dgrad[0]), t.base.data_ptr(), _DT[t.base.dtype], self.block.data_ptr(),
                     None if self.buf is None else self.buf.data_ptr(), t.n_ctx, t.H, t.cls_eot.data_ptr(), t.n_cls, t.rows, features.data_ptr(),
                     features.stride(0), labels_d.data_ptr(), features.shape[0], self.scale)
            how = (sc.block.data_ptr(), *sc.args(), lr_d.data_ptr()) if self.dynamic else (self.grad_scale, lr_d.data_ptr(), int(first))
            with m._launch_lock:
                check(getattr(lib, name)(*front, *how, *self._sgd, loss.data_ptr(), None, ws.data_ptr(), ws.numel(), t.stash.data_ptr(), t.stash.numel(),
                                         ops._stream()), name)
        else:
            gs = self._head_scale
            text = t.forward(self._views, features)
            _, d_text = ops.cocoop_head(features, labels_d, text, self.scale, gs, loss)
            self._scale_rows(d_text)
            grad = t.reduce(t.backward(d_text), self._views[NAMES[3]], gs)
            self._apply_block(grad, lr_d, lambda: self._static_step(grad, lr_d, first))
        self.steps += 1
        return loss if want_loss else None


def init_params(clip_model, n_ctx: int = 4, ctx_init_ids: Optional[torch.Tensor] = None, seed: int = 0) -> Dict[str, torch.Tensor]:
    """The reference's initialisation (cocoop.py:82-108) as fp32 tensors on the host: ``ctx`` from N(0, 0.02^2) [n_ctx, D], or, with
    ``ctx_init_ids`` (the ids of e.g. "a photo of a", [1, context_length]), the embeddings of its words; ``meta_net`` as ``nn.Linear``
    initialises Linear(E, E // 16) and Linear(E // 16, D) under ``seed``."""
    D, E = int(clip_model.ln_final.weight.shape[0]), int(clip_model.geometry.embed_dim)
    g = torch.Generator().manual_seed(seed)
    if ctx_init_ids is not None:
        ids = torch.as_tensor(ctx_init_ids).reshape(1, -1)
        n = int(ids[0].argmax()) - 1
        if n < 1:
            raise ValueError("init_params: ctx_init_ids holds no word between SOS and EOT")
        with torch.no_grad():
            ctx = clip_model.token_embedding(ids.to(clip_model.device))[0, 1:1 + n].detach().float().cpu().clone()
    else:
        ctx = 0.02 * torch.randn(int(n_ctx), D, generator=g)
    H = max(E // 16, 1)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        l1, l2 = torch.nn.Linear(E, H), torch.nn.Linear(H, D)
    return collections.OrderedDict(zip(NAMES, (ctx, l1.weight.detach().clone(), l1.bias.detach().clone(), l2.weight.detach().clone(),
                                               l2.bias.detach().clone())))


def fit_prompt_learner(features: torch.Tensor, labels, clip_model, tokenized_prompts, params=None, n_ctx: int = 4, logit_scale: float = 4.6052,
                       lr: float = 0.002, epochs: int = 10, batch_size: int = 1, momentum: float = 0.9,
                       dampening: float = 0.0, weight_decay: float = 5e-4, nesterov: bool = False, grad_scale: float = DEFAULT_GRAD_SCALE, seq_rows: Optional[int] = None,
                       lr_per_epoch: Optional[Sequence[float]] = None, order=None, drop_last: bool = False, return_history: bool = False,
                       scaler: Optional[dict] = None, val=None, val_batch_size: Optional[int] = None, val_bins: int = 10,
                       final_model: str = "last_step", val_criterion: str = "accuracy", return_monitor: bool = False, val_stream_f16: bool = True, optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8,
                       shard: Optional[Shard] = None):
    """Train CoCoOp's prompt learner on cached ``features`` fp32 [N, E] and ``labels`` [N], starting from ``params`` (a dict of the five
    tensors, not modified; None = ``init_params(clip_model, n_ctx)``).  The loop and its arguments are ``coopfit.fit_context``'s:
    ``epochs`` passes of ``torch.optim.SGD`` over batches of ``batch_size``, ``lr_per_epoch`` (None: ``cosine_warmup_schedule``),
    ``order`` [epochs, N], ``drop_last``; everything is checked on the host before the first launch and nothing synchronises until the
    one wait at the end.  Returns the fitted fp32 tensors on the device as a dict (views of one block), or ``(dict, per-step batch
    losses)`` with ``return_history``.  The defaults are unverified restatements of the reference's config (module docstring).
    ``grad_scale="dynamic"`` with ``scaler`` (module docstring): a step that overflows fp16 is skipped on the device and the scale adapts;
    the history keeps one loss per step, skipped steps included, and the run still synchronises once.

    ``val=(val_features, val_labels)`` (raw image features [N_val, E] on the GPU and their labels): behind the last step of every epoch
    ``CoCoOpFitState.validate`` scores the parameters against them on the device as the inference forward would, in chunks of
    ``val_batch_size`` images (None: ``batch_size``; a validation costs N_val x C prompts through the text tower), into ``val_bins``
    confidence bins -- the fitted tensors are bit for bit those of the same call without ``val``, and the run still synchronises once.
    ``final_model``, ``val_criterion`` and ``return_monitor`` as ``coopfit.fit_context`` takes them: "best_val" returns the five tensors of
    the epoch that was strictly better than every earlier one (the starting values when no epoch was taken) and is refused without
    ``val``; ``return_monitor`` adds ``CoCoOpFitState.monitor()``'s dict behind the history.  ``val_stream_f16``: the validation's tower
    call asks for the fp16 residual stream where the model allows it, as ``trainers.cocoop.CustomCLIP(text_stream_f16=True)`` does.

    ``optimizer``, ``betas``, ``eps``: "sgd" (the default; ``momentum``, ``dampening``, ``nesterov``), "adam" or
    "adamw", as ``coopfit.fit_context`` takes them; ``weight_decay`` keeps this fit's default of 5e-4 under all three (torch's AdamW
    default of 1e-2 is NOT taken over).  DESIGN.md "Adam steps for the prompt fits".

    ``shard=Shard(world, rank, gather)``: the class-sharded fit (module docstring).  Every rank makes this call with the same arguments
    -- the whole prompt set, all features -- and returns the same tensors.  With a ``LocalGather`` the one call runs all ``world`` shard
    states in this process.  Both loss scales and all three optimisers work; validation and ``final_model="best_val"`` are refused."""
    who = "fit_prompt_learner"
    fitmonitor.check_args(who, val, val_bins, final_model, val_criterion)
    if val is not None and val_batch_size is not None:
        fitmonitor._batch_size(who, val_batch_size)
    if params is None:
        params = init_params(clip_model, n_ctx)
    Cn, n_ctx, H, _ = _check_prompts(who, clip_model, tokenized_prompts, params, seq_rows)
    if shard is not None:
        sharding.check(who, shard, n_cls=Cn, val=val, final_model=final_model)
    E, D = int(clip_model.geometry.embed_dim), int(clip_model.ln_final.weight.shape[0])
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] < 1 or features.shape[1] != E:
        raise ValueError(f"{who}: features must be a [N >= 1, E = {E}] tensor")
    N = features.shape[0]
    epochs, batch_size = fitloop.check_run(who, epochs, batch_size)
    fitoptim.check_fit(who, optimizer, momentum, dampening, nesterov, weight_decay, betas, eps, grad_scale, scaler)
    lab = fitloop._labels(who, labels, N, Cn)
    order = fitloop.check_order(who, order, epochs, N)
    per_epoch = steps_per_epoch(N, batch_size, drop_last)
    dev = features.device
    _, lr_steps = fitloop.schedule(who, lr, epochs, lr_per_epoch, per_epoch, dev)
    if val is not None:
        vf, vl = fitmonitor.check_val(who, val, E, Cn)
    if epochs * per_epoch == 0:
        out = collections.OrderedDict((k, params[k].detach().to(torch.float32).clone().to(dev if features.is_cuda else "cpu")) for k in NAMES)
        return fitmonitor.pack(out, np.zeros(0, np.float32), fitmonitor.empty_monitor(val_bins), return_history, return_monitor)
    _need_gpu(features, "features")
    make = lambda sh: CoCoOpFitState(clip_model, tokenized_prompts, params, logit_scale, momentum, dampening, weight_decay, nesterov, grad_scale, seq_rows,
                                     scaler, optimizer, betas, eps, shard=sh)
    state = shard_states(make, shard)     # under a LocalGather all the world's states live here; a step of one steps them all
    end_epoch = None
    if val is not None:
        _need_gpu(vf, "val_features")
        vl = vl.to(vf.device)
        state.val_stream_f16 = bool(val_stream_f16)
        state.start_monitor(epochs, val_bins, select=final_model == "best_val", val_criterion=val_criterion)
        end_epoch = lambda e: state.validate(vf, vl, e, batch_size if val_batch_size is None else val_batch_size)
    history = fitloop.run_cached(lambda f, y, r, want: state.step(f, y, r, want_loss=want), features, fitloop.labels_on(labels, lab, dev),
                                 fitloop.order_on(order, np.int64, dev), batch_size, per_epoch, epochs, lr_steps, return_history, end_epoch)
    out = state.best_params() if final_model == "best_val" else state.params()
    return fitmonitor.pack(out, history, fitmonitor.returned_monitor(state, val is not None, val_bins, return_monitor), return_history, return_monitor)
