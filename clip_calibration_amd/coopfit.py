"""CoOp's context vectors trained on the GPU (reference trainers/classification/coop.py:70-144, 192-222, 282-309), and KgCoOp's and
ProGrad's on the same forward and backward (kgcoop.py:246-269, prograd.py:291-304, 371-409).

The reference trains one tensor, the prompt learner's ``ctx`` ([n_ctx, D], or [C, n_ctx, D] with class-specific contexts), with Dassl's
epoch loop: every step builds the prompts ``[SOS | ctx | class tokens, EOS, padding]``, runs the frozen text tower on them and the frozen
image tower on the batch, normalises both sides, takes ``F.cross_entropy`` of ``exp(logit_scale)`` times the cosine and one
``torch.optim.SGD`` step on ``ctx``.  ``ctx`` reaches the loss only through the text tower, so a step needs the gradient of the text
features with respect to the tower's input embeddings.  csrc/text_backward.hip computes it with the tower frozen: a training forward that
keeps what the backward needs in a stash and the backward (every Linear's backward is the forward's fp16 GEMM on a transposed copy of
the weight, packed once per bound model); csrc/prompt_train.hip has the loss head and the context's gradient with the optimiser's rule
-- no autograd graph.  fp16 GEMM
operands, fp32 accumulation, fp32 residual and gradient streams, an fp32 master copy of ``ctx``.  DESIGN.md "CoOp fit" has the data flow.

``grad_scale``: fp16 operands flush small gradients, so the whole backward carries ``grad_scale`` times the gradient (a power of two: the
scaling itself is exact); the loss head multiplies and the context step divides.  The default, 2^12, comes from the measurement in
profiles/coopfit_parity.txt (ViT-B/16 text geometry); a model with much larger gradients needs a smaller one -- or
``grad_scale="dynamic"``, the reference's ``prec == "amp"`` branch (coop.py:286-291, ``torch.cuda.amp.GradScaler``) for CoOp and KgCoOp:
the scale lives in a small block on the device, a step whose context gradient holds an inf or a NaN is skipped (neither the context nor the
momentum buffer changes, and the buffer starts on the first step that is applied), the scale is multiplied by ``backoff_factor`` after a
skipped step and by ``growth_factor`` after ``growth_interval`` clean steps in a row.  ``scaler`` is a dict of ``init_scale``,
``growth_factor``, ``backoff_factor`` and ``growth_interval`` (torch's defaults: 2^16, 2, 0.5, 2000; the scale and both factors powers
of two, so the scaling stays exact).  No step reads anything back; ``CoOpFitState.scaler_state()`` does, once.  With a scale that never
changes the dynamic path gives the static path's bits.  DESIGN.md "Dynamic loss scale".

Three ways in.  ``context_gradient`` returns one batch's loss and gradient (the diagnostic entry point of the tests).  ``fit_context``
trains from a cached [N, E] matrix of image features and enqueues every step of every epoch with one synchronisation at the end: that
equals the reference's loop only when the train transform is deterministic.  ``CoOpFitState.step`` takes one batch of features at a time,
for callers that run the image tower on every step (``CustomCLIP.fit_context(loader, transform=TrainPreprocess(...))``).

Dassl is not part of this repository's environment.  The defaults below -- SGD at 0.002 with momentum 0.9 and weight decay 5e-4, no
dampening, no Nesterov; 200 epochs in batches of 32; a constant warm-up epoch at 1e-5 that hands over to a cosine schedule; 16 context
vectors drawn from N(0, 0.02^2) -- restate configs/trainers/CoOp/vit_b16_c16_ep200_batch32.yaml and Dassl's public defaults and are
UNVERIFIED here; that is why each of them is an argument.  Dassl's random sampler is the caller's ``order``.

``method``: "coop" (the default, everything above), "kgcoop" or "prograd"; the latter two need ``teacher``, the frozen zero-shot text
features fp32 [C, E] on the device (the head normalises the rows).  KgCoOp adds ``w (1 - mean_c cos(u_c, teacher_c))`` to the loss
(``w`` = 8.0, the reference's TRAINER.KGCOOP.W) and costs what CoOp costs.  ProGrad takes two losses of one forward -- the
cross-entropy and ``T^2`` times the cross-entropy of ``softmax(z / T)`` against ``softmax(z_teacher / T)`` --, runs the backward once
for each (one after the other: they share the tower's workspace), and applies the cross-entropy's gradient ``a`` with its component
along the other one, ``b``, taken out when they conflict: ``a - lam (a.b / b.b) b`` if ``a.b < 0``, else ``a``; then the same SGD step.
``T`` = 1.0 and ``lam`` = 1.0 are what every shipped config sets.  DESIGN.md "KgCoOp / ProGrad fit" has the formulas and the
rounding points.  Unverified, besides Dassl's defaults above: the reference's ``amp`` branch of ProGrad (prograd.py:415-424) hands
``GradScaler.scale`` a tuple and is not mirrored.

``class_token_position``: "end" (the default and every shipped config's), "middle" or "front", the reference's
TRAINER.{COOP,KGCOOP,PROGRAD}.CLASS_TOKEN_POSITION (coop.py:128-192), for all three methods, generic and class-specific contexts, and both
loss scales that a method has.  "end" is the route described above, untouched.  For the other two csrc/prompt_position.hip assembles
the prompts in one launch in front of the tower (``ops.prompt_place``; the tower then takes them as they are) and one copy launch behind
the backward gathers the rows that hold the context into the [C, 1 + n_ctx, D] layout the existing steps read (``ops.prompt_unplace``), so
the class sums, the SGD rule, the scaler's rule and ProGrad's projection are the same code.  ``name_lens``: every class's name length in
tokens; None derives ``eot - n_ctx - 2``, the reference's layout ``[SOT, X * n_ctx, name, '.', EOT]``.

Validation: ``fit_context(val=(val_features, val_labels), final_model="last_step" | "best_val", val_criterion=, return_monitor=)``
scores the context behind every epoch on the device (``CoOpFitState.validate``, csrc/fit_monitor.hip) and keeps the context of the
strictly best epoch in a device slot, the reference's TEST.FINAL_MODEL (base_learner.py:41-47), with no read-back before the run's one
wait.  DESIGN.md "Fit monitor".

``shard=Shard(world, rank, gather)`` on ``CoOpFitState``, ``fit_context`` and ``context_gradient``: the class-sharded fit, this project's
form of the reference's ``nn.DataParallel`` around the text encoder (coop.py:266-272); ``shard.py`` has ``Shard``, ``LocalGather`` and the
protocol every sharded fit follows.  Rank r owns the contiguous classes of the balanced split and runs the tower's forward and backward
over its own prompts only; the raw text features are gathered and compacted (csrc/shard_train.hip), the loss head runs replicated on every
rank, and the context's gradient is the ranks' partial class sums gathered and added in rank order, so every rank ends a step with the
same bits.  A class-specific context keeps its own rows per rank (``gathered_context()``).  With ``world == 1`` the bits are the unsharded
path's.  Refused under ``shard``, each by name (``shard.check``): C < world, a class-token position other than "end",
``grad_scale="dynamic"``, ``val=`` / ``final_model="best_val"``, ``one_call=True``.  DESIGN.md "Class-sharded CoOp fit".

``optimizer``: "sgd" (the default: everything above, the same launches and bits), "adam" or "adamw" with ``betas`` and ``eps``, the
reference's OPTIM.NAME, for all three methods.  The context's gradient is formed by the step entry without being applied and
clipmi_block_step_adam (csrc/optim_step.hip) applies ``torch.optim.Adam``'s or ``torch.optim.AdamW``'s rule to the master context;
``fitoptim._AdamBlock`` keeps the moments and the bias-correction table beside it.  DESIGN.md "Adam steps for the prompt fits".

The loss scale's argument rules, the scaler's device block, Adam's moments and the mix-in every fit state takes them through
(``fitoptim.Optimised``) live in ``fitoptim.py``, for this fit and the five others; this module re-exports ``DYNAMIC`` from there and
keeps ``DEFAULT_GRAD_SCALE``.  DESIGN.md "Fit optimiser: shared plumbing".

Not covered: ``nn.DataParallel`` itself in one process (``shard=`` stands in for it, with the refusals above), ProGrad under a dynamic loss
scale, and models whose text tower carries deep prompts.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, fitloop, fitmonitor, fitoptim, ops
from . import shard as sharding      # under its own name: ``shard`` is every entry point's argument
from ._lib import _DT, check, lib
from .fitloop import _host_int_array, _need_gpu, steps_per_epoch
from .shard import LocalGather, Shard, shard_classes, shard_states

# 2^12, measured on the ViT-B/16 text geometry with synthetic weights (profiles/coopfit_parity.txt, "grad_scale"): the smallest of 2^0, 2^4,
# 2^8, 2^12, 2^16 that leaves under 1 % of the fp16 dgrad-GEMM operand elements subnormal (0.76 %; 6.8 % at 2^8, 52 % at 2^0) with at least
# 2^4 of headroom below fp16's largest value (2^5.9; 2^1.9 at 2^16).  A model whose gradients are much larger than that model's overflows
# fp16 at this scale -- the context then turns NaN, it does not go wrong silently; pass a smaller power of two, or grad_scale="dynamic".
DEFAULT_GRAD_SCALE = 4096.0


DYNAMIC = fitoptim.DYNAMIC     # re-exported: the value of ``grad_scale`` that asks for the dynamic loss scale (``fitoptim``)


def _static_prograd(who: str, method: str, grad_scale) -> None:
    """ProGrad has no dynamic loss scale: its two gradients share one step."""
    if method == "prograd" and fitoptim._is_dynamic(who, grad_scale):
        raise ValueError(f"{who}: grad_scale={DYNAMIC!r} covers method 'coop' and 'kgcoop'; ProGrad keeps a static scale")


def _check_prompts(who: str, clip_model, tokenized_prompts, ctx) -> Tuple[int, int, bool, int]:
    """(C, n_ctx, per_class, last EOT position) after the host-side checks of the prompt set against the model and the context."""
    L, D = int(clip_model.context_length), int(clip_model.ln_final.weight.shape[0])
    if getattr(clip_model, "ivlp_text_prompts", None) is not None and clip_model.ivlp_text_prompts()[0]:
        raise ValueError(f"{who}: the model's text tower carries deep prompts; the training forward does not support them")
    ids = _host_int_array(who, tokenized_prompts, "tokenized_prompts")
    if ids.ndim != 2 or ids.shape[1] != L or ids.shape[0] < 2:
        raise ValueError(f"{who}: tokenized_prompts {ids.shape} must be [C >= 2, {L}]")
    if not isinstance(ctx, torch.Tensor) or ctx.dim() not in (2, 3) or ctx.shape[-1] != D or not ctx.dtype.is_floating_point:
        raise ValueError(f"{who}: ctx {tuple(getattr(ctx, 'shape', ()))} must be [n_ctx, {D}] or [C, n_ctx, {D}]")
    per_class = ctx.dim() == 3
    if per_class and ctx.shape[0] != ids.shape[0]:
        raise ValueError(f"{who}: a class-specific ctx {tuple(ctx.shape)} needs one context per prompt ({ids.shape[0]})")
    n_ctx = int(ctx.shape[-2])
    eot = ids.argmax(axis=1)
    if n_ctx < 1 or not 1 + n_ctx < L or int(eot.min()) <= n_ctx:
        raise ValueError(f"{who}: n_ctx={n_ctx} does not fit the prompts (context of {L} tokens, first EOT at {int(eot.min())}): the layout is "
                         "[SOS | ctx | class tokens, EOS]")
    return ids.shape[0], n_ctx, per_class, int(eot.max())


def _check_batch(who: str, features, labels, C: int, E: int) -> torch.Tensor:
    """The batch's labels on the features' device after the checks of both (``fitloop.step_labels``)."""
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] < 1 or features.shape[1] != E:
        raise ValueError(f"{who}: features {tuple(getattr(features, 'shape', ()))} must be [B >= 1, E = {E}]")
    return fitloop.step_labels(who, labels, features.shape[0], C, features.device)


POSITIONS = ("end", "middle", "front")


def _placement(who: str, tokenized_prompts, n_ctx: int, class_token_position, name_lens):
    """The host-side checks of the class-token position and the name lengths: None for "end" (today's route: nothing is placed), else
    ``(position code, name lengths as an int32 array [C])``.  ``name_lens=None`` derives ``eot - n_ctx - 2``; an explicit sequence must
    have one entry per class with ``0 <= nl`` and ``1 + n_ctx + nl <= eot[c]``, so that the name stays in front of the EOT row."""
    if not isinstance(class_token_position, str) or class_token_position not in POSITIONS:
        raise ValueError(f"{who}: class_token_position={class_token_position!r} must be one of {POSITIONS}")
    eot = _host_int_array(who, tokenized_prompts, "tokenized_prompts").argmax(axis=1)
    if name_lens is None:
        lens = np.maximum(eot - n_ctx - 2, 0)
    else:
        lens = np.asarray(name_lens.detach().cpu() if isinstance(name_lens, torch.Tensor) else name_lens)
        if lens.ndim != 1 or lens.shape[0] != eot.shape[0] or lens.dtype.kind not in "iu":
            raise ValueError(f"{who}: name_lens must be a sequence of {eot.shape[0]} integers (one per class)")
        bad = np.nonzero((lens < 0) | (1 + n_ctx + lens.astype(np.int64) > eot))[0]
        if bad.size:
            c = int(bad[0])
            raise ValueError(f"{who}: name_lens[{c}]={int(lens[c])} outside [0, {int(eot[c]) - 1 - n_ctx}]: the name of class {c} has to end in front of "
                             f"its EOT on row {int(eot[c])}")
    if class_token_position == "end":
        return None
    return ops.PROMPT_POSITIONS[class_token_position], np.ascontiguousarray(lens, dtype=np.int32)


MAX_LIVE_ROWS = 80     # token rows per prompt that clipmi_text_encoder_backward takes (include/clipmi.h; the attention backward's limit)


def _live_rows(clip_model, last_eot: int, seq_rows: Optional[int]) -> int:
    """The ``seq_rows`` handed to the library (0: the whole context) for a prompt set whose last EOT sits on row ``last_eot``: None cuts
    behind it, rounded up to a multiple of 8, unless the model runs every row; a number is taken as it is when it cuts anything."""
    Lc = int(clip_model.context_length)
    if seq_rows is None:
        rows = min(Lc, (last_eot + 1 + 7) // 8 * 8) if clip_model.text_dead_row_elimination else Lc
    else:
        rows = int(seq_rows)
    return rows if 0 < rows < Lc else 0


METHODS = ("coop", "kgcoop", "prograd")


def _check_method(who: str, method: str, teacher, w: float, T: float, lam: float, C: int, E: int) -> None:
    """The host-side checks of the method's own arguments; nothing is launched before they pass."""
    if method not in METHODS:
        raise ValueError(f"{who}: method={method!r} must be one of {METHODS}")
    if method == "coop":
        return
    if not isinstance(teacher, torch.Tensor) or teacher.dtype != torch.float32 or tuple(teacher.shape) != (C, E):
        raise ValueError(f"{who}: method={method!r} needs teacher, the frozen text features fp32 [C, E] = [{C}, {E}], got "
                         f"{tuple(teacher.shape) if isinstance(teacher, torch.Tensor) else type(teacher).__name__}"
                         f"{' ' + str(teacher.dtype) if isinstance(teacher, torch.Tensor) else ''}")
    if not (math.isfinite(w) and w >= 0.0):
        raise ValueError(f"{who}: w={w} (finite, >= 0)")
    if not (math.isfinite(T) and T > 0.0):
        raise ValueError(f"{who}: T={T} (finite, > 0)")
    if not math.isfinite(lam):
        raise ValueError(f"{who}: lam={lam} (finite)")


def _pack_dgrad(model, blocks, projection: torch.Tensor, struct, slot: str):
    """The transposed fp16 copies of a frozen tower's weights (``struct``: clipmi_text_dgrad or clipmi_vision_dgrad, ``projection`` as it
    lies), packed once per bound model and again when a weight's version moves; the model keeps them under ``slot``."""
    per_block = [(b.attn.in_proj_weight, b.attn.out_proj.weight, b.mlp.c_fc.weight, b.mlp.c_proj.weight) for b in blocks]
    key = (id(model._bound),) + tuple((w.data_ptr(), w._version) for w in [projection] + [w for ws in per_block for w in ws])
    hit = model.__dict__.get(slot)
    if hit is not None and hit[0] == key:
        return hit[1]
    keep = [w.detach().to(torch.float16).t().contiguous() for ws in per_block for w in ws]
    arr = (_lib.BlockDgrad * len(per_block))(*[_lib.BlockDgrad(*[t.data_ptr() for t in keep[4 * i:4 * i + 4]]) for i in range(len(per_block))])
    keep.append(projection.detach().to(torch.float16).contiguous())
    packed = (struct(keep[-1].data_ptr(), arr), arr, keep)
    model.__dict__[slot] = (key, packed)
    return packed


def _dgrad(model):
    """The transposed fp16 copies of the frozen text weights (clipmi_text_dgrad), packed once per bound model and again when a text
    weight's version moves."""
    model._ensure_bound()
    return _pack_dgrad(model, model.transformer.resblocks, model.text_projection, _lib.TextDgrad, "_coop_dgrad")


class _Tower:
    """The frozen text tower in training mode for one prompt set: base embeddings, EOT indices, workspace, stash and the gradient stream."""

    def __init__(self, who: str, clip_model, tokenized_prompts, n_cls: int, n_ctx: int, per_class: bool, last_eot: int, seq_rows: Optional[int],
                 placement=None):
        dev = clip_model.device
        if dev.type != "cuda":
            raise RuntimeError(f"clipmi: {who} needs the model on a ROCm GPU (model.to('cuda')); the HIP path has no CPU fallback")
        if dev.index != torch.cuda.current_device():
            raise RuntimeError(f"clipmi: the model is on {dev} but the current device is cuda:{torch.cuda.current_device()}")
        self.model, self.C, self.n_ctx, self.per_class = clip_model, n_cls, n_ctx, per_class
        g = clip_model.geometry
        self.Lc, self.D, self.E = g.context_length, g.transformer_width, g.embed_dim
        ids = torch.as_tensor(tokenized_prompts).to(dev)
        with torch.no_grad():
            self.base = clip_model.token_embedding(ids).type(clip_model.dtype).contiguous()   # [C, Lc, D]; rows 1 .. n_ctx are placeholders
        if self.base.dtype not in _DT:
            raise TypeError(f"{who}: the model's dtype {self.base.dtype} is not fp16 or fp32")
        self.eot = ids.argmax(dim=-1).to(torch.int32).contiguous()
        if seq_rows is not None and int(seq_rows) and int(seq_rows) <= last_eot:
            raise ValueError(f"{who}: seq_rows={int(seq_rows)} cuts the EOT row {last_eot}")
        self.rows = _live_rows(clip_model, last_eot, seq_rows)
        self.L = self.rows or self.Lc
        clip_model._ensure_bound()
        self.dgrad = _dgrad(clip_model)
        wsb, stb = C.c_size_t(0), C.c_size_t(0)
        check(lib.clipmi_text_train_bytes(clip_model._handle, self.C, self.rows, C.byref(wsb), C.byref(stb)), "clipmi_text_train_bytes")
        self.stash_bytes = stb.value
        self.ws = torch.empty(max(wsb.value, 256), dtype=torch.uint8, device=dev)
        self.stash = torch.empty(max(stb.value, 256), dtype=torch.uint8, device=dev)
        self.text = torch.empty(self.C, self.E, dtype=torch.float32, device=dev)
        self.d_embed = torch.empty(self.C * self.L, self.D, dtype=torch.float32, device=dev)
        self.d_embed_kl = None    # ProGrad's second gradient stream, made on first use
        self.step_ws = None
        # a class-token position other than "end" (_placement): the placed prompts and the compact gradient streams [C (1 + n_ctx), D]
        self.position = None
        if placement is not None:
            self.position = placement[0]
            self.name_lens = torch.from_numpy(placement[1]).to(dev)
            self.prompts = torch.empty(self.C, self.Lc, self.D, dtype=torch.float32, device=dev)
            self.compact = torch.empty(self.C * (1 + n_ctx), self.D, dtype=torch.float32, device=dev)
            self.compact_kl = None

    def forward(self, ctx: torch.Tensor) -> torch.Tensor:
        m = self.model
        if self.position is None:
            src = (self.base.data_ptr(), _DT[self.base.dtype], ctx.data_ptr(), self.n_ctx, int(self.per_class))
        else:   # the context already lies on its rows of the fp32 prompts: the tower splices nothing
            ops.prompt_place(self.base, ctx, self.position, self.name_lens, self.rows, self.prompts)
            src = (self.prompts.data_ptr(), _lib.F32, None, 0, 0)
        with m._launch_lock:
            check(lib.clipmi_text_encoder_train(m._handle, *src, self.eot.data_ptr(), self.C, self.rows, None, self.text.data_ptr(), self.ws.data_ptr(),
                                                self.ws.numel(), self.stash.data_ptr(), self.stash.numel(), _lib.CALL_DEFAULT, ops._stream()),
                  "clipmi_text_encoder_train")
        return self.text

    def context_rows(self, d_embed: torch.Tensor, second: bool = False) -> torch.Tensor:
        """What the context steps read: ``d_embed`` itself at "end", else its rows that hold the context, gathered into [C (1 + n_ctx), D]."""
        if self.position is None:
            return d_embed
        if second and self.compact_kl is None:
            self.compact_kl = torch.empty_like(self.compact)
        return ops.prompt_unplace(d_embed, self.position, self.name_lens, self.n_ctx, self.compact_kl if second else self.compact)

    def backward(self, d_text: torch.Tensor, stats: Optional[torch.Tensor] = None, second: bool = False) -> torch.Tensor:
        """``second``: into ProGrad's second stream.  The stash is only read, the workspace is reused: the calls run one after the other."""
        m = self.model
        if second and self.d_embed_kl is None:
            self.d_embed_kl = torch.empty_like(self.d_embed)
        out = self.d_embed_kl if second else self.d_embed
        with m._launch_lock:
            check(lib.clipmi_text_encoder_backward(m._handle, C.byref(self.dgrad[0]), d_text.data_ptr(), self.C, self.rows, out.data_ptr(),
                                                   self.ws.data_ptr(), self.ws.numel(), self.stash.data_ptr(), self.stash.numel(),
                                                   None if stats is None else stats.data_ptr(), ops._stream()), "clipmi_text_encoder_backward")
        return out

    def one_call_workspace(self, B: int, method: str = "coop", scaled: bool = False) -> torch.Tensor:
        if self.position is None:
            sizer = lib.clipmi_prompt_train_step_scaled_bytes if scaled else lib.clipmi_prompt_train_step_bytes
        else:
            sizer = lib.clipmi_prompt_train_step_scaled_placed_bytes if scaled else lib.clipmi_prompt_train_step_placed_bytes
        need = sizer(self.model._handle, self.C, self.rows, B, ops.PROMPT_MODES[method], self.n_ctx, int(self.per_class))
        if self.step_ws is None or self.step_ws.numel() < need:
            self.step_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.ws.device)
        return self.step_ws


def operand_stats_dict(stats: torch.Tensor) -> dict:
    """The four words a backward's ``operand_stats`` leaves (include/clipmi.h) as ``elements``, ``zeros``, ``subnormals`` and ``max``, the
    largest magnitude decoded from its fp16 bits.  One read-back."""
    s = stats.cpu().numpy()
    top = float(np.array([int(s[3])], dtype=np.uint16).view(np.float16)[0])
    return {"elements": int(s[0]), "zeros": int(s[1]), "subnormals": int(s[2]), "max": top}


def _new_losses(method: str, dev) -> torch.Tensor:
    """The head's losses fp32 [3].  CoOp's head writes the first alone and nothing here reads the others: no fill launch for it."""
    return (torch.empty if method == "coop" else torch.zeros)(3, dtype=torch.float32, device=dev)


def context_gradient(clip_model, tokenized_prompts, ctx: torch.Tensor, features: torch.Tensor, labels, logit_scale: float = 4.6052,
                     grad_scale: float = DEFAULT_GRAD_SCALE, seq_rows: Optional[int] = None, return_operand_stats: bool = False,
                     method: str = "coop", teacher: Optional[torch.Tensor] = None, w: float = 8.0, T: float = 1.0, lam: float = 1.0,
                     return_parts: bool = False, class_token_position: str = "end", name_lens=None, shard: Optional[Shard] = None):
    """``(loss, grad)`` of ``F.cross_entropy(exp(logit_scale) * normalise(features) @ normalise(text_encoder(prompts(ctx))).T, labels)``
    with respect to ``ctx`` ([n_ctx, D] generic or [C, n_ctx, D] class-specific), on the GPU: loss fp32 [1], grad fp32 of ctx's shape.
    ``features`` fp32 [B, E] raw image features (the rows may be a column slice), ``tokenized_prompts`` [C, context_length] the ids of
    ``"X .. X name."``.  ``seq_rows``: the live token rows per prompt (None: behind the last EOT, rounded up to a multiple of 8; 0: the
    whole context).  ``return_operand_stats`` adds a dict over every fp16 dgrad-GEMM operand element: ``elements``, ``zeros``,
    ``subnormals``, ``max`` -- the measurement behind the default ``grad_scale``.

    ``method`` "kgcoop": the loss is the total ``CE + w score`` and the gradient its gradient; "prograd": the loss is ``xe`` and the
    gradient the one ProGrad applies (module docstring; ``teacher``, ``w``, ``T``, ``lam``).  ``return_parts`` adds a dict (before the
    operand statistics): KgCoOp ``ce``, ``score`` (fp32 [1] each); ProGrad ``xe``, ``kl``, ``grad_xe``, ``grad_kl``, ``projected``
    (int32 [1]) and ``dots`` (float64 [3]: a.a, b.b, a.b of a = grad_xe, b = grad_kl); CoOp an empty one.
    ``class_token_position``, ``name_lens``: the prompts' layout (module docstring).

    ``shard``: the gradient the class-sharded step would apply (module docstring), reduced over the ranks in rank order -- the same
    bits on every rank, of the whole context's shape also for a class-specific one.  ProGrad's parts are then ``xe``, ``kl``,
    ``projected`` and ``dots``; the operand statistics are per rank and are not returned."""
    who = "context_gradient"
    Cn, n_ctx, per_class, last = _check_prompts(who, clip_model, tokenized_prompts, ctx)
    if shard is not None:
        sharding.check(who, shard, "coop", n_cls=Cn, class_token_position=class_token_position, grad_scale=grad_scale,
                       return_operand_stats=return_operand_stats)
        return _sharded_gradient(clip_model, tokenized_prompts, ctx, features, labels, logit_scale, grad_scale, seq_rows, method, teacher, w, T, lam,
                                 return_parts, shard)
    placement = _placement(who, tokenized_prompts, n_ctx, class_token_position, name_lens)
    gs = fitoptim.static_grad_scale(who, grad_scale, "CoOpFitState", "fit_context")
    scale = fitloop.exp_logit_scale(who, logit_scale)
    E = int(clip_model.geometry.embed_dim)
    _check_method(who, method, teacher, w, T, lam, Cn, E)
    labels_d = _check_batch(who, features, labels, Cn, E)
    _need_gpu(features, "features")
    if method != "coop":
        _need_gpu(teacher, "teacher")
    tower = _Tower(who, clip_model, tokenized_prompts, Cn, n_ctx, per_class, last, seq_rows, placement)
    dev = features.device
    master = fitloop.master(ctx, dev)
    text = tower.forward(master)
    stats = torch.zeros(4, dtype=torch.int64, device=dev) if return_operand_stats else None
    losses, d_text, d_kl = ops.prompt_head(features, labels_d, text, scale, gs, method, teacher, w, T, _new_losses(method, dev))
    loss = losses[0:1]
    d_embed = tower.context_rows(tower.backward(d_text, stats))
    if method != "prograd":
        grad = ops.ctx_step(d_embed, Cn, n_ctx, per_class, gs)
        parts = {"ce": losses[1:2], "score": losses[2:3]} if method == "kgcoop" else {}
    else:
        d_embed_kl = tower.context_rows(tower.backward(d_kl, stats, second=True), second=True)
        grad, projected, dots = ops.prograd_step(d_embed, d_embed_kl, Cn, n_ctx, per_class, gs, lam)
        parts = {"xe": losses[0:1], "kl": losses[1:2], "projected": projected, "dots": dots}
        if return_parts:
            parts["grad_xe"] = ops.ctx_step(d_embed, Cn, n_ctx, per_class, gs)
            parts["grad_kl"] = ops.ctx_step(d_embed_kl, Cn, n_ctx, per_class, gs)
    out = (loss, grad) + ((parts,) if return_parts else ())
    if not return_operand_stats:
        return out
    return out + (operand_stats_dict(stats),)


def _sharded_gradient(clip_model, tokenized_prompts, ctx, features, labels, logit_scale, grad_scale, seq_rows, method, teacher, w, T, lam, return_parts,
                      shard: Shard):
    """``context_gradient`` under ``shard``: the sharded step's phases with a report in the step's place."""
    make = lambda sh: CoOpFitState(clip_model, tokenized_prompts, ctx, logit_scale, 0.0, 0.0, False, 0.0, grad_scale, seq_rows, method, teacher, w, T, lam,
                                   shard=sh)
    state = shard_states(make, shard)
    labels_d = _check_batch("context_gradient", features, labels, state.C, state.tower.E)
    _need_gpu(features, "features")

    def phases(s, report):
        report["losses"] = _new_losses(method, features.device)
        return s._shard_phases(features, labels_d, None, report["losses"], True, report)
    report = sharding.report_all(shard, state, "context_gradient", phases)
    loss3, parts = report["losses"], {}
    if method == "kgcoop":
        parts = {"ce": loss3[1:2], "score": loss3[2:3]}
    elif method == "prograd":
        parts = {"xe": loss3[0:1], "kl": loss3[1:2], "projected": report["projected"], "dots": report["dots"]}
    return (loss3[0:1], report["grad"]) + ((parts,) if return_parts else ())


def text_features(clip_model, tokenized_prompts, ctx: torch.Tensor, seq_rows: Optional[int] = None, class_token_position: str = "end",
                  name_lens=None) -> torch.Tensor:
    """The raw text features fp32 [C, E] of the training forward at ``ctx``: what the loss head is given."""
    who = "text_features"
    Cn, n_ctx, per_class, last = _check_prompts(who, clip_model, tokenized_prompts, ctx)
    placement = _placement(who, tokenized_prompts, n_ctx, class_token_position, name_lens)
    tower = _Tower(who, clip_model, tokenized_prompts, Cn, n_ctx, per_class, last, seq_rows, placement)
    return tower.forward(fitloop.master(ctx, clip_model.device)).clone()


class CoOpFitState(fitmonitor.Monitored, fitoptim.Optimised):
    """The training state of CoOp's context: the fp32 master ``ctx``, SGD's momentum buffer, the tower's stash and the number of steps
    taken.  ``step`` enqueues one forward, backward and update and does not synchronise.  ``validate`` scores cached validation features
    on the device (``start_monitor``, ``monitor``, ``best_context``, ``val_logits``: ``fitmonitor.Monitored`` on a ``fitmonitor.Monitor``).
    The loss scale, the optimiser's arguments and moments and ``scaler_state`` are ``fitoptim.Optimised``'s."""
    _who, _unseen_summary = "CoOpFitState", True

    def __init__(self, clip_model, tokenized_prompts, ctx: torch.Tensor, logit_scale: float = 4.6052, momentum: float = 0.9,
                 dampening: float = 0.0, nesterov: bool = False, weight_decay: float = 5e-4,
                 grad_scale: float = DEFAULT_GRAD_SCALE, seq_rows: Optional[int] = None, method: str = "coop", teacher: Optional[torch.Tensor] = None,
                 w: float = 8.0, T: float = 1.0, lam: float = 1.0, scaler: Optional[dict] = None, class_token_position: str = "end", name_lens=None,
                 shard: Optional[Shard] = None, optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8):
        """``optimizer``: "sgd" (``momentum``, ``dampening``, ``nesterov``), "adam" or "adamw" (``betas``, ``eps``;
        ``weight_decay`` keeps the fit's default of 5e-4 under all three -- torch's AdamW default of 1e-2 is NOT taken over)."""
        who = "CoOpFitState"
        self.C, self.n_ctx, self.per_class, last = _check_prompts(who, clip_model, tokenized_prompts, ctx)
        self.shard = shard
        if shard is not None:
            sharding.check(who, shard, "coop", n_cls=self.C, class_token_position=class_token_position, grad_scale=grad_scale)
        placement = _placement(who, tokenized_prompts, self.n_ctx, class_token_position, name_lens)
        _static_prograd(who, method, grad_scale)
        self._init_optimiser(who, logit_scale, momentum, dampening, nesterov, weight_decay, grad_scale, scaler, optimizer, betas, eps, sgd_shard=shard)
        _check_method(who, method, teacher, w, T, lam, self.C, int(clip_model.geometry.embed_dim))
        self.method, self.w, self.T, self.lam = method, float(w), float(T), float(lam)
        self.teacher = None
        if method != "coop":
            _need_gpu(teacher, "teacher")
            self.teacher = teacher.detach().contiguous()
        dev = clip_model.device
        if shard is None:
            self.tower = _Tower(who, clip_model, tokenized_prompts, self.C, self.n_ctx, self.per_class, last, seq_rows, placement)
            self.ctx = fitloop.master(ctx, dev)
        else:   # the tower over the rank's own prompts (the live-row cut is the full prompt set's), a class-specific context's own rows
            self.lo, self.hi = shard_classes(self.C, shard.world, shard.rank)
            ids = _host_int_array(who, tokenized_prompts, "tokenized_prompts")[self.lo:self.hi]
            self.tower = _Tower(who, clip_model, ids, self.hi - self.lo, self.n_ctx, self.per_class, last, seq_rows)
            self.ctx = fitloop.master(ctx[self.lo:self.hi] if self.per_class else ctx, dev)
            self._shard_buffers(dev)
        self._init_moments(self.ctx)

    # ---- the class-sharded step (csrc/shard_train.hip, DESIGN.md "Class-sharded CoOp fit")

    def _shard_buffers(self, dev) -> None:
        """The send and receive blocks of the step's two gathers, made once.  The tower writes its text features straight into the
        first rows of the padded send block."""
        sh, t = self.shard, self.tower
        G, P = sh.world, -(-self.C // sh.world)
        f32 = dict(dtype=torch.float32, device=dev)
        self._send_text = torch.empty(P, t.E, **f32)
        t.text = self._send_text[:t.C]
        self._all_text = torch.empty(G, P, t.E, **f32)
        self._text = torch.empty(self.C, t.E, **f32)
        prograd = self.method == "prograd"
        if not self.per_class:      # the partial gradient(s): ProGrad's two travel in one gather
            k = 2 if prograd else 1
            self._send_part = torch.empty(k, t.n_ctx, t.D, **f32)
            self._all_part = torch.empty(G, k, t.n_ctx, t.D, **f32)
        if prograd:                 # class-specific: every rank's dots travel; generic: the reduced vectors' dots are every rank's own
            n = G if self.per_class else 1
            self._send_dots = torch.empty(3, dtype=torch.float64, device=dev) if self.per_class else None
            self._all_dots = torch.empty(n, 3, dtype=torch.float64, device=dev)
            self._prograd_ws = ops.shard_prograd_workspace(self.ctx.numel(), dev)
        self._rows = None           # gathered_context's blocks, made on first use
        sharding.file_state(sh, self)

    def _gather_rows(self, own: torch.Tensor):
        """A phase: the ranks' own rows of a class-specific [C_r, n_ctx, D] block gathered into the full [C, n_ctx, D]; the result is
        left in ``self._rows[2]``."""
        t, sh = self.tower, self.shard
        if self._rows is None:
            P, n = self._send_text.shape[0], t.n_ctx * t.D
            f32 = dict(dtype=torch.float32, device=own.device)
            self._rows = (torch.empty(P, n, **f32), torch.empty(sh.world, P, n, **f32), torch.empty(self.C, t.n_ctx, t.D, **f32))
        send, recv, full = self._rows
        send[:t.C].copy_(own.view(t.C, -1))
        sh.gather(send, recv, send.numel() * 4, ops._stream())
        yield
        ops.shard_compact(recv, self.C, full)

    def _shard_phases(self, features, labels_d, lr_d, losses, first: bool, report: Optional[dict] = None):
        """One sharded step as phases, a ``yield`` behind every gather.  ``report``: a dict that receives the reduced gradient (and
        ProGrad's decision) INSTEAD of a step: neither the context nor the momentum buffer is touched."""
        t, sh, st = self.tower, self.shard, ops._stream()
        step = report is None
        ctx, buf, lr_d = (self.ctx, self.buf, lr_d) if step else (None, None, None)
        sgd = self._sgd
        prograd = self.method == "prograd"
        t.forward(self.ctx)                                                                  # the rank's own prompts
        sh.gather(self._send_text, self._all_text, self._send_text.numel() * 4, st)
        yield
        text = ops.shard_compact(self._all_text, self.C, self._text)
        _, d_text, d_kl = ops.prompt_head(features, labels_d, text, self.scale, self.grad_scale, self.method, self.teacher, self.w, self.T, losses)
        d_embed = t.backward(d_text[self.lo:self.hi])                                        # the rank's own rows of the replicated d_text
        d_embed_kl = t.backward(d_kl[self.lo:self.hi], second=True) if prograd else None
        out = None
        if not self.per_class:
            ops.ctx_partial(d_embed, t.C, t.n_ctx, self._send_part[0])
            if prograd:
                ops.ctx_partial(d_embed_kl, t.C, t.n_ctx, self._send_part[1])
            sh.gather(self._send_part, self._all_part, self._send_part.numel() * 4, st)
            yield
            if not prograd:
                out = ops.ctx_step_gathered(self._all_part.view(sh.world, -1), t.n_ctx, t.D, self.grad_scale, ctx, buf, lr_d, first, *sgd, want_grad=not step)
            else:
                ops.shard_prograd_dots(self._all_part[:, 0], self._all_part[:, 1], 1, t.n_ctx, False, self.grad_scale, self._prograd_ws, self._all_dots[0])
        elif not prograd:           # every rank steps its own classes' rows with the unsharded rule: nothing is reduced
            out = ops.ctx_step(d_embed, t.C, t.n_ctx, True, self.grad_scale, ctx, buf, lr_d, first, *sgd, want_grad=not step)
        else:
            ops.shard_prograd_dots(d_embed, d_embed_kl, t.C, t.n_ctx, True, self.grad_scale, self._prograd_ws, self._send_dots)
            sh.gather(self._send_dots, self._all_dots, 24, st)
            yield
        if prograd:
            out = ops.shard_prograd_apply(self._all_dots, self.lam, self._prograd_ws, self.ctx.shape, ctx, buf, lr_d, first, *sgd, want_report=not step)
        if step:
            return
        grad = out[0] if prograd else out
        if prograd:
            report["projected"], report["dots"] = out[1], out[2]
        if self.per_class:
            yield from self._gather_rows(grad)
            grad = self._rows[2].clone()
        report["grad"] = grad

    def gathered_context(self) -> torch.Tensor:
        """The whole context on the device: ``ctx`` itself for a generic context (every rank holds the same bits) and without ``shard``;
        for a class-specific context under ``shard`` the ranks' rows gathered into a fresh [C, n_ctx, D] -- one all-gather that every
        rank enters (under a local gather this call runs it for all of them)."""
        if self.shard is None or not self.per_class:
            return self.ctx
        sharding.run_all(self.shard, self, "CoOpFitState.gathered_context", lambda s: s._gather_rows(s.ctx))
        return self._rows[2].clone()

    # ---- per-epoch validation and best-epoch selection on the device (csrc/fit_monitor.hip, DESIGN.md "Fit monitor")

    def _master(self) -> torch.Tensor:
        return self.ctx

    def validate(self, val_features: torch.Tensor, val_labels, epoch: int) -> None:
        """Enqueue one validation of the current master context into slot ``epoch`` of the device history; no host read.

        The state's own training forward runs on the context (same prompts, placement and live-row cut: the text features the next step
        would see; the stash it overwrites is rewritten by that step), the text features and ``val_features`` (raw image features fp32 or
        fp16 [N_val, E] on the GPU) are L2-normalised in fp32 and ``clipmi_logits`` forms ``exp(logit_scale)`` times their cosines, fp32
        [N_val, C], in a workspace the state owns (4 N_val C bytes, plus 4 N_val E for the normalised features, both kept for the next
        epoch); ``clipmi_val_score`` scores them into the record and, when the monitor selects, ``clipmi_best_select`` compares the record
        with the best block and copies the context into the best slot.  ``val_labels`` [N_val]: an int64 tensor on the GPU is taken as it
        is (a label outside [0, C) then counts as wrong with a NaN nll), anything else is range-checked on the host, once per set.
        Without ``start_monitor`` the history starts with ``epoch + 1`` slots of 10 bins and no selection; it grows when ``epoch``
        lies behind its end."""
        who = "CoOpFitState.validate"
        if self.shard is not None:
            raise ValueError(f"{who}: shard has no validation (the first version of the sharded fit scores nothing between epochs)")
        mon, t = self._monitor_for(epoch), self.tower
        epoch = mon.slot(who, epoch)
        img_n, labels_d = mon.operands(who, val_features, val_labels, t.E, self.C, ops.l2_normalize)
        txt_n = ops.l2_normalize(t.forward(self.ctx))
        check(lib.clipmi_logits(img_n.data_ptr(), txt_n.data_ptr(), self.scale, None, mon.logits.data_ptr(), None, None, img_n.shape[0], t.C, t.E,
                                ops._stream()), "clipmi_logits")
        mon.score(epoch, labels_d, self.ctx)

    def best_context(self) -> torch.Tensor:
        """The best slot on the device: the context of the best epoch so far, or the context ``start_monitor`` saw while no epoch has
        been taken.  No read-back."""
        return self._best_block("best_context")

    def _one_call(self, features, labels_d, lr_d, losses, first: bool) -> None:
        """``step`` through the library's one-call step: one of four symbols (static or scaled, the class token at the end or placed) on
        one run of arguments, each with its own tail."""
        t, m, sc = self.tower, self.tower.model, self._scaler
        ws = t.one_call_workspace(features.shape[0], self.method, scaled=self.dynamic)
        name = "clipmi_prompt_train_step" + ("_scaled" if self.dynamic else "") + ("" if t.position is None else "_placed")
        buf, teacher = (None if x is None else x.data_ptr() for x in (self.buf, self.teacher))
        head = (m._handle, C.byref(t.dgrad[0]), t.base.data_ptr(), _DT[t.base.dtype], self.ctx.data_ptr(), buf, t.n_ctx, int(t.per_class),
                *(() if t.position is None else (t.position, t.name_lens.data_ptr())), t.eot.data_ptr(), t.C, t.rows, features.data_ptr(),
                features.stride(0), labels_d.data_ptr(), features.shape[0], self.scale)
        sgd = self._sgd
        tail = (ws.data_ptr(), ws.numel(), t.stash.data_ptr(), t.stash.numel(), ops._stream())
        mode = ops.PROMPT_MODES[self.method]
        if self.dynamic:
            mid = (sc.block.data_ptr(), *sc.args(), mode, teacher, self.w, lr_d.data_ptr(), *sgd, losses.data_ptr(), None)
        else:
            mid = (self.grad_scale, mode, teacher, self.w, self.T, self.lam, lr_d.data_ptr(), int(first), *sgd, losses.data_ptr(), None, None, None)
        with m._launch_lock:
            check(getattr(lib, name)(*head, *mid, *tail), name)

    def _apply_scaled(self, d_embed: torch.Tensor, lr_d: torch.Tensor) -> None:
        """SGD under the dynamic scale is CoOp's own kernel, not the block's: clipmi_ctx_step_scaled is handed the tower's input gradient,
        forms the class sums itself and decides on the device whether the step is applied."""
        t, sc = self.tower, self._scaler
        if sc.ws is None:
            need = lib.clipmi_ctx_step_scaled_workspace_bytes(t.C, t.D, t.n_ctx, int(t.per_class))
            sc.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.ctx.device)
        ops.ctx_step_scaled(d_embed, t.C, t.n_ctx, t.per_class, sc.block, self.ctx, self.buf, lr_d, *sc.args(), *self._sgd, want_grad=False, workspace=sc.ws)

    def _separate_calls(self, features, labels_d, lr_d, losses, first: bool) -> None:
        """``step`` launch by launch: the forward, the head at the head's scale, under the dynamic scale its d_text times the block's
        scale, the backward(s), and the step.  Static SGD: the step entry (ProGrad's with its projection) forms the gradient and applies
        it.  Dynamic SGD: ``_apply_scaled``.  Adam or AdamW: the same entry forms the gradient WITHOUT applying it (``context_gradient``'s
        way; ProGrad's is the projected one; under the dynamic scale at ``grad_scale = 1``, since clipmi_ctx_step_scaled's own first
        launch cannot be reached without its step) and ``_AdamBlock.step`` applies the rule -- clipmi_block_step_adam_scaled divides by
        the scale, as that launch does.  ``T`` is 1 under the dynamic scale, where ProGrad is refused anyway."""
        t, gs, prograd = self.tower, self._head_scale, self.method == "prograd"
        text = t.forward(self.ctx)
        _, d_text, d_kl = ops.prompt_head(features, labels_d, text, self.scale, gs, self.method, self.teacher, self.w, 1.0 if self.dynamic else self.T, losses)
        self._scale_rows(d_text)
        d_embed = t.context_rows(t.backward(d_text))
        d_embed_kl = t.context_rows(t.backward(d_kl, second=True), second=True) if prograd else None
        grad = d_embed
        if self._adam is not None and prograd:
            grad = ops.prograd_step(d_embed, d_embed_kl, t.C, t.n_ctx, t.per_class, gs, self.lam)[0]
        elif self._adam is not None:
            grad = ops.ctx_step(d_embed, t.C, t.n_ctx, t.per_class, gs)

        def static_step():
            if prograd:
                ops.prograd_step(d_embed, d_embed_kl, t.C, t.n_ctx, t.per_class, gs, self.lam, self.ctx, self.buf, lr_d, first, *self._sgd, want_report=False)
            else:
                ops.ctx_step(d_embed, t.C, t.n_ctx, t.per_class, gs, self.ctx, self.buf, lr_d, first, *self._sgd, want_grad=False)
        self._apply_block(grad, lr_d, static_step)

    def step(self, features: torch.Tensor, labels, lr, want_loss: bool = False, one_call: bool = False) -> Optional[torch.Tensor]:
        """One optimiser step on the batch ``features`` fp32 [B, E] (raw image features on the GPU) and ``labels`` [B] at the rate ``lr``:
        an fp32 tensor of one element on the device is read where it lies (``rates[k:k + 1]``); a Python number is uploaded on every call.
        A label tensor on the GPU is taken as it is -- a label outside [0, C) then makes the context NaN, it is never used as an address;
        host labels are range-checked.  ``one_call``: the same launches through the library's one-call step
        (clipmi_prompt_train_step; clipmi_prompt_train_step_scaled under the dynamic scale).  Returns the batch loss, fp32 [1] on the
        device, when ``want_loss``: the total for KgCoOp, ``xe`` for ProGrad.  Under the dynamic scale a skipped step still counts in
        ``steps`` and still returns its loss; whether it was applied is in ``scaler_state()``."""
        labels_d = _check_batch("CoOpFitState.step", features, labels, self.C, self.tower.E)
        _need_gpu(features, "features")
        if features.dtype != torch.float32 or features.stride(1) != 1:
            raise TypeError("CoOpFitState.step: features must be fp32 with unit column stride")
        dev = features.device
        lr_d = ops._dev(fitloop.lr_operand(lr, dev), "lr", (torch.float32,))
        first = self.steps == 0
        losses = _new_losses(self.method, dev)
        if self.shard is not None:
            # every rank is given the same batch; under a local gather this call steps all the world's states, one phase at a time
            sharding.check("CoOpFitState.step", self.shard, "coop", one_call=one_call)
            sharding.step_all(sharding.drive(self.shard, self, "CoOpFitState.step"), self,
                              lambda s: s._shard_phases(features, labels_d, lr_d, losses if s is self else _new_losses(s.method, dev), first))
        else:
            self._no_one_call_adam("CoOpFitState.step", one_call)
            (self._one_call if one_call else self._separate_calls)(features, labels_d, lr_d, losses, first)
        self.steps += 1
        return losses[0:1] if want_loss else None


FINAL_MODELS, empty_monitor = fitmonitor.FINAL_MODELS, fitmonitor.empty_monitor    # shared with the other monitored fits


def init_context(clip_model, n_ctx: int = 16, n_cls: Optional[int] = None, seed: int = 0) -> torch.Tensor:
    """The reference's random initialisation (coop.py:92-99): N(0, 0.02^2), [n_ctx, D] or, with ``n_cls``, class-specific [n_cls, n_ctx, D]."""
    D = int(clip_model.ln_final.weight.shape[0])
    g = torch.Generator().manual_seed(seed)
    shape = (n_ctx, D) if n_cls is None else (n_cls, n_ctx, D)
    return 0.02 * torch.randn(*shape, generator=g)


def fit_context(features: torch.Tensor, labels, clip_model, tokenized_prompts, ctx: Optional[torch.Tensor] = None, n_ctx: int = 16,
                csc: bool = False, logit_scale: float = 4.6052, lr: float = 0.002, epochs: int = 200, batch_size: int = 32,
                momentum: float = 0.9, dampening: float = 0.0, weight_decay: float = 5e-4, nesterov: bool = False,
                grad_scale: float = DEFAULT_GRAD_SCALE, seq_rows: Optional[int] = None, lr_per_epoch: Optional[Sequence[float]] = None,
                order=None, drop_last: bool = False, return_history: bool = False, method: str = "coop", teacher: Optional[torch.Tensor] = None,
                w: float = 8.0, T: float = 1.0, lam: float = 1.0, scaler: Optional[dict] = None, class_token_position: str = "end", name_lens=None,
                val=None, val_bins: int = 10, final_model: str = "last_step", val_criterion: str = "accuracy", return_monitor: bool = False,
                shard: Optional[Shard] = None, optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8):
    """Train CoOp's context on cached ``features`` fp32 [N, E] (raw image features on the GPU; the rows may be a column slice) and
    ``labels`` [N], starting from ``ctx`` (not modified; None = ``init_context(clip_model, n_ctx, C if csc else None)``): ``epochs``
    passes of ``torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov)`` over batches of ``batch_size``.

    ``lr_per_epoch`` gives every epoch's rate; None takes ``cosine_warmup_schedule(lr, epochs)``.  ``order`` is an integer [epochs, N]
    array of sample indices, batch k of epoch e being ``order[e, k * batch_size : (k + 1) * batch_size]``; None is 0 .. N-1 in every
    epoch.  The last batch of an epoch is short unless ``drop_last`` drops it.  Labels and ``order`` are checked on the host before
    anything is launched; from the first launch on nothing synchronises until the one wait at the end.  Returns the fitted fp32 context
    on the device, or ``(ctx, per-step batch losses as a float32 numpy array)`` with ``return_history``.  The defaults are unverified
    restatements of the reference's config and Dassl's (module docstring).  ``method``, ``teacher``, ``w``, ``T``, ``lam``: KgCoOp's
    or ProGrad's step in CoOp's place (module docstring); the history then holds KgCoOp's total loss or ProGrad's ``xe``.
    ``grad_scale="dynamic"`` with ``scaler`` (module docstring; CoOp and KgCoOp): a step that overflows fp16 is skipped on the device and
    the scale adapts; the history keeps one loss per step, skipped steps included, and the run still synchronises once.
    ``class_token_position``, ``name_lens``: the prompts' layout (module docstring); checked, like everything else, before the first launch.

    ``val=(val_features, val_labels)`` (raw image features [N_val, E] on the GPU and their labels): behind the last step of every epoch
    ``CoOpFitState.validate`` scores the context against them on the device, into ``val_bins`` confidence bins -- the fitted context is bit
    for bit the one of the same call without ``val``, and the run still synchronises once.  ``final_model``: "last_step" returns the last
    epoch's context; "best_val" (the reference's TEST.FINAL_MODEL, base_learner.py:41-47) the context of the epoch that was strictly
    better than every earlier one under ``val_criterion`` -- "accuracy" (Dassl's rule) or "nll", where an epoch with a non-finite nll is
    never taken; the starting context when no epoch was taken.  "best_val" without ``val`` is refused.  ``return_monitor`` adds a dict
    behind everything else, read once after the run's one wait: per-epoch ``accuracy``, ``nll`` and ``ece``, the raw ``bins``,
    ``records`` and ``best_epoch`` (``CoOpFitState.monitor``); empty without ``val`` or without steps.

    ``optimizer``: "sgd" (the default: ``momentum``, ``dampening``, ``nesterov`` -- the launches and bits of the
    fit without this argument), "adam" or "adamw": ``torch.optim.Adam`` / ``torch.optim.AdamW`` (no amsgrad) with ``betas`` and ``eps`` on
    the same forward, head and backward; the context's gradient is formed without being applied and clipmi_block_step_adam applies it
    (clipmi_block_step_adam_scaled under ``grad_scale="dynamic"``, where a skipped step leaves the context and both moments as they are
    and is not one of Adam's steps; ProGrad keeps its static scale).  ``weight_decay`` keeps this fit's default of 5e-4 under all three:
    torch's AdamW default of 1e-2 is NOT taken over.  Refused by name before any device call: an unknown optimiser, a ``momentum``,
    ``dampening`` or ``nesterov`` other than the signature's default together with an Adam optimiser, and ``shard`` with one.  DESIGN.md "Adam steps for the prompt fits".

    ``shard=Shard(world, rank, gather)``: the class-sharded fit (module docstring).  Every rank makes this call with the same arguments
    -- the whole prompt set, the whole context, all features -- and returns the same whole context; with a ``LocalGather`` the one call
    runs all ``world`` shard states in this process."""
    who = "fit_context"
    fitmonitor.check_args(who, val, val_bins, final_model, val_criterion)
    ids = _host_int_array(who, tokenized_prompts, "tokenized_prompts")
    if ctx is None:
        ctx = init_context(clip_model, n_ctx, ids.shape[0] if csc else None)
    Cn, n_ctx, per_class, _ = _check_prompts(who, clip_model, tokenized_prompts, ctx)
    if shard is not None:
        sharding.check(who, shard, "coop", n_cls=Cn, class_token_position=class_token_position, grad_scale=grad_scale, val=val, final_model=final_model)
    E = int(clip_model.geometry.embed_dim)
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] < 1 or features.shape[1] != E:
        raise ValueError(f"{who}: features must be a [N >= 1, E = {E}] tensor")
    N = features.shape[0]
    epochs, batch_size = fitloop.check_run(who, epochs, batch_size)
    fitoptim.check_fit(who, optimizer, momentum, dampening, nesterov, weight_decay, betas, eps, grad_scale, scaler, shard=shard,
                       between=lambda: _static_prograd(who, method, grad_scale))
    _check_method(who, method, teacher, w, T, lam, Cn, E)
    _placement(who, tokenized_prompts, n_ctx, class_token_position, name_lens)
    lab = fitloop._labels(who, labels, N, Cn)
    order = fitloop.check_order(who, order, epochs, N)
    per_epoch = steps_per_epoch(N, batch_size, drop_last)
    dev = features.device
    _, lr_steps = fitloop.schedule(who, lr, epochs, lr_per_epoch, per_epoch, dev)
    if val is not None:
        vf, vl = fitmonitor.check_val(who, val, E, Cn)
    if epochs * per_epoch == 0:
        out = ctx.detach().to(torch.float32).clone()
        out = out.to(dev) if features.is_cuda else out
        return fitmonitor.pack(out, np.zeros(0, np.float32), empty_monitor(val_bins), return_history, return_monitor)
    _need_gpu(features, "features")
    make = lambda sh: CoOpFitState(clip_model, tokenized_prompts, ctx, logit_scale, momentum, dampening, nesterov, weight_decay, grad_scale, seq_rows,
                                   method, teacher, w, T, lam, scaler, class_token_position, name_lens, sh, optimizer, betas, eps)
    state = shard_states(make, shard)     # under a LocalGather all the world's states live here; a step of one steps them all
    end_epoch = None
    if val is not None:
        _need_gpu(vf, "val_features")
        vl = vl.to(dev)
        state.start_monitor(epochs, val_bins, select=final_model == "best_val", val_criterion=val_criterion)
        end_epoch = lambda e: state.validate(vf, vl, e)
    history = fitloop.run_cached(lambda f, y, r, want: state.step(f, y, r, want_loss=want), features, fitloop.labels_on(labels, lab, dev),
                                 fitloop.order_on(order, np.int64, dev), batch_size, per_epoch, epochs, lr_steps, return_history, end_epoch)
    out = state.best_context() if final_model == "best_val" else state.gathered_context()
    return fitmonitor.pack(out, history, state.monitor() if return_monitor else None, return_history, return_monitor)
