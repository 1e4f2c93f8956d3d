"""MaPLe's multi-modal prompts trained on the GPU (reference trainers/classification/maple.py:77-216; clip/model.py:259-331).

The reference trains the prompt learner's parameters with both towers frozen: ``ctx`` [n_ctx, Dt], which replaces token rows 1 .. n_ctx
of every class prompt; ``compound_prompts_text.{i}`` [n_ctx, Dt] (i < depth - 1), which overwrite those rows in front of text block i + 1;
``proj`` (a half ``Linear(Dt, Dv)``), whose image of ``ctx`` is the image tower's ``shared_ctx``; and
``compound_prompt_projections.{i}`` (``Linear(Dt, Dv)``), whose images of the deep text prompts overwrite the image tower's last n_ctx
token rows in front of image block i + 1.  Every step runs both towers, normalises both sides, takes ``F.cross_entropy`` of
``exp(logit_scale)`` times the cosine and one ``torch.optim.SGD`` step on the whole list.  It is the first method here whose loss reaches
its parameters through BOTH towers: a step is the coupling functions (csrc/maple_train.hip), the text tower's training forward with deep
prompts (csrc/text_backward.hip, ``clipmi_text_encoder_train_deep``), the image tower's (csrc/vision_backward.hip), the joint head
(csrc/prompt_train.hip, ``clipmi_maple_head``), both backwards, and one step over one fp32 master block
``[ctx | compound text | proj W | proj b | deep W | deep b]`` -- no autograd graph.  DESIGN.md "MaPLe fit" has the data flow.

The parameters travel as a dict under the prompt learner's own ``state_dict`` names: ``ctx``, ``compound_prompts_text.{i}``,
``proj.weight``, ``proj.bias``, ``compound_prompt_projections.{i}.weight``, ``compound_prompt_projections.{i}.bias``.

``grad_scale``: as in ``coopfit`` / ``vptfit`` -- one power of two covers both towers' backwards, the head multiplies both gradients by
it and the step divides.  profiles/maplefit_parity.txt has the measurement behind the default.  ``grad_scale="dynamic"`` with
``scaler=dict(init_scale, growth_factor, backoff_factor, growth_interval)`` is the reference's ``prec == "amp"`` branch (maple.py:269,
``torch.cuda.amp.GradScaler``) as ``coopfit`` has it: the scale lives in a block on the device, a step whose gradient block holds an inf
or a NaN changes neither the parameters nor the momentum buffer, and the scale backs off and grows again.  No step reads anything back;
``MaPLeFitState.scaler_state()`` does, once.  DESIGN.md "Dynamic loss scale for the block fits"; the reference's ``autocast`` casts
differ from this path's fixed fp16 operand points (unverified).

``gradients`` returns one batch's loss and every parameter's gradient (the diagnostic entry point of the tests).
``MaPLeFitState.step`` takes one batch of preprocessed images; ``fit_prompt_learner`` runs epochs over a tensor of images or a loader of
(images, labels) batches and enqueues every step with one synchronisation at the end.  Both towers run on every step.

The defaults -- SGD at 0.0035 with momentum 0.9 and weight decay 5e-4, 5 epochs in batches of 4, a constant warm-up epoch handing over to
a cosine schedule, n_ctx 2, depth 9 -- restate configs/trainers/MaPLe/vit_b16_c2_ep5_batch4.yaml; the momentum and the weight decay
are Dassl's public defaults and are UNVERIFIED here; each is an argument.

ViT-L lengths (more than 224 token rows per image; configs/trainers/MaPLe/vit_l14_c2_ep5_batch4.yaml): refused by default, taken up to
640 rows with the library option ``vision_train_long`` at 1 (``vptfit.max_rows()``; DESIGN.md "Long attention backward").  ViT-L/14's
patches of 14 pixels are served by the image tower's training forward (the patchify + GEMM route of ``vptfit``'s docstring), so with
the option on that configuration's own towers train here.

``shard=coopfit.Shard(world, rank, gather)`` on ``MaPLeFitState``, ``fit_prompt_learner`` and ``gradients``: the batch-sharded fit of
``vptfit``'s docstring (the reference's ``nn.DataParallel``, maple.py:273-277); only the image batch is sharded, the text tower runs over
all C prompts on every rank.  DESIGN.md "Batch-sharded image-tower fits".

Not covered (IVLP and PromptSRC train through ``promptsrcfit``): ``nn.DataParallel`` itself in one process, the ResNet towers, class-token positions other
than ``end``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib, fitloop, fitmonitor, fitoptim, ops
from ._lib import _DT, check, lib
from . import coopfit, vptfit
from . import shard as sharding
from .coopfit import Shard

# 2^10, one power of two for both towers' backwards, measured at ViT-B/16 with synthetic weights, n_ctx 2, depth 9, batch 4, 100 classes
# (profiles/maplefit_parity.txt, "grad_scale"): the text tower's dgrad-GEMM operands reach 1413 there (2^5.5 of headroom below fp16's
# largest value; the image tower's 77, 2^9.7) with 2.3 % / 2.1 % of the elements subnormal.  2^12, CoOp's and VPT's value, leaves the text
# tower 2^3.5 of headroom only (0.82 % / 0.62 % subnormal) and 2^16 overflows it; the gradients at 2^10 and 2^12 agree to 1e-4.  A model
# with much larger gradients overflows fp16 at this scale -- the parameters then turn NaN, they do not go wrong silently; pass a smaller
# power of two.
DEFAULT_GRAD_SCALE = 1024.0


def param_names(depth: int):
    """The parameter names in the master block's order."""
    return (["ctx"] + [f"compound_prompts_text.{i}" for i in range(depth - 1)] + ["proj.weight", "proj.bias"]
            + [f"compound_prompt_projections.{i}.weight" for i in range(depth - 1)] + [f"compound_prompt_projections.{i}.bias" for i in range(depth - 1)])


def _shapes(n_ctx: int, depth: int, Dt: int, Dv: int):
    return ([(n_ctx, Dt)] * depth + [(Dv, Dt), (Dv,)] + [(Dv, Dt)] * (depth - 1) + [(Dv,)] * (depth - 1))


def _check_design(who: str, model, learner_params, class_token_position: str = "end"):
    """(n_ctx, depth) after the refusals of the design."""
    if getattr(model, "is_resnet", False):
        raise ValueError(f"{who}: prompt tokens apply to the ViT towers only (the ResNet tower has none)")
    if model.design_details.get("trainer") != "MaPLe":
        raise ValueError(f"{who}: needs a CLIP built with design_details trainer='MaPLe', got trainer={model.design_details.get('trainer')!r}")
    if class_token_position != "end":
        raise ValueError(f"{who}: class_token_position={class_token_position!r}; only 'end' is trained (the layout is [SOS | ctx | class tokens, EOS])")
    if not isinstance(learner_params, dict) or "ctx" not in learner_params:
        raise ValueError(f"{who}: learner_params must be a dict with the prompt learner's names ('ctx', 'proj.weight', ...)")
    g = model.geometry
    Dt, Dv = int(g.transformer_width), int(g.vision_width)
    ctx = learner_params["ctx"]
    if not isinstance(ctx, torch.Tensor) or ctx.dim() != 2 or ctx.shape[1] != Dt:
        raise ValueError(f"{who}: ctx {tuple(getattr(ctx, 'shape', ()))} must be [n_ctx, {Dt}] (a generic context)")
    n_ctx = int(ctx.shape[0])
    depth = 1 + len([k for k in learner_params if k.startswith("compound_prompts_text.")])
    if depth > min(g.transformer_layers, g.vision_layers):
        raise ValueError(f"{who}: depth={depth} for {g.transformer_layers} text and {g.vision_layers} image layers")
    for name, shape in zip(param_names(depth), _shapes(n_ctx, depth, Dt, Dv)):
        t = learner_params.get(name)
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or not t.dtype.is_floating_point:
            raise ValueError(f"{who}: {name} {tuple(getattr(t, 'shape', ()))} must be a floating-point tensor {shape}")
    want = int(model.design_details.get("maple_length", n_ctx))
    if want != n_ctx:
        raise ValueError(f"{who}: n_ctx={n_ctx} does not match the model's maple_length ({want})")
    tokens = (g.image_resolution // g.vision_patch_size) ** 2 + 1
    vptfit.check_rows(who, tokens, n_ctx)
    return n_ctx, depth


def pack_block(learner_params: Dict[str, torch.Tensor], depth: int, dev) -> torch.Tensor:
    """The fp32 master block of the parameters, on ``dev`` (a copy)."""
    return torch.cat([learner_params[n].detach().to(device=dev, dtype=torch.float32).reshape(-1) for n in param_names(depth)]).contiguous()


def unpack_block(block: torch.Tensor, n_ctx: int, depth: int, Dt: int, Dv: int) -> Dict[str, torch.Tensor]:
    """Views of a block (or of a gradient of its shape) under the parameter names."""
    out, at = {}, 0
    for name, shape in zip(param_names(depth), _shapes(n_ctx, depth, Dt, Dv)):
        n = int(np.prod(shape))
        out[name] = block[at:at + n].view(shape)
        at += n
    assert at == block.numel()
    return out


def couple(block: torch.Tensor, n_ctx: int, depth: int, Dt: int, Dv: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """clipmi_maple_couple: the image tower's prompt block fp32 [depth, n_ctx, Dv] (slot 0: shared_ctx)."""
    vis = torch.empty(depth, n_ctx, Dv, dtype=torch.float32, device=block.device) if out is None else out
    check(lib.clipmi_maple_couple(block.data_ptr(), n_ctx, depth, Dt, Dv, vis.data_ptr(), ops._stream()), "clipmi_maple_couple")
    return vis


def maple_head(feats: torch.Tensor, labels: torch.Tensor, text: torch.Tensor, scale: float, grad_scale: float, loss: Optional[torch.Tensor] = None,
               want_f16: bool = False):
    """clipmi_maple_head: ``(loss fp32 [1], d_feats fp32 [B, E], d_text fp32 [C, E])`` and, with ``want_f16``, d_text's fp16 copy."""
    B, E = feats.shape
    Cn = text.shape[0]
    dev = feats.device
    ws = torch.empty(max(lib.clipmi_maple_head_workspace_bytes(B, E, Cn), 8), dtype=torch.uint8, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev) if loss is None else loss
    d_feats = torch.empty(B, E, dtype=torch.float32, device=dev)
    d_text = torch.empty(Cn, E, dtype=torch.float32, device=dev)
    d16 = torch.empty(Cn, E, dtype=torch.float16, device=dev) if want_f16 else None
    check(lib.clipmi_maple_head(feats.data_ptr(), feats.stride(0), labels.data_ptr(), text.data_ptr(), B, E, Cn, scale, grad_scale, loss.data_ptr(),
                                d_feats.data_ptr(), d_text.data_ptr(), None if d16 is None else d16.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()),
          "clipmi_maple_head")
    return (loss, d_feats, d_text) + ((d16,) if want_f16 else ())


def maple_step(d_embed: torch.Tensor, d_deep: Optional[torch.Tensor], d_vis: torch.Tensor, block: torch.Tensor, Cn: int, L: int, n_ctx: int, depth: int,
               Dt: int, Dv: int, grad_scale: float, buf: Optional[torch.Tensor] = None, lr=None, first_step: bool = True, momentum: float = 0.0,
               dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False, apply: bool = True, want_grad: bool = True,
               ws: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """clipmi_maple_step: the whole block's gradient (returned with ``want_grad``) and, with ``apply``, SGD's step on ``block`` in place."""
    grad = torch.empty_like(block) if want_grad else None
    if ws is None:
        ws = torch.empty(max(lib.clipmi_maple_step_workspace_bytes(n_ctx, depth, Dt), 256), dtype=torch.uint8, device=block.device)
    check(lib.clipmi_maple_step(d_embed.data_ptr(), None if d_deep is None else d_deep.data_ptr(), d_vis.data_ptr(), block.data_ptr(),
                                None if buf is None else buf.data_ptr(), None if grad is None else grad.data_ptr(), int(bool(apply)), Cn, L, n_ctx, depth,
                                Dt, Dv, grad_scale, None if lr is None else lr.data_ptr(), int(first_step), float(momentum), float(dampening),
                                float(weight_decay), int(bool(nesterov)), ws.data_ptr(), ws.numel(), ops._stream()), "clipmi_maple_step")
    return grad


class _TwoTowers:
    """Both frozen towers in training mode for one prompt set: coopfit's text tower driven with deep prompts and vptfit's image tower.
    ``nt`` / ``dt`` and ``nv`` / ``dv`` are the prompt rows and the prompt depth of the text side and of the image side; the text side's
    prompts are the front of the master block, [ctx [nt, Dt] | deep [dt - 1, nt, Dt]].  A method supplies ``image_prompts`` (where the
    image tower's prompts come from) and ``_step_bytes`` (its one-call sizing symbols)."""

    def __init__(self, who: str, model, tokenized_prompts, Cn: int, last_eot: int, nt: int, dt: int, nv: int, dv: int, seq_rows: Optional[int]):
        self.nt, self.dt, self.nv, self.dv = nt, dt, nv, dv
        self.model, self.C = model, Cn
        self.text = coopfit._Tower(who, model, tokenized_prompts, Cn, nt, False, last_eot, seq_rows)
        self.vision = vptfit._Tower(who, model, dv, nv)
        g = model.geometry
        self.Dt, self.Dv, self.E = int(g.transformer_width), int(g.vision_width), int(g.embed_dim)
        self.d_deep = torch.empty(max(dt - 1, 1), nt, self.Dt, dtype=torch.float32, device=model.device)
        self.one_ws = None

    def text_forward(self, block: torch.Tensor) -> torch.Tensor:
        """The text features [C, E] at the block."""
        t, m = self.text, self.model
        deep = block.data_ptr() + 4 * self.nt * self.Dt if self.dt > 1 else None
        with m._launch_lock:
            check(lib.clipmi_text_encoder_train_deep(m._handle, t.base.data_ptr(), _DT[t.base.dtype], block.data_ptr(), self.nt, 0, t.eot.data_ptr(), t.C,
                                                     t.rows, deep, self.dt - 1, t.text.data_ptr(), t.ws.data_ptr(), t.ws.numel(), t.stash.data_ptr(),
                                                     t.stash.numel(), _lib.CALL_DEFAULT, ops._stream()), "clipmi_text_encoder_train_deep")
        return t.text

    def forward(self, block: torch.Tensor, images: torch.Tensor):
        """(text features [C, E], image features [B, E]) at the block: the image tower's prompts, the text forward, the image forward."""
        vis = self.image_prompts(block)
        return self.text_forward(block), self.vision.forward(images, vis)

    def backward(self, d_text: torch.Tensor, d_feats: torch.Tensor, stats_text: Optional[torch.Tensor] = None, stats_vision: Optional[torch.Tensor] = None):
        """(d_embed, d_deep, d_vis): the text tower's backward, then the image tower's."""
        t, m = self.text, self.model
        with m._launch_lock:
            check(lib.clipmi_text_encoder_backward_deep(m._handle, C.byref(t.dgrad[0]), d_text.data_ptr(), t.C, t.rows, self.nt, self.dt - 1,
                                                        t.d_embed.data_ptr(), self.d_deep.data_ptr() if self.dt > 1 else None, t.ws.data_ptr(),
                                                        t.ws.numel(), t.stash.data_ptr(), t.stash.numel(),
                                                        None if stats_text is None else stats_text.data_ptr(), ops._stream()),
                  "clipmi_text_encoder_backward_deep")
        return t.d_embed, (self.d_deep if self.dt > 1 else None), self.vision.backward(d_feats, stats_vision)

    def one_call_workspace(self, B: int, scaled: bool = False) -> torch.Tensor:
        """The one-call step's workspace: grown when a call needs more, never shrunk."""
        need = self._step_bytes(B, scaled)
        if self.one_ws is None or self.one_ws.numel() < need:
            self.one_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.model.device)
        return self.one_ws

    def one_call_front(self, images: torch.Tensor, B: int, labels_d: torch.Tensor):
        """The arguments every two-tower one-call symbol begins with, up to the labels."""
        t, v = self.text, self.vision
        return (self.model._handle, C.byref(t.dgrad[0]), C.byref(v.dgrad[0]), t.base.data_ptr(), _DT[t.base.dtype], t.eot.data_ptr(), t.C, t.rows,
                images.data_ptr(), _DT[images.dtype], B, labels_d.data_ptr())

    def stashes(self):
        t, v = self.text, self.vision
        return t.stash.data_ptr(), t.stash.numel(), v.stash.data_ptr(), v.stash.numel()


class _Towers(_TwoTowers):
    """MaPLe's towers: one rows / depth pair for both sides (``n_ctx``, ``depth``), the image tower's prompts coupled into ``vis``."""

    def __init__(self, who: str, model, tokenized_prompts, learner_params, seq_rows: Optional[int], class_token_position: str = "end"):
        self.n_ctx, self.depth = n_ctx, depth = _check_design(who, model, learner_params, class_token_position)
        Cn, _, _, last = coopfit._check_prompts(who, model, tokenized_prompts, learner_params["ctx"])
        super().__init__(who, model, tokenized_prompts, Cn, last, n_ctx, depth, n_ctx, depth, seq_rows)
        dev = model.device
        self.vis = torch.empty(depth, n_ctx, self.Dv, dtype=torch.float32, device=dev)
        self.step_ws = torch.empty(max(lib.clipmi_maple_step_workspace_bytes(n_ctx, depth, self.Dt), 256), dtype=torch.uint8, device=dev)

    def image_prompts(self, block: torch.Tensor) -> torch.Tensor:
        return couple(block, self.n_ctx, self.depth, self.Dt, self.Dv, self.vis)

    def _step_bytes(self, B: int, scaled: bool) -> int:
        sizer = lib.clipmi_maple_train_step_scaled_bytes if scaled else lib.clipmi_maple_train_step_bytes
        return sizer(self.model._handle, self.C, self.text.rows, B, self.n_ctx, self.depth)


def gradients(model, learner_params: Dict[str, torch.Tensor], images: torch.Tensor, labels, tokenized_prompts, logit_scale: float = 4.6052,
              grad_scale: float = DEFAULT_GRAD_SCALE, seq_rows: Optional[int] = None, return_operand_stats: bool = False,
              class_token_position: str = "end", shard: Optional[Shard] = None):
    """``(loss, grads)`` of ``F.cross_entropy(exp(logit_scale) * normalise(image features) @ normalise(text features).T, labels)`` with
    respect to every prompt-learner parameter, on the GPU: loss fp32 [1], grads a dict of fp32 tensors under ``learner_params``' names.
    ``images`` [B, 3, R, R] preprocessed, ``tokenized_prompts`` [C, context_length] the ids of ``"X .. X name."``; ``seq_rows`` as
    ``coopfit.context_gradient`` takes it.  ``return_operand_stats`` adds ``{"text": {...}, "vision": {...}}``: per tower, over every
    fp16 dgrad-GEMM operand element, ``elements``, ``zeros``, ``subnormals``, ``max`` -- the measurement behind the default
    ``grad_scale``.  A diagnostic entry point: every call allocates both towers' workspaces and stashes.
    ``shard``: the loss and the gradients the batch-sharded step would apply, reduced over the ranks in rank order -- the same bits on
    every rank; every rank passes the whole batch, and the operand statistics (per rank) are refused."""
    who = "maplefit.gradients"
    gs = fitoptim.static_grad_scale(who, grad_scale, "MaPLeFitState", "fit_prompt_learner")
    if shard is not None:
        sharding.check(who, shard, "block", return_operand_stats=return_operand_stats)
        state = coopfit.shard_states(lambda sh: MaPLeFitState(model, tokenized_prompts, learner_params, logit_scale, 0.0, 0.0, False, 0.0, gs, seq_rows,
                                                              class_token_position, shard=sh), shard)
        losses, grad = state._shard_gradient(who, images, labels)
        return losses[:1], {k: v.clone() for k, v in state.params(grad).items()}
    scale = fitloop.exp_logit_scale(who, logit_scale)
    tw = _Towers(who, model, tokenized_prompts, learner_params, seq_rows, class_token_position)
    images = tw.vision.images(who, images)
    dev = images.device
    labels_d = fitloop.step_labels(who, labels, images.shape[0], tw.C, dev, "images")
    block = pack_block(learner_params, tw.depth, dev)
    text, feats = tw.forward(block, images)
    st = torch.zeros(4, dtype=torch.int64, device=dev) if return_operand_stats else None
    sv = torch.zeros(4, dtype=torch.int64, device=dev) if return_operand_stats else None
    loss, d_feats, d_text = maple_head(feats, labels_d, text, scale, gs)
    d_embed, d_deep, d_vis = tw.backward(d_text, d_feats, st, sv)
    grad = maple_step(d_embed, d_deep, d_vis, block, tw.C, tw.text.L, tw.n_ctx, tw.depth, tw.Dt, tw.Dv, gs, apply=False, ws=tw.step_ws)
    grads = {k: v.clone() for k, v in unpack_block(grad, tw.n_ctx, tw.depth, tw.Dt, tw.Dv).items()}
    if not return_operand_stats:
        return loss, grads
    return loss, grads, {"text": coopfit.operand_stats_dict(st), "vision": coopfit.operand_stats_dict(sv)}


def features(model, learner_params: Dict[str, torch.Tensor], images: torch.Tensor, tokenized_prompts, seq_rows: Optional[int] = None):
    """``(text features fp32 [C, E], image features fp32 [B, E])`` of the training forwards at ``learner_params``, raw: what the joint
    head is given.  Allocates both towers' workspaces and stashes per call, as ``gradients`` does."""
    who = "maplefit.features"
    tw = _Towers(who, model, tokenized_prompts, learner_params, seq_rows)
    images = tw.vision.images(who, images)
    text, feats = tw.forward(pack_block(learner_params, tw.depth, images.device), images)
    return text.clone(), feats.clone()


class MaPLeFitState(vptfit._BlockFitState):
    """The training state of MaPLe's prompt learner: the fp32 master ``block``, SGD's momentum buffer, both towers' stashes and the number
    of steps taken.  ``step`` enqueues one forward, backward and update and does not synchronise.  ``params()`` names the block's views.
    ``validate`` scores validation images on the device (``start_monitor``, ``monitor``, ``best_params``, ``val_row_results``; DESIGN.md
    "Fit monitor", "The image-tower fits")."""
    _who = "MaPLeFitState"

    def __init__(self, model, tokenized_prompts, learner_params: Dict[str, torch.Tensor], logit_scale: float = 4.6052,
                 momentum: float = 0.9, dampening: float = 0.0, nesterov: bool = False, weight_decay: float = 5e-4,
                 grad_scale: float = DEFAULT_GRAD_SCALE, seq_rows: Optional[int] = None, class_token_position: str = "end", scaler: Optional[dict] = None,
                 optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8, shard: Optional[Shard] = None):
        who = "MaPLeFitState"
        self._init_optimiser(who, logit_scale, momentum, dampening, nesterov, weight_decay, grad_scale, scaler, optimizer, betas, eps, shard)
        self.towers = _Towers(who, model, tokenized_prompts, learner_params, seq_rows, class_token_position)
        self.C = self.towers.C
        self._init_block(pack_block(learner_params, self.towers.depth, model.device))
        self._scaled_grad = self._grad_block()    # scale * gradient, as clipmi_maple_step leaves it (under shard: the send block's front)

    def params(self, block: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        t = self.towers
        return unpack_block(self.block if block is None else block, t.n_ctx, t.depth, t.Dt, t.Dv)

    def validate(self, val_images_or_loader, val_labels, epoch: int, val_batch_size: int = 32, one_call: bool = True) -> None:
        """Enqueue one validation of the current master block into slot ``epoch`` of the device history; no host read.  The text side's
        training forward runs ONCE on the block (couple, deep text prompts), its features are normalised, and the validation images --
        [N_val, 3, R, R] on the GPU with ``val_labels``, in chunks of ``val_batch_size``, or a sized iterable of (images, labels) batches
        on the GPU with None -- run through the image tower's training forward at the coupled prompts, chunk by chunk
        (``VPTFitState.validate`` has the rest: row results, finish, selection of the whole block, labels)."""
        who = "MaPLeFitState.validate"
        self._no_shard_validate(who)
        mon, tw = self._monitor_for(epoch), self.towers
        vis = tw.image_prompts(self.block)
        text_n = ops.l2_normalize(tw.text_forward(self.block))
        mon.validate(who, tw.vision, vis, text_n, self.scale, val_images_or_loader, val_labels, epoch, val_batch_size, self.block, one_call)

    def best_params(self) -> Dict[str, torch.Tensor]:
        """The best slot on the device under ``params()``' names: the block of the best epoch so far, or the block ``start_monitor`` saw
        while no epoch has been taken."""
        return self.params(self._best_block("best_params"))

    def _vision(self):
        return self.towers.vision

    def _one_call(self, images, B, labels_d):
        tw = self.towers
        front = tw.one_call_front(images, B, labels_d) + (self.block.data_ptr(), None if self.buf is None else self.buf.data_ptr(), tw.n_ctx, tw.depth)
        return "clipmi_maple_train_step", tw.one_call_workspace(B, self.dynamic), front, (), tw.stashes()

    def _head(self, images, labels_d, grad_scale, loss):
        text, feats = self.towers.forward(self.block, images)
        _, d_feats, d_text = maple_head(feats, labels_d, text, self.scale, grad_scale, loss)
        return d_text, d_feats

    def _apply(self, outs, lr_d, first, sgd):
        """Under the dynamic scale and under Adam clipmi_maple_step leaves scale * gradient in ``_scaled_grad`` and applies nothing."""
        tw = self.towers
        d_embed, d_deep, d_vis = tw.backward(*outs)
        grad, buf, gs, lr, first = (self._scaled_grad, None, 1.0, None, 0) if self._defer else (None, self.buf, self.grad_scale, lr_d, first)
        check(lib.clipmi_maple_step(d_embed.data_ptr(), None if d_deep is None else d_deep.data_ptr(), d_vis.data_ptr(), self.block.data_ptr(),
                                    None if buf is None else buf.data_ptr(), None if grad is None else grad.data_ptr(), int(not self._defer), tw.C,
                                    tw.text.L, tw.n_ctx, tw.depth, tw.Dt, tw.Dv, gs, None if lr is None else lr.data_ptr(), int(first), *sgd,
                                    tw.step_ws.data_ptr(), tw.step_ws.numel(), ops._stream()), "clipmi_maple_step")
        return grad


def init_learner_params(model, n_ctx: int = 2, depth: int = 9, seed: int = 0) -> Dict[str, torch.Tensor]:
    """A random initialisation in the reference's manner (maple.py:101-127): the prompts from N(0, 0.02^2), the Linears as ``nn.Linear``
    initialises them; ``proj`` rounded through fp16 (it is a half Linear)."""
    g = model.geometry
    Dt, Dv = int(g.transformer_width), int(g.vision_width)
    gen = torch.Generator().manual_seed(seed)
    out = {"ctx": 0.02 * torch.randn(n_ctx, Dt, generator=gen)}
    for i in range(depth - 1):
        out[f"compound_prompts_text.{i}"] = 0.02 * torch.randn(n_ctx, Dt, generator=gen)
    bound = 1.0 / math.sqrt(Dt)
    for name in ["proj"] + [f"compound_prompt_projections.{i}" for i in range(depth - 1)]:
        out[name + ".weight"] = (torch.rand(Dv, Dt, generator=gen) * 2 - 1) * bound
        out[name + ".bias"] = (torch.rand(Dv, generator=gen) * 2 - 1) * bound
    out["proj.weight"], out["proj.bias"] = out["proj.weight"].half().float(), out["proj.bias"].half().float()
    return out


def fit_prompt_learner(images_or_loader, labels, model, tokenized_prompts, learner_params: Optional[Dict[str, torch.Tensor]] = None, n_ctx: int = 2,
                       depth: int = 9, logit_scale: float = 4.6052, lr: float = 0.0035, epochs: int = 5, batch_size: int = 4,
                       momentum: float = 0.9, dampening: float = 0.0, weight_decay: float = 5e-4, nesterov: bool = False, grad_scale: float = DEFAULT_GRAD_SCALE,
                       seq_rows: Optional[int] = None, lr_per_epoch: Optional[Sequence[float]] = None, drop_last: bool = False,
                       return_history: bool = False, class_token_position: str = "end", scaler: Optional[dict] = None, optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8,
                       shard: Optional[Shard] = None, val=None, val_batch_size: int = 32, val_bins: int = 10, final_model: str = "last_step", val_criterion: str = "accuracy",
                       return_monitor: bool = False):
    """Train MaPLe's prompt learner starting from ``learner_params`` (not modified; None = ``init_learner_params(model, n_ctx, depth)``):
    ``epochs`` passes of ``torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov)`` over the whole parameter list.
    ``images_or_loader`` is a tensor of preprocessed images [N, 3, R, R] with ``labels`` [N], cut into batches of ``batch_size`` in order
    (the last one short unless ``drop_last``), or a sized iterable of (images, labels) batches iterated once per epoch (``labels`` None,
    ``batch_size`` unused).  ``lr_per_epoch`` gives every epoch's rate; None takes ``cosine_warmup_schedule(lr, epochs)``.  Both towers
    run on every step; nothing synchronises until the one wait at the end.  Returns the fitted parameters, a dict of fp32 tensors on the
    device (views of one block), or ``(params, per-step batch losses)`` with ``return_history``.  The model's prompt learner is NOT
    written: ``trainers.maple.CustomCLIP.fit_prompt_learner`` does that.  ``grad_scale="dynamic"`` with ``scaler`` (module docstring): a
    step that overflows fp16 is skipped on the device and the scale adapts; the history keeps one loss per step, skipped steps included,
    and the run still synchronises once.

    ``val=(val_images_or_loader, val_labels)``, ``val_batch_size``, ``val_bins``, ``final_model``, ``val_criterion`` and
    ``return_monitor`` as ``vptfit.fit_prompts`` takes them: behind every epoch ``MaPLeFitState.validate`` scores the block on the device;
    the fitted parameters are bit for bit those of the same call without ``val``; "best_val" returns the best epoch's parameters.

    ``optimizer``, ``betas``, ``eps``: "sgd" (the default; ``momentum``, ``dampening``, ``nesterov``), "adam" or
    "adamw", as ``coopfit.fit_context`` takes them; ``weight_decay`` keeps this fit's default of 5e-4 under all three (torch's AdamW
    default of 1e-2 is NOT taken over).  DESIGN.md "Adam steps for the prompt fits".

    ``shard=coopfit.Shard(world, rank, gather)``: the batch-sharded fit as ``vptfit.fit_prompts`` takes it (DESIGN.md "Batch-sharded
    image-tower fits"; the reference's ``nn.DataParallel``, maple.py:273-277).  Only the image batch is sharded: the text tower runs
    over all C prompts on every rank."""
    who = "fit_prompt_learner"
    if shard is not None:
        sharding.check(who, shard, "block", val=val, final_model=final_model)
    fitmonitor.check_image_args(who, val, val_batch_size, val_bins, final_model, val_criterion)
    epochs = int(epochs)
    if epochs < 0:
        raise ValueError(f"{who}: epochs={epochs} (>= 0)")
    if optimizer != "sgd":      # by this function's name; SGD's arguments are the state's to check, as before
        fitloop.check_optimizer(who, optimizer, momentum, dampening, nesterov, weight_decay, betas, eps)
    if learner_params is None:
        learner_params = init_learner_params(model, n_ctx, depth)
    sharding.check_batches(who, shard, images_or_loader, batch_size, drop_last)
    state = coopfit.shard_states(lambda sh: MaPLeFitState(model, tokenized_prompts, learner_params, logit_scale, momentum, dampening, nesterov, weight_decay,
                                                          grad_scale, seq_rows, class_token_position, scaler, optimizer, betas, eps, sh), shard)
    batches = fitloop.cut_batches(who, images_or_loader, labels, state.C, batch_size, drop_last, model.device)
    _, lr_steps = fitloop.schedule(who, lr, epochs, lr_per_epoch, len(batches), model.device)
    end_epoch = None
    if val is not None and epochs * len(batches) > 0:
        state.start_monitor(epochs, val_bins, val_criterion=val_criterion, select=final_model == "best_val")
        end_epoch = lambda e: state.validate(val[0], val[1], e, val_batch_size)
    history = fitloop.run_batches(lambda e, k, b, r, want: state.step(b[0], b[1], r, want_loss=want), batches, epochs, lr_steps, return_history, end_epoch)
    out = state.best_params() if final_model == "best_val" and end_epoch is not None else state.params()
    return fitmonitor.pack(out, history, fitmonitor.returned_monitor(state, end_epoch is not None, val_bins, return_monitor),
                           return_history, return_monitor)
