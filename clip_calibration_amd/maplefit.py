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

Not covered (IVLP and PromptSRC train through ``promptsrcfit``): ``nn.DataParallel``, the ResNet towers, class-token positions other
than ``end``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib, fitloop, fitmonitor, ops
from ._lib import check, lib
from . import coopfit, vptfit
from .coopfit import DYNAMIC, _BlockScaler, _check_grad_scale, _is_dynamic, _scale_args

# 2^10, one power of two for both towers' backwards, measured at ViT-B/16 with synthetic weights, n_ctx 2, depth 9, batch 4, 100 classes
# (profiles/maplefit_parity.txt, "grad_scale"): the text tower's dgrad-GEMM operands reach 1413 there (2^5.5 of headroom below fp16's
# largest value; the image tower's 77, 2^9.7) with 2.3 % / 2.1 % of the elements subnormal.  2^12, CoOp's and VPT's value, leaves the text
# tower 2^3.5 of headroom only (0.82 % / 0.62 % subnormal) and 2^16 overflows it; the gradients at 2^10 and 2^12 agree to 1e-4.  A model
# with much larger gradients overflows fp16 at this scale -- the parameters then turn NaN, they do not go wrong silently; pass a smaller
# power of two.
DEFAULT_GRAD_SCALE = 1024.0

_DT = {torch.float16: _lib.F16, torch.float32: _lib.F32}


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


class _Towers:
    """Both frozen towers in training mode for one prompt set: coopfit's text tower and vptfit's image tower, driven with deep prompts."""

    def __init__(self, who: str, model, tokenized_prompts, learner_params, seq_rows: Optional[int], class_token_position: str = "end"):
        self.n_ctx, self.depth = _check_design(who, model, learner_params, class_token_position)
        Cn, n_ctx, per_class, last = coopfit._check_prompts(who, model, tokenized_prompts, learner_params["ctx"])
        self.model, self.C = model, Cn
        self.text = coopfit._Tower(who, model, tokenized_prompts, Cn, n_ctx, False, last, seq_rows)
        self.vision = vptfit._Tower(who, model, self.depth, n_ctx)
        g = model.geometry
        self.Dt, self.Dv, self.E = int(g.transformer_width), int(g.vision_width), int(g.embed_dim)
        dev = model.device
        self.vis = torch.empty(self.depth, n_ctx, self.Dv, dtype=torch.float32, device=dev)
        self.d_deep = torch.empty(max(self.depth - 1, 1), n_ctx, self.Dt, dtype=torch.float32, device=dev)
        self.step_ws = torch.empty(max(lib.clipmi_maple_step_workspace_bytes(n_ctx, self.depth, self.Dt), 256), dtype=torch.uint8, device=dev)
        self.one_ws = None

    def deep_ptr(self, block: torch.Tensor):
        return block.data_ptr() + 4 * self.n_ctx * self.Dt if self.depth > 1 else None

    def text_forward(self, block: torch.Tensor) -> torch.Tensor:
        """The text half of ``forward``: couple (the image tower's prompts into ``self.vis``), then the text features [C, E]."""
        t, m = self.text, self.model
        couple(block, self.n_ctx, self.depth, self.Dt, self.Dv, self.vis)
        with m._launch_lock:
            check(lib.clipmi_text_encoder_train_deep(m._handle, t.base.data_ptr(), _DT[t.base.dtype], block.data_ptr(), self.n_ctx, 0, t.eot.data_ptr(), t.C,
                                                     t.rows, self.deep_ptr(block), self.depth - 1, t.text.data_ptr(), t.ws.data_ptr(), t.ws.numel(),
                                                     t.stash.data_ptr(), t.stash.numel(), _lib.CALL_DEFAULT, ops._stream()),
                  "clipmi_text_encoder_train_deep")
        return t.text

    def forward(self, block: torch.Tensor, images: torch.Tensor):
        """(text features [C, E], image features [B, E]) at the block: couple, text forward, image forward."""
        return self.text_forward(block), self.vision.forward(images, self.vis)

    def backward(self, d_text: torch.Tensor, d_feats: torch.Tensor, stats_text: Optional[torch.Tensor] = None, stats_vision: Optional[torch.Tensor] = None):
        """(d_embed, d_deep, d_vis): the text tower's backward, then the image tower's."""
        t, m = self.text, self.model
        with m._launch_lock:
            check(lib.clipmi_text_encoder_backward_deep(m._handle, C.byref(t.dgrad[0]), d_text.data_ptr(), t.C, t.rows, self.n_ctx, self.depth - 1,
                                                        t.d_embed.data_ptr(), self.d_deep.data_ptr() if self.depth > 1 else None, t.ws.data_ptr(),
                                                        t.ws.numel(), t.stash.data_ptr(), t.stash.numel(),
                                                        None if stats_text is None else stats_text.data_ptr(), ops._stream()),
                  "clipmi_text_encoder_backward_deep")
        return t.d_embed, (self.d_deep if self.depth > 1 else None), self.vision.backward(d_feats, stats_vision)

    def one_call_workspace(self, B: int, scaled: bool = False) -> torch.Tensor:
        sizer = lib.clipmi_maple_train_step_scaled_bytes if scaled else lib.clipmi_maple_train_step_bytes
        need = sizer(self.model._handle, self.C, self.text.rows, B, self.n_ctx, self.depth)
        if self.one_ws is None or self.one_ws.numel() < need:
            self.one_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.model.device)
        return self.one_ws


def gradients(model, learner_params: Dict[str, torch.Tensor], images: torch.Tensor, labels, tokenized_prompts, logit_scale: float = 4.6052,
              grad_scale: float = DEFAULT_GRAD_SCALE, seq_rows: Optional[int] = None, return_operand_stats: bool = False,
              class_token_position: str = "end"):
    """``(loss, grads)`` of ``F.cross_entropy(exp(logit_scale) * normalise(image features) @ normalise(text features).T, labels)`` with
    respect to every prompt-learner parameter, on the GPU: loss fp32 [1], grads a dict of fp32 tensors under ``learner_params``' names.
    ``images`` [B, 3, R, R] preprocessed, ``tokenized_prompts`` [C, context_length] the ids of ``"X .. X name."``; ``seq_rows`` as
    ``coopfit.context_gradient`` takes it.  ``return_operand_stats`` adds ``{"text": {...}, "vision": {...}}``: per tower, over every
    fp16 dgrad-GEMM operand element, ``elements``, ``zeros``, ``subnormals``, ``max`` -- the measurement behind the default
    ``grad_scale``.  A diagnostic entry point: every call allocates both towers' workspaces and stashes."""
    who = "maplefit.gradients"
    if _is_dynamic(who, grad_scale):
        raise ValueError(f"{who}: grad_scale={DYNAMIC!r} belongs to a fit (MaPLeFitState, fit_prompt_learner); one gradient needs a number")
    gs = _check_grad_scale(who, grad_scale)
    if not math.isfinite(logit_scale):
        raise ValueError(f"{who}: logit_scale={logit_scale} (finite)")
    tw = _Towers(who, model, tokenized_prompts, learner_params, seq_rows, class_token_position)
    images = tw.vision.images(who, images)
    dev = images.device
    labels_d = fitloop.step_labels(who, labels, images.shape[0], tw.C, dev, "images")
    block = pack_block(learner_params, tw.depth, dev)
    text, feats = tw.forward(block, images)
    scale = float(np.float32(math.exp(logit_scale)))
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


class MaPLeFitState(fitmonitor.ImageMonitored):
    """The training state of MaPLe's prompt learner: the fp32 master ``block``, SGD's momentum buffer, both towers' stashes and the number
    of steps taken.  ``step`` enqueues one forward, backward and update and does not synchronise.  ``params()`` names the block's views.
    ``validate`` scores validation images on the device (``start_monitor``, ``monitor``, ``best_params``, ``val_row_results``; DESIGN.md
    "Fit monitor", "The image-tower fits")."""
    _who = "MaPLeFitState"

    def __init__(self, model, tokenized_prompts, learner_params: Dict[str, torch.Tensor], logit_scale: float = 4.6052, momentum: float = 0.9,
                 dampening: float = 0.0, nesterov: bool = False, weight_decay: float = 5e-4, grad_scale: float = DEFAULT_GRAD_SCALE,
                 seq_rows: Optional[int] = None, class_token_position: str = "end", scaler: Optional[dict] = None):
        who = "MaPLeFitState"
        self.dynamic, self.grad_scale, self.scaler = _scale_args(who, grad_scale, scaler)
        fitloop.check_sgd(who, momentum, dampening, weight_decay, nesterov)
        if not math.isfinite(logit_scale):
            raise ValueError(f"{who}: logit_scale={logit_scale} (finite)")
        self.towers = _Towers(who, model, tokenized_prompts, learner_params, seq_rows, class_token_position)
        self.C = self.towers.C
        self.block = pack_block(learner_params, self.towers.depth, model.device)
        self.buf = torch.zeros_like(self.block) if momentum != 0.0 else None
        self.scale = float(np.float32(math.exp(logit_scale)))
        self.momentum, self.dampening, self.nesterov, self.weight_decay = momentum, dampening, nesterov, weight_decay
        self.steps = 0
        self._scaler = _BlockScaler(self.scaler, model.device) if self.dynamic else None
        self._scaled_grad = torch.empty_like(self.block) if self.dynamic else None    # scale * gradient, as clipmi_maple_step leaves it

    def params(self, block: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        t = self.towers
        return unpack_block(self.block if block is None else block, t.n_ctx, t.depth, t.Dt, t.Dv)

    def _master(self) -> torch.Tensor:
        return self.block

    def validate(self, val_images_or_loader, val_labels, epoch: int, val_batch_size: int = 32, one_call: bool = True) -> None:
        """Enqueue one validation of the current master block into slot ``epoch`` of the device history; no host read.  The text side's
        training forward runs ONCE on the block (couple, deep text prompts), its features are normalised, and the validation images --
        [N_val, 3, R, R] on the GPU with ``val_labels``, in chunks of ``val_batch_size``, or a sized iterable of (images, labels) batches
        on the GPU with None -- run through the image tower's training forward at the coupled prompts, chunk by chunk
        (``VPTFitState.validate`` has the rest: row results, finish, selection of the whole block, labels)."""
        who = "MaPLeFitState.validate"
        mon, tw = self._monitor_for(epoch), self.towers
        text_n = ops.l2_normalize(tw.text_forward(self.block))
        mon.validate(who, tw.vision, tw.vis, text_n, self.scale, val_images_or_loader, val_labels, epoch, val_batch_size, self.block, one_call)

    def best_params(self) -> Dict[str, torch.Tensor]:
        """The best slot on the device under ``params()``' names: the block of the best epoch so far, or the block ``start_monitor`` saw
        while no epoch has been taken."""
        return self.params(self._best_block("best_params"))

    def scaler_state(self) -> dict:
        """The dynamic scale's block as ``dict(scale, growth_tracker, skipped_steps, applied_steps, found_inf)`` (``found_inf``: of the
        last step).  It waits for the steps enqueued so far: one synchronisation, the only read-back of the dynamic path."""
        if not self.dynamic:
            raise ValueError(f"MaPLeFitState.scaler_state: the state was made with a static grad_scale={self.grad_scale}")
        return self._scaler.state()

    def step(self, images: torch.Tensor, labels, lr, want_loss: bool = False, one_call: bool = False) -> Optional[torch.Tensor]:
        """One optimiser step on the batch ``images`` [B, 3, R, R] (preprocessed, fp16 or fp32, on the GPU) and ``labels`` [B] at the rate
        ``lr``: an fp32 tensor of one element on the device is read where it lies; a Python number is uploaded on every call.  A label
        tensor on the GPU is taken as it is -- a label outside [0, C) then makes the parameters NaN, it is never used as an address; host
        labels are range-checked.  ``one_call``: the same launches through clipmi_maple_train_step, whose workspace holds both towers'.
        Returns the batch loss, fp32 [1] on the device, when ``want_loss``.  Under ``grad_scale="dynamic"`` the head runs at
        ``grad_scale = 1``, ``d_text`` and ``d_feats`` are multiplied by the device block's scale, clipmi_maple_step forms the gradient
        without applying it and clipmi_block_step_scaled decides on the device whether the step is applied (one call:
        clipmi_maple_train_step_scaled); a skipped step still counts in ``steps`` and still returns its loss; whether it was applied is in
        ``scaler_state()``."""
        who = "MaPLeFitState.step"
        tw = self.towers
        t, v, m = tw.text, tw.vision, tw.model
        images = v.images(who, images)
        dev, B = images.device, images.shape[0]
        labels_d = fitloop.step_labels(who, labels, B, self.C, dev, "images")
        lr_d = ops._dev(fitloop.lr_operand(lr, dev), "lr", (torch.float32,))
        first = self.steps == 0
        sgd = (float(self.momentum), float(self.dampening), float(self.weight_decay), int(bool(self.nesterov)))
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        if self.dynamic and one_call:
            v.size(B, tower_ws=False)
            ws, sc = tw.one_call_workspace(B, scaled=True), self._scaler
            with m._launch_lock:
                check(lib.clipmi_maple_train_step_scaled(m._handle, C.byref(t.dgrad[0]), C.byref(v.dgrad[0]), t.base.data_ptr(), _DT[t.base.dtype],
                                                         t.eot.data_ptr(), t.C, t.rows, images.data_ptr(), _DT[images.dtype], B, labels_d.data_ptr(),
                                                         self.block.data_ptr(), None if self.buf is None else self.buf.data_ptr(), tw.n_ctx, tw.depth,
                                                         self.scale, sc.block.data_ptr(), *sc.args(), lr_d.data_ptr(), *sgd, loss.data_ptr(), None,
                                                         ws.data_ptr(), ws.numel(), t.stash.data_ptr(), t.stash.numel(), v.stash.data_ptr(),
                                                         v.stash.numel(), ops._stream()),
                      "clipmi_maple_train_step_scaled")
        elif self.dynamic:
            text, feats = tw.forward(self.block, images)
            _, d_feats, d_text = maple_head(feats, labels_d, text, self.scale, 1.0, loss)
            ops.grad_scale_rows(d_text, self._scaler.block)
            ops.grad_scale_rows(d_feats, self._scaler.block)
            d_embed, d_deep, d_vis = tw.backward(d_text, d_feats)
            check(lib.clipmi_maple_step(d_embed.data_ptr(), None if d_deep is None else d_deep.data_ptr(), d_vis.data_ptr(), self.block.data_ptr(), None,
                                        self._scaled_grad.data_ptr(), 0, t.C, t.L, tw.n_ctx, tw.depth, tw.Dt, tw.Dv, 1.0, None, 0, *sgd,
                                        tw.step_ws.data_ptr(), tw.step_ws.numel(), ops._stream()), "clipmi_maple_step")
            self._scaler.step(self._scaled_grad, self.block, self.buf, lr_d, *sgd)
        elif one_call:
            v.size(B, tower_ws=False)
            ws = tw.one_call_workspace(B)
            with m._launch_lock:
                check(lib.clipmi_maple_train_step(m._handle, C.byref(t.dgrad[0]), C.byref(v.dgrad[0]), t.base.data_ptr(), _DT[t.base.dtype], t.eot.data_ptr(),
                                                  t.C, t.rows, images.data_ptr(), _DT[images.dtype], B, labels_d.data_ptr(), self.block.data_ptr(),
                                                  None if self.buf is None else self.buf.data_ptr(), tw.n_ctx, tw.depth, self.scale, self.grad_scale,
                                                  lr_d.data_ptr(), int(first), *sgd, loss.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                                  t.stash.data_ptr(), t.stash.numel(), v.stash.data_ptr(), v.stash.numel(), ops._stream()),
                      "clipmi_maple_train_step")
        else:
            text, feats = tw.forward(self.block, images)
            _, d_feats, d_text = maple_head(feats, labels_d, text, self.scale, self.grad_scale, loss)
            d_embed, d_deep, d_vis = tw.backward(d_text, d_feats)
            maple_step(d_embed, d_deep, d_vis, self.block, t.C, t.L, tw.n_ctx, tw.depth, tw.Dt, tw.Dv, self.grad_scale, self.buf, lr_d, first, *sgd,
                       want_grad=False, ws=tw.step_ws)
        self.steps += 1
        return loss if want_loss else None


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
                       depth: int = 9, logit_scale: float = 4.6052, lr: float = 0.0035, epochs: int = 5, batch_size: int = 4, momentum: float = 0.9,
                       dampening: float = 0.0, weight_decay: float = 5e-4, nesterov: bool = False, grad_scale: float = DEFAULT_GRAD_SCALE,
                       seq_rows: Optional[int] = None, lr_per_epoch: Optional[Sequence[float]] = None, drop_last: bool = False,
                       return_history: bool = False, class_token_position: str = "end", scaler: Optional[dict] = None, val=None,
                       val_batch_size: int = 32, val_bins: int = 10, final_model: str = "last_step", val_criterion: str = "accuracy",
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
    the fitted parameters are bit for bit those of the same call without ``val``; "best_val" returns the best epoch's parameters."""
    who = "fit_prompt_learner"
    fitmonitor.check_image_args(who, val, val_batch_size, val_bins, final_model, val_criterion)
    epochs = int(epochs)
    if epochs < 0:
        raise ValueError(f"{who}: epochs={epochs} (>= 0)")
    if learner_params is None:
        learner_params = init_learner_params(model, n_ctx, depth)
    state = MaPLeFitState(model, tokenized_prompts, learner_params, logit_scale, momentum, dampening, nesterov, weight_decay, grad_scale, seq_rows,
                          class_token_position, scaler)
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
