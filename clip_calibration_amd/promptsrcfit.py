"""PromptSRC's and IVLP's independent prompts trained on the GPU (reference trainers/classification/promptsrc.py:73-317;
clip/model.py:191-256).

The reference builds CLIP with ``design_details trainer='IVLP'`` and trains, with both towers frozen, the learner's ``ctx`` [nt, Dt]
(token rows 1 .. nt of every class prompt), the text blocks' ``transformer.resblocks.{i}.VPT_shallow`` [nt, Dt] (1 <= i < language_depth,
which overwrite those rows in front of block i), ``visual.VPT`` [nv, Dv] (appended behind the patch rows) and the image blocks'
``visual.transformer.resblocks.{i}.VPT_shallow`` [nv, Dv] (1 <= i < vision_depth, which overwrite the last nv token rows in front of block
i).  Every step runs both prompted towers and a second, frozen plain image tower on the batch and takes one ``torch.optim.SGD`` step on

    loss = mean_b CE(z_b, label_b) + w_text mean |u - o| + w_image mean |x - y| + w_logit sum q (log q - log p) / (B C)

with u, x the normalised prompted text / image features, o the normalised ``teacher`` (the reference's ``fixed_embeddings``), y the frozen
tower's normalised features, z = s X U^T, zz = s Y O^T, p = softmax(z), q = softmax(zz).  At the end of epoch e the parameters times
``gpa_weights(...)[e - 1]`` are added to a running sum (Gaussian-weighted prompt aggregation, GPA), which replaces them after the last
epoch.  IVLP (``method="ivlp"``) is the same path with the three weights 0 and no GPA: plain cross-entropy.

A step here is: the frozen forward (``clipmi_encode_image`` with no hook on the same model handle, fp32 residual stream), the text tower's
training forward with deep prompts, the image tower's, the four-term head (csrc/prompt_train.hip, ``clipmi_promptsrc_head``), both
backwards and one step over one fp32 master block ``[ctx | text deep | visual.VPT and image deep]`` (csrc/promptsrc_train.hip) -- no
autograd graph.  DESIGN.md "PromptSRC fit" has the data flow and the deviations from the reference.

The parameters travel as a dict under the reference's names (``param_names``).  ``gradients`` returns one batch's five loss terms and every
parameter's gradient (the diagnostic entry point of the tests).  ``PromptSRCFitState.step`` takes one batch of preprocessed images,
``.end_epoch(weight)`` accumulates GPA; ``fit_prompts`` runs epochs over a tensor of images or a loader of (images, labels) batches and
enqueues everything with one synchronisation at the end.

The defaults -- SGD at 0.0025, 50 epochs in batches of 4, a constant warm-up epoch handing over to a cosine schedule, weights 25 / 10 / 1,
GPA mean 30 and std 30 -- restate configs/trainers/PromptSRC/vit_b16_c4_ep50_batch4.yaml (w_logit is fixed at 1 in the reference's
code); momentum 0.9 and weight decay 5e-4 are Dassl's public defaults and are UNVERIFIED here; each is an argument.

``grad_scale="dynamic"`` with ``scaler=dict(init_scale, growth_factor, backoff_factor, growth_interval)`` (both methods) is the
reference's ``prec == "amp"`` branch (promptsrc.py:272, ``torch.cuda.amp.GradScaler``) as ``coopfit`` has it: the scale lives in a block
on the device, a step whose gradient block holds an inf or a NaN changes neither the parameters nor the momentum buffer, and the scale
backs off and grows again; ``end_epoch`` aggregates whatever the block holds.  No step reads anything back;
``PromptSRCFitState.scaler_state()`` does, once.  DESIGN.md "Dynamic loss scale for the block fits"; the reference's ``autocast`` casts
differ from this path's fixed fp16 operand points (unverified).

ViT-L lengths (more than 224 token rows per image; configs/trainers/PromptSRC/vit_l14_c4_ep50_batch4.yaml): refused by default, taken
up to 640 rows with the library option ``vision_train_long`` at 1 (``vptfit.max_rows()``; DESIGN.md "Long attention backward").  ViT-L/14's
patches of 14 pixels are served by the image tower's training forward (the patchify + GEMM route of ``vptfit``'s docstring) as they are
by the frozen plain tower's ``clipmi_encode_image``, so with the option on that configuration's own towers train here.

``shard=coopfit.Shard(world, rank, gather)`` on ``PromptSRCFitState``, ``fit_prompts`` and ``gradients`` (both methods): the
batch-sharded fit of ``vptfit``'s docstring (the reference's ``nn.DataParallel``, promptsrc.py:278); only the image batch is sharded,
the text tower runs over all C prompts on every rank and every rank keeps GPA's sum.  DESIGN.md "Batch-sharded image-tower fits".

Not covered: ``nn.DataParallel`` itself in one process, the ResNet towers, class-token positions other than ``end``.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, fitloop, fitmonitor, fitoptim, ops
from ._lib import _DT, check, lib
from . import coopfit, maplefit, vptfit
from . import shard as sharding
from .coopfit import Shard
from .fitloop import _need_gpu

# 2^10, one power of two for both towers' backwards, measured at ViT-B/16 with synthetic weights, nt = nv = 4, depths 9 / 9, batch 4, 100
# classes and the weights 25 / 10 / 1 (profiles/promptsrcfit_parity.txt, "grad_scale"): the text tower's dgrad-GEMM operands reach 1556
# there (2^5.4 of headroom below fp16's largest value; the image tower's 94, 2^9.4) with 1.3 % / 2.1 % of the elements subnormal.  2^12
# leaves the text tower 2^3.4 only (0.44 % / 0.64 % subnormal) and 2^16 overflows it; the gradients' norms agree to three digits from 2^0
# to 2^14.  A model with much larger gradients overflows fp16 at this
# scale -- the parameters then turn NaN, they do not go wrong silently; pass a smaller power of two.
DEFAULT_GRAD_SCALE = 1024.0
METHODS = ("promptsrc", "ivlp")
LOSS_NAMES = ("total", "ce", "text_l1", "image_l1", "logit_kl")


def param_names(dt: int, dv: int):
    """The parameter names in the master block's order: the text depth ``dt`` and the image depth ``dv`` count ctx / visual.VPT as 1."""
    return (["ctx"] + [f"transformer.resblocks.{i}.VPT_shallow" for i in range(1, dt)] + ["visual.VPT"]
            + [f"visual.transformer.resblocks.{i}.VPT_shallow" for i in range(1, dv)])


def _shapes(nt: int, dt: int, Dt: int, nv: int, dv: int, Dv: int):
    return [(nt, Dt)] * dt + [(nv, Dv)] * dv


def _depths(params) -> Tuple[int, int]:
    dt = 1 + len([k for k in params if k.startswith("transformer.resblocks.")])
    dv = 1 + len([k for k in params if k.startswith("visual.transformer.resblocks.")])
    return dt, dv


def model_params(model, ctx: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The model's own prompt parameters and the learner's ``ctx`` under the master block's names (the tensors themselves, not copies)."""
    deep_t, _ = model.ivlp_text_prompts()
    shallow, deep_v = model.ivlp_vision_prompts()
    if shallow is None:
        raise ValueError("promptsrcfit: the model carries no visual.VPT (needs design_details trainer='IVLP' with vision_depth >= 1)")
    tensors = [ctx] + list(deep_t or []) + [shallow] + list(deep_v)
    return dict(zip(param_names(1 + len(deep_t or []), 1 + len(deep_v)), tensors))


def _check_design(who: str, model, params, class_token_position: str = "end"):
    """(nt, dt, nv, dv) after the refusals of the design."""
    if getattr(model, "is_resnet", False):
        raise ValueError(f"{who}: prompt tokens apply to the ViT towers only (the ResNet tower has none)")
    dd = model.design_details
    if dd.get("trainer") != "IVLP":
        raise ValueError(f"{who}: needs a CLIP built with design_details trainer='IVLP', got trainer={dd.get('trainer')!r}")
    if int(dd.get("vision_depth", 0)) < 1:
        raise ValueError(f"{who}: vision_depth={dd.get('vision_depth', 0)}; the image prompts need vision_depth >= 1")
    if class_token_position != "end":
        raise ValueError(f"{who}: class_token_position={class_token_position!r}; only 'end' is trained (the layout is [SOS | ctx | class tokens, EOS])")
    if not isinstance(params, dict) or "ctx" not in params or "visual.VPT" not in params:
        raise ValueError(f"{who}: params must be a dict with the names 'ctx', 'visual.VPT', 'transformer.resblocks.1.VPT_shallow', ...")
    g = model.geometry
    Dt, Dv = int(g.transformer_width), int(g.vision_width)
    if int(dd.get("language_depth", 0)) > g.transformer_layers or int(dd.get("vision_depth", 0)) > g.vision_layers:
        raise ValueError(f"{who}: language_depth={dd.get('language_depth')} / vision_depth={dd.get('vision_depth')} for {g.transformer_layers} text and "
                         f"{g.vision_layers} image layers")
    ctx, vpt = params["ctx"], params["visual.VPT"]
    if not isinstance(ctx, torch.Tensor) or ctx.dim() != 2 or ctx.shape[1] != Dt:
        raise ValueError(f"{who}: ctx {tuple(getattr(ctx, 'shape', ()))} must be [n_ctx, {Dt}] (a generic context)")
    if not isinstance(vpt, torch.Tensor) or vpt.dim() != 2 or vpt.shape[1] != Dv:
        raise ValueError(f"{who}: visual.VPT {tuple(getattr(vpt, 'shape', ()))} must be [n_ctx, {Dv}]")
    nt, nv = int(ctx.shape[0]), int(vpt.shape[0])
    dt, dv = _depths(params)
    if dt > g.transformer_layers or dv > g.vision_layers:
        raise ValueError(f"{who}: text depth {dt} / image depth {dv} for {g.transformer_layers} text and {g.vision_layers} image layers")
    if len(params) != dt + dv:
        raise ValueError(f"{who}: unknown parameter names {sorted(set(params) - set(param_names(dt, dv)))}")
    for name, shape in zip(param_names(dt, dv), _shapes(nt, dt, Dt, nv, dv, Dv)):
        t = params.get(name)
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or not t.dtype.is_floating_point:
            raise ValueError(f"{who}: {name} {tuple(getattr(t, 'shape', ()))} must be a floating-point tensor {shape}")
    if nt != int(dd.get("language_ctx", nt)):
        raise ValueError(f"{who}: ctx has {nt} rows but the model's language_ctx is {dd.get('language_ctx')}")
    if nv != int(dd.get("vision_ctx", nv)):
        raise ValueError(f"{who}: visual.VPT has {nv} rows but the model's vision_ctx is {dd.get('vision_ctx')}")
    tokens = (g.image_resolution // g.vision_patch_size) ** 2 + 1
    vptfit.check_rows(who, tokens, nv)
    return nt, dt, nv, dv


def _check_ids(who: str, model, tokenized_prompts, nt: int):
    """(C, last EOT position): coopfit's checks of the prompt set, without its refusal of a model that carries deep text prompts."""
    L = int(model.context_length)
    ids = fitloop._host_int_array(who, tokenized_prompts, "tokenized_prompts")
    if ids.ndim != 2 or ids.shape[1] != L or ids.shape[0] < 2:
        raise ValueError(f"{who}: tokenized_prompts {ids.shape} must be [C >= 2, {L}]")
    eot = ids.argmax(axis=1)
    if not 1 + nt < L or int(eot.min()) <= nt:
        raise ValueError(f"{who}: n_ctx={nt} does not fit the prompts (context of {L} tokens, first EOT at {int(eot.min())}): the layout is "
                         "[SOS | ctx | class tokens, EOS]")
    return int(ids.shape[0]), int(eot.max())


def _check_weights(who: str, w_text: float, w_image: float, w_logit: float):
    for name, w in (("w_text", w_text), ("w_image", w_image), ("w_logit", w_logit)):
        if not (math.isfinite(w) and w >= 0.0):
            raise ValueError(f"{who}: {name}={w} (finite, >= 0)")
    return float(w_text), float(w_image), float(w_logit)


def _check_teacher(who: str, model, teacher, Cn: int) -> torch.Tensor:
    E = int(model.geometry.embed_dim)
    if not isinstance(teacher, torch.Tensor) or tuple(teacher.shape) != (Cn, E) or not teacher.dtype.is_floating_point:
        raise ValueError(f"{who}: teacher {tuple(getattr(teacher, 'shape', ()))} must be the frozen text features [C, E] = [{Cn}, {E}]")
    _need_gpu(teacher, "teacher")
    return teacher.detach().to(torch.float32).contiguous()


def pack_block(params: Dict[str, torch.Tensor], dev) -> torch.Tensor:
    """The fp32 master block of the parameters, on ``dev`` (a copy)."""
    return torch.cat([params[n].detach().to(device=dev, dtype=torch.float32).reshape(-1) for n in param_names(*_depths(params))]).contiguous()


def unpack_block(block: torch.Tensor, nt: int, dt: int, Dt: int, nv: int, dv: int, Dv: int) -> Dict[str, torch.Tensor]:
    """Views of a block (or of a gradient of its shape) under the parameter names."""
    out, at = {}, 0
    for name, shape in zip(param_names(dt, dv), _shapes(nt, dt, Dt, nv, dv, Dv)):
        n = int(np.prod(shape))
        out[name] = block[at:at + n].view(shape)
        at += n
    assert at == block.numel()
    return out


def gpa_weights(epochs: int, mean: float = 30.0, std: float = 30.0) -> np.ndarray:
    """The Gaussian density of (mean, std) at the epochs 1 .. ``epochs``, normalised to sum 1: float64 [epochs] (promptsrc.py:267-271)."""
    epochs = int(epochs)
    if epochs < 1 or not (math.isfinite(mean) and math.isfinite(std) and std > 0.0):
        raise ValueError(f"gpa_weights: epochs={epochs} (>= 1), mean={mean}, std={std} (finite, std > 0)")
    e = np.arange(1, epochs + 1, dtype=np.float64)
    g = (1.0 / (std * np.sqrt(2.0 * np.pi))) * np.exp(-0.5 * ((e - mean) / std) ** 2)
    return g / g.sum()


def promptsrc_head(feats: torch.Tensor, zs_feats: torch.Tensor, text: torch.Tensor, teacher: torch.Tensor, labels: torch.Tensor, scale: float,
                   grad_scale: float, w_text: float, w_image: float, w_logit: float, losses: Optional[torch.Tensor] = None, want_f16: bool = False,
                   ws: Optional[torch.Tensor] = None):
    """clipmi_promptsrc_head: ``(losses fp32 [5] = total, CE, text L1, image L1, logit KL; d_feats fp32 [B, E]; d_text fp32 [C, E])`` and, with
    ``want_f16``, d_text's fp16 copy."""
    B, E = feats.shape
    Cn = text.shape[0]
    dev = feats.device
    if ws is None:
        ws = torch.empty(max(lib.clipmi_promptsrc_head_workspace_bytes(B, E, Cn), 8), dtype=torch.uint8, device=dev)
    losses = torch.empty(5, dtype=torch.float32, device=dev) if losses is None else losses
    d_feats = torch.empty(B, E, dtype=torch.float32, device=dev)
    d_text = torch.empty(Cn, E, dtype=torch.float32, device=dev)
    d16 = torch.empty(Cn, E, dtype=torch.float16, device=dev) if want_f16 else None
    check(lib.clipmi_promptsrc_head(feats.data_ptr(), feats.stride(0), zs_feats.data_ptr(), text.data_ptr(), teacher.data_ptr(), labels.data_ptr(), B, E, Cn,
                                    scale, grad_scale, w_text, w_image, w_logit, losses.data_ptr(), d_feats.data_ptr(), d_text.data_ptr(),
                                    None if d16 is None else d16.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()), "clipmi_promptsrc_head")
    return (losses, d_feats, d_text) + ((d16,) if want_f16 else ())


def promptsrc_step(d_embed: torch.Tensor, d_deep: Optional[torch.Tensor], d_vis: torch.Tensor, block: torch.Tensor, Cn: int, L: int, nt: int, dt: int,
                   Dt: int, nv: int, dv: int, Dv: int, grad_scale: float, buf: Optional[torch.Tensor] = None, lr=None, first_step: bool = True,
                   momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False, apply: bool = True,
                   want_grad: bool = True) -> Optional[torch.Tensor]:
    """clipmi_promptsrc_step: the whole block's gradient (returned with ``want_grad``) and, with ``apply``, SGD's step on ``block`` in place."""
    grad = torch.empty_like(block) if want_grad else None
    check(lib.clipmi_promptsrc_step(d_embed.data_ptr(), None if d_deep is None else d_deep.data_ptr(), d_vis.data_ptr(), block.data_ptr(),
                                    None if buf is None else buf.data_ptr(), None if grad is None else grad.data_ptr(), int(bool(apply)), Cn, L, nt, dt, Dt,
                                    nv, dv, Dv, grad_scale, None if lr is None else lr.data_ptr(), int(first_step), float(momentum), float(dampening),
                                    float(weight_decay), int(bool(nesterov)), ops._stream()), "clipmi_promptsrc_step")
    return grad


def gpa_accumulate(block: torch.Tensor, gpa: torch.Tensor, weight: float, first: bool) -> torch.Tensor:
    """clipmi_gpa_accumulate: ``gpa = weight * block`` (``first``) or ``fma(weight, block, gpa)``, in place on ``gpa``."""
    check(lib.clipmi_gpa_accumulate(block.data_ptr(), gpa.data_ptr(), block.numel(), float(weight), int(bool(first)), ops._stream()), "clipmi_gpa_accumulate")
    return gpa


class _Towers(maplefit._TwoTowers):
    """PromptSRC's and IVLP's towers: the image tower's prompts are the block's own tail, and the frozen plain image forward runs on the
    same handle."""

    def __init__(self, who: str, model, tokenized_prompts, params, seq_rows: Optional[int], class_token_position: str = "end"):
        nt, dt, nv, dv = _check_design(who, model, params, class_token_position)
        Cn, last = _check_ids(who, model, tokenized_prompts, nt)
        super().__init__(who, model, tokenized_prompts, Cn, last, nt, dt, nv, dv, seq_rows)
        self.text_floats = dt * nt * self.Dt
        self.zs = self.head_ws = None

    def shape(self):
        return self.nt, self.dt, self.Dt, self.nv, self.dv, self.Dv

    def image_prompts(self, block: torch.Tensor) -> torch.Tensor:
        return block[self.text_floats:]

    def frozen(self, images: torch.Tensor) -> torch.Tensor:
        """The frozen plain tower's features fp32 [B, E]: no prompt hook whatever the model carries, fp32 residual stream."""
        m, B = self.model, images.shape[0]
        if self.zs is None or self.zs.shape[0] < B:
            self.zs = torch.empty(B, self.E, dtype=torch.float32, device=images.device)
        nbytes = lib.clipmi_vision_workspace_bytes(m._handle, B, 0)
        with m._launch_lock:
            ws = m._workspace("vision", max(nbytes, 256))
            check(lib.clipmi_encode_image(m._handle, images.data_ptr(), _DT[images.dtype], B, None, self.zs.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _lib.CALL_STREAM_F32, ops._stream()), "clipmi_encode_image")
        return self.zs[:B]

    def head_workspace(self, B: int) -> torch.Tensor:
        need = lib.clipmi_promptsrc_head_workspace_bytes(B, self.E, self.C)
        if self.head_ws is None or self.head_ws.numel() < need:
            self.head_ws = torch.empty(max(need, 8), dtype=torch.uint8, device=self.model.device)
        return self.head_ws

    def _step_bytes(self, B: int, scaled: bool) -> int:
        if scaled:
            return lib.clipmi_promptsrc_train_step_scaled_bytes(self.model._handle, self.C, self.text.rows, B, self.nt, self.dt, self.nv, self.dv)
        return lib.clipmi_promptsrc_train_step_bytes(self.model._handle, self.C, self.text.rows, B, self.nt, self.dt, self.nv)


def _method_weights(who: str, method: str, w_text: float, w_image: float, w_logit: float):
    if method not in METHODS:
        raise ValueError(f"{who}: method={method!r} must be one of {METHODS}")
    return (0.0, 0.0, 0.0) if method == "ivlp" else _check_weights(who, w_text, w_image, w_logit)


def gradients(model, params: Dict[str, torch.Tensor], images: torch.Tensor, labels, tokenized_prompts, teacher: torch.Tensor, logit_scale: float = 4.6052,
              w_text: float = 25.0, w_image: float = 10.0, w_logit: float = 1.0, grad_scale: float = DEFAULT_GRAD_SCALE, seq_rows: Optional[int] = None,
              return_operand_stats: bool = False, return_features: bool = False, method: str = "promptsrc", class_token_position: str = "end",
              shard: Optional[Shard] = None):
    """``(losses, grads)`` of PromptSRC's loss on one batch with respect to every prompt parameter, on the GPU: losses fp32 [5] (total, CE,
    text L1, image L1, logit KL; the last three unweighted), grads a dict of fp32 tensors under ``params``' names.  ``images`` [B, 3, R, R]
    preprocessed, ``tokenized_prompts`` [C, context_length] the ids of ``"X .. X name."``, ``teacher`` [C, E] the frozen text features;
    ``seq_rows`` as ``coopfit.context_gradient`` takes it.  ``return_operand_stats`` adds ``{"text": {...}, "vision": {...}}`` as
    ``maplefit.gradients`` does; ``return_features`` adds ``{"text", "feats", "zs"}``, the raw features the head was given.  A diagnostic
    entry point: every call allocates both towers' workspaces and stashes.
    ``shard``: the five losses and the gradients the batch-sharded step would apply, reduced over the ranks in rank order -- the same bits
    on every rank; every rank passes the whole batch; the operand statistics and the features (per rank) are refused."""
    who = "promptsrcfit.gradients"
    gs = fitoptim.static_grad_scale(who, grad_scale, "PromptSRCFitState", "fit_prompts")
    wt, wi, wl = _method_weights(who, method, w_text, w_image, w_logit)
    if shard is not None:
        sharding.check(who, shard, "block", return_operand_stats=return_operand_stats)
        if return_features:
            raise ValueError(f"{who}: shard returns no features (return_features=True): they are per rank")
        state = coopfit.shard_states(lambda sh: PromptSRCFitState(model, tokenized_prompts, params, teacher, logit_scale, w_text, w_image, w_logit, 0.0, 0.0,
                                                                  False, 0.0, gs, seq_rows, method, class_token_position, shard=sh), shard)
        losses, grad = state._shard_gradient(who, images, labels)
        return losses, {k: v.clone() for k, v in state.params(grad).items()}
    scale = fitloop.exp_logit_scale(who, logit_scale)
    tw = _Towers(who, model, tokenized_prompts, params, seq_rows, class_token_position)
    teacher = _check_teacher(who, model, teacher, tw.C)
    images = tw.vision.images(who, images)
    dev = images.device
    labels_d = fitloop.step_labels(who, labels, images.shape[0], tw.C, dev, "images")
    block = pack_block(params, dev)
    zs = tw.frozen(images)
    text, feats = tw.forward(block, images)
    st = torch.zeros(4, dtype=torch.int64, device=dev) if return_operand_stats else None
    sv = torch.zeros(4, dtype=torch.int64, device=dev) if return_operand_stats else None
    losses, d_feats, d_text = promptsrc_head(feats, zs, text, teacher, labels_d, scale, gs, wt, wi, wl)
    d_embed, d_deep, d_vis = tw.backward(d_text, d_feats, st, sv)
    grad = promptsrc_step(d_embed, d_deep, d_vis, block, tw.C, tw.text.L, *tw.shape(), gs, apply=False)
    out = (losses, {k: v.clone() for k, v in unpack_block(grad, *tw.shape()).items()})
    if return_operand_stats:
        out += ({"text": coopfit.operand_stats_dict(st), "vision": coopfit.operand_stats_dict(sv)},)
    if return_features:
        out += ({"text": text.clone(), "feats": feats.clone(), "zs": zs.clone()},)
    return out


class PromptSRCFitState(vptfit._BlockFitState):
    """The training state of PromptSRC's (or IVLP's) prompts: the fp32 master ``block``, SGD's momentum buffer, GPA's running sum, both
    towers' stashes and the number of steps taken.  ``step`` enqueues one forward, backward and update, ``end_epoch`` one accumulation;
    neither synchronises.  ``params()`` names the block's views.  ``validate`` scores validation images on the device
    (``start_monitor``, ``monitor``, ``best_params``, ``val_row_results``; DESIGN.md "Fit monitor", "The image-tower fits")."""
    _who, _n_losses = "PromptSRCFitState", 5

    def __init__(self, model, tokenized_prompts, params: Dict[str, torch.Tensor], teacher: torch.Tensor, logit_scale: float = 4.6052,
                 w_text: float = 25.0, w_image: float = 10.0, w_logit: float = 1.0, momentum: float = 0.9, dampening: float = 0.0,
                 nesterov: bool = False, weight_decay: float = 5e-4, grad_scale: float = DEFAULT_GRAD_SCALE, seq_rows: Optional[int] = None,
                 method: str = "promptsrc", class_token_position: str = "end", scaler: Optional[dict] = None, optimizer: str = "sgd", betas=(0.9, 0.999),
                 eps: float = 1e-8, shard: Optional[Shard] = None):
        who = "PromptSRCFitState"
        self._init_optimiser(who, logit_scale, momentum, dampening, nesterov, weight_decay, grad_scale, scaler, optimizer, betas, eps, shard)
        self.weights = _method_weights(who, method, w_text, w_image, w_logit)
        self.towers = _Towers(who, model, tokenized_prompts, params, seq_rows, class_token_position)
        self.C = self.towers.C
        self.teacher = _check_teacher(who, model, teacher, self.C)
        self._init_block(pack_block(params, model.device))
        self.gpa = None
        self.epochs_seen = 0
        self._scaled_grad = self._grad_block()    # scale * gradient, as clipmi_promptsrc_step leaves it (under shard: the send block's front)

    def params(self, block: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        return unpack_block(self.block if block is None else block, *self.towers.shape())

    def validate(self, val_images_or_loader, val_labels, epoch: int, val_batch_size: int = 32, one_call: bool = True) -> None:
        """Enqueue one validation of the master block as it stands into slot ``epoch`` of the device history; no host read.  The text
        side's training forward runs ONCE on the block, its features are normalised, and the validation images -- [N_val, 3, R, R] on the
        GPU with ``val_labels``, in chunks of ``val_batch_size``, or a sized iterable of (images, labels) batches on the GPU with None --
        run through the image tower's training forward at the block's visual prompts, chunk by chunk (``VPTFitState.validate`` has the
        rest: row results, finish, selection of the whole block, labels).  The frozen tower and the teacher take no part: validation
        scores the prompted model's logits.  After ``apply_gpa`` the block is the aggregate, and that is what is scored."""
        who = "PromptSRCFitState.validate"
        self._no_shard_validate(who)
        mon, tw = self._monitor_for(epoch), self.towers
        text_n = ops.l2_normalize(tw.text_forward(self.block))
        mon.validate(who, tw.vision, tw.image_prompts(self.block), text_n, self.scale, val_images_or_loader, val_labels, epoch, val_batch_size,
                     self.block, one_call)

    def best_params(self) -> Dict[str, torch.Tensor]:
        """The best slot on the device under ``params()``' names: the block of the best epoch so far, or the block ``start_monitor`` saw
        while no epoch has been taken.  GPA's running sum, the optimiser state and the scaler block are not part of it."""
        return self.params(self._best_block("best_params"))

    def _vision(self):
        return self.towers.vision

    def _one_call(self, images, B, labels_d):
        tw = self.towers
        front = tw.one_call_front(images, B, labels_d) + (self.teacher.data_ptr(), self.block.data_ptr(),
                                                          None if self.buf is None else self.buf.data_ptr(), tw.nt, tw.dt, tw.nv, tw.dv)
        return "clipmi_promptsrc_train_step", tw.one_call_workspace(B, self.dynamic), front, self.weights, tw.stashes()

    def _head(self, images, labels_d, grad_scale, losses):
        """The frozen plain tower first; ``losses`` (kept in ``last_losses``): total, CE, text L1, image L1, logit KL."""
        tw = self.towers
        zs = tw.frozen(images)
        text, feats = tw.forward(self.block, images)
        _, d_feats, d_text = promptsrc_head(feats, zs, text, self.teacher, labels_d, self.scale, grad_scale, *self.weights, losses=losses,
                                            ws=tw.head_workspace(images.shape[0]))
        return d_text, d_feats

    def _apply(self, outs, lr_d, first, sgd):
        """Under the dynamic scale and under Adam clipmi_promptsrc_step leaves scale * gradient in ``_scaled_grad`` and applies nothing."""
        tw = self.towers
        d_embed, d_deep, d_vis = tw.backward(*outs)
        grad, buf, gs, lr, first = (self._scaled_grad, None, 1.0, None, 0) if self._defer else (None, self.buf, self.grad_scale, lr_d, first)
        check(lib.clipmi_promptsrc_step(d_embed.data_ptr(), None if d_deep is None else d_deep.data_ptr(), d_vis.data_ptr(), self.block.data_ptr(),
                                        None if buf is None else buf.data_ptr(), None if grad is None else grad.data_ptr(), int(not self._defer), tw.C,
                                        tw.text.L, *tw.shape(), gs, None if lr is None else lr.data_ptr(), int(first), *sgd, ops._stream()),
              "clipmi_promptsrc_step")
        return grad

    def end_epoch(self, weight: float) -> None:
        """GPA: add ``weight`` times the block as it stands to the running sum (one launch; the first call initialises the sum).  Under
        ``shard`` every rank keeps its own sum of the same bits; with a ``LocalGather`` this call serves all the world's states, as
        ``step`` does."""
        for s in sharding.world_states(self.shard, self, "PromptSRCFitState.end_epoch"):
            if s.gpa is None:
                s.gpa = torch.empty_like(s.block)
            gpa_accumulate(s.block, s.gpa, weight, s.epochs_seen == 0)
            s.epochs_seen += 1

    def apply_gpa(self) -> None:
        """The running sum replaces the parameters (after the last epoch)."""
        for s in sharding.world_states(self.shard, self, "PromptSRCFitState.apply_gpa"):
            if s.gpa is not None:
                s.block.copy_(s.gpa)


def _gpa_for(who: str, gpa, epochs: int) -> Optional[np.ndarray]:
    if gpa is None or epochs < 1:
        return None
    if isinstance(gpa, (tuple, list)) and len(gpa) == 2:
        return gpa_weights(epochs, float(gpa[0]), float(gpa[1]))
    w = np.asarray(gpa, np.float64)
    if w.shape != (epochs,):
        raise ValueError(f"{who}: gpa must be None, (mean, std) or {epochs} weights, got {gpa!r}")
    return w


def init_params(model, seed: int = 0) -> Dict[str, torch.Tensor]:
    """The model's own prompt tokens (copies) and a ``ctx`` from N(0, 0.02^2) of the model's ``language_ctx`` rows."""
    nt = int(model.design_details.get("language_ctx", 0))
    if nt < 1:
        raise ValueError("promptsrcfit: the model's design_details carry no language_ctx")
    ctx = 0.02 * torch.randn(nt, int(model.geometry.transformer_width), generator=torch.Generator().manual_seed(seed))
    return {k: v.detach().float().clone() for k, v in model_params(model, ctx).items()}


def fit_prompts(images_or_loader, labels, model, tokenized_prompts, teacher: torch.Tensor, params: Optional[Dict[str, torch.Tensor]] = None,
                method: str = "promptsrc", logit_scale: float = 4.6052, lr: float = 0.0025, epochs: int = 50, batch_size: int = 4,
                momentum: float = 0.9, dampening: float = 0.0, weight_decay: float = 5e-4, nesterov: bool = False, w_text: float = 25.0, w_image: float = 10.0,
                w_logit: float = 1.0, gpa=(30.0, 30.0), grad_scale: float = DEFAULT_GRAD_SCALE, seq_rows: Optional[int] = None,
                lr_per_epoch: Optional[Sequence[float]] = None, drop_last: bool = False, return_history: bool = False, one_call: bool = False,
                class_token_position: str = "end", scaler: Optional[dict] = None, optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8,
                shard: Optional[Shard] = None, val=None, val_batch_size: int = 32, val_bins: int = 10, final_model: str = "last_step", val_criterion: str = "accuracy",
                return_monitor: bool = False):
    """Train the prompts starting from ``params`` (not modified; None = ``init_params(model)``): ``epochs`` passes of
    ``torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov)`` over the whole parameter list on PromptSRC's loss.
    ``images_or_loader`` is a tensor of preprocessed images [N, 3, R, R] with ``labels`` [N], cut into batches of ``batch_size`` in order
    (the last one short unless ``drop_last``), or a sized iterable of (images, labels) batches iterated once per epoch (``labels`` None,
    ``batch_size`` unused).  ``lr_per_epoch`` gives every epoch's rate; None takes ``cosine_warmup_schedule(lr, epochs)``.  ``gpa``:
    ``(mean, std)`` of ``gpa_weights``, or the epochs' weights themselves, or None for the last epoch's parameters;
    ``method="ivlp"`` sets the three weights to 0 and ``gpa`` to None.  Three towers run on every step; nothing synchronises until the one
    wait at the end.  Returns the fitted parameters, a dict of fp32 tensors on the device (views of one block), or ``(params, per-step
    total losses)`` with ``return_history``.  The model's parameters are NOT written: ``trainers.promptsrc.CustomCLIP.fit_prompts`` does
    that.  ``grad_scale="dynamic"`` with ``scaler`` (module docstring; both methods): a step that overflows fp16 is skipped on the device
    and the scale adapts; the history keeps one loss per step, skipped steps included, GPA aggregates whatever the block holds at the end
    of an epoch, and the run still synchronises once.

    ``val=(val_images_or_loader, val_labels)``, ``val_batch_size``, ``val_bins``, ``final_model``, ``val_criterion`` and
    ``return_monitor`` as ``vptfit.fit_prompts`` takes them.  Behind every epoch the GPA work comes first and the validation second, the
    reference's order (promptsrc.py:321-336 inside ``forward_backward``, ahead of Dassl's ``after_epoch``): epochs 0 .. E-2 score the
    block the epoch trained, the last epoch scores the aggregate GPA has just loaded.  The fitted parameters are bit for bit those of the
    same call without ``val``; "best_val" returns the best epoch's block (the aggregate when the last epoch is the best).

    ``optimizer``, ``betas``, ``eps``: "sgd" (the default; ``momentum``, ``dampening``, ``nesterov``), "adam" or
    "adamw", as ``coopfit.fit_context`` takes them; ``weight_decay`` keeps this fit's default of 5e-4 under all three (torch's AdamW
    default of 1e-2 is NOT taken over).  ``one_call=True`` with an Adam optimiser is refused.  DESIGN.md "Adam steps for the prompt fits".

    ``shard=coopfit.Shard(world, rank, gather)``: the batch-sharded fit as ``vptfit.fit_prompts`` takes it (DESIGN.md "Batch-sharded
    image-tower fits"; the reference's ``nn.DataParallel``, promptsrc.py:278), both methods.  Only the image batch is sharded: the text
    tower runs over all C prompts on every rank, and every rank keeps GPA's sum.  ``one_call=True`` is refused as well."""
    who = "fit_prompts"
    if shard is not None:
        sharding.check(who, shard, "block", one_call=one_call, val=val, final_model=final_model)
    fitmonitor.check_image_args(who, val, val_batch_size, val_bins, final_model, val_criterion)
    epochs = int(epochs)
    if epochs < 0:
        raise ValueError(f"{who}: epochs={epochs} (>= 0)")
    if method not in METHODS:
        raise ValueError(f"{who}: method={method!r} must be one of {METHODS}")
    if optimizer != "sgd":      # by this function's name; SGD's arguments are the state's to check, as before
        fitloop.check_optimizer(who, optimizer, momentum, dampening, nesterov, weight_decay, betas, eps, one_call=one_call)
    if params is None:
        params = init_params(model)
    sharding.check_batches(who, shard, images_or_loader, batch_size, drop_last)
    state = coopfit.shard_states(lambda sh: PromptSRCFitState(model, tokenized_prompts, params, teacher, logit_scale, w_text, w_image, w_logit, momentum,
                                                              dampening, nesterov, weight_decay, grad_scale, seq_rows, method, class_token_position, scaler,
                                                              optimizer, betas, eps, sh), shard)
    weights = None if method == "ivlp" else _gpa_for(who, gpa, epochs)

    batches = fitloop.cut_batches(who, images_or_loader, labels, state.C, batch_size, drop_last, model.device)
    monitored = val is not None and epochs * len(batches) > 0

    def end_epoch(e: int) -> None:
        """GPA: the epoch's weighted block joins the running sum; behind the last epoch the sum replaces the parameters.  Then the
        validation, of the block as it stands."""
        if weights is not None:
            state.end_epoch(float(weights[e]))
            if e == epochs - 1:
                state.apply_gpa()
        if monitored:
            state.validate(val[0], val[1], e, val_batch_size)

    if monitored:
        state.start_monitor(epochs, val_bins, val_criterion=val_criterion, select=final_model == "best_val")
    _, lr_steps = fitloop.schedule(who, lr, epochs, lr_per_epoch, len(batches), model.device)
    history = fitloop.run_batches(lambda e, k, b, r, want: state.step(b[0], b[1], r, want_loss=want, one_call=one_call), batches, epochs, lr_steps, return_history,
                                  None if weights is None and not monitored else end_epoch)
    out = state.best_params() if final_model == "best_val" and monitored else state.params()
    return fitmonitor.pack(out, history, fitmonitor.returned_monitor(state, monitored, val_bins, return_monitor),
                           return_history, return_monitor)
