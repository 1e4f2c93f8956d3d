"""VPT's visual prompts trained on the GPU (reference trainers/classification/vpt.py; clip/model.py VisionTransformer with prompt rows).

The reference trains the prompt tokens inside the image tower -- ``visual.VPT`` [n_ctx, Dv], appended behind the patch rows after the
positional embedding, and ``visual.transformer.resblocks.{i}.VPT_shallow`` [n_ctx, Dv] for 1 <= i < depth, which overwrite the last
``n_ctx`` token rows before block i -- against fixed text features: every step runs the image tower on the batch, normalises, takes
``F.cross_entropy`` of ``exp(logit_scale)`` times the cosine and one ``torch.optim.SGD`` step on the prompts.  The prompts reach the loss
only through the image tower, so a step needs that tower's backward.  csrc/vision_backward.hip computes it with the tower frozen: a
training forward that keeps what the backward needs in a stash, and the backward (every Linear's backward is the forward's fp16 GEMM on
a transposed copy of the weight, packed once per bound model; the attention backward is ``clipmi_attention_backward_full``);
csrc/prompt_train.hip has the image-side loss head and the SGD step -- no autograd graph.  fp16 GEMM operands, fp32 accumulation, fp32
residual and gradient streams, an fp32 master block ``[depth, n_ctx, Dv]`` of the prompts (slot 0 is ``visual.VPT``); the forward reads
the masters rounded through fp16, the reference's ``.half()``.  DESIGN.md "VPT fit" has the data flow.

``grad_scale``: as in ``coopfit`` -- the whole backward carries ``grad_scale`` times the gradient (a power of two), the head multiplies
and the step divides.  profiles/vptfit_parity.txt has the measurement behind the default.  ``grad_scale="dynamic"`` with
``scaler=dict(init_scale, growth_factor, backoff_factor, growth_interval)`` is the reference's ``prec == "amp"`` branch (vpt.py:164,
``torch.cuda.amp.GradScaler``) as ``coopfit`` describes it and ``fitoptim`` holds it for every fit: the scale lives in a block on the
device, a step whose gradient holds an inf or a NaN changes neither the prompts nor the momentum buffer, and the scale backs off and grows again.  No step reads anything back;
``VPTFitState.scaler_state()`` does, once.  DESIGN.md "Dynamic loss scale for the block fits"; the reference's ``autocast`` casts differ
from this path's fixed fp16 operand points (unverified).

``prompt_gradient`` returns one batch's loss and gradient (the diagnostic entry point of the tests).  ``VPTFitState.step`` takes one
batch of preprocessed images; ``fit_prompts`` runs epochs over a tensor of images or a loader of (images, labels) batches and enqueues
every step with one synchronisation at the end.  The image tower runs on every step: nothing is cached.

The defaults -- SGD at 0.0025 with momentum 0.9 and weight decay 5e-4, 5 epochs, a constant warm-up epoch handing over to a cosine
schedule -- restate the reference's VPT config and Dassl's public defaults and are UNVERIFIED here; each is an argument.

ViT-L lengths: by default the backward takes at most 224 token rows per image (tokens + prompt rows).  With the library option
``vision_train_long`` at 1 (``_lib.set_option``, CLIPMI_VISION_TRAIN_LONG; opt-in until measured on real checkpoints) it takes 640 --
ViT-L/14's 257 and 577 tokens with their prompt rows -- through ``clipmi_attention_backward_long``; ``max_rows()`` is the limit in
force, for ``maplefit`` and ``promptsrcfit`` as well, and ``stash_bytes(model, batch, n_ctx)`` the workspace and stash a batch needs
(DESIGN.md "Long attention backward").  The training forward takes any patch size that divides the resolution: patches of 8, 16 and 32
pixels through the im2col-free loader, every other size -- ViT-L/14's and ViT-L/14@336px's patches of 14 -- through the inference pass's
patchify + GEMM route, whose im2col matrix takes the place of the fp16 image copy in the workspace (``stash_bytes`` reports it).  With
the option on, real ViT-L/14 towers train here, in ``maplefit`` and in ``promptsrcfit``, monitored validation included.

``shard=coopfit.Shard(world, rank, gather)`` on ``VPTFitState``, ``fit_prompts`` and ``prompt_gradient``: the batch-sharded fit, this
project's form of the reference's ``nn.DataParallel`` (vpt.py:171), shared with ``maplefit`` and ``promptsrcfit`` through
``_BlockFitState``.  One process per GPU; every rank is given the whole batch and runs the tower over its own B / G rows; one all-gather
moves the ranks' blocks ``[scale * gradient | losses]``, clipmi_block_rank_mean (csrc/shard_train.hip) forms their rank-ordered mean and
the unsharded route's step applies it, so every rank ends a step with the same bits; with ``world == 1`` they are the unsharded bits.
All three optimisers and both loss scales.  Refused, each by name: a batch that is no multiple of ``world``, ``one_call=True``,
``val=`` / ``final_model="best_val"`` / ``validate``, ``return_operand_stats``.  DESIGN.md "Batch-sharded image-tower fits".

Not covered (MaPLe trains through ``maplefit`` and PromptSRC / IVLP through ``promptsrcfit``, on this tower): ``nn.DataParallel`` itself
in one process (``shard=`` stands in for it), the ResNet towers.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib, fitloop, fitmonitor, fitoptim, ops
from . import shard as sharding
from ._lib import _DT, check, lib
from .coopfit import _pack_dgrad, operand_stats_dict
from .fitloop import _need_gpu
from .shard import Shard, shard_states

# 2^12: CoOp's value (profiles/coopfit_parity.txt) holds for the image tower's backward at the ViT-B/16 geometry as well
# (profiles/vptfit_parity.txt, "grad_scale").  A model with much larger gradients overflows fp16 at this scale -- the prompts then turn
# NaN, they do not go wrong silently; pass a smaller power of two.
DEFAULT_GRAD_SCALE = 4096.0
MAX_ROWS = 224         # token rows per image that clipmi_vision_encoder_backward takes by default (clipmi_attention_backward_full's limit)
MAX_ROWS_LONG = 640    # with the library option vision_train_long = 1 (clipmi_attention_backward_long's limit)


def max_rows() -> int:
    """Token rows per image (tokens + prompt rows) that the image tower's training path takes now: 224, or 640 with the library option
    ``vision_train_long`` (``_lib.set_option``, CLIPMI_VISION_TRAIN_LONG) at 1."""
    return MAX_ROWS_LONG if _lib.get_option("vision_train_long") else MAX_ROWS


def check_rows(who: str, tokens: int, n_ctx: int) -> None:
    """The refusal ``vptfit``, ``maplefit`` and ``promptsrcfit`` share."""
    limit = max_rows()
    if tokens + n_ctx > limit:
        raise ValueError(f"{who}: {tokens} tokens + {n_ctx} prompt rows = {tokens + n_ctx} rows per image; the backward takes at most {limit}")


def stash_bytes(model, batch: int, n_ctx: int):
    """``(workspace_bytes, stash_bytes)`` of the image tower's training path for ``batch`` images with ``n_ctx`` prompt rows
    (clipmi_vision_train_bytes): the stash grows with rows x layers x width -- 49 fp32 streams, 24 qkv and 24 c_fc outputs at ViT-L/14."""
    model._ensure_bound()
    wsb, stb = C.c_size_t(0), C.c_size_t(0)
    check(lib.clipmi_vision_train_bytes(model._handle, int(batch), int(n_ctx), C.byref(wsb), C.byref(stb)), "clipmi_vision_train_bytes")
    return wsb.value, stb.value


def model_prompts(model) -> torch.Tensor:
    """The model's own prompt parameters as one fp32 block [depth, n_ctx, Dv] (slot 0: ``visual.VPT``), after the checks of the design."""
    who = "vptfit"
    if getattr(model, "is_resnet", False):
        raise ValueError(f"{who}: prompt tokens apply to the ViT towers only (the ResNet tower has none)")
    dd = model.design_details
    if dd.get("trainer") != "VPT" or int(dd.get("vision_depth", 0)) < 1:
        raise ValueError(f"{who}: needs a CLIP built with design_details trainer='VPT' and vision_depth >= 1, got trainer={dd.get('trainer')!r}")
    shallow, deep = model.ivlp_vision_prompts()
    if shallow is None:
        raise ValueError(f"{who}: the model carries no visual.VPT")
    return torch.stack([shallow.detach().float()] + [p.detach().float() for p in deep])


def _check_prompts(who: str, model, prompts: torch.Tensor):
    model_prompts(model)     # the design's checks
    g = model.geometry
    own, _ = model.ivlp_vision_prompts()
    if not isinstance(prompts, torch.Tensor) or prompts.dim() != 3 or prompts.shape[2] != g.vision_width or not prompts.dtype.is_floating_point:
        raise ValueError(f"{who}: prompts {tuple(getattr(prompts, 'shape', ()))} must be [depth, n_ctx, {g.vision_width}]")
    depth, n_ctx = int(prompts.shape[0]), int(prompts.shape[1])
    if n_ctx != int(own.shape[0]):
        raise ValueError(f"{who}: n_ctx={n_ctx} does not match the model's visual.VPT ({int(own.shape[0])} rows)")
    if not 1 <= depth <= g.vision_layers:
        raise ValueError(f"{who}: depth={depth} for {g.vision_layers} layers")
    tokens = (g.image_resolution // g.vision_patch_size) ** 2 + 1
    check_rows(who, tokens, n_ctx)
    return depth, n_ctx


def _dgrad(model):
    """The transposed fp16 copies of the frozen image tower's weights (clipmi_vision_dgrad), packed once per bound model and again when a
    vision weight's version moves."""
    model._ensure_bound()
    return _pack_dgrad(model, model.visual.transformer.resblocks, model.visual.proj, _lib.VisionDgrad, "_vpt_dgrad")


def _check_text(who: str, model, text_features) -> torch.Tensor:
    E = int(model.geometry.embed_dim)
    if not isinstance(text_features, torch.Tensor) or text_features.dim() != 2 or text_features.shape[0] < 2 or text_features.shape[1] != E:
        raise ValueError(f"{who}: text_features {tuple(getattr(text_features, 'shape', ()))} must be [C >= 2, E = {E}]")
    _need_gpu(text_features, "text_features")
    return text_features.detach().to(torch.float32).contiguous()


class _Tower:
    """The frozen image tower in training mode: workspace, stash, features and the prompts' gradient for batches of up to ``B`` images."""

    def __init__(self, who: str, model, depth: int, n_ctx: int):
        dev = model.device
        if dev.type != "cuda":
            raise RuntimeError(f"clipmi: {who} needs the model on a ROCm GPU (model.to('cuda')); the HIP path has no CPU fallback")
        if dev.index != torch.cuda.current_device():
            raise RuntimeError(f"clipmi: the model is on {dev} but the current device is cuda:{torch.cuda.current_device()}")
        self.model, self.depth, self.n_ctx = model, depth, n_ctx
        g = model.geometry
        self.D, self.E, self.R = g.vision_width, g.embed_dim, g.image_resolution
        model._ensure_bound()
        self.dgrad = _dgrad(model)
        self.B = self.ws_B = 0
        self.ws = self.stash = self.feats = self.step_ws = None
        self.step_key = None
        self.val_ws = None      # clipmi_vision_val_chunk's workspace
        self.d_prompts = torch.empty(depth, n_ctx, self.D, dtype=torch.float32, device=dev)

    def images(self, who: str, images) -> torch.Tensor:
        images = ops._dev(images, "images", (torch.float16, torch.float32))
        if images.dim() != 4 or tuple(images.shape[1:]) != (3, self.R, self.R) or images.shape[0] < 1:
            raise ValueError(f"{who}: expected images [B >= 1, 3, {self.R}, {self.R}], got {tuple(images.shape)}")
        return images

    def size(self, B: int, tower_ws: bool = True) -> None:
        """Room for a batch of ``B``: the stash always, the separate calls' workspace and feature rows only with ``tower_ws``."""
        dev = self.model.device
        wsb, stb = C.c_size_t(0), C.c_size_t(0)
        if B > self.B or (tower_ws and B > self.ws_B):
            check(lib.clipmi_vision_train_bytes(self.model._handle, B, self.n_ctx, C.byref(wsb), C.byref(stb)), "clipmi_vision_train_bytes")
        if B > self.B:
            self.stash = torch.empty(max(stb.value, 256), dtype=torch.uint8, device=dev)
            self.B = B
        if tower_ws and B > self.ws_B:
            self.ws = torch.empty(max(wsb.value, 256), dtype=torch.uint8, device=dev)
            self.feats = torch.empty(B, self.E, dtype=torch.float32, device=dev)
            self.ws_B = B

    def forward(self, images: torch.Tensor, prompts: torch.Tensor, flags: int = _lib.CALL_DEFAULT) -> torch.Tensor:
        m, B = self.model, images.shape[0]
        self.size(B)
        with m._launch_lock:
            check(lib.clipmi_vision_encoder_train(m._handle, images.data_ptr(), _DT[images.dtype], B, prompts.data_ptr(), self.n_ctx, self.depth,
                                                  self.feats.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self.stash.data_ptr(), self.stash.numel(),
                                                  int(flags), ops._stream()), "clipmi_vision_encoder_train")
        return self.feats[:B]

    def backward(self, d_feats: torch.Tensor, stats: Optional[torch.Tensor] = None) -> torch.Tensor:
        m, B = self.model, d_feats.shape[0]
        with m._launch_lock:
            check(lib.clipmi_vision_encoder_backward(m._handle, C.byref(self.dgrad[0]), d_feats.data_ptr(), B, self.n_ctx, self.depth,
                                                     self.d_prompts.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self.stash.data_ptr(),
                                                     self.stash.numel(), None if stats is None else stats.data_ptr(), ops._stream()),
                  "clipmi_vision_encoder_backward")
        return self.d_prompts

    def val_chunk(self, mon, images: torch.Tensor, prompts: torch.Tensor, text_n: torch.Tensor, scale: float, labels_d: torch.Tensor, n_bins: int,
                  rows: torch.Tensor, row0: int, one_call: bool = True) -> None:
        """One chunk of validation images into ``rows[row0 : row0 + B]`` (``fitmonitor.ImageMonitor``): the training forward at ``prompts``,
        the features normalised, the cosine logits against ``text_n`` [C, E] at ``scale`` and ``ops.val_score_rows`` --
        clipmi_vision_val_chunk, or with ``one_call=False`` the four calls, which give the same bits.  The stash is overwritten, as a
        training step's forward overwrites it."""
        m, B, Cn = self.model, images.shape[0], int(text_n.shape[0])
        if not one_call:
            feats = self.forward(images, prompts)
            feats_n, logits = mon.logits_for(B, Cn, self.E, images.device)
            check(lib.clipmi_l2_normalize(feats.data_ptr(), _lib.F32, feats_n.data_ptr(), B, self.E, ops._stream()), "clipmi_l2_normalize")
            check(lib.clipmi_logits(feats_n.data_ptr(), text_n.data_ptr(), scale, None, logits.data_ptr(), None, None, B, Cn, self.E, ops._stream()),
                  "clipmi_logits")
            ops.val_score_rows(logits, labels_d, n_bins, rows, row0)
            return
        self.size(B, tower_ws=False)
        need = lib.clipmi_vision_val_chunk_bytes(m._handle, B, self.n_ctx, Cn)
        if self.val_ws is None or self.val_ws.numel() < need:
            self.val_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=m.device)
        pr = ops._row_results("val_chunk", rows, B, row0)
        with m._launch_lock:
            check(lib.clipmi_vision_val_chunk(m._handle, images.data_ptr(), _DT[images.dtype], B, prompts.data_ptr(), self.n_ctx, self.depth,
                                              text_n.data_ptr(), Cn, scale, labels_d.data_ptr(), n_bins, pr, self.val_ws.data_ptr(), self.val_ws.numel(),
                                              self.stash.data_ptr(), self.stash.numel(), ops._stream()), "clipmi_vision_val_chunk")

    def one_call_workspace(self, B: int, n_cls: int, scaled: bool = False) -> torch.Tensor:
        if scaled:
            need = lib.clipmi_vpt_train_step_scaled_bytes(self.model._handle, B, self.n_ctx, self.depth, n_cls)
        else:
            need = lib.clipmi_vpt_train_step_bytes(self.model._handle, B, self.n_ctx, n_cls)
        if self.step_ws is None or self.step_ws.numel() < need:
            self.step_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.model.device)
        return self.step_ws


def vpt_head(feats: torch.Tensor, labels: torch.Tensor, text: torch.Tensor, scale: float, grad_scale: float, loss: Optional[torch.Tensor] = None):
    """clipmi_vpt_head: ``(loss fp32 [1], d_feats fp32 [B, E])`` of the batch (include/clipmi.h)."""
    B, E = feats.shape
    Cn = text.shape[0]
    need = lib.clipmi_vpt_head_workspace_bytes(B, E, Cn)
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=feats.device)
    loss = torch.empty(1, dtype=torch.float32, device=feats.device) if loss is None else loss
    d_feats = torch.empty(B, E, dtype=torch.float32, device=feats.device)
    check(lib.clipmi_vpt_head(feats.data_ptr(), feats.stride(0), labels.data_ptr(), text.data_ptr(), B, E, Cn, scale, grad_scale, loss.data_ptr(),
                              d_feats.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()), "clipmi_vpt_head")
    return loss, d_feats


def vpt_step(d_prompts: torch.Tensor, grad_scale: float, prompts: Optional[torch.Tensor] = None, buf: Optional[torch.Tensor] = None, lr=None,
             first_step: bool = True, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False,
             want_grad: bool = True) -> Optional[torch.Tensor]:
    """clipmi_vpt_step: the gradient ``d_prompts / grad_scale`` (returned with ``want_grad``) and, with ``prompts``, SGD's step in place."""
    depth, n_ctx, D = d_prompts.shape
    grad = torch.empty_like(d_prompts) if want_grad else None
    check(lib.clipmi_vpt_step(d_prompts.data_ptr(), None if prompts is None else prompts.data_ptr(), None if buf is None else buf.data_ptr(),
                              None if grad is None else grad.data_ptr(), depth, n_ctx, D, grad_scale, None if lr is None else lr.data_ptr(),
                              int(first_step), float(momentum), float(dampening), float(weight_decay), int(bool(nesterov)), ops._stream()),
          "clipmi_vpt_step")
    return grad


def prompt_gradient(model, prompts: torch.Tensor, images: torch.Tensor, labels, text_features: torch.Tensor, logit_scale: float = 4.6052,
                    grad_scale: float = DEFAULT_GRAD_SCALE, return_operand_stats: bool = False, flags: int = _lib.CALL_DEFAULT,
                    shard: Optional[Shard] = None):
    """``(loss, grad)`` of ``F.cross_entropy(exp(logit_scale) * normalise(encode_image(images; prompts)) @ normalise(text_features).T,
    labels)`` with respect to ``prompts`` [depth, n_ctx, Dv] (slot 0: ``visual.VPT``), on the GPU: loss fp32 [1], grad fp32 of the block's
    shape.  ``return_operand_stats`` adds a dict over every fp16 dgrad-GEMM operand element: ``elements``, ``zeros``, ``subnormals``,
    ``max`` -- the measurement behind the default ``grad_scale``.  A diagnostic entry point: every call allocates a workspace and a stash
    of its own (41.6 MB per image at ViT-B/16 with 8 prompt rows); a training loop keeps a ``VPTFitState``.

    ``shard``: the loss and the gradient the batch-sharded step would apply (module docstring), reduced over the ranks in rank order --
    the same bits on every rank.  Every rank passes the whole batch; the operand statistics are per rank and are not returned, and the
    forward takes the default ``flags``."""
    who = "prompt_gradient"
    depth, n_ctx = _check_prompts(who, model, prompts)
    gs = fitoptim.static_grad_scale(who, grad_scale, "VPTFitState", "fit_prompts")
    if shard is not None:
        sharding.check(who, shard, "block", return_operand_stats=return_operand_stats)
        if flags != _lib.CALL_DEFAULT:
            raise ValueError(f"{who}: shard takes the default call flags (flags={flags})")
        state = shard_states(lambda sh: VPTFitState(model, text_features, logit_scale, prompts, 0.0, 0.0, False, 0.0, gs, shard=sh), shard)
        losses, grad = state._shard_gradient(who, images, labels)
        return losses[:1], grad
    scale = fitloop.exp_logit_scale(who, logit_scale)
    text = _check_text(who, model, text_features)
    tower = _Tower(who, model, depth, n_ctx)
    images = tower.images(who, images)
    dev = images.device
    labels_d = fitloop.step_labels(who, labels, images.shape[0], text.shape[0], dev, "images")
    master = fitloop.master(prompts, dev)
    feats = tower.forward(images, master, flags)
    stats = torch.zeros(4, dtype=torch.int64, device=dev) if return_operand_stats else None
    loss, d_feats = vpt_head(feats, labels_d, text, scale, gs)
    grad = vpt_step(tower.backward(d_feats, stats), gs)
    if not return_operand_stats:
        return loss, grad
    return loss, grad, operand_stats_dict(stats)


def image_features(model, prompts: torch.Tensor, images: torch.Tensor) -> torch.Tensor:
    """The raw image features fp32 [B, E] of the training forward at ``prompts``: what the loss head is given.  Allocates a workspace and
    a stash per call, as ``prompt_gradient`` does."""
    who = "image_features"
    depth, n_ctx = _check_prompts(who, model, prompts)
    tower = _Tower(who, model, depth, n_ctx)
    images = tower.images(who, images)
    return tower.forward(images, fitloop.master(prompts, images.device)).clone()


class _BlockFitState(fitmonitor.ImageMonitored, fitoptim.Optimised):
    """What the states of the fits through the image tower share (VPTFitState, maplefit.MaPLeFitState, promptsrcfit.PromptSRCFitState): one
    fp32 master block under ``_master_name``, the one ``step`` and the batch-sharded step; the optimiser's arguments and moments, the static
    or dynamic loss scale and ``scaler_state`` are ``fitoptim.Optimised``'s.  A state supplies ``_vision`` (the image tower), ``_one_call`` (its one-call symbol and that symbol's own arguments), ``_head`` (forward
    and head at a grad_scale) and ``_apply`` (backward and the block's step)."""
    _master_name = "block"
    _n_losses = 1

    def _init_optimiser(self, who: str, logit_scale: float, momentum, dampening, nesterov, weight_decay: float, grad_scale, scaler,
                        optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8, shard: Optional[Shard] = None) -> None:
        """``shard``: the batch-sharded fit (``shard.check``), which takes all three optimisers; then ``fitoptim.Optimised``'s refusals."""
        self.shard = shard
        if shard is not None:
            sharding.check(who, shard, "block")
        super()._init_optimiser(who, logit_scale, momentum, dampening, nesterov, weight_decay, grad_scale, scaler, optimizer, betas, eps)
        # the block's step entry forms the gradient at grad_scale = 1 and applies nothing: under the dynamic scale, under Adam, and
        # under ``shard``, where the block it leaves is what the rank sends
        self._defer = self.dynamic or self.optimizer != "sgd" or shard is not None

    def _init_block(self, master: torch.Tensor) -> None:
        """``master`` becomes the block the steps update (``_init_moments`` beside it).  Under ``shard`` also the step's send block
        [scale * gradient | losses], the receive block [G, the same] and the reduced block, made once; the state files itself with a
        local gather."""
        setattr(self, self._master_name, master)
        self._init_moments(master)
        if self.shard is not None:
            n = master.numel() + self._n_losses
            stride = (n + 3) // 4 * 4       # whole 16-byte vectors per rank: every row of the receive block starts on the first row's phase
            self._send = torch.zeros(stride, dtype=torch.float32, device=master.device)
            self._recv = torch.empty(self.shard.world, stride, dtype=torch.float32, device=master.device)
            self._reduced = torch.empty(n, dtype=torch.float32, device=master.device)
            sharding.file_state(self.shard, self)

    def _grad_block(self) -> Optional[torch.Tensor]:
        """Where a deferred step entry leaves scale * gradient: the front of the send block under ``shard``, a block of the state's own
        under the dynamic scale and under Adam, nothing on the static SGD route (the entry applies the step itself)."""
        master = self._master()
        if self.shard is not None:
            return self._send[:master.numel()].view_as(master)
        return torch.empty_like(master) if self._defer else None

    def _master(self) -> torch.Tensor:
        return getattr(self, self._master_name)

    def step(self, images: torch.Tensor, labels, lr, want_loss: bool = False, one_call: bool = False) -> Optional[torch.Tensor]:
        """One optimiser step on the batch ``images`` [B, 3, R, R] (preprocessed, fp16 or fp32, on the GPU) and ``labels`` [B] at the rate
        ``lr``: an fp32 tensor of one element on the device is read where it lies; a Python number is uploaded on every call.  A label
        tensor on the GPU is taken as it is -- a label outside [0, C) then makes the parameters NaN, it is never used as an address; host
        labels are range-checked.  ``one_call``: the same launches through the fit's one-call symbol, whose workspace holds the towers'
        (the separate calls' workspace is then not allocated; the stashes are the same).  Returns the batch loss, fp32 [1] on the device
        (the first of the head's losses, all kept in ``last_losses``), when ``want_loss``.  Under ``grad_scale="dynamic"`` the head runs at
        ``grad_scale = 1``, the head's output gradients are multiplied by the device block's scale, the gradient block is formed without
        being applied and clipmi_block_step_scaled decides on the device whether the step is applied (one call: the ``_scaled`` symbol);
        a skipped step still counts in ``steps`` and still returns its loss; whether it was applied is in ``scaler_state()``.  Under
        ``optimizer="adam" | "adamw"`` the gradient block is formed the same way -- at ``grad_scale = 1``, not applied -- and
        clipmi_block_step_adam divides it by ``grad_scale`` and applies the rule (clipmi_block_step_adam_scaled under the dynamic scale);
        ``one_call`` is then refused: the one-call steps stay SGD.  Under ``shard`` every rank is given the WHOLE batch (B a multiple of
        the world size) and steps on its own B / G rows, views of it; ``last_losses`` and the returned loss are the reduced ones, the
        same bits on every rank; ``one_call`` is refused; under a ``LocalGather`` the step of one state steps them all."""
        who = f"{self._who}.step"
        if self.shard is not None:
            sharding.check(who, self.shard, "block", one_call=one_call)
        self._no_one_call_adam(who, one_call)
        v = self._vision()
        images = v.images(who, images)
        dev, B = images.device, images.shape[0]
        if self.shard is not None:
            sharding.check_batch(who, self.shard, B)
        labels_d = fitloop.step_labels(who, labels, B, self.C, dev, "images")
        lr_d = ops._dev(fitloop.lr_operand(lr, dev), "lr", (torch.float32,))
        if self.shard is not None:
            # every rank is given the same batch; under a local gather this call steps all the world's states, one phase at a time
            sharding.step_all(sharding.drive(self.shard, self, who), self, lambda s: s._shard_phases(images, labels_d, lr_d))
            self.steps += 1
            return self.last_losses[:1] if want_loss else None
        first, sgd = self.steps == 0, self._sgd
        loss = torch.empty(self._n_losses, dtype=torch.float32, device=dev)
        if one_call:
            v.size(B, tower_ws=False)
            stem, ws, front, weights, stashes = self._one_call(images, B, labels_d)
            if self.dynamic:
                name, how, rate = stem + "_scaled", (self._scaler.block.data_ptr(), *self._scaler.args()), (lr_d.data_ptr(),)
            else:
                name, how, rate = stem, (self.grad_scale,), (lr_d.data_ptr(), int(first))
            with v.model._launch_lock:
                check(getattr(lib, name)(*front, self.scale, *how, *weights, *rate, *sgd, loss.data_ptr(), None, ws.data_ptr(), ws.numel(), *stashes,
                                         ops._stream()), name)
        else:
            outs = self._head(images, labels_d, self._head_scale, loss)
            self._scale_rows(*outs)
            grad = self._apply(outs, lr_d, first, sgd)      # static SGD: the block's step entry has applied the step itself
            if self._defer:     # the block of grad_scale * gradient (the scaler's scale * gradient under the dynamic scale): Adam is told which
                self._apply_block(grad, lr_d, None, self._head_scale)
        self.steps += 1
        self.last_losses = loss
        return loss[:1] if want_loss else None

    # ---- the batch-sharded step (csrc/shard_train.hip, DESIGN.md "Batch-sharded image-tower fits")

    def _no_shard_validate(self, who: str) -> None:
        if self.shard is not None:
            raise ValueError(f"{who}: shard has no validation (validate: the sharded fit scores nothing between epochs)")

    def _shard_phases(self, images: torch.Tensor, labels_d: torch.Tensor, lr_d: Optional[torch.Tensor], report: Optional[dict] = None):
        """One sharded step as phases, a ``yield`` behind the gather (``shard.run_phases``).  The rank's own rows of the whole batch
        go through the unsharded step's launches up to the block's step entry, which leaves scale * gradient in the send block beside
        the head's losses; one all-gather; the rank-ordered mean; the unsharded route's step on the block every rank agrees on.
        ``report``: a dict that receives the reduced ``grad`` and ``losses`` INSTEAD of a step (static scale): nothing is updated."""
        sh, master = self.shard, self._master()
        total, n = master.numel(), images.shape[0] // sh.world
        rows = slice(sh.rank * n, (sh.rank + 1) * n)
        first, sgd = self.steps == 0, self._sgd
        outs = self._head(images[rows], labels_d[rows], self._head_scale, self._send[total:total + self._n_losses])
        self._scale_rows(*outs)
        self._apply(outs, None, first, sgd)
        sh.gather(self._send, self._recv, self._send.numel() * 4, ops._stream())
        yield
        if report is not None:
            report["grad"] = ops.block_step_gathered(self._recv, total, self.grad_scale).view_as(master)
            report["losses"] = ops.block_rank_mean(self._recv[:, total:], self._n_losses)
        elif not self.dynamic and self._adam is None:      # the mean, 1 / grad_scale and SGD's rule in one launch; the losses' mean beside it
            ops.block_step_gathered(self._recv, total, self.grad_scale, master, self.buf, lr_d, first, *sgd, want_grad=False)
            self.last_losses = ops.block_rank_mean(self._recv[:, total:], self._n_losses)
        else:
            ops.block_rank_mean(self._recv, total + self._n_losses, self._reduced)
            self._apply_block(self._reduced[:total], lr_d, None, self._head_scale)      # static SGD took the branch above
            self.last_losses = self._reduced[total:].clone()     # the reduced block is the next step's as well: the history keeps its own

    def _shard_gradient(self, who: str, images: torch.Tensor, labels):
        """``(losses fp32 [n_losses], grad of the master's shape)`` of the whole batch, reduced over the ranks: the diagnostic entry
        points under ``shard``.  Under a local gather this call runs every rank's phases."""
        images = self._vision().images(who, images)
        sharding.check_batch(who, self.shard, images.shape[0])
        labels_d = fitloop.step_labels(who, labels, images.shape[0], self.C, images.device, "images")
        report = sharding.report_all(self.shard, self, who, lambda s, r: s._shard_phases(images, labels_d, None, r))
        return report["losses"], report["grad"]


class VPTFitState(_BlockFitState):
    """The training state of VPT's prompts: the fp32 master block ``prompts`` [depth, n_ctx, Dv] (None: the model's own parameters), SGD's
    momentum buffer, the tower's stash and the number of steps taken.  ``step`` enqueues one forward, backward and update and does not
    synchronise.  ``validate`` scores validation images on the device (``start_monitor``, ``monitor``, ``best_prompts``,
    ``val_row_results``; DESIGN.md "Fit monitor", "The image-tower fits")."""
    _who, _master_name = "VPTFitState", "prompts"

    def __init__(self, model, text_features: torch.Tensor, logit_scale: float = 4.6052, prompts: Optional[torch.Tensor] = None,
                 momentum: float = 0.9, dampening: float = 0.0, nesterov: bool = False, weight_decay: float = 5e-4,
                 grad_scale: float = DEFAULT_GRAD_SCALE, scaler: Optional[dict] = None, optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8,
                 shard: Optional[Shard] = None):
        who = "VPTFitState"
        if prompts is None:
            prompts = model_prompts(model)
        self.depth, self.n_ctx = _check_prompts(who, model, prompts)
        self._init_optimiser(who, logit_scale, momentum, dampening, nesterov, weight_decay, grad_scale, scaler, optimizer, betas, eps, shard)
        self.text = _check_text(who, model, text_features)
        self.C = int(self.text.shape[0])
        self.tower = _Tower(who, model, self.depth, self.n_ctx)
        self._init_block(fitloop.master(prompts, model.device))
        if shard is not None:   # the tower's backward writes the prompts' gradient straight into the send block
            self.tower.d_prompts = self._grad_block()
        self._text_n = None     # the fixed text features, normalised by the first validate

    def validate(self, val_images_or_loader, val_labels, epoch: int, val_batch_size: int = 32, one_call: bool = True) -> None:
        """Enqueue one validation of the current master prompts into slot ``epoch`` of the device history; no host read.
        ``val_images_or_loader``: preprocessed images [N_val, 3, R, R] on the GPU with ``val_labels`` [N_val], scored in chunks of
        ``val_batch_size``, or a sized iterable of (images, labels) batches on the GPU (``val_labels`` None).  Every chunk runs the tower's
        TRAINING forward at the prompts (the features the next step would see; the stash it overwrites is rewritten by that step), and
        its rows are scored against the text features, normalised once (clipmi_vision_val_chunk; ``one_call=False``: the four separate
        calls, the same bits); ``ops.val_score_finish`` folds the 16 N_val bytes of row results into the record, byte for byte
        ``ops.val_score``'s on the whole logits, and ``clipmi_best_select`` keeps the prompts of the best epoch when the monitor selects.
        Labels: an int64 tensor on the GPU is taken as it is; anything else is range-checked on the host.  Memory: the tower's stash grows
        to ``val_batch_size`` images when that exceeds the training batch, and stays (41.6 MB per image at ViT-B/16).  Without ``start_monitor`` the
        history starts with ``epoch + 1`` slots of 10 bins and no selection."""
        who = "VPTFitState.validate"
        self._no_shard_validate(who)
        mon = self._monitor_for(epoch)
        if self._text_n is None:
            self._text_n = ops.l2_normalize(self.text)
        mon.validate(who, self.tower, self.prompts, self._text_n, self.scale, val_images_or_loader, val_labels, epoch, val_batch_size, self.prompts,
                     one_call)

    def best_prompts(self) -> torch.Tensor:
        """The best slot on the device: the prompts of the best epoch so far, or the prompts ``start_monitor`` saw while no epoch has
        been taken."""
        return self._best_block("best_prompts").view_as(self.prompts)

    def _vision(self):
        return self.tower

    def _one_call(self, images, B, labels_d):
        t = self.tower
        ws = t.one_call_workspace(B, self.C, scaled=self.dynamic)
        front = (t.model._handle, C.byref(t.dgrad[0]), images.data_ptr(), _DT[images.dtype], B, self.prompts.data_ptr(),
                 None if self.buf is None else self.buf.data_ptr(), self.n_ctx, self.depth, self.text.data_ptr(), self.C, labels_d.data_ptr())
        return "clipmi_vpt_train_step", ws, front, (), (t.stash.data_ptr(), t.stash.numel())

    def _head(self, images, labels_d, grad_scale, loss):
        return vpt_head(self.tower.forward(images, self.prompts), labels_d, self.text, self.scale, grad_scale, loss)[1:]

    def _apply(self, outs, lr_d, first, sgd):
        """The tower's backward leaves the prompts' gradient as it is: under the dynamic scale and under Adam that is the block the
        step behind it takes."""
        grad = self.tower.backward(outs[0])
        return grad if self._defer else vpt_step(grad, self.grad_scale, self.prompts, self.buf, lr_d, first, *sgd, want_grad=False)


def fit_prompts(images_or_loader, labels, model, text_features: torch.Tensor, prompts: Optional[torch.Tensor] = None, logit_scale: float = 4.6052,
                lr: float = 0.0025, epochs: int = 5, batch_size: int = 32, momentum: float = 0.9, dampening: float = 0.0,
                weight_decay: float = 5e-4, nesterov: bool = False, grad_scale: float = DEFAULT_GRAD_SCALE,
                lr_per_epoch: Optional[Sequence[float]] = None, drop_last: bool = False, return_history: bool = False,
                scaler: Optional[dict] = None, optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8, shard: Optional[Shard] = None,
                val=None, val_batch_size: int = 32,
                val_bins: int = 10, final_model: str = "last_step", val_criterion: str = "accuracy", return_monitor: bool = False):
    """Train VPT's prompts starting from ``prompts`` (not modified; None = the model's own parameters): ``epochs`` passes of
    ``torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov)``.  ``images_or_loader`` is a tensor of preprocessed images
    [N, 3, R, R] with ``labels`` [N], cut into batches of ``batch_size`` in order (the last one short unless ``drop_last``), or a sized
    iterable of (images, labels) batches iterated once per epoch (``labels`` None, ``batch_size`` unused).  ``lr_per_epoch`` gives every
    epoch's rate; None takes ``cosine_warmup_schedule(lr, epochs)``.  The image tower runs on every step; nothing synchronises until the
    one wait at the end.  Returns the fitted fp32 block [depth, n_ctx, Dv] on the device, or ``(prompts, per-step batch losses)`` with
    ``return_history``.  The model's parameters are NOT written: ``trainers.vpt.CustomCLIP.fit_prompts`` does that.
    ``grad_scale="dynamic"`` with ``scaler`` (module docstring): a step that overflows fp16 is skipped on the device and the scale adapts;
    the history keeps one loss per step, skipped steps included, and the run still synchronises once.

    ``val=(val_images_or_loader, val_labels)`` (preprocessed validation images [N_val, 3, R, R] on the GPU and their labels, or a sized
    iterable of (images, labels) batches on the GPU with None): behind the last step of every epoch ``VPTFitState.validate`` scores the
    prompts against them on the device in chunks of ``val_batch_size``, into ``val_bins`` confidence bins -- the fitted prompts are bit for
    bit those of the same call without ``val``, and the run still synchronises once.  ``final_model``, ``val_criterion`` and
    ``return_monitor`` as ``coopfit.fit_context`` takes them: "best_val" returns the prompts of the epoch that was strictly better than
    every earlier one (the starting prompts when no epoch was taken) and is refused without ``val``.

    ``optimizer``, ``betas``, ``eps``: "sgd" (the default; ``momentum``, ``dampening``, ``nesterov``), "adam" or
    "adamw", as ``coopfit.fit_context`` takes them; ``weight_decay`` keeps this fit's default of 5e-4 under all three (torch's AdamW
    default of 1e-2 is NOT taken over).  DESIGN.md "Adam steps for the prompt fits".

    ``shard=coopfit.Shard(world, rank, gather)``: the batch-sharded fit (DESIGN.md "Batch-sharded image-tower fits"), this project's form
    of the reference's ``nn.DataParallel`` (vpt.py:171).  Every rank makes this call with the same arguments -- all images, whole batches
    whose sizes are multiples of ``world`` -- runs the tower over its own rows of every batch and returns the same prompts; with a
    ``LocalGather`` the one call runs all ``world`` states in this process.  All three optimisers and both loss scales; ``val`` and
    ``final_model="best_val"`` are refused."""
    who = "fit_prompts"
    if shard is not None:
        sharding.check(who, shard, "block", val=val, final_model=final_model)
    fitmonitor.check_image_args(who, val, val_batch_size, val_bins, final_model, val_criterion)
    epochs = int(epochs)
    if epochs < 0:
        raise ValueError(f"{who}: epochs={epochs} (>= 0)")
    if optimizer != "sgd":      # by this function's name; SGD's arguments are the state's to check, as before
        fitloop.check_optimizer(who, optimizer, momentum, dampening, nesterov, weight_decay, betas, eps)
    sharding.check_batches(who, shard, images_or_loader, batch_size, drop_last)
    state = shard_states(lambda sh: VPTFitState(model, text_features, logit_scale, prompts, momentum, dampening, nesterov, weight_decay, grad_scale,
                                                scaler, optimizer, betas, eps, sh), shard)
    batches = fitloop.cut_batches(who, images_or_loader, labels, state.C, batch_size, drop_last, model.device)
    _, lr_steps = fitloop.schedule(who, lr, epochs, lr_per_epoch, len(batches), model.device)
    end_epoch = None
    if val is not None and epochs * len(batches) > 0:
        state.start_monitor(epochs, val_bins, val_criterion=val_criterion, select=final_model == "best_val")
        end_epoch = lambda e: state.validate(val[0], val[1], e, val_batch_size)
    history = fitloop.run_batches(lambda e, k, b, r, want: state.step(b[0], b[1], r, want_loss=want), batches, epochs, lr_steps, return_history, end_epoch)
    out = state.best_prompts() if final_model == "best_val" and end_epoch is not None else state.prompts
    return fitmonitor.pack(out, history, fitmonitor.returned_monitor(state, end_epoch is not None, val_bins, return_monitor),
                           return_history, return_monitor)
