"""What did the context learn?  The nearest vocabulary words of learned prompt vectors (reference
interpret_prompts/interpret_prompt.py) -- the table every prompt-learning paper prints.

The reference forms the whole ``[rows, 49408]`` ``torch.cdist`` matrix, argsorts all of it, refuses class-specific contexts
(``ctx.dim() == 3``) and has its checkpoint path written into the script.  Here every row of every text-side prompt layer goes
through ONE ``ops.nearest_rows`` call (``csrc/nearest.hip``: top-k rows with indices, fp32 difference-form distances, ties to the
lower token id), class-specific contexts included, and the report is a string the caller prints::

    from clip_calibration_amd import interpret
    from clip_calibration_amd.tokenizer import ClipTokenizer
    results = interpret.interpret_prompt_learner(".../prompt_learner/model.pth.tar-5", clip_model.token_embedding,
                                                 topk=10, tokenizer=ClipTokenizer())
    print(interpret.format_report(results))
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import ops

_COMPOUND = re.compile(r"(?:^|\.)compound_prompts_text\.(\d+)$")
_VPT_SHALLOW = re.compile(r"^(.*?)transformer\.resblocks\.(\d+)\.VPT_shallow$")
_IMAGE_SIDE = ("visual", "image_encoder")


@dataclass
class NearestWords:
    """``indices`` int32 and ``distances`` fp32, device tensors shaped like the context with the last axis replaced by ``topk``
    (ascending in (distance, token id)); ``words`` the same shape as nested lists of vocabulary symbols, or None without a tokenizer;
    ``name`` the state-dict key of the layer when it came from a checkpoint."""
    indices: torch.Tensor
    distances: torch.Tensor
    words: Optional[list] = None
    name: str = ""


def _embedding_weight(token_embedding) -> torch.Tensor:
    w = getattr(token_embedding, "weight", token_embedding)
    if not isinstance(w, torch.Tensor) or w.dim() != 2 or not w.is_floating_point():
        raise TypeError("token_embedding must be the [V, D] float weight or a module with .weight")
    return w.detach()


def _device_f32(t: torch.Tensor, device: torch.device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _words(tokenizer, ids):
    return [_words(tokenizer, row) for row in ids] if isinstance(ids, list) else tokenizer.symbol(ids)


def _nearest(rows: Sequence[torch.Tensor], weight: torch.Tensor, topk: int, tokenizer, splits: int) -> List[NearestWords]:
    """One launch for all the contexts in ``rows`` (each [n_ctx, D] or [C, n_ctx, D], any float dtype)."""
    D = weight.shape[1]
    for ctx in rows:
        if not isinstance(ctx, torch.Tensor) or ctx.dim() not in (2, 3) or not ctx.is_floating_point():
            raise TypeError("ctx must be a float tensor [n_ctx, D] or [C, n_ctx, D]")
        if ctx.shape[-1] != D:
            raise ValueError(f"ctx width {ctx.shape[-1]} is not the embedding width {D}")
    device = weight.device if weight.is_cuda else next((c.device for c in rows if c.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    with torch.cuda.device(device):
        refs = _device_f32(weight, device)
        flat = torch.cat([_device_f32(c, device).reshape(-1, D) for c in rows], dim=0)
        dist, idx = ops.nearest_rows(flat, refs, topk, splits)
    out, at = [], 0
    for ctx in rows:
        n = ctx.numel() // D
        shape = tuple(ctx.shape[:-1]) + (int(topk),)
        i, d = idx[at:at + n].reshape(shape), dist[at:at + n].reshape(shape)
        out.append(NearestWords(i, d, _words(tokenizer, i.cpu().tolist()) if tokenizer is not None else None))
        at += n
    return out


def nearest_words(ctx: torch.Tensor, token_embedding, topk: int = 10, tokenizer=None, splits: int = 0) -> NearestWords:
    """The ``topk`` token embeddings nearest to every context vector (interpret_prompt.py:66-76).  ``ctx`` [n_ctx, D], or
    [C, n_ctx, D] for a class-specific context (which the reference refuses), any float dtype; ``token_embedding`` the [V, D] weight or
    a module with ``.weight``.  Both are converted to fp32 on the device, as the reference's ``.float()`` does."""
    return _nearest([ctx], _embedding_weight(token_embedding), topk, tokenizer, splits)[0]


def prompt_layers(state_dict: Dict) -> List[Tuple[str, torch.Tensor]]:
    """The text-side prompts of a Dassl ``prompt_learner`` state dict (or of the dict ``checkpoint.load_checkpoint`` returns), in the
    order the text tower meets them: the key ending in ``ctx``; ``compound_prompts_text.{i}`` ascending (MaPLe);
    ``text_encoder.transformer.resblocks.{i}.VPT_shallow`` ascending (IVLP / PromptSRC).  Image-side prompts (``visual.`` /
    ``image_encoder.`` keys, ``VPT``), projections and the fixed token buffers are not prompts over the vocabulary and are left out."""
    if isinstance(state_dict.get("state_dict"), dict):
        state_dict = state_dict["state_dict"]
    ctx, compound, shallow = [], [], []
    for key, value in state_dict.items():
        if not isinstance(value, torch.Tensor):
            continue
        if key == "ctx" or key.endswith(".ctx"):
            ctx.append((key, value))
            continue
        m = _COMPOUND.search(key)
        if m:
            compound.append((int(m.group(1)), key, value))
            continue
        m = _VPT_SHALLOW.match(key)
        if m and not any(part in _IMAGE_SIDE for part in m.group(1).split(".")):
            shallow.append((int(m.group(2)), key, value))
    if len(ctx) > 1:
        raise ValueError(f"more than one context in the state dict: {[k for k, _ in ctx]}")
    return ctx + [(k, v) for _, k, v in sorted(compound, key=lambda t: t[0])] + [(k, v) for _, k, v in sorted(shallow, key=lambda t: t[0])]


def interpret_prompt_learner(state_dict_or_path: Union[str, Dict], token_embedding, topk: int = 10, tokenizer=None) -> List[NearestWords]:
    """``nearest_words`` of every text-side prompt layer of a checkpoint (a path, the loaded dict or its ``state_dict``), in
    ``prompt_layers`` order; all layers share one launch."""
    if isinstance(state_dict_or_path, str):
        from .checkpoint import load_checkpoint
        state_dict_or_path = load_checkpoint(state_dict_or_path)
    layers = prompt_layers(state_dict_or_path)
    if not layers:
        raise KeyError("no text-side prompt (ctx, compound_prompts_text.*, text VPT_shallow) in the state dict")
    results = _nearest([v for _, v in layers], _embedding_weight(token_embedding), topk, tokenizer, 0)
    for (name, _), r in zip(layers, results):
        r.name = name
    return results


def format_report(results: Union[NearestWords, Sequence[NearestWords]]) -> str:
    """The lines the reference script prints (interpret_prompt.py:63-83), as one string: per layer the header, per context row
    ``{m+1}: {words} {distances}`` with the distances as ``f"{d:.4f}"`` strings, and the two closing rules.  Token ids stand in for the
    words of a result that has none; a class-specific context gets a ``Class {c}:`` line in front of each class's rows."""
    if isinstance(results, NearestWords):
        results = [results]
    lines = []
    for n, r in enumerate(results):
        lines.append(f"SHOWING RESULTS FOR CTX Vectors of Layer:  {n + 1}")
        words = r.words if r.words is not None else r.indices.cpu().tolist()
        dists = r.distances.cpu().tolist()
        classes = [(None, words, dists)] if r.indices.dim() == 2 else [(c, w, d) for c, (w, d) in enumerate(zip(words, dists))]
        for c, w_rows, d_rows in classes:
            if c is not None:
                lines.append(f"Class {c}:")
            for m, (w, d) in enumerate(zip(w_rows, d_rows)):
                lines.append(f"{m + 1}: {w} {[f'{x:.4f}' for x in d]}")
        lines += ["#" * 30, "#" * 30]
    return "\n".join(lines) + "\n"
