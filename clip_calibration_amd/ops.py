"""Operator-level Python entry points: torch tensors in, HIP kernels through the C ABI, torch tensors out.

torch is used for device memory and streams only; every wrapper checks device / dtype / contiguity and raises if the
input is not a ROCm tensor -- nothing here computes on the CPU or with torch ops (the one exception is weight
preparation: fold_layernorm_linear).
"""
from __future__ import annotations

import collections
import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import _DT, F16, F32, check, lib


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, name: str, dtypes=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"clipmi: `{name}` must be a tensor on the GPU (got {getattr(t, 'device', type(t))}); "
                           "the HIP path has no CPU fallback")
    if dtypes is not None and t.dtype not in dtypes:
        raise TypeError(f"clipmi: `{name}` has dtype {t.dtype}, expected one of {dtypes}")
    # launches go to the CURRENT device's stream with raw pointers: a tensor that lives on another GPU would be handed to
    # the wrong device.  One process drives one GPU here; anything else must say so with torch.cuda.device(...).
    if t.device.index != torch.cuda.current_device():
        raise RuntimeError(f"clipmi: `{name}` is on {t.device} but the current device is cuda:{torch.cuda.current_device()}; "
                           f"run the call under `with torch.cuda.device({t.device.index}):`")
    return t if t.is_contiguous() else t.contiguous()


def _opt(t: Optional[torch.Tensor], name: str, dtypes) -> Tuple[Optional[torch.Tensor], Optional[int]]:
    if t is None:
        return None, None
    t = _dev(t, name, dtypes)
    return t, t.data_ptr()


def _in_place(t, dtype: torch.dtype, message: str, exc=TypeError, numel: Optional[int] = None) -> None:
    """A tensor the kernel works on where it lies (no ``.contiguous()`` copy may stand in for it): contiguous, on the GPU, of ``dtype``."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and (numel is None or t.numel() == numel)):
        raise exc(message)


def _dac(dac_conf: Optional[torch.Tensor], classes: int, who: str) -> Tuple[Optional[torch.Tensor], Optional[int]]:
    """The optional DAC factors, fp32 with one entry per class: (tensor, pointer)."""
    dac_conf, pd = _opt(dac_conf, "dac_conf", (torch.float32,))
    if dac_conf is not None and dac_conf.numel() != classes:
        raise ValueError(f"{who}: dac_conf must have one entry per class")
    return dac_conf, pd


def _conf_pred(want: bool, rows: int, device):
    """The optional top-1 outputs: (conf fp32 [rows], pred int32 [rows], their pointers), or four None."""
    if not want:
        return None, None, None, None
    conf = torch.empty(rows, dtype=torch.float32, device=device)
    pred = torch.empty(rows, dtype=torch.int32, device=device)
    return conf, pred, conf.data_ptr(), pred.data_ptr()


def gemm_f16(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
             residual: Optional[torch.Tensor] = None, epilogue: int = _lib.EPI_NONE,
             out_dtype: torch.dtype = torch.float16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``epi(a[M,K] @ w[N,K]^T)`` -- nn.Linear and friends (reference clip/model.py:174-176,183,422,611)."""
    a = _dev(a, "a", (torch.float16,))
    w = _dev(w, "w", (torch.float16,))
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"gemm: a is [{M},{K}] but w is {tuple(w.shape)}")
    bias, pb = _opt(bias, "bias", (torch.float32,))
    residual, pr = _opt(residual, "residual", (torch.float16,) if epilogue == _lib.EPI_BIAS_RESIDUAL16_RELU else (torch.float32,))
    if residual is not None and tuple(residual.shape) != (M, N):
        raise ValueError(f"gemm: residual is {tuple(residual.shape)}, expected [{M},{N}]")
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=a.device)
    check(lib.clipmi_gemm_f16(a.data_ptr(), K, w.data_ptr(), K, pb, pr, out.data_ptr(), N, _DT[out.dtype],
                              M, N, K, epilogue, _stream()), "clipmi_gemm_f16")
    return out


def gemm_residual_f16(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, x16: torch.Tensor):
    """``x16 <- fp16(x16 + a @ w^T + bias)`` in place (one rounding of the fp32 sum): the residual GEMM of a block on the fp16
    stream (reference clip/model.py:186-187).  Returns (stats fp32 [8, M, 2], parts): the LayerNorm-fold row partials
    ``stats[t, m] = (sum, sum of squares)`` over the t-th column tile of the rounded row m, ``parts`` tiles of them."""
    a = _dev(a, "a", (torch.float16,))
    w = _dev(w, "w", (torch.float16,))
    bias = _dev(bias, "bias", (torch.float32,))
    _in_place(x16, torch.float16, "gemm_residual_f16: x16 must be a contiguous fp16 GPU tensor (it is updated in place)")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or tuple(x16.shape) != (M, N) or bias.numel() != N:
        raise ValueError(f"gemm_residual_f16: a {tuple(a.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)}, x16 {tuple(x16.shape)}")
    stats = torch.empty(8, M, 2, dtype=torch.float32, device=a.device)
    parts = ctypes.c_int(0)
    check(lib.clipmi_gemm_residual_f16(a.data_ptr(), K, w.data_ptr(), K, bias.data_ptr(), x16.data_ptr(), N, stats.data_ptr(),
                                       ctypes.byref(parts), M, N, K, _stream()), "clipmi_gemm_residual_f16")
    return stats, parts.value


def fold_layernorm_linear(w: torch.Tensor, b: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor):
    """Weight preparation of the LayerNorm fold (csrc/gemm.hip "LayerNorm folded into the GEMMs"), on the device the weights are on:
    ``Linear(LayerNorm(x)) = rstd * (x @ w_f^T) - rstd * mean * g + c`` with w_f = fp16(gamma * W), g = row sums of that fp16 w_f (what
    the MFMA multiplies, so the mean term cancels as inside a LayerNorm) and c = W beta + b, all in fp32.  Returns (w_f, g, c), contiguous."""
    w32 = w.detach().float()
    wf = (w32 * gamma.detach().float()[None, :]).to(torch.float16).contiguous()
    g = wf.float().sum(dim=1).contiguous()
    c = (w32 @ beta.detach().float() + b.detach().float()).contiguous()
    return wf, g, c


def gemm_residual_fold(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, x: torch.Tensor, x16: Optional[torch.Tensor] = None):
    """``x <- x + a @ w^T + bias`` in place on the fp32 stream (reference clip/model.py:186-187), plus the LayerNorm-fold outputs:
    x16 = fp16(x) and the row partials ``stats[t, m] = (sum, sum of squares)`` of the fp32 row m over column tile t.
    Returns (x16, stats fp32 [8, M, 2], parts)."""
    a = _dev(a, "a", (torch.float16,))
    w = _dev(w, "w", (torch.float16,))
    bias = _dev(bias, "bias", (torch.float32,))
    _in_place(x, torch.float32, "gemm_residual_fold: x must be a contiguous fp32 GPU tensor (it is updated in place)")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or tuple(x.shape) != (M, N) or bias.numel() != N:
        raise ValueError(f"gemm_residual_fold: a {tuple(a.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)}, x {tuple(x.shape)}")
    if x16 is None:
        x16 = torch.empty(M, N, dtype=torch.float16, device=a.device)
    x16 = _dev(x16, "x16", (torch.float16,))
    if tuple(x16.shape) != (M, N):
        raise ValueError(f"gemm_residual_fold: x16 {tuple(x16.shape)}, expected [{M},{N}]")
    stats = torch.empty(8, M, 2, dtype=torch.float32, device=a.device)
    parts = ctypes.c_int(0)
    check(lib.clipmi_gemm_residual_fold(a.data_ptr(), K, w.data_ptr(), K, bias.data_ptr(), x.data_ptr(), N, x16.data_ptr(),
                                        stats.data_ptr(), ctypes.byref(parts), M, N, K, _stream()), "clipmi_gemm_residual_fold")
    return x16, stats, parts.value


def gemm_ln_fold(a: torch.Tensor, w_f: torch.Tensor, c: torch.Tensor, g: torch.Tensor, stats: torch.Tensor, parts: int,
                 ln_dim: int, eps: float = 1e-5, ln_plane: int = 0, ln_row_stride: int = 1, ln_rows: Optional[torch.Tensor] = None,
                 epilogue: int = _lib.EPI_BIAS, out_dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """``epi(LayerNorm(x) @ W^T + b)`` as the LayerNorm-folded consumer GEMM (in-proj / c_fc): a = fp16(x) [M, K],
    (w_f, g, c) from fold_layernorm_linear, row statistics from ``parts`` producer partials: row m's partial p is the float pair at
    ``stats.view(-1)[2 * (p * ln_plane + m * ln_row_stride)]`` (ln_plane 0 = M; pass a 1-d view that starts at a later row to offset them).
    ln_rows: optional fp32 [M, 2] scratch (lets the streamed kernel take more than 4 partials).  epilogue EPI_BIAS or EPI_BIAS_QUICKGELU."""
    a = _dev(a, "a", (torch.float16,))
    w_f = _dev(w_f, "w_f", (torch.float16,))
    c = _dev(c, "c", (torch.float32,))
    g = _dev(g, "g", (torch.float32,))
    _in_place(stats, torch.float32, "gemm_ln_fold: stats must be a contiguous fp32 GPU tensor")
    N, K = w_f.shape
    M = a.shape[0]
    if a.shape[1] != K:
        raise ValueError(f"gemm_ln_fold: a is {tuple(a.shape)} but w_f is {tuple(w_f.shape)}")
    plane = ln_plane if ln_plane > 0 else M
    if M > 0 and stats.numel() < 2 * ((parts - 1) * plane + (M - 1) * ln_row_stride + 1):
        raise ValueError(f"gemm_ln_fold: stats has {stats.numel()} floats, {parts} partials of plane {plane} need more")
    if c.numel() != N or g.numel() != N:
        raise ValueError("gemm_ln_fold: c and g must have N elements")
    pr = None
    if ln_rows is not None:
        ln_rows = _dev(ln_rows, "ln_rows", (torch.float32,))
        if ln_rows.numel() < 2 * M:
            raise ValueError("gemm_ln_fold: ln_rows needs [M, 2]")
        pr = ln_rows.data_ptr()
    out = torch.empty(M, N, dtype=out_dtype, device=w_f.device)
    check(lib.clipmi_gemm_ln_fold(a.data_ptr(), K, w_f.data_ptr(), K, c.data_ptr(), g.data_ptr(), stats.data_ptr(), int(parts),
                                  int(ln_plane), int(ln_row_stride), int(ln_dim), float(eps), pr, out.data_ptr(), N, _DT[out_dtype],
                                  M, N, K, int(epilogue), _stream()), "clipmi_gemm_ln_fold")
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
              out_dtype: Optional[torch.dtype] = None, gather_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32-statistics LayerNorm over the last dim (reference clip/model.py:153-159)."""
    x = _dev(x, "x", (torch.float16, torch.float32))
    gamma = _dev(gamma, "gamma", (torch.float32,))
    beta = _dev(beta, "beta", (torch.float32,))
    D = x.shape[-1]
    x2 = x.reshape(-1, D)
    out_dtype = out_dtype or x.dtype
    if gather_rows is not None:
        gather_rows = _dev(gather_rows, "gather_rows", (torch.int32,))
        rows = gather_rows.numel()
        y = torch.empty(rows, D, dtype=out_dtype, device=x.device)
        pg = gather_rows.data_ptr()
    else:
        rows = x2.shape[0]
        y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
        pg = None
    check(lib.clipmi_layernorm(x2.data_ptr(), _DT[x.dtype], D, pg, gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                               _DT[out_dtype], D, rows, D, eps, _stream()), "clipmi_layernorm")
    return y


def attention(qkv: torch.Tensor, n_seq: int, seq_len: int, n_head: int, causal: bool) -> torch.Tensor:
    """qkv fp16 [n_seq*seq_len, 3*64*n_head] -> fp16 [n_seq*seq_len, 64*n_head] (SURVEY a-5a)."""
    qkv = _dev(qkv, "qkv", (torch.float16,))
    D = 64 * n_head
    if qkv.shape != (n_seq * seq_len, 3 * D):
        raise ValueError(f"attention: qkv shape {tuple(qkv.shape)} != {(n_seq * seq_len, 3 * D)}")
    out = torch.empty(n_seq * seq_len, D, dtype=torch.float16, device=qkv.device)
    check(lib.clipmi_attention(qkv.data_ptr(), out.data_ptr(), n_seq, seq_len, n_head, int(bool(causal)), _stream()),
          "clipmi_attention")
    return out


def attention_cls(qkv: torch.Tensor, n_seq: int, seq_len: int, n_head: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """qkv fp16 [n_seq*seq_len, 3*64*n_head] -> fp16 [n_seq*seq_len, 64*n_head] of which only row 0 of every sequence (the class
    token's, never masked) is written; ``out`` (same shape) keeps its other rows, a fresh one has them zero."""
    qkv = _dev(qkv, "qkv", (torch.float16,))
    D = 64 * n_head
    if qkv.shape != (n_seq * seq_len, 3 * D):
        raise ValueError(f"attention_cls: qkv shape {tuple(qkv.shape)} != {(n_seq * seq_len, 3 * D)}")
    if out is None:
        out = torch.zeros(n_seq * seq_len, D, dtype=torch.float16, device=qkv.device)
    else:
        out = _dev(out, "out", (torch.float16,))
        if out.shape != (n_seq * seq_len, D):
            raise ValueError(f"attention_cls: out shape {tuple(out.shape)} != {(n_seq * seq_len, D)}")
    check(lib.clipmi_attention_cls(qkv.data_ptr(), out.data_ptr(), n_seq, seq_len, n_head, _stream()), "clipmi_attention_cls")
    return out


def patchify(image: torch.Tensor, patch: int, kpad: Optional[int] = None) -> torch.Tensor:
    image = _dev(image, "image", (torch.float16, torch.float32))
    B, ch, R, R2 = image.shape
    if ch != 3 or R != R2:
        raise ValueError(f"patchify: expected [B,3,R,R], got {tuple(image.shape)}")
    kpad = kpad or (3 * patch * patch + 63) // 64 * 64
    g = R // patch
    col = torch.empty(B * g * g, kpad, dtype=torch.float16, device=image.device)
    check(lib.clipmi_patchify(image.data_ptr(), _DT[image.dtype], col.data_ptr(), B, R, patch, kpad, _stream()),
          "clipmi_patchify")
    return col


def l2_normalize(f: torch.Tensor, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``f / f.norm(dim=-1, keepdim=True)`` in fp32 (reference zsclip.py:99); ``out_dtype=torch.float16`` rounds the
    quotient once (the exchange format of the multi-GPU path)."""
    f = _dev(f, "features", (torch.float16, torch.float32))
    rows, E = f.shape
    out = torch.empty(rows, E, dtype=out_dtype, device=f.device)
    with torch.cuda.device(f.device):
        check(lib.clipmi_l2_normalize_to(f.data_ptr(), _DT[f.dtype], out.data_ptr(), _DT[out_dtype], rows, E, _stream()),
              "clipmi_l2_normalize_to")
    return out


def logits_fused(img_n: torch.Tensor, txt_n: torch.Tensor, scale: float, dac_conf: Optional[torch.Tensor] = None,
                 want_conf_pred: bool = True):
    """(scale*img_n) @ txt_n^T  [+ DAC row scale]  [+ softmax top-1 conf / pred] on features that are ALREADY normalised
    (the gathered embeddings of the multi-GPU path, CoCoOp's shared image features): one launch of the fused tail."""
    logits, _, conf, pred = fused_tail(img_n, txt_n, scale, dac_conf, want_conf_pred, normalize=False)
    return logits, conf, pred


_TAIL_WS = collections.OrderedDict()   # (device index, stream) -> zeroed int32 ticket counters (the kernel leaves them zero); LRU, bounded
_TAIL_WS_MAX = 16                       # streams with a live workspace: short-lived per-thread streams must not pin buffers for ever


def _tail_workspace(device: torch.device, batch: int, classes: int):
    """Ticket counters of the fused tail: one buffer per (device, stream).  Launches on ONE stream run in order and each leaves the
    counters zero; two launches in flight on different streams must not share them (a foreign ticket would skip or double a row pass).
    Returns (key, buffer); the least recently used entries beyond _TAIL_WS_MAX are dropped (the caching allocator keeps a dropped buffer
    alive until the work queued on its stream is done), and `_tail_workspace_failed` drops the entry of a launch that raised."""
    need = lib.clipmi_fused_tail_workspace_bytes(batch, classes)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _TAIL_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.zeros(max(need, 4096), dtype=torch.uint8, device=device)
        _TAIL_WS[key] = ws
    _TAIL_WS.move_to_end(key)
    while len(_TAIL_WS) > _TAIL_WS_MAX:
        _TAIL_WS.popitem(last=False)
    return key, ws


def _tail_workspace_failed(key) -> None:
    """A launch that raised may have left tickets behind: the next call on this stream starts from a freshly zeroed buffer."""
    _TAIL_WS.pop(key, None)


def fused_tail(img: torch.Tensor, txt_n: torch.Tensor, scale: float, dac_conf: Optional[torch.Tensor] = None,
               want_conf_pred: bool = True, normalize: bool = True, labels: Optional[torch.Tensor] = None,
               bins: Optional[torch.Tensor] = None, n_bins: int = 0):
    """The tail of the path in ONE launch (include/clipmi.h, clipmi_fused_tail): L2-normalise the image features,
    ``scale * img_n @ txt_n^T``, DAC row scale, softmax top-1 and -- when ``labels`` and ``bins`` are given -- the ECE bin
    accumulation.  Returns (logits, img_n, conf, pred); img_n is ``img`` itself when ``normalize`` is False."""
    img = _dev(img, "img", (torch.float32, torch.float16))
    txt_n = _dev(txt_n, "txt_n", (torch.float32,))
    if txt_n.device != img.device:
        raise RuntimeError(f"fused_tail: img on {img.device}, txt_n on {txt_n.device}")
    B, E = img.shape
    Cn = txt_n.shape[0]
    if txt_n.shape[1] != E:
        raise ValueError("fused_tail: feature widths differ")
    dac_conf, pd = _dac(dac_conf, Cn, "fused_tail")
    labels, pl = _opt(labels, "labels", (torch.int64,))
    bins, pb = _opt(bins, "bins", (torch.float64,))
    if (pb is None) != (pl is None):
        raise ValueError("fused_tail: labels and bins come together")
    if bins is not None and (bins.numel() != 3 * (n_bins + 1) or labels.numel() != B):
        raise ValueError("fused_tail: bins must hold 3*(n_bins+1) float64 and labels one entry per image")
    logits = torch.empty(B, Cn, dtype=torch.float32, device=img.device)
    img_n = torch.empty(B, E, dtype=torch.float32, device=img.device) if normalize else img
    conf, pred, pc, pp = _conf_pred(want_conf_pred or bins is not None, B, img.device)
    key, ws = _tail_workspace(img.device, B, Cn)
    try:
        with torch.cuda.device(img.device):
            check(lib.clipmi_fused_tail(img.data_ptr(), _DT[img.dtype], int(normalize), txt_n.data_ptr(), float(scale), pd, logits.data_ptr(),
                                        img_n.data_ptr() if normalize else None, pc, pp, pl, pb, int(n_bins), ws.data_ptr(), ws.numel(),
                                        B, Cn, E, _stream()), "clipmi_fused_tail")
    except Exception:
        _tail_workspace_failed(key)
        raise
    return logits, img_n, conf, pred


def softmax_rows(logits: torch.Tensor, dac_conf: Optional[torch.Tensor] = None, want_conf_pred: bool = False):
    """probs = softmax(logits * dac_conf[argmax]) row-wise (vl_calibrator.py:83-109, DAC / plain branches); logits untouched."""
    logits = _dev(logits, "logits", (torch.float32,))
    B, Cn = logits.shape
    dac_conf, pd = _dac(dac_conf, Cn, "softmax_rows")
    probs = torch.empty_like(logits)
    conf, pred, pc, pp = _conf_pred(want_conf_pred, B, logits.device)
    check(lib.clipmi_softmax_rows(logits.data_ptr(), pd, probs.data_ptr(), pc, pp, B, Cn, _stream()), "clipmi_softmax_rows")
    return (probs, conf, pred) if want_conf_pred else probs


def ece_accumulate(conf: torch.Tensor, pred: torch.Tensor, labels: torch.Tensor, bins: torch.Tensor, n_bins: int) -> None:
    conf = _dev(conf, "conf", (torch.float32,))
    pred = _dev(pred, "pred", (torch.int32,))
    labels = _dev(labels, "labels", (torch.int64,))
    bins = _dev(bins, "bins", (torch.float64,))
    if bins.numel() != 3 * (n_bins + 1):
        raise ValueError("ece_accumulate: bins must hold 3*(n_bins+1) float64")
    check(lib.clipmi_ece_accumulate(conf.data_ptr(), pred.data_ptr(), labels.data_ptr(), conf.numel(), bins.data_ptr(),
                                    n_bins, _stream()), "clipmi_ece_accumulate")


def procal_kde(model: "_lib.ProcalModel", conf: torch.Tensor, proximity: torch.Tensor) -> torch.Tensor:
    """ProCal's c* = T / max(T + ratio F, 1e-10) per (conf, proximity) pair (density_ratio_calibration.py:100-105) for a fitted
    ``model`` whose point sets live on this device (procal.DensityRatioCalibration.device_model)."""
    conf = _dev(conf, "conf", (torch.float32,))
    proximity = _dev(proximity, "proximity", (torch.float32,))
    if conf.dim() != 1 or proximity.shape != conf.shape:
        raise ValueError(f"procal_kde: conf {tuple(conf.shape)} and proximity {tuple(proximity.shape)} must be equal 1-d shapes")
    cstar = torch.empty_like(conf)
    check(lib.clipmi_procal_kde(model, conf.data_ptr(), proximity.data_ptr(), cstar.data_ptr(), conf.numel(), _stream()),
          "clipmi_procal_kde")
    return cstar


def procal_rows(model: "_lib.ProcalModel", logits: torch.Tensor, proximity: torch.Tensor, dac_conf: Optional[torch.Tensor] = None,
                want_probs: bool = False, want_cstar: bool = False):
    """softmax(DAC(logits)) -> ProCal -> the evaluator's top-1 (vl_calibrator.py:83-109, vl_evaluator.py:68,83), one launch:
    returns (probs fp32 [N,C] or None, conf' fp32 [N], pred' int32 [N], c* fp32 [N] or None); logits untouched."""
    logits = _dev(logits, "logits", (torch.float32,))
    proximity = _dev(proximity, "proximity", (torch.float32,))
    if logits.dim() != 2 or proximity.dim() != 1 or proximity.shape[0] != logits.shape[0]:
        raise ValueError(f"procal_rows: logits {tuple(logits.shape)} need a proximity of one entry per row, got {tuple(proximity.shape)}")
    N, Cn = logits.shape
    dac_conf, pd = _dac(dac_conf, Cn, "procal_rows")
    probs = torch.empty_like(logits) if want_probs else None
    cstar = torch.empty(N, dtype=torch.float32, device=logits.device) if want_cstar else None
    conf = torch.empty(N, dtype=torch.float32, device=logits.device)
    pred = torch.empty(N, dtype=torch.int32, device=logits.device)
    check(lib.clipmi_procal_rows(model, logits.data_ptr(), pd, proximity.data_ptr(), None if probs is None else probs.data_ptr(),
                                 conf.data_ptr(), pred.data_ptr(), None if cstar is None else cstar.data_ptr(), N, Cn, _stream()),
          "clipmi_procal_rows")
    return probs, conf, pred, cstar


def isotonic_rows(model: "_lib.IsotonicModel", logits: torch.Tensor, proximity: Optional[torch.Tensor] = None,
                  dac_conf: Optional[torch.Tensor] = None, want_probs: bool = False, want_x: bool = False, from_probs: bool = False):
    """softmax(DAC(logits)) -> second softmax -> isotonic table of the row's proximity bin -> the evaluator's top-1
    (vl_calibrator.py:83-109 on 'bin_based' / 'multi_isotonic_regression', vl_evaluator.py:68,83), one launch: returns (calibrated rows
    fp32 [N,C] or None, conf fp32 [N], pred int32 [N], x fp32 [N,C] or None); logits untouched."""
    logits = _dev(logits, "logits", (torch.float32,))
    if logits.dim() != 2:
        raise ValueError(f"isotonic_rows: logits {tuple(logits.shape)} must be [N, C]")
    N, Cn = logits.shape
    proximity, pp = _opt(proximity, "proximity", (torch.float32,))
    if proximity is not None and (proximity.dim() != 1 or proximity.shape[0] != N):
        raise ValueError(f"isotonic_rows: logits {tuple(logits.shape)} need a proximity of one entry per row, got {tuple(proximity.shape)}")
    dac_conf, pd = _dac(dac_conf, Cn, "isotonic_rows")
    probs = torch.empty_like(logits) if want_probs else None
    xs = torch.empty_like(logits) if want_x else None
    conf = torch.empty(N, dtype=torch.float32, device=logits.device)
    pred = torch.empty(N, dtype=torch.int32, device=logits.device)
    check(lib.clipmi_isotonic_rows(model, logits.data_ptr(), pd, pp, int(from_probs), None if probs is None else probs.data_ptr(),
                                   None if xs is None else xs.data_ptr(), conf.data_ptr(), pred.data_ptr(), N, Cn, _stream()),
          "clipmi_isotonic_rows")
    return probs, conf, pred, xs


def isotonic_keys(logits: torch.Tensor, labels: torch.Tensor, from_probs: bool = False) -> torch.Tensor:
    """The positive keys of the isotonic fit: x[i, labels[i]] fp32 [N] (NaN where a label is outside the classes)."""
    logits = _dev(logits, "logits", (torch.float32,))
    labels = _dev(labels, "labels", (torch.int64,))
    if logits.dim() != 2 or labels.shape != (logits.shape[0],):
        raise ValueError(f"isotonic_keys: logits {tuple(logits.shape)} need one label per row, got {tuple(labels.shape)}")
    keys = torch.empty(logits.shape[0], dtype=torch.float32, device=logits.device)
    check(lib.clipmi_isotonic_keys(logits.data_ptr(), labels.data_ptr(), keys.data_ptr(), logits.shape[0], logits.shape[1],
                                   int(from_probs), _stream()), "clipmi_isotonic_keys")
    return keys


def isotonic_gap_stats(logits: torch.Tensor, labels: torch.Tensor, keys: torch.Tensor, key_offset, bin_index: Optional[torch.Tensor] = None,
                       from_probs: bool = False):
    """The per-gap statistics of the isotonic fit (include/clipmi.h, clipmi_isotonic_gap_stats): ``keys`` fp32 holds each bin's sorted
    distinct positive keys, ``key_offset`` (host ints, n_bins + 1) where each bin's start.  Returns (stats int32 [3, total], status
    int32 [1]), both on the device."""
    logits = _dev(logits, "logits", (torch.float32,))
    labels = _dev(labels, "labels", (torch.int64,))
    keys = _dev(keys, "keys", (torch.float32,))
    if logits.dim() != 2 or labels.shape != (logits.shape[0],):
        raise ValueError(f"isotonic_gap_stats: logits {tuple(logits.shape)} need one label per row, got {tuple(labels.shape)}")
    bin_index, pb = _opt(bin_index, "bin_index", (torch.int32,))
    if bin_index is not None and bin_index.shape != (logits.shape[0],):
        raise ValueError("isotonic_gap_stats: bin_index must have one entry per row")
    off = [int(o) for o in key_offset]
    n_bins = len(off) - 1
    if n_bins < 1 or off[-1] != keys.numel():
        raise ValueError(f"isotonic_gap_stats: key_offset {off} does not describe {keys.numel()} keys")
    total = 3 * off[-1] + n_bins
    stats = torch.empty(3, total, dtype=torch.int32, device=logits.device)
    status = torch.empty(1, dtype=torch.int32, device=logits.device)
    c_off = (ctypes.c_int32 * len(off))(*off)
    check(lib.clipmi_isotonic_gap_stats(logits.data_ptr(), labels.data_ptr(), pb, keys.data_ptr(), c_off, n_bins, stats.data_ptr(),
                                        status.data_ptr(), logits.shape[0], logits.shape[1], int(from_probs), _stream()),
          "clipmi_isotonic_gap_stats")
    return stats, status


# ---- sample-level metrics (vl_evaluator.py:77-82, tools/metrics.py:132-178, 212-236) --------------------------------
def order_stats(x: torch.Tensor, ranks) -> Tuple[torch.Tensor, torch.Tensor]:
    """``np.sort(x)[ranks]`` without a sort (include/clipmi.h, clipmi_order_stats): ``x`` fp32 [n] on the device, ``ranks`` host ints,
    non-decreasing, each in [0, n), at most 64 of them.  Returns (values fp32 [k], NaN count int32 [1]), both on the device; nothing is
    synchronised."""
    x = _dev(x, "x", (torch.float32,))
    if x.dim() != 1 or x.numel() < 1:
        raise ValueError(f"order_stats: x {tuple(x.shape)} must be a non-empty vector")
    r = [int(v) for v in ranks]
    if not 1 <= len(r) <= _lib.ORDER_STATS_MAX_RANKS:
        raise ValueError(f"order_stats: {len(r)} ranks (1 .. {_lib.ORDER_STATS_MAX_RANKS})")
    n, k = x.numel(), len(r)
    if any(not 0 <= v < n for v in r) or any(b < a for a, b in zip(r, r[1:])):
        raise ValueError(f"order_stats: ranks {r} must ascend inside [0, {n})")
    out = torch.empty(k, dtype=torch.float32, device=x.device)
    nans = torch.empty(1, dtype=torch.int32, device=x.device)
    ws = torch.empty(lib.clipmi_order_stats_workspace_bytes(n, k), dtype=torch.uint8, device=x.device)
    c_ranks = (ctypes.c_int32 * k)(*r)
    check(lib.clipmi_order_stats(x.data_ptr(), n, c_ranks, k, out.data_ptr(), nans.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "clipmi_order_stats")
    return out, nans


def nearest_rows(queries: torch.Tensor, refs: torch.Tensor, k: int, splits: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The ``k`` rows of ``refs`` nearest to every row of ``queries`` in L2 distance (include/clipmi.h, clipmi_nearest_rows): what
    ``torch.cdist(queries, refs).argsort(1)[:, :k]`` selects, without the [Nq, Nr] matrix.  fp32 contiguous device tensors [Nq, E] and
    [Nr, E]; half inputs are refused, the caller converts.  Returns (dist fp32 [Nq, k], idx int32 [Nq, k]), ascending in (distance, index).
    ``splits``: slices of the reference rows that share the work of one query block, 0 = the library chooses; the result is the same
    bits for every value."""
    queries = _dev(queries, "queries", (torch.float32,))
    refs = _dev(refs, "refs", (torch.float32,))
    if queries.dim() != 2 or refs.dim() != 2 or queries.shape[1] != refs.shape[1]:
        raise ValueError(f"nearest_rows: queries {tuple(queries.shape)} and refs {tuple(refs.shape)} must be [Nq, E] and [Nr, E]")
    nq, e = queries.shape
    nr, k, splits = refs.shape[0], int(k), int(splits)
    dist = torch.empty(nq, k, dtype=torch.float32, device=queries.device)
    idx = torch.empty(nq, k, dtype=torch.int32, device=queries.device)
    ws = torch.empty(lib.clipmi_nearest_rows_workspace(nq, nr, k, splits), dtype=torch.uint8, device=queries.device)
    check(lib.clipmi_nearest_rows(queries.data_ptr(), refs.data_ptr(), dist.data_ptr(), idx.data_ptr(), nq, nr, e, k, splits,
                                  ws.data_ptr(), ws.numel(), _stream()), "clipmi_nearest_rows")
    return dist, idx


def _edges(edges, name: str, device) -> Tuple[Optional[torch.Tensor], Optional[int], int]:
    """Host float64 edges (numpy / list) -> device float64; a device float64 tensor is taken as it is.  (tensor, pointer, count)."""
    if edges is None:
        return None, None, 0
    if not isinstance(edges, torch.Tensor):
        import numpy as np
        edges = torch.from_numpy(np.ascontiguousarray(np.asarray(edges, dtype=np.float64))).to(device)
    if edges.numel() == 0:
        return None, None, 0
    edges = _dev(edges, name, (torch.float64,))
    if edges.dim() != 1:
        raise ValueError(f"group_gap_accumulate: {name} {tuple(edges.shape)} must be a vector")
    return edges, edges.data_ptr(), edges.numel()


def group_gap_accumulate(conf: torch.Tensor, pred: torch.Tensor, labels: torch.Tensor, key: Optional[torch.Tensor] = None, key_edges=None,
                         conf_edges=None, groups: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(count, sum_conf, sum_correct) per group = key bin * (len(conf_edges) + 1) + confidence bin, a bin being the number of edges <= the
    value in float64 (include/clipmi.h, clipmi_group_gap_accumulate).  The edge lists are host float64 arrays (uploaded as they are) or
    device float64 tensors, ascending; None or empty = one bin.  Adds into ``groups`` float64 [3, G] when given, else into zeros."""
    conf = _dev(conf, "conf", (torch.float32,))
    pred = _dev(pred, "pred", (torch.int32,))
    labels = _dev(labels, "labels", (torch.int64,))
    if conf.dim() != 1 or pred.shape != conf.shape or labels.shape != conf.shape:
        raise ValueError(f"group_gap_accumulate: conf {tuple(conf.shape)}, pred {tuple(pred.shape)}, labels {tuple(labels.shape)} must be equal vectors")
    key_edges, pke, nk = _edges(key_edges, "key_edges", conf.device)
    conf_edges, pce, nc = _edges(conf_edges, "conf_edges", conf.device)
    key, pk = _opt(key, "key", (torch.float32,))
    if nk and key is None:
        raise ValueError("group_gap_accumulate: key_edges need a key")
    if key is not None and key.shape != conf.shape:
        raise ValueError(f"group_gap_accumulate: key {tuple(key.shape)} must have one entry per sample")
    G = (nk + 1) * (nc + 1)
    if G > _lib.GROUP_GAP_MAX_GROUPS:
        raise ValueError(f"group_gap_accumulate: {G} groups (at most {_lib.GROUP_GAP_MAX_GROUPS})")
    if groups is None:
        groups = torch.zeros(3, G, dtype=torch.float64, device=conf.device)
    else:
        _in_place(groups, torch.float64, f"group_gap_accumulate: groups must be a contiguous float64 GPU tensor of 3 * {G} (it is updated in place)",
                  exc=ValueError, numel=3 * G)
    check(lib.clipmi_group_gap_accumulate(conf.data_ptr(), pred.data_ptr(), labels.data_ptr(), pk, pke, nk, pce, nc, groups.data_ptr(),
                                          conf.numel(), _stream()), "clipmi_group_gap_accumulate")
    return groups


def class_counts(pred: torch.Tensor, labels: torch.Tensor, n_classes: int) -> torch.Tensor:
    """int64 [3 C + 1] on the device: true positives | predicted | labelled per class, then the number of samples whose label or
    prediction lies outside [0, C) -- those count nowhere else (include/clipmi.h, clipmi_class_counts)."""
    pred = _dev(pred, "pred", (torch.int32,))
    labels = _dev(labels, "labels", (torch.int64,))
    if pred.dim() != 1 or labels.shape != pred.shape:
        raise ValueError(f"class_counts: pred {tuple(pred.shape)} and labels {tuple(labels.shape)} must be equal vectors")
    n_classes = int(n_classes)
    if n_classes < 1:
        raise ValueError(f"class_counts: n_classes={n_classes} (>= 1)")
    counts = torch.zeros(3 * n_classes + 1, dtype=torch.int64, device=pred.device)
    check(lib.clipmi_class_counts(pred.data_ptr(), labels.data_ptr(), pred.numel(), n_classes, counts.data_ptr(), _stream()),
          "clipmi_class_counts")
    return counts


# ---- TempScaling fit (tempscaling.py:146-169) ----------------------------------------------------------------------
def _cosine_rows(cosine: torch.Tensor, labels: torch.Tensor, who: str):
    """fp32 [N, C] whose rows are contiguous (a column slice of a wider matrix keeps its row stride: ld > C) and int64 labels [N]."""
    if (isinstance(cosine, torch.Tensor) and cosine.dim() == 2 and cosine.shape[0] > 0 and cosine.stride(1) == 1
            and cosine.stride(0) >= cosine.shape[1]):
        _dev(cosine[:1], "cosine_logits", (torch.float32,))     # read in place with its row stride: the device and dtype checks only
    else:
        cosine = _dev(cosine, "cosine_logits", (torch.float32,))
    labels = _dev(labels, "labels", (torch.int64,))
    if cosine.dim() != 2 or labels.shape != (cosine.shape[0],):
        raise ValueError(f"{who}: cosine logits {tuple(cosine.shape)} must be [N, C] with one label per row, got labels {tuple(labels.shape)}")
    if cosine.shape[0] < 1 or cosine.shape[1] < 2:
        raise ValueError(f"{who}: cosine logits {tuple(cosine.shape)} need at least one row and two classes")
    return cosine, labels


def _tempscale_workspace(rows: int, device) -> torch.Tensor:
    return torch.empty(lib.clipmi_tempscale_workspace_bytes(rows), dtype=torch.uint8, device=device)


def tempscale_batch(cosine: torch.Tensor, labels: torch.Tensor, theta: torch.Tensor, rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One batch of TempScaling's loss at the device-resident ``theta`` (fp32, one element): fp32 [2] on the device,
    (mean cross-entropy of exp(theta) * cosine, its derivative by theta) over the samples ``rows`` (int32 indices; None = every row)."""
    cosine, labels = _cosine_rows(cosine, labels, "tempscale_batch")
    theta = _dev(theta, "theta", (torch.float32,))
    if theta.numel() != 1:
        raise ValueError(f"tempscale_batch: theta {tuple(theta.shape)} must hold one element")
    rows, pr = _opt(rows, "rows", (torch.int32,))
    if rows is not None and (rows.dim() != 1 or rows.numel() < 1):
        raise ValueError(f"tempscale_batch: rows {tuple(rows.shape)} must be a non-empty index vector")
    N, Cn = cosine.shape
    n_rows = N if rows is None else rows.numel()
    out = torch.empty(2, dtype=torch.float32, device=cosine.device)
    ws = _tempscale_workspace(n_rows, cosine.device)
    check(lib.clipmi_tempscale_batch(cosine.data_ptr(), cosine.stride(0), labels.data_ptr(), pr, n_rows, N, Cn, theta.data_ptr(),
                                     out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "clipmi_tempscale_batch")
    return out


def tempscale_fit(cosine: torch.Tensor, labels: torch.Tensor, state: torch.Tensor, lr: torch.Tensor, batch_size: int, epochs: int,
                  momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False,
                  order: Optional[torch.Tensor] = None, drop_last: bool = False, want_losses: bool = False) -> Optional[torch.Tensor]:
    """The whole SGD run on the scalar, enqueued without a host synchronisation (include/clipmi.h, clipmi_tempscale_fit).  ``state``
    fp32 [4] on the device is updated in place: (theta, momentum buffer, steps taken as int32 bits, last batch loss) -- (init, 0, 0, 0)
    starts a fresh fit.  ``lr`` fp32 [steps], one rate per step; ``order`` int32 [epochs, N] or None (0 .. N-1 every epoch).  Returns
    the per-step batch losses fp32 [steps] when ``want_losses``."""
    cosine, labels = _cosine_rows(cosine, labels, "tempscale_fit")
    N, Cn = cosine.shape
    batch_size, epochs = int(batch_size), int(epochs)
    if batch_size < 1 or epochs < 0:
        raise ValueError(f"tempscale_fit: batch_size={batch_size} (>= 1), epochs={epochs} (>= 0)")
    steps = epochs * (N // batch_size if drop_last else -(-N // batch_size))
    state = _dev(state, "state", (torch.float32,))
    if state.shape != (4,):
        raise ValueError(f"tempscale_fit: state {tuple(state.shape)} must be fp32 [4]")
    lr = _dev(lr, "lr", (torch.float32,))
    if lr.shape != (steps,):
        raise ValueError(f"tempscale_fit: lr {tuple(lr.shape)} must hold one rate per step ({steps})")
    order, po = _opt(order, "order", (torch.int32,))
    if order is not None and order.shape != (epochs, N):
        raise ValueError(f"tempscale_fit: order {tuple(order.shape)} must be [epochs, N] = [{epochs}, {N}]")
    losses = torch.empty(steps, dtype=torch.float32, device=cosine.device) if want_losses else None
    ws = _tempscale_workspace(min(batch_size, N), cosine.device)
    check(lib.clipmi_tempscale_fit(cosine.data_ptr(), cosine.stride(0), labels.data_ptr(), po, N, Cn, batch_size, epochs, int(bool(drop_last)),
                                   lr.data_ptr(), float(momentum), float(dampening), float(weight_decay), int(bool(nesterov)),
                                   state.data_ptr(), None if losses is None else losses.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "clipmi_tempscale_fit")
    return losses


# ---- Parameterized temperature scaling (CALIBRATION.SCALING.MODE 'ParameterizedTempScaling', train.py:238-247) ------
def _pts_rows(logits: torch.Tensor, who: str) -> torch.Tensor:
    """fp32 [N, C] whose rows are contiguous (a column slice of a wider matrix keeps its row stride: ld > C); N may be 0."""
    if (isinstance(logits, torch.Tensor) and logits.dim() == 2 and logits.shape[0] > 0 and logits.stride(1) == 1
            and logits.stride(0) >= logits.shape[1]):
        _dev(logits[:1], "logits", (torch.float32,))     # read in place with its row stride: the device and dtype checks only
    else:
        logits = _dev(logits, "logits", (torch.float32,))
    if logits.dim() != 2:
        raise ValueError(f"{who}: logits {tuple(logits.shape)} must be [N, C]")
    return logits


def _pts_net(who: str, n_layers: int, n_nodes: int, top_k: int, C: int) -> int:
    """The parameter count of the net after the library's own limits (include/clipmi.h, clipmi_pts_param_count)."""
    n_layers, n_nodes, top_k = int(n_layers), int(n_nodes), int(top_k)
    P = lib.clipmi_pts_param_count(n_layers, n_nodes, top_k)
    if P == 0:
        raise ValueError(f"{who}: n_layers={n_layers} (0 .. 4), n_nodes={n_nodes} (1 .. 32), top_k={top_k} (1 .. 32)")
    if C < top_k or C < 2:
        raise ValueError(f"{who}: {C} classes (at least 2, and at least top_k={top_k})")
    return P


def pts_topk(logits: torch.Tensor, top_k: int) -> torch.Tensor:
    """fp32 [N, top_k]: the ``top_k`` largest values of every row, descending -- ``torch.sort(descending=True)``'s first columns, bit for
    bit (+0.0 and -0.0 compare equal and come in index order).  -inf is an ordinary value; a row that holds a NaN gives NaNs
    (include/clipmi.h, clipmi_pts_topk)."""
    logits = _pts_rows(logits, "pts_topk")
    N, Cn = logits.shape
    top_k = int(top_k)
    _pts_net("pts_topk", 0, 1, top_k, Cn)
    out = torch.empty(N, top_k, dtype=torch.float32, device=logits.device)
    check(lib.clipmi_pts_topk(logits.data_ptr(), logits.stride(0) if N else Cn, N, Cn, top_k, out.data_ptr(), _stream()), "clipmi_pts_topk")
    return out


def pts_apply(logits: torch.Tensor, params: torch.Tensor, n_layers: int, n_nodes: int, top_k: int, out: Optional[torch.Tensor] = None,
              want_temperature: bool = False):
    """``logits / T`` with every row's own temperature from the PTS net ``params`` (fp32 [P], include/clipmi.h), in one launch.  ``out``
    (fp32 [N, C] with contiguous rows) may be ``logits`` itself; None allocates.  Returns out, or (out, T fp32 [N]) with
    ``want_temperature``."""
    logits = _pts_rows(logits, "pts_apply")
    N, Cn = logits.shape
    P = _pts_net("pts_apply", n_layers, n_nodes, top_k, Cn)
    params = _dev(params, "params", (torch.float32,))
    if params.shape != (P,):
        raise ValueError(f"pts_apply: params {tuple(params.shape)} must be fp32 [{P}]")
    if out is None:
        out = torch.empty(N, Cn, dtype=torch.float32, device=logits.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.shape == logits.shape and out.device == logits.device
              and (N == 0 or (out.stride(1) == 1 and out.stride(0) >= Cn))):
        raise ValueError(f"pts_apply: out must be an fp32 GPU tensor {tuple(logits.shape)} with contiguous rows")
    temp = torch.empty(N, dtype=torch.float32, device=logits.device) if want_temperature else None
    check(lib.clipmi_pts_apply(logits.data_ptr(), logits.stride(0) if N else Cn, N, Cn, params.data_ptr(), int(n_layers), int(n_nodes), int(top_k),
                               out.data_ptr(), out.stride(0) if N else Cn, None if temp is None else temp.data_ptr(), _stream()), "clipmi_pts_apply")
    return (out, temp) if want_temperature else out


def _pts_problem(who: str, logits, labels, n_layers, n_nodes, top_k):
    logits = _pts_rows(logits, who)
    labels = _dev(labels, "labels", (torch.int64,))
    N, Cn = logits.shape
    if N < 1 or labels.shape != (N,):
        raise ValueError(f"{who}: logits {tuple(logits.shape)} must be [N >= 1, C] with one label per row, got labels {tuple(labels.shape)}")
    return logits, labels, _pts_net(who, n_layers, n_nodes, top_k, Cn)


def pts_eval(features: torch.Tensor, logits: torch.Tensor, labels: torch.Tensor, params: torch.Tensor, n_layers: int, n_nodes: int, top_k: int,
             rows: Optional[torch.Tensor] = None, first: int = 0, n_rows: Optional[int] = None) -> torch.Tensor:
    """One batch of the PTS loss at ``params``, nothing updated: fp32 [1 + P] on the device, (mean loss, the mean gradient of every
    parameter) over the samples ``rows`` (int32 indices), or ``first .. first + n_rows - 1`` (every row by default).  ``features`` is
    ``pts_topk(logits, top_k)``."""
    logits, labels, P = _pts_problem("pts_eval", logits, labels, n_layers, n_nodes, top_k)
    N, Cn = logits.shape
    features = _dev(features, "features", (torch.float32,))
    params = _dev(params, "params", (torch.float32,))
    if features.shape != (N, int(top_k)) or params.shape != (P,):
        raise ValueError(f"pts_eval: features {tuple(features.shape)} must be [{N}, {int(top_k)}] and params {tuple(params.shape)} [{P}]")
    rows, pr = _opt(rows, "rows", (torch.int32,))
    if rows is not None:
        if rows.dim() != 1 or rows.numel() < 1:
            raise ValueError(f"pts_eval: rows {tuple(rows.shape)} must be a non-empty index vector")
        first, n = 0, rows.numel()
    else:
        first = int(first)
        n = N - first if n_rows is None else int(n_rows)
        if first < 0 or n < 1 or first + n > N:
            raise ValueError(f"pts_eval: rows {first} .. {first + n} of {N}")
    out = torch.empty(1 + P, dtype=torch.float32, device=logits.device)
    ws = torch.empty(n * (2 + 2 * int(n_layers) * int(n_nodes)), dtype=torch.float32, device=logits.device)
    check(lib.clipmi_pts_eval(features.data_ptr(), logits.data_ptr(), logits.stride(0), labels.data_ptr(), pr, first, n, N, Cn, params.data_ptr(),
                              int(n_layers), int(n_nodes), int(top_k), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "clipmi_pts_eval")
    return out


def pts_fit(logits: torch.Tensor, labels: torch.Tensor, state: torch.Tensor, n_layers: int, n_nodes: int, top_k: int, lr: torch.Tensor,
            batch_size: int, epochs: int, optimizer: int = _lib.OPTIM_SGD, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
            nesterov: bool = False, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, order: Optional[torch.Tensor] = None,
            drop_last: bool = False, want_losses: bool = False) -> Optional[torch.Tensor]:
    """The whole PTS run, enqueued without a host synchronisation (include/clipmi.h, clipmi_pts_fit).  ``state`` fp32 [3 P + 2] on the
    device is updated in place: (params, two optimiser buffers, steps taken as int32 bits, last batch loss) -- (init, zeros) starts a
    fresh fit, a returned state continues one.  ``lr`` fp32 [steps], one rate per step; ``order`` int32 [epochs, N] or None (0 .. N-1
    every epoch).  Returns the per-step batch losses fp32 [steps] when ``want_losses``."""
    logits, labels, P = _pts_problem("pts_fit", logits, labels, n_layers, n_nodes, top_k)
    N, Cn = logits.shape
    batch_size, epochs = int(batch_size), int(epochs)
    if batch_size < 1 or epochs < 0:
        raise ValueError(f"pts_fit: batch_size={batch_size} (>= 1), epochs={epochs} (>= 0)")
    if optimizer not in (_lib.OPTIM_SGD, _lib.OPTIM_ADAM):
        raise ValueError(f"pts_fit: optimizer={optimizer!r} (OPTIM_SGD or OPTIM_ADAM)")
    steps = epochs * (N // batch_size if drop_last else -(-N // batch_size))
    _in_place(state, torch.float32, f"pts_fit: state must be a contiguous fp32 GPU tensor of 3 * {P} + 2 (it is updated in place)", exc=ValueError,
              numel=3 * P + 2)
    lr = _dev(lr, "lr", (torch.float32,))
    if lr.shape != (steps,):
        raise ValueError(f"pts_fit: lr {tuple(lr.shape)} must hold one rate per step ({steps})")
    order, po = _opt(order, "order", (torch.int32,))
    if order is not None and order.shape != (epochs, N):
        raise ValueError(f"pts_fit: order {tuple(order.shape)} must be [epochs, N] = [{epochs}, {N}]")
    losses = torch.empty(steps, dtype=torch.float32, device=logits.device) if want_losses else None
    if steps == 0:   # nothing to launch, and an empty lr has no address to hand over
        return losses
    ws = torch.empty(N * int(top_k) + min(batch_size, N) * (2 + 2 * int(n_layers) * int(n_nodes)), dtype=torch.float32, device=logits.device)
    check(lib.clipmi_pts_fit(logits.data_ptr(), logits.stride(0), labels.data_ptr(), po, N, Cn, int(n_layers), int(n_nodes), int(top_k), batch_size,
                             epochs, int(bool(drop_last)), lr.data_ptr(), int(optimizer), float(momentum), float(dampening), float(weight_decay),
                             int(bool(nesterov)), float(betas[0]), float(betas[1]), float(eps), state.data_ptr(),
                             None if losses is None else losses.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "clipmi_pts_fit")
    return losses


# ---- CLIP-Adapter training (clip_adapter.py:138-187) ---------------------------------------------------------------
def _adapter_problem(features, labels, text, w1, w2, m1, m2, momentum: float, who: str):
    """The tensors of one adapter training call, checked: raw features fp32 [N, E] (contiguous rows, row stride kept), labels int64 [N],
    text fp32 [C, E], and the weights and momentum buffers fp32, contiguous, updated where they lie.  Returns (features, labels, text)."""
    if (isinstance(features, torch.Tensor) and features.dim() == 2 and features.shape[0] > 0 and features.stride(1) == 1
            and features.stride(0) >= features.shape[1]):
        _dev(features[:1], "features", (torch.float32,))     # read in place with its row stride: the device and dtype checks only
    else:
        features = _dev(features, "features", (torch.float32,))
    labels = _dev(labels, "labels", (torch.int64,))
    text = _dev(text, "text_features", (torch.float32,))
    if features.dim() != 2 or features.shape[0] < 1 or labels.shape != (features.shape[0],):
        raise ValueError(f"{who}: features {tuple(features.shape)} must be [N >= 1, E] with one label per row, got labels {tuple(labels.shape)}")
    E = features.shape[1]
    if text.dim() != 2 or text.shape[1] != E or text.shape[0] < 2:
        raise ValueError(f"{who}: text features {tuple(text.shape)} must be [C >= 2, E = {E}]")
    if not isinstance(w1, torch.Tensor) or w1.dim() != 2 or w1.shape[1] != E or w1.shape[0] < 1 or tuple(getattr(w2, "shape", ())) != (E, w1.shape[0]):
        raise ValueError(f"{who}: adapter shapes do not chain (E = {E}, w1 {tuple(getattr(w1, 'shape', ()))}, w2 {tuple(getattr(w2, 'shape', ()))})")
    for t, name in ((w1, "w1"), (w2, "w2")) + (((m1, "m1"), (m2, "m2")) if momentum != 0.0 else ()):
        _dev(t, name, (torch.float32,))
        _in_place(t, torch.float32, f"{who}: {name} is updated in place: a contiguous fp32 tensor on the GPU")
    if momentum != 0.0 and (m1.shape != w1.shape or m2.shape != w2.shape):
        raise ValueError(f"{who}: the momentum buffers {tuple(m1.shape)}, {tuple(m2.shape)} must have the weights' shapes")
    return features, labels, text


def _adapter_workspace(rows: int, E: int, H: int, Cn: int, device) -> torch.Tensor:
    return torch.empty(lib.clipmi_adapter_train_workspace_bytes(rows, E, H, Cn), dtype=torch.uint8, device=device)


def adapter_train_step(features: torch.Tensor, labels: torch.Tensor, text: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor,
                       m1: Optional[torch.Tensor], m2: Optional[torch.Tensor], lr: torch.Tensor, ratio: float, scale: float, first_step: bool,
                       momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False,
                       want_loss: bool = False) -> Optional[torch.Tensor]:
    """One SGD step of CLIP-Adapter's bottleneck on the batch ``features`` fp32 [B, E] (raw image features), enqueued without a host
    synchronisation (include/clipmi.h, clipmi_adapter_train_step).  ``w1`` [H, E], ``w2`` [E, H] and the momentum buffers are updated in
    place; ``lr`` fp32 [1] on the device; ``scale`` = exp(logit_scale); ``first_step`` initialises the buffers from this step's gradient.
    Returns the batch loss fp32 [1] on the device when ``want_loss``."""
    features, labels, text = _adapter_problem(features, labels, text, w1, w2, m1, m2, momentum, "adapter_train_step")
    lr = _dev(lr, "lr", (torch.float32,))
    if lr.numel() != 1:
        raise ValueError(f"adapter_train_step: lr {tuple(lr.shape)} must hold one rate")
    (B, E), H, Cn = features.shape, w1.shape[0], text.shape[0]
    loss = torch.empty(1, dtype=torch.float32, device=features.device) if want_loss else None
    ws = _adapter_workspace(B, E, H, Cn, features.device)
    pm1, pm2 = (m1.data_ptr(), m2.data_ptr()) if momentum != 0.0 else (None, None)
    check(lib.clipmi_adapter_train_step(features.data_ptr(), features.stride(0), labels.data_ptr(), text.data_ptr(), w1.data_ptr(), w2.data_ptr(),
                                        pm1, pm2, B, E, H, Cn, float(ratio), float(scale), lr.data_ptr(), int(bool(first_step)), float(momentum),
                                        float(dampening), float(weight_decay), int(bool(nesterov)), None if loss is None else loss.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _stream()), "clipmi_adapter_train_step")
    return loss


def adapter_fit(features: torch.Tensor, labels: torch.Tensor, text: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor,
                m1: Optional[torch.Tensor], m2: Optional[torch.Tensor], lr: torch.Tensor, ratio: float, scale: float, batch_size: int, epochs: int,
                momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False,
                order: Optional[torch.Tensor] = None, drop_last: bool = False, first_step: bool = True,
                want_losses: bool = False, monitor: Optional[dict] = None) -> Optional[torch.Tensor]:
    """The whole SGD run of CLIP-Adapter's bottleneck from the cached ``features`` fp32 [N, E], enqueued without a host synchronisation
    (include/clipmi.h, clipmi_adapter_fit).  ``w1``, ``w2`` and the momentum buffers are updated in place; ``lr`` fp32 [steps], one rate
    per step; ``order`` int32 [epochs, N] or None (0 .. N-1 every epoch).  Returns the per-step batch losses fp32 [steps] when
    ``want_losses``.

    ``monitor`` (``fit_monitor(...)``): the monitored form, clipmi_adapter_fit_monitored -- behind every epoch the validation logits, the
    epoch record and, with a best slot, the selection of the block [w1 | w2], which ``w1`` and ``w2`` must then be views of
    (``adapter_master_block``).  The same steps, the same fitted bits; still nothing synchronises."""
    features, labels, text = _adapter_problem(features, labels, text, w1, w2, m1, m2, momentum, "adapter_fit")
    (N, E), H, Cn = features.shape, w1.shape[0], text.shape[0]
    batch_size, epochs = int(batch_size), int(epochs)
    if batch_size < 1 or epochs < 0:
        raise ValueError(f"adapter_fit: batch_size={batch_size} (>= 1), epochs={epochs} (>= 0)")
    steps = epochs * (N // batch_size if drop_last else -(-N // batch_size))
    lr = _dev(lr, "lr", (torch.float32,))
    if lr.shape != (steps,):
        raise ValueError(f"adapter_fit: lr {tuple(lr.shape)} must hold one rate per step ({steps})")
    order, po = _opt(order, "order", (torch.int32,))
    if order is not None and order.shape != (epochs, N):
        raise ValueError(f"adapter_fit: order {tuple(order.shape)} must be [epochs, N] = [{epochs}, {N}]")
    losses = torch.empty(steps, dtype=torch.float32, device=features.device) if want_losses else None
    ws = _adapter_workspace(min(batch_size, N), E, H, Cn, features.device)
    pm1, pm2 = (m1.data_ptr(), m2.data_ptr()) if momentum != 0.0 else (None, None)
    args = (features.data_ptr(), features.stride(0), labels.data_ptr(), po, text.data_ptr(), w1.data_ptr(), w2.data_ptr(),
            pm1, pm2, N, E, H, Cn, batch_size, epochs, int(bool(drop_last)), float(ratio), float(scale), lr.data_ptr(),
            int(bool(first_step)), float(momentum), float(dampening), float(weight_decay), int(bool(nesterov)),
            None if losses is None else losses.data_ptr(), ws.data_ptr(), ws.numel())
    if monitor is None:
        check(lib.clipmi_adapter_fit(*args, _stream()), "clipmi_adapter_fit")
    else:
        tail = _fit_monitor_args("adapter_fit", monitor, E, Cn, epochs, 2 * E * H, lib.clipmi_adapter_fit_monitored_workspace_bytes)
        check(lib.clipmi_adapter_fit_monitored(*args, *tail, _stream()), "clipmi_adapter_fit_monitored")
    return losses


# ---- TaskRes training (taskres.py:96-210) --------------------------------------------------------------------------
_OPTIMISERS = {"sgd": _lib.OPTIM_SGD, "adam": _lib.OPTIM_ADAM}


def _taskres_problem(features, labels, base, residuals, state1, state2, optimizer: str, momentum: float, who: str):
    """The tensors of one TaskRes training call, checked: raw features fp32 [N, E] (contiguous rows, row stride kept), labels int64 [N],
    base text features fp32 [C, E], and the residuals and the optimiser's state fp32 [C, E], contiguous, updated where they lie.
    Returns (features, labels, base, optimiser code, state1 pointer, state2 pointer)."""
    if optimizer not in _OPTIMISERS:
        raise ValueError(f"{who}: optimizer {optimizer!r} must be 'adam' or 'sgd'")
    if (isinstance(features, torch.Tensor) and features.dim() == 2 and features.shape[0] > 0 and features.stride(1) == 1
            and features.stride(0) >= features.shape[1]):
        _dev(features[:1], "features", (torch.float32,))     # read in place with its row stride: the device and dtype checks only
    else:
        features = _dev(features, "features", (torch.float32,))
    labels = _dev(labels, "labels", (torch.int64,))
    base = _dev(base, "base_text_features", (torch.float32,))
    if features.dim() != 2 or features.shape[0] < 1 or labels.shape != (features.shape[0],):
        raise ValueError(f"{who}: features {tuple(features.shape)} must be [N >= 1, E] with one label per row, got labels {tuple(labels.shape)}")
    E = features.shape[1]
    if base.dim() != 2 or base.shape[1] != E or base.shape[0] < 2:
        raise ValueError(f"{who}: base text features {tuple(base.shape)} must be [C >= 2, E = {E}]")
    used = [(residuals, "residuals")]
    if optimizer == "adam":
        used += [(state1, "state1"), (state2, "state2")]
    elif momentum != 0.0:
        used += [(state1, "state1")]
    for t, name in used:
        _dev(t, name, (torch.float32,))
        _in_place(t, torch.float32, f"{who}: {name} is updated in place: a contiguous fp32 tensor on the GPU")
        if t.shape != base.shape:
            raise ValueError(f"{who}: {name} {tuple(t.shape)} must have the base text features' shape {tuple(base.shape)}")
    p1 = used[1][0].data_ptr() if len(used) > 1 else None
    p2 = used[2][0].data_ptr() if len(used) > 2 else None
    return features, labels, base, _OPTIMISERS[optimizer], p1, p2


def _taskres_workspace(rows: int, E: int, Cn: int, device) -> torch.Tensor:
    return torch.empty(lib.clipmi_taskres_train_workspace_bytes(rows, E, Cn), dtype=torch.uint8, device=device)


def taskres_train_step(features: torch.Tensor, labels: torch.Tensor, base: torch.Tensor, residuals: torch.Tensor,
                       state1: Optional[torch.Tensor], state2: Optional[torch.Tensor], lr: torch.Tensor, alpha: float, scale: float,
                       steps_done: int, optimizer: str = "adam", weight_decay: float = 0.0, momentum: float = 0.0, dampening: float = 0.0,
                       nesterov: bool = False, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                       want_loss: bool = False) -> Optional[torch.Tensor]:
    """One optimiser step of TaskRes' residuals on the batch ``features`` fp32 [B, E] (raw image features), enqueued without a host
    synchronisation (include/clipmi.h, clipmi_taskres_train_step).  ``residuals`` [C, E] and the state are updated in place: ``state1``
    is SGD's momentum buffer or Adam's first moment, ``state2`` Adam's second moment; ``lr`` fp32 [1] on the device; ``scale`` =
    exp(logit_scale); ``steps_done`` counts the steps taken before this one.  Returns the batch loss fp32 [1] on the device when
    ``want_loss``."""
    features, labels, base, kind, p1, p2 = _taskres_problem(features, labels, base, residuals, state1, state2, optimizer, momentum,
                                                            "taskres_train_step")
    lr = _dev(lr, "lr", (torch.float32,))
    if lr.numel() != 1:
        raise ValueError(f"taskres_train_step: lr {tuple(lr.shape)} must hold one rate")
    (B, E), Cn = features.shape, base.shape[0]
    loss = torch.empty(1, dtype=torch.float32, device=features.device) if want_loss else None
    ws = _taskres_workspace(B, E, Cn, features.device)
    check(lib.clipmi_taskres_train_step(features.data_ptr(), features.stride(0), labels.data_ptr(), base.data_ptr(), residuals.data_ptr(), p1, p2,
                                        B, E, Cn, float(alpha), float(scale), lr.data_ptr(), kind, int(steps_done), float(weight_decay),
                                        float(momentum), float(dampening), int(bool(nesterov)), float(betas[0]), float(betas[1]), float(eps),
                                        None if loss is None else loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "clipmi_taskres_train_step")
    return loss


def taskres_fit(features: torch.Tensor, labels: torch.Tensor, base: torch.Tensor, residuals: torch.Tensor, state1: Optional[torch.Tensor],
                state2: Optional[torch.Tensor], lr: torch.Tensor, alpha: float, scale: float, batch_size: int, epochs: int,
                optimizer: str = "adam", weight_decay: float = 0.0, momentum: float = 0.0, dampening: float = 0.0, nesterov: bool = False,
                betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, order: Optional[torch.Tensor] = None, drop_last: bool = False,
                steps_done: int = 0, want_losses: bool = False, monitor: Optional[dict] = None) -> Optional[torch.Tensor]:
    """The whole training run of TaskRes' residuals from the cached ``features`` fp32 [N, E], enqueued without a host synchronisation
    (include/clipmi.h, clipmi_taskres_fit).  ``residuals`` and the state are updated in place; ``lr`` fp32 [steps], one rate per step;
    ``order`` int32 [epochs, N] or None (0 .. N-1 every epoch).  Returns the per-step batch losses fp32 [steps] when ``want_losses``.

    ``monitor`` (``fit_monitor(...)``): the monitored form, clipmi_taskres_fit_monitored -- behind every epoch the validation logits, the
    epoch record and, with a best slot, the selection of ``residuals``.  The same steps, the same fitted bits; still nothing synchronises."""
    features, labels, base, kind, p1, p2 = _taskres_problem(features, labels, base, residuals, state1, state2, optimizer, momentum, "taskres_fit")
    (N, E), Cn = features.shape, base.shape[0]
    batch_size, epochs = int(batch_size), int(epochs)
    if batch_size < 1 or epochs < 0:
        raise ValueError(f"taskres_fit: batch_size={batch_size} (>= 1), epochs={epochs} (>= 0)")
    steps = epochs * (N // batch_size if drop_last else -(-N // batch_size))
    lr = _dev(lr, "lr", (torch.float32,))
    if lr.shape != (steps,):
        raise ValueError(f"taskres_fit: lr {tuple(lr.shape)} must hold one rate per step ({steps})")
    order, po = _opt(order, "order", (torch.int32,))
    if order is not None and order.shape != (epochs, N):
        raise ValueError(f"taskres_fit: order {tuple(order.shape)} must be [epochs, N] = [{epochs}, {N}]")
    losses = torch.empty(steps, dtype=torch.float32, device=features.device) if want_losses else None
    ws = _taskres_workspace(min(batch_size, N), E, Cn, features.device)
    args = (features.data_ptr(), features.stride(0), labels.data_ptr(), po, base.data_ptr(), residuals.data_ptr(), p1, p2,
            N, E, Cn, batch_size, epochs, int(bool(drop_last)), float(alpha), float(scale), lr.data_ptr(), kind,
            int(steps_done), float(weight_decay), float(momentum), float(dampening), int(bool(nesterov)), float(betas[0]),
            float(betas[1]), float(eps), None if losses is None else losses.data_ptr(), ws.data_ptr(), ws.numel())
    if monitor is None:
        check(lib.clipmi_taskres_fit(*args, _stream()), "clipmi_taskres_fit")
    else:
        tail = _fit_monitor_args("taskres_fit", monitor, E, Cn, epochs, Cn * E, lib.clipmi_taskres_fit_monitored_workspace_bytes)
        check(lib.clipmi_taskres_fit_monitored(*args, *tail, _stream()), "clipmi_taskres_fit_monitored")
    return losses


# ---- CoCoOp glue (cocoop.py:154-199) -------------------------------------------------------------------------------
def cocoop_ctx(img_n: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
               ctx: torch.Tensor) -> torch.Tensor:
    """ctx + meta_net(img_n) per image -> fp32 [B, n_ctx, D]."""
    f32 = (torch.float32,)
    img_n, w1, b1, w2, b2, ctx = (_dev(t, n, f32) for t, n in ((img_n, "img_n"), (w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2"), (ctx, "ctx")))
    B, E = img_n.shape
    H, D, n_ctx = w1.shape[0], w2.shape[0], ctx.shape[0]
    if w1.shape != (H, E) or b1.shape != (H,) or w2.shape != (D, H) or b2.shape != (D,) or ctx.shape != (n_ctx, D):
        raise ValueError("cocoop_ctx: meta-net shapes do not chain")
    out = torch.empty(B, n_ctx, D, dtype=torch.float32, device=img_n.device)
    check(lib.clipmi_cocoop_ctx(img_n.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), ctx.data_ptr(),
                                out.data_ptr(), B, E, H, D, n_ctx, _stream()), "clipmi_cocoop_ctx")
    return out


def cocoop_prompts(base: torch.Tensor, ctx_shifted: torch.Tensor) -> torch.Tensor:
    """[C,L,D] base embeddings x [nb,n_ctx,D] shifted contexts -> fp16 prompts [nb*C, L, D]."""
    base = _dev(base, "base", (torch.float16, torch.float32))
    ctx_shifted = _dev(ctx_shifted, "ctx_shifted", (torch.float32,))
    Cn, L, D = base.shape
    nb, n_ctx, d2 = ctx_shifted.shape
    if d2 != D:
        raise ValueError("cocoop_prompts: widths differ")
    out = torch.empty(nb * Cn, L, D, dtype=torch.float16, device=base.device)
    check(lib.clipmi_cocoop_prompts(base.data_ptr(), _DT[base.dtype], ctx_shifted.data_ptr(), out.data_ptr(), nb, Cn, L, D, n_ctx,
                                    _stream()), "clipmi_cocoop_prompts")
    return out


def logits_per_image(img_n: torch.Tensor, txt: torch.Tensor, scale: float, dac_conf: Optional[torch.Tensor] = None,
                     want_conf_pred: bool = True, want_last_text: bool = True):
    """logits[b,c] = scale * <img_n[b], normalise(txt[b,c])>; txt [B,C,E] un-normalised."""
    img_n = _dev(img_n, "img_n", (torch.float32,))
    txt = _dev(txt, "txt", (torch.float32,))
    B, E = img_n.shape
    if txt.dim() != 3 or txt.shape[0] != B or txt.shape[2] != E:
        raise ValueError(f"logits_per_image: txt must be [B={B}, C, E={E}], got {tuple(txt.shape)}")
    Cn = txt.shape[1]
    dac_conf, pd = _dac(dac_conf, Cn, "logits_per_image")
    logits = torch.empty(B, Cn, dtype=torch.float32, device=img_n.device)
    conf, pred, pc, pp = _conf_pred(want_conf_pred, B, img_n.device)
    last = pl = None
    if want_last_text:
        last = torch.empty(Cn, E, dtype=torch.float32, device=img_n.device)
        pl = last.data_ptr()
    check(lib.clipmi_logits_per_image(img_n.data_ptr(), txt.data_ptr(), float(scale), pd, logits.data_ptr(), pc, pp, pl, B, Cn, E,
                                      _stream()), "clipmi_logits_per_image")
    return logits, conf, pred, last


def group_mean(x: torch.Tensor, group: int) -> torch.Tensor:
    """[G*group, E] -> [G, E] mean over consecutive groups of rows (ProDA's prompt-ensemble mean, proda.py:328-332)."""
    x = _dev(x, "x", (torch.float32,))
    rows, E = x.shape
    if group <= 0 or rows % group:
        raise ValueError(f"group_mean: {rows} rows do not split into groups of {group}")
    out = torch.empty(rows // group, E, dtype=torch.float32, device=x.device)
    check(lib.clipmi_group_mean(x.data_ptr(), out.data_ptr(), rows // group, group, E, _stream()), "clipmi_group_mean")
    return out


def adapter_blend(feats: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, ratio: float) -> torch.Tensor:
    """ratio * relu(W2 relu(W1 f)) + (1 - ratio) * f  (CLIP-Adapter, clip_adapter.py:138-172)."""
    feats, w1, w2 = (_dev(t, n, (torch.float32,)) for t, n in ((feats, "feats"), (w1, "w1"), (w2, "w2")))
    B, E = feats.shape
    H = w1.shape[0]
    if w1.shape != (H, E) or w2.shape != (E, H):
        raise ValueError("adapter_blend: adapter shapes do not chain")
    out = torch.empty_like(feats)
    check(lib.clipmi_adapter_blend(feats.data_ptr(), w1.data_ptr(), w2.data_ptr(), float(ratio), out.data_ptr(), B, E, H, _stream()),
          "clipmi_adapter_blend")
    return out


def scale_add(a: torch.Tensor, b: torch.Tensor, alpha: float) -> torch.Tensor:
    """a + alpha * b (TaskRes, taskres.py:105-106)."""
    a, b = _dev(a, "a", (torch.float32,)), _dev(b, "b", (torch.float32,))
    if a.shape != b.shape:
        raise ValueError("scale_add: shapes differ")
    out = torch.empty_like(a)
    check(lib.clipmi_scale_add(a.data_ptr(), b.data_ptr(), float(alpha), out.data_ptr(), a.numel(), _stream()), "clipmi_scale_add")
    return out


# ---- CoOp's training path at operator level (include/clipmi.h "CoOp's context trained on the device", csrc/text_backward.hip, csrc/prompt_train.hip) ----
def layernorm_backward(x: torch.Tensor, gamma: torch.Tensor, dy: torch.Tensor, g: torch.Tensor, g16: Optional[torch.Tensor] = None,
                       row_idx: Optional[torch.Tensor] = None, eps: float = 1e-5) -> None:
    """LayerNorm's backward from the saved fp32 rows ``x`` [R, D] (the rows may be a column slice): ``g[row(r)] += dX(r)`` in place and
    ``g16[row(r)] = fp16(g[row(r)])``; ``dy`` fp32 or fp16 [rows, D] dense, ``row(r) = row_idx[r]`` (int32) or r."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        raise TypeError("layernorm_backward: x must be an fp32 [R, D] tensor on the GPU with unit column stride")
    gamma = _dev(gamma, "gamma", (torch.float32,))
    dy = _dev(dy, "dy", (torch.float16, torch.float32))
    rows, D = dy.shape
    _in_place(g, torch.float32, "layernorm_backward: g must be a contiguous fp32 tensor on the GPU")
    if g16 is not None:
        _in_place(g16, torch.float16, "layernorm_backward: g16 must be a contiguous fp16 tensor on the GPU", numel=g.numel())
    if x.dim() != 2 or x.shape[1] != D or gamma.shape != (D,) or g.dim() != 2 or g.shape[1] != D:
        raise ValueError("layernorm_backward: x [R, D], gamma [D], dy [rows, D] and g [R, D] do not agree")
    row_idx, pi = _opt(row_idx, "row_idx", (torch.int32,))
    if row_idx is None and (x.shape[0] < rows or g.shape[0] < rows):
        raise ValueError("layernorm_backward: fewer rows in x or g than in dy")
    if row_idx is not None and row_idx.shape != (rows,):
        raise ValueError("layernorm_backward: one row index per row of dy")
    check(lib.clipmi_layernorm_backward(x.data_ptr(), x.stride(0), pi, gamma.data_ptr(), dy.data_ptr(), _DT[dy.dtype], g.data_ptr(),
                                        None if g16 is None else g16.data_ptr(), rows, D, float(eps), _stream()), "clipmi_layernorm_backward")


def quickgelu_backward(h: torch.Tensor, d_a: torch.Tensor) -> torch.Tensor:
    """``d_a * d/dh (h sigmoid(1.702 h))`` from the saved fp16 pre-activation ``h``; fp16 in and out."""
    h, d_a = _dev(h, "h", (torch.float16,)), _dev(d_a, "d_a", (torch.float16,))
    if h.shape != d_a.shape:
        raise ValueError("quickgelu_backward: shapes differ")
    out = torch.empty_like(h)
    check(lib.clipmi_quickgelu_backward(h.data_ptr(), d_a.data_ptr(), out.data_ptr(), h.numel(), _stream()), "clipmi_quickgelu_backward")
    return out


def attention_backward(qkv: torch.Tensor, d_out: torch.Tensor, n_seq: int, n_head: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The backward of the causal ``attention``: ``qkv`` fp16 [N * L, 3 * 64 * H], ``d_out`` fp16 [N * L, 64 * H] -> dqkv fp16 in qkv's
    layout (written into ``out`` when given: only its first N * L rows are touched)."""
    qkv, d_out = _dev(qkv, "qkv", (torch.float16,)), _dev(d_out, "d_out", (torch.float16,))
    M, D3 = qkv.shape
    if n_seq < 0 or n_head < 1 or D3 != 3 * 64 * n_head or (n_seq and M % n_seq) or d_out.shape != (M, 64 * n_head):
        raise ValueError(f"attention_backward: qkv {tuple(qkv.shape)} / d_out {tuple(d_out.shape)} do not fit {n_seq} sequences of {n_head} heads")
    if out is None:
        out = torch.empty_like(qkv)
    else:
        _in_place(out, torch.float16, "attention_backward: out must be a contiguous fp16 tensor on the GPU")
        if out.numel() < qkv.numel():
            raise ValueError("attention_backward: out is too small")
    L = M // n_seq if n_seq else 1
    check(lib.clipmi_attention_backward(qkv.data_ptr(), d_out.data_ptr(), out.data_ptr(), n_seq, L, n_head, _stream()), "clipmi_attention_backward")
    return out


def attention_backward_long(qkv: torch.Tensor, d_out: torch.Tensor, n_seq: int, n_head: int, out: Optional[torch.Tensor] = None,
                            workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The backward of the ``attention`` WITHOUT a mask for up to 640 token rows per sequence (ViT-L/14's lengths with prompt rows;
    clipmi_attention_backward_long): operands and result as ``attention_backward``.  ``workspace``: a contiguous uint8 tensor on the GPU of
    at least ``clipmi_attention_backward_long_bytes(N, L, H)`` = 12 N H L bytes, allocated here when not given."""
    qkv, d_out = _dev(qkv, "qkv", (torch.float16,)), _dev(d_out, "d_out", (torch.float16,))
    M, D3 = qkv.shape
    if n_seq < 0 or n_head < 1 or D3 != 3 * 64 * n_head or (n_seq and M % n_seq) or d_out.shape != (M, 64 * n_head):
        raise ValueError(f"attention_backward_long: qkv {tuple(qkv.shape)} / d_out {tuple(d_out.shape)} do not fit {n_seq} sequences of {n_head} heads")
    if out is None:
        out = torch.empty_like(qkv)
    else:
        _in_place(out, torch.float16, "attention_backward_long: out must be a contiguous fp16 tensor on the GPU")
        if out.numel() < qkv.numel():
            raise ValueError("attention_backward_long: out is too small")
    L = M // n_seq if n_seq else 1
    need = lib.clipmi_attention_backward_long_bytes(n_seq, L, n_head)
    if workspace is None:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=qkv.device)
    else:
        _in_place(workspace, torch.uint8, "attention_backward_long: workspace must be a contiguous uint8 tensor on the GPU")
    check(lib.clipmi_attention_backward_long(qkv.data_ptr(), d_out.data_ptr(), out.data_ptr(), workspace.data_ptr(), workspace.numel(), n_seq, L, n_head,
                                             _stream()), "clipmi_attention_backward_long")
    return out


def _head_inputs(who: str, features, labels, text):
    """(labels, text, B, E, C) of a loss head after the checks coop_head and prompt_head share."""
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.stride(1) != 1:
        raise ValueError(f"{who}: features must be a [B, E] tensor with unit column stride")
    if not features.is_cuda or features.dtype != torch.float32:
        raise TypeError(f"{who}: features must be fp32 on the GPU")
    labels, text = _dev(labels, "labels", (torch.int64,)), _dev(text, "text", (torch.float32,))
    B, E = features.shape
    if text.dim() != 2 or text.shape[1] != E or labels.shape != (B,):
        raise ValueError(f"{who}: features {tuple(features.shape)}, labels {tuple(labels.shape)}, text {tuple(text.shape)} do not agree")
    return labels, text, B, E, text.shape[0]


def coop_head(features: torch.Tensor, labels: torch.Tensor, text: torch.Tensor, scale: float, grad_scale: float = 1.0, want16: bool = False):
    """CoOp's loss head: (loss fp32 [1], grad_scale * d loss / d text fp32 [C, E][, the same in fp16]) for raw image ``features`` fp32
    [B, E] (the rows may be a column slice), ``labels`` int64 [B] and raw ``text`` features fp32 [C, E]; ``scale`` = exp(logit_scale)."""
    labels, text, B, E, Cn = _head_inputs("coop_head", features, labels, text)
    loss = torch.empty(1, dtype=torch.float32, device=text.device)
    d_text = torch.empty_like(text)
    d16 = torch.empty(Cn, E, dtype=torch.float16, device=text.device) if want16 else None
    ws = torch.empty(max(lib.clipmi_coop_head_workspace_bytes(B, E, Cn), 8), dtype=torch.uint8, device=text.device)
    check(lib.clipmi_coop_head(features.data_ptr(), features.stride(0), labels.data_ptr(), text.data_ptr(), B, E, Cn, float(scale),
                               float(grad_scale), loss.data_ptr(), d_text.data_ptr(), None if d16 is None else d16.data_ptr(), ws.data_ptr(),
                               ws.numel(), _stream()), "clipmi_coop_head")
    return (loss, d_text, d16) if want16 else (loss, d_text)


def _ctx_step_inputs(who: str, d_embed: torch.Tensor, n_prompts: int, n_ctx: int, per_class: bool, ctx, buf, lr):
    """(rows per prompt, D, ctx's shape, the pointers of ctx, buf and lr or None) after the checks ctx_step and prograd_step share."""
    M, D = d_embed.shape
    if n_prompts < 1 or M % n_prompts:
        raise ValueError(f"{who}: {M} rows do not split into {n_prompts} prompts")
    shape = (n_prompts, n_ctx, D) if per_class else (n_ctx, D)
    pc = pb = pl = None
    if ctx is not None:
        _in_place(ctx, torch.float32, f"{who}: ctx must be a contiguous fp32 tensor on the GPU")
        if tuple(ctx.shape) != shape:
            raise ValueError(f"{who}: ctx {tuple(ctx.shape)} must be {shape}")
        pc = ctx.data_ptr()
        if buf is not None:
            _in_place(buf, torch.float32, f"{who}: buf must be a contiguous fp32 tensor on the GPU", numel=ctx.numel())
            pb = buf.data_ptr()
        lr = _dev(lr, "lr", (torch.float32,))
        if lr.numel() != 1:
            raise ValueError(f"{who}: lr must hold one rate")
        pl = lr.data_ptr()
    return M // n_prompts, D, shape, pc, pb, pl


def ctx_step(d_embed: torch.Tensor, n_prompts: int, n_ctx: int, per_class: bool, grad_scale: float, ctx: Optional[torch.Tensor] = None,
             buf: Optional[torch.Tensor] = None, lr: Optional[torch.Tensor] = None, first_step: bool = False, momentum: float = 0.0,
             dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False, want_grad: bool = True) -> Optional[torch.Tensor]:
    """The context's gradient from ``d_embed`` fp32 [C * L, D] (the classes summed in ascending order unless ``per_class``, divided by
    ``grad_scale``) and, with ``ctx``, torch.optim.SGD's step on it in place at the rate ``lr`` fp32 [1] (``buf``: momentum buffer).
    Returns the gradient (ctx's shape) when ``want_grad``."""
    d_embed = _dev(d_embed, "d_embed", (torch.float32,))
    L, D, shape, pc, pb, pl = _ctx_step_inputs("ctx_step", d_embed, n_prompts, n_ctx, per_class, ctx, buf, lr)
    grad = torch.empty(shape, dtype=torch.float32, device=d_embed.device) if want_grad else None
    check(lib.clipmi_ctx_step(d_embed.data_ptr(), pc, pb, None if grad is None else grad.data_ptr(), n_prompts, L, D, int(n_ctx),
                              int(bool(per_class)), float(grad_scale), pl, int(bool(first_step)), float(momentum), float(dampening),
                              float(weight_decay), int(bool(nesterov)), _stream()), "clipmi_ctx_step")
    return grad


SCALER_DEFAULTS = {"init_scale": 2.0 ** 16, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000}   # torch.cuda.amp.GradScaler's


def new_scaler_state(init_scale: float, device) -> torch.Tensor:
    """clipmi_scaler_state on ``device``: int32 [5] = {the fp32 bits of ``init_scale``, 0, 0, 0, 0}, one upload."""
    words = np.zeros(5, np.int32)
    words[:1].view(np.float32)[0] = init_scale
    return torch.from_numpy(words).to(device)


def scaler_state_dict(state: torch.Tensor) -> dict:
    """The block as ``dict(scale, growth_tracker, skipped_steps, applied_steps, found_inf)``.  One read-back (it synchronises)."""
    words = state.cpu().numpy()
    return {"scale": float(words[:1].view(np.float32)[0]), "growth_tracker": int(words[1]), "skipped_steps": int(words[2]),
            "applied_steps": int(words[3]), "found_inf": int(words[4])}


def _scaler_state(who: str, state) -> int:
    _in_place(state, torch.int32, f"{who}: state must be a contiguous int32 [5] tensor on the GPU (new_scaler_state)", numel=5)
    return state.data_ptr()


def grad_scale_rows(x: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
    """``x`` (contiguous fp32 matrix on the GPU) times the scale of the scaler's ``state`` block, in place; the scale is read on the device."""
    _in_place(x, torch.float32, "grad_scale_rows: x must be a contiguous fp32 tensor on the GPU")
    if x.dim() != 2:
        raise ValueError(f"grad_scale_rows: x {tuple(x.shape)} must be a matrix")
    check(lib.clipmi_grad_scale_rows(x.data_ptr(), x.shape[0], x.shape[1], _scaler_state("grad_scale_rows", state), _stream()),
          "clipmi_grad_scale_rows")
    return x


def ctx_step_scaled(d_embed: torch.Tensor, n_prompts: int, n_ctx: int, per_class: bool, state: torch.Tensor, ctx: torch.Tensor,
                    buf: Optional[torch.Tensor], lr: torch.Tensor, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                    growth_interval: int = 2000, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                    nesterov: bool = False, want_grad: bool = True, workspace: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """``ctx_step`` under the dynamic loss scale of ``state`` (``new_scaler_state``): the gradient is ``d_embed``'s context rows divided
    by the block's scale; a gradient with an inf or a NaN leaves ``ctx`` and ``buf`` as they are and backs the scale off, a clean one is
    applied (the momentum buffer starts on the first applied step) and counts towards the next growth.  Nothing is read back.
    ``workspace``: a uint8 tensor to reuse between steps.  Returns the unscaled gradient (ctx's shape) when ``want_grad``."""
    who = "ctx_step_scaled"
    d_embed = _dev(d_embed, "d_embed", (torch.float32,))
    if ctx is None:
        raise ValueError(f"{who}: ctx is required (the step decides whether to write it)")
    L, D, shape, pc, pb, pl = _ctx_step_inputs(who, d_embed, n_prompts, n_ctx, per_class, ctx, buf, lr)
    ps = _scaler_state(who, state)
    grad = torch.empty(shape, dtype=torch.float32, device=d_embed.device) if want_grad else None
    need = lib.clipmi_ctx_step_scaled_workspace_bytes(n_prompts, D, int(n_ctx), int(bool(per_class)))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=d_embed.device)
    check(lib.clipmi_ctx_step_scaled(d_embed.data_ptr(), pc, pb, None if grad is None else grad.data_ptr(), n_prompts, L, D, int(n_ctx),
                                     int(bool(per_class)), ps, float(growth_factor), float(backoff_factor), int(growth_interval), pl,
                                     float(momentum), float(dampening), float(weight_decay), int(bool(nesterov)), workspace.data_ptr(),
                                     workspace.numel(), _stream()), "clipmi_ctx_step_scaled")
    return grad


def block_step_scaled(grad: torch.Tensor, state: torch.Tensor, params: torch.Tensor, buf: Optional[torch.Tensor], lr: torch.Tensor,
                      growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000, momentum: float = 0.0,
                      dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False, want_grad: bool = True,
                      workspace: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """clipmi_block_step_scaled: the scaler's rule (``ctx_step_scaled``) over a whole fp32 master block ``params``.  ``grad``, of as many
    elements, is the block's gradient times the scale of ``state``, as a fit's own launches leave it at ``grad_scale = 1`` behind
    ``grad_scale_rows``; it is divided by the scale on the device, a gradient with an inf or a NaN leaves ``params`` and ``buf`` as they
    are and backs the scale off, a clean one is applied.  Nothing is read back.  ``workspace``: a uint8 tensor to reuse between steps.
    Returns the unscaled gradient (``params``' shape) when ``want_grad``."""
    who = "block_step_scaled"
    _in_place(grad, torch.float32, f"{who}: grad must be a contiguous fp32 tensor on the GPU")
    _in_place(params, torch.float32, f"{who}: params must be a contiguous fp32 tensor on the GPU")
    total = params.numel()
    if total < 1 or grad.numel() != total:
        raise ValueError(f"{who}: grad {tuple(grad.shape)} and params {tuple(params.shape)} must hold the same number of elements (>= 1)")
    if buf is not None:
        _in_place(buf, torch.float32, f"{who}: buf must be a contiguous fp32 tensor on the GPU", numel=total)
    lr = _dev(lr, "lr", (torch.float32,))
    if lr.numel() != 1:
        raise ValueError(f"{who}: lr {tuple(lr.shape)} must hold one element")
    ps = _scaler_state(who, state)
    out = torch.empty_like(params) if want_grad else None
    need = lib.clipmi_block_step_scaled_workspace_bytes(total)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=params.device)
    check(lib.clipmi_block_step_scaled(grad.data_ptr(), params.data_ptr(), None if buf is None else buf.data_ptr(),
                                       None if out is None else out.data_ptr(), total, ps, float(growth_factor), float(backoff_factor),
                                       int(growth_interval), lr.data_ptr(), float(momentum), float(dampening), float(weight_decay),
                                       int(bool(nesterov)), workspace.data_ptr(), workspace.numel(), _stream()), "clipmi_block_step_scaled")
    return out


def _adam_operands(who: str, grad, params, exp_avg, exp_avg_sq, lr, bias_table, betas, eps, weight_decay):
    """(total, the table's rows) after the checks ``block_step_adam`` and ``block_step_adam_scaled`` share."""
    _in_place(grad, torch.float32, f"{who}: grad must be a contiguous fp32 tensor on the GPU")
    _in_place(params, torch.float32, f"{who}: params must be a contiguous fp32 tensor on the GPU")
    total = params.numel()
    if total < 1 or grad.numel() != total:
        raise ValueError(f"{who}: grad {tuple(grad.shape)} and params {tuple(params.shape)} must hold the same number of elements (>= 1)")
    _in_place(exp_avg, torch.float32, f"{who}: exp_avg must be a contiguous fp32 tensor on the GPU", numel=total)
    _in_place(exp_avg_sq, torch.float32, f"{who}: exp_avg_sq must be a contiguous fp32 tensor on the GPU", numel=total)
    if lr.numel() != 1:
        raise ValueError(f"{who}: lr {tuple(lr.shape)} must hold one element")
    _in_place(bias_table, torch.float64, f"{who}: bias_table must be a contiguous float64 [steps, 2] tensor on the GPU (fitloop.adam_bias_table)")
    if bias_table.dim() != 2 or bias_table.shape[1] != 2 or bias_table.shape[0] < 1:
        raise ValueError(f"{who}: bias_table {tuple(bias_table.shape)} must be [steps >= 1, 2]")
    if len(betas) != 2:
        raise ValueError(f"{who}: betas={betas!r} must be a pair")
    return total, bias_table.shape[0]


def block_step_adam(grad: torch.Tensor, params: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, lr: torch.Tensor, t: int,
                    bias_table: torch.Tensor, grad_scale: float = 1.0, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                    decoupled: bool = False, want_grad: bool = True) -> Optional[torch.Tensor]:
    """clipmi_block_step_adam: torch.optim.Adam's step (``decoupled``: torch.optim.AdamW's) number ``t`` >= 1 on the fp32 master block
    ``params`` with the moments ``exp_avg`` and ``exp_avg_sq`` (zeros before the first step), in place, at the rate ``lr`` fp32 [1].
    ``grad``, of as many elements, is ``grad_scale`` times the gradient.  ``bias_table``: ``fitloop.adam_bias_table(betas, steps)`` on the
    device, ``steps >= t``.  One launch.  Returns the unscaled gradient (``params``' shape) when ``want_grad``."""
    who = "block_step_adam"
    lr = _dev(lr, "lr", (torch.float32,))
    total, rows = _adam_operands(who, grad, params, exp_avg, exp_avg_sq, lr, bias_table, betas, eps, weight_decay)
    out = torch.empty_like(params) if want_grad else None
    check(lib.clipmi_block_step_adam(grad.data_ptr(), params.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                     None if out is None else out.data_ptr(), total, float(grad_scale), lr.data_ptr(), int(t), bias_table.data_ptr(),
                                     rows, float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(bool(decoupled)), _stream()),
          "clipmi_block_step_adam")
    return out


def block_step_adam_scaled(grad: torch.Tensor, state: torch.Tensor, params: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
                           lr: torch.Tensor, bias_table: torch.Tensor, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                           growth_interval: int = 2000, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, decoupled: bool = False,
                           want_grad: bool = True, workspace: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """clipmi_block_step_adam_scaled: ``block_step_adam`` under the dynamic loss scale of ``state`` (``new_scaler_state``), as
    ``block_step_scaled`` is SGD's: ``grad`` is the block's gradient times the state's scale; a gradient with an inf or a NaN leaves
    ``params`` and both moments as they are, backs the scale off and does not count as one of Adam's steps; a clean one is applied at
    ``t`` = the state's applied steps.  ``bias_table`` must have a row for every step enqueued so far and this one.  Nothing is read
    back.  ``workspace``: a uint8 tensor to reuse between steps.  Returns the unscaled gradient when ``want_grad``."""
    who = "block_step_adam_scaled"
    lr = _dev(lr, "lr", (torch.float32,))
    total, rows = _adam_operands(who, grad, params, exp_avg, exp_avg_sq, lr, bias_table, betas, eps, weight_decay)
    ps = _scaler_state(who, state)
    out = torch.empty_like(params) if want_grad else None
    need = lib.clipmi_block_step_adam_scaled_workspace_bytes(total)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=params.device)
    check(lib.clipmi_block_step_adam_scaled(grad.data_ptr(), params.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                            None if out is None else out.data_ptr(), total, ps, float(growth_factor), float(backoff_factor),
                                            int(growth_interval), lr.data_ptr(), bias_table.data_ptr(), rows, float(betas[0]), float(betas[1]),
                                            float(eps), float(weight_decay), int(bool(decoupled)), workspace.data_ptr(), workspace.numel(), _stream()),
          "clipmi_block_step_adam_scaled")
    return out


# ---- fit monitor (csrc/fit_monitor.hip).  The helpers below are the only place that knows the byte layout of the epoch record and of the
# best block (include/clipmi.h "Fit monitor").

VAL_CRITERIA = {"accuracy": 0, "nll": 1}    # `criterion` of clipmi_best_select (plain integers there)
VAL_MAX_BINS = 64
_BEST_DTYPE = np.dtype([("best_epoch", "<i4"), ("best_correct", "<i4"), ("best_nll_sum", "<f8"), ("epochs_seen", "<i4"), ("pad", "<i4")])


def _val_bins(who: str, n_bins) -> int:
    if isinstance(n_bins, bool) or int(n_bins) != n_bins or not 1 <= int(n_bins) <= VAL_MAX_BINS:
        raise ValueError(f"{who}: n_bins={n_bins} must be an integer in 1..{VAL_MAX_BINS}")
    return int(n_bins)


def _record_dtype(n_bins: int) -> np.dtype:
    bins = np.dtype([("count", "<i4"), ("hits", "<i4"), ("conf_sum", "<f8")])
    return np.dtype([("n", "<i4"), ("correct", "<i4"), ("nll_sum", "<f8"), ("bins", bins, (n_bins + 1,))])


def val_record_bytes(n_bins: int) -> int:
    """The size of one epoch record: 16 + 16 (n_bins + 1) bytes."""
    return _record_dtype(_val_bins("val_record_bytes", n_bins)).itemsize


def new_val_records(slots: int, n_bins: int, device) -> torch.Tensor:
    """``slots`` zeroed epoch records on ``device``: uint8 [slots, val_record_bytes(n_bins)]; row ``e`` is what ``val_score`` takes as
    ``record``."""
    return torch.zeros(int(slots), val_record_bytes(n_bins), dtype=torch.uint8, device=device)


def decode_val_records(records, n_bins: int) -> list:
    """Every record of ``records`` (a uint8 tensor or array [slots, bytes] or [bytes]) as ``dict(n, correct, nll_sum, count, hits,
    conf_sum)``: Python numbers and three arrays [n_bins + 1], bin ``b`` being ``metrics.digitize_bins``' bin ``b`` (the last holds
    conf == 1.0).  A tensor on the GPU is read back: it synchronises."""
    raw = records.detach().cpu().numpy() if isinstance(records, torch.Tensor) else np.asarray(records)
    rec = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, val_record_bytes(n_bins)).view(_record_dtype(n_bins))[:, 0]
    return [{"n": int(r["n"]), "correct": int(r["correct"]), "nll_sum": float(r["nll_sum"]), "count": r["bins"]["count"].astype(np.int64),
             "hits": r["bins"]["hits"].astype(np.int64), "conf_sum": r["bins"]["conf_sum"].astype(np.float64)} for r in rec]


def encode_val_records(recs, n_bins: int) -> np.ndarray:
    """The inverse of ``decode_val_records`` on the host: uint8 [len(recs), val_record_bytes(n_bins)] from dicts with ``n``, ``correct``,
    ``nll_sum`` and, optionally, ``count``, ``hits``, ``conf_sum`` (zero when absent) -- records written by hand, for ``best_select``."""
    out = np.zeros(len(recs), _record_dtype(_val_bins("encode_val_records", n_bins)))
    for o, r in zip(out, recs):
        o["n"], o["correct"], o["nll_sum"] = r.get("n", 0), r["correct"], r["nll_sum"]
        for k in ("count", "hits", "conf_sum"):
            if k in r:
                o["bins"][k] = r[k]
    return out.view(np.uint8).reshape(len(recs), -1)


def val_record_bins(rec: dict) -> np.ndarray:
    """A decoded record's bins as ``metrics.ece_from_bins`` takes them: float64 [3, n_bins + 1] = (count, sum_conf, sum_correct)."""
    return np.stack([rec["count"].astype(np.float64), rec["conf_sum"], rec["hits"].astype(np.float64)])


def new_best_block(device) -> torch.Tensor:
    """The best block of ``best_select`` before the first epoch, uint8 [24] on ``device``: {-1, -1, +inf, 0}, one upload."""
    b = np.zeros(1, _BEST_DTYPE)
    b["best_epoch"], b["best_correct"], b["best_nll_sum"] = -1, -1, np.inf
    return torch.from_numpy(b.view(np.uint8).copy()).to(device)


def decode_best_block(block) -> dict:
    """The best block as ``dict(best_epoch, best_correct, best_nll_sum, epochs_seen)``; ``best_epoch`` is -1 while no epoch has been
    taken.  A tensor on the GPU is read back: it synchronises."""
    raw = block.detach().cpu().numpy() if isinstance(block, torch.Tensor) else np.asarray(block)
    b = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1).view(_BEST_DTYPE)[0]
    return {"best_epoch": int(b["best_epoch"]), "best_correct": int(b["best_correct"]), "best_nll_sum": float(b["best_nll_sum"]),
            "epochs_seen": int(b["epochs_seen"])}


def _monitor_bytes(who: str, t, name: str, nbytes: int) -> int:
    _in_place(t, torch.uint8, f"{who}: {name} must be a contiguous uint8 tensor of {nbytes} bytes on the GPU", numel=nbytes)
    return t.data_ptr()


def val_score(logits: torch.Tensor, labels: torch.Tensor, n_bins: int, record: Optional[torch.Tensor] = None,
              workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """clipmi_val_score: the fp32 ``logits`` [N, C] (the rows may be a column slice) against ``labels`` int64 [N] into one epoch record --
    n, the correct rows (arg-max with the lowest index on a tie), the sum of the rows' negative log-likelihoods and, per confidence bin of
    ``metrics.digitize_bins(conf, n_bins)``, the rows, the correct rows and the sum of the confidences.  A label outside [0, C) counts
    as wrong with a NaN nll and is never used as an address; a row that holds a NaN counts as wrong and its NaN reaches ``nll_sum``.
    Nothing is read back; the same inputs give the same bytes.  ``record``: uint8 [val_record_bytes(n_bins)] on the GPU (a row of
    ``new_val_records``), made when None; ``workspace``: a uint8 tensor to reuse.  Returns the record (``decode_val_records``)."""
    who = "val_score"
    n_bins = _val_bins(who, n_bins)
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"{who}: logits {tuple(getattr(logits, 'shape', ()))} must be [N >= 1, C >= 1]")
    if not logits.is_cuda:
        raise RuntimeError(f"clipmi: `logits` must be a tensor on the GPU (got {logits.device}); the HIP path has no CPU fallback")
    if logits.dtype != torch.float32:
        raise TypeError(f"clipmi: `logits` has dtype {logits.dtype}, expected torch.float32")
    if logits.stride(1) != 1 or logits.stride(0) < logits.shape[1] or logits.data_ptr() % 16:
        logits = logits.contiguous()
    labels = _dev(labels, "labels", (torch.int64,))
    N, Cn = logits.shape
    if labels.shape != (N,):
        raise ValueError(f"{who}: {N} rows need {N} labels, got {tuple(labels.shape)}")
    if record is None:
        record = new_val_records(1, n_bins, logits.device)[0]
    pr = _monitor_bytes(who, record, "record", val_record_bytes(n_bins))
    need = lib.clipmi_val_score_workspace_bytes(N, n_bins)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=logits.device)
    check(lib.clipmi_val_score(logits.data_ptr(), logits.stride(0), labels.data_ptr(), N, Cn, n_bins, pr, workspace.data_ptr(), workspace.numel(),
                               _stream()), "clipmi_val_score")
    return record


VAL_ROW_BYTES = 16     # one row result of clipmi_val_score_rows: {float conf, float nll, int32 hit, int32 bin}
_ROW_DTYPE = np.dtype([("conf", "<f4"), ("nll", "<f4"), ("hit", "<i4"), ("bin", "<i4")])


def new_val_row_results(N: int, device) -> torch.Tensor:
    """The row-result buffer of a validation set of ``N`` rows: zeroed uint8 [N, 16] on ``device``."""
    return torch.zeros(int(N), VAL_ROW_BYTES, dtype=torch.uint8, device=device)


def decode_val_row_results(row_results) -> np.ndarray:
    """Row results (uint8 [N, 16] tensor or array) as a structured array with ``conf``, ``nll``, ``hit``, ``bin``.  A tensor on the GPU is
    read back: it synchronises."""
    raw = row_results.detach().cpu().numpy() if isinstance(row_results, torch.Tensor) else np.asarray(row_results)
    return np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, VAL_ROW_BYTES).view(_ROW_DTYPE)[:, 0]


def _row_results(who: str, row_results, N: int, row0: int = 0):
    if not (isinstance(row_results, torch.Tensor) and row_results.is_cuda and row_results.dtype == torch.uint8 and row_results.is_contiguous()
            and row_results.dim() == 2 and row_results.shape[1] == VAL_ROW_BYTES and row_results.data_ptr() % 16 == 0):
        raise TypeError(f"{who}: row_results must be a contiguous uint8 [rows, {VAL_ROW_BYTES}] tensor on the GPU (new_val_row_results)")
    if isinstance(row0, bool) or int(row0) != row0 or row0 < 0 or row0 + N > row_results.shape[0]:
        raise ValueError(f"{who}: rows {row0} .. {row0 + N} lie outside the {row_results.shape[0]} row results")
    return row_results.data_ptr() + VAL_ROW_BYTES * int(row0)


def val_score_rows(logits: torch.Tensor, labels: torch.Tensor, n_bins: int, row_results: Optional[torch.Tensor] = None, row0: int = 0) -> torch.Tensor:
    """clipmi_val_score_rows: a chunk of fp32 ``logits`` [rows, C] (the rows may be a column slice) against ``labels`` int64 [rows], the
    chunk's own, into ``row_results[row0 : row0 + rows]`` (uint8 [N, 16] on the GPU, ``new_val_row_results``; made for the chunk alone when
    None) -- per row ``val_score``'s code: confidence, nll, hit and confidence bin.  Nothing else is written and nothing is read back.
    ``val_score_finish`` folds the rows of every chunk into the record.  Returns ``row_results``."""
    who = "val_score_rows"
    n_bins = _val_bins(who, n_bins)
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"{who}: logits {tuple(getattr(logits, 'shape', ()))} must be [rows >= 1, C >= 1]")
    if not logits.is_cuda:
        raise RuntimeError(f"clipmi: `logits` must be a tensor on the GPU (got {logits.device}); the HIP path has no CPU fallback")
    if logits.dtype != torch.float32:
        raise TypeError(f"clipmi: `logits` has dtype {logits.dtype}, expected torch.float32")
    if logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
        logits = logits.contiguous()
    if logits.data_ptr() % 16:      # a row slice that starts off a 16-byte boundary: a copy of its own (contiguous() would return the slice)
        logits = logits.clone(memory_format=torch.contiguous_format)
    labels = _dev(labels, "labels", (torch.int64,))
    N, Cn = logits.shape
    if labels.shape != (N,):
        raise ValueError(f"{who}: {N} rows need {N} labels, got {tuple(labels.shape)}")
    if row_results is None:
        row_results = new_val_row_results(row0 + N, logits.device)
    pr = _row_results(who, row_results, N, row0)
    check(lib.clipmi_val_score_rows(logits.data_ptr(), logits.stride(0), labels.data_ptr(), N, Cn, n_bins, pr, _stream()), "clipmi_val_score_rows")
    return row_results


def val_score_finish(row_results: torch.Tensor, n_bins: int, record: Optional[torch.Tensor] = None,
                     workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """clipmi_val_score_finish: every row of ``row_results`` (uint8 [N, 16] on the GPU, filled by ``val_score_rows``) into one epoch record,
    byte for byte the record ``val_score`` writes for the whole [N, C] logits, however the rows were cut into chunks.  ``record`` and
    ``workspace`` as ``val_score`` takes them.  Returns the record."""
    who = "val_score_finish"
    n_bins = _val_bins(who, n_bins)
    N = int(row_results.shape[0]) if isinstance(row_results, torch.Tensor) and row_results.dim() == 2 else 0
    if N < 1:
        raise ValueError(f"{who}: row_results {tuple(getattr(row_results, 'shape', ()))} must be [N >= 1, {VAL_ROW_BYTES}]")
    pr = _row_results(who, row_results, N)
    if record is None:
        record = new_val_records(1, n_bins, row_results.device)[0]
    prec = _monitor_bytes(who, record, "record", val_record_bytes(n_bins))
    need = lib.clipmi_val_score_finish_workspace_bytes(N, n_bins)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=row_results.device)
    check(lib.clipmi_val_score_finish(pr, N, n_bins, prec, workspace.data_ptr(), workspace.numel(), _stream()), "clipmi_val_score_finish")
    return record


def best_select(record: torch.Tensor, best_block: torch.Tensor, criterion, epoch: int, params: torch.Tensor, best_params: torch.Tensor,
                workspace: Optional[torch.Tensor] = None) -> None:
    """clipmi_best_select: when the epoch ``record`` is strictly better than ``best_block``'s (``criterion`` "accuracy": more correct
    rows; "nll": a finite, smaller ``nll_sum``), the block takes ``epoch`` and the record's figures and ``params`` is copied into
    ``best_params`` (contiguous fp32 on the GPU, as many elements); otherwise ``best_params`` is not written.  The decision is made and
    applied on the device: nothing is read back."""
    who = "best_select"
    if criterion not in VAL_CRITERIA:
        raise ValueError(f"{who}: criterion={criterion!r} must be one of {sorted(VAL_CRITERIA)}")
    if isinstance(epoch, bool) or int(epoch) != epoch or int(epoch) < 0:
        raise ValueError(f"{who}: epoch={epoch} must be an integer >= 0")
    _in_place(params, torch.float32, f"{who}: params must be a contiguous fp32 tensor on the GPU")
    _in_place(best_params, torch.float32, f"{who}: best_params must be a contiguous fp32 tensor on the GPU of params' size", numel=params.numel())
    if params.numel() < 1:
        raise ValueError(f"{who}: params is empty")
    if not (isinstance(record, torch.Tensor) and record.is_cuda and record.dtype == torch.uint8 and record.is_contiguous() and record.numel() >= 32):
        raise TypeError(f"{who}: record must be a contiguous uint8 tensor on the GPU (val_score)")
    pb = _monitor_bytes(who, best_block, "best_block", _BEST_DTYPE.itemsize)
    need = lib.clipmi_best_select_workspace_bytes(params.numel())
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=params.device)
    check(lib.clipmi_best_select(record.data_ptr(), pb, VAL_CRITERIA[criterion], int(epoch), params.data_ptr(), best_params.data_ptr(), params.numel(),
                                 workspace.data_ptr(), workspace.numel(), _stream()), "clipmi_best_select")


# ---- validation inside the cached-feature fits (csrc/adapter_train.hip, csrc/taskres_train.hip; DESIGN.md "Fit monitor")

def _val_rows(who: str, features, E: int) -> torch.Tensor:
    """Validation features fp32 [N_val >= 1, E] on the GPU, read in place with their row stride when the rows are contiguous."""
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] < 1 or features.shape[1] != E:
        raise ValueError(f"{who}: features {tuple(getattr(features, 'shape', ()))} must be [N_val >= 1, E = {E}]")
    if features.stride(1) == 1 and features.stride(0) >= E:
        _dev(features[:1], "features", (torch.float32,))     # the device and dtype checks only
        return features
    return _dev(features, "features", (torch.float32,))


def _val_out(who: str, out: Optional[torch.Tensor], N: int, Cn: int, device) -> torch.Tensor:
    if out is None:
        return torch.empty(N, Cn, dtype=torch.float32, device=device)
    _in_place(out, torch.float32, f"{who}: out must be a contiguous fp32 [{N}, {Cn}] tensor on the GPU", numel=N * Cn)
    return out


def adapter_val_logits(features: torch.Tensor, text: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, ratio: float, scale: float,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """clipmi_adapter_val_logits: ``scale * normalise(ratio * relu(relu(f W1^T) W2^T) + (1 - ratio) * f) @ text.T`` for the validation
    ``features`` fp32 [N_val, E] (raw image features; the rows may be a column slice), fp32 [N_val, C] -- the forward half of the training
    step on the weights as they are, the same code in the same order, so the logits a step on those rows would see.  Enqueued; no
    workspace; the same inputs give the same bytes.  ``out``: a contiguous fp32 [N_val, C] tensor to write into."""
    who = "adapter_val_logits"
    text, w1, w2 = (_dev(t, n, (torch.float32,)) for t, n in ((text, "text_features"), (w1, "w1"), (w2, "w2")))
    if text.dim() != 2 or text.shape[0] < 2:
        raise ValueError(f"{who}: text features {tuple(text.shape)} must be [C >= 2, E]")
    Cn, E = text.shape
    if w1.dim() != 2 or w1.shape[1] != E or w1.shape[0] < 1 or tuple(w2.shape) != (E, w1.shape[0]):
        raise ValueError(f"{who}: adapter shapes do not chain (E = {E}, w1 {tuple(w1.shape)}, w2 {tuple(w2.shape)})")
    features = _val_rows(who, features, E)
    N = features.shape[0]
    out = _val_out(who, out, N, Cn, features.device)
    check(lib.clipmi_adapter_val_logits(features.data_ptr(), features.stride(0), text.data_ptr(), w1.data_ptr(), w2.data_ptr(), N, E, w1.shape[0], Cn,
                                        float(ratio), float(scale), out.data_ptr(), _stream()), "clipmi_adapter_val_logits")
    return out


def taskres_val_logits(features: torch.Tensor, base: torch.Tensor, residuals: torch.Tensor, alpha: float, scale: float,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """clipmi_taskres_val_logits: ``scale * normalise(f) @ normalise(base + alpha * residuals).T`` for the validation ``features`` fp32
    [N_val, E] (raw image features; the rows may be a column slice), fp32 [N_val, C] -- the training step's own logits kernel on the
    validation rows.  Enqueued; no workspace; the same inputs give the same bytes.  ``out``: a contiguous fp32 [N_val, C] tensor."""
    who = "taskres_val_logits"
    base, residuals = _dev(base, "base_text_features", (torch.float32,)), _dev(residuals, "residuals", (torch.float32,))
    if base.dim() != 2 or base.shape[0] < 2 or residuals.shape != base.shape:
        raise ValueError(f"{who}: base text features {tuple(base.shape)} must be [C >= 2, E] and the residuals {tuple(residuals.shape)} of that shape")
    Cn, E = base.shape
    features = _val_rows(who, features, E)
    N = features.shape[0]
    out = _val_out(who, out, N, Cn, features.device)
    check(lib.clipmi_taskres_val_logits(features.data_ptr(), features.stride(0), base.data_ptr(), residuals.data_ptr(), N, E, Cn, float(alpha),
                                        float(scale), out.data_ptr(), _stream()), "clipmi_taskres_val_logits")
    return out


def adapter_master_block(w1: torch.Tensor, w2: torch.Tensor, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(block, w1, w2)``: fresh fp32 master copies of the two matrices as views of one contiguous block [w1 | w2] on ``device`` -- what
    ``clipmi_best_select`` copies in one piece."""
    block = torch.empty(w1.numel() + w2.numel(), dtype=torch.float32, device=device)
    m1, m2 = block[:w1.numel()].view(w1.shape), block[w1.numel():].view(w2.shape)
    m1.copy_(w1.detach())
    m2.copy_(w2.detach())
    return block, m1, m2


def fit_monitor(val_features: torch.Tensor, val_labels: torch.Tensor, n_bins: int, records: torch.Tensor, criterion: str = "accuracy",
                best_block: Optional[torch.Tensor] = None, best_params: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None) -> dict:
    """The ``monitor=`` of ``adapter_fit`` / ``taskres_fit``: validation features fp32 [N_val, E] and labels int64 [N_val] on the GPU,
    ``records`` (``new_val_records(epochs, n_bins, device)``), and for the selection ``best_block`` (``new_best_block``) with
    ``best_params`` (contiguous fp32 on the GPU, the size of the selected parameters) -- both or neither.  ``workspace``: a uint8 tensor to
    reuse (4 N_val C bytes and the scoring's; made by the call when absent or short)."""
    if criterion not in VAL_CRITERIA:
        raise ValueError(f"fit_monitor: criterion={criterion!r} must be one of {sorted(VAL_CRITERIA)}")
    if (best_block is None) != (best_params is None):
        raise ValueError("fit_monitor: best_block and best_params come together")
    return {"val_features": val_features, "val_labels": val_labels, "n_bins": _val_bins("fit_monitor", n_bins), "records": records,
            "criterion": criterion, "best_block": best_block, "best_params": best_params, "workspace": workspace}


def _fit_monitor_args(who: str, m: dict, E: int, Cn: int, epochs: int, n_floats: int, workspace_bytes) -> tuple:
    """The monitored calls' extra arguments from a ``fit_monitor`` dict, checked; the workspace it makes stays in the dict."""
    vf = _val_rows(who, m["val_features"], E)
    N = vf.shape[0]
    vl = _dev(m["val_labels"], "val_labels", (torch.int64,))
    if vl.shape != (N,):
        raise ValueError(f"{who}: {N} validation rows need {N} labels, got {tuple(vl.shape)}")
    n_bins = _val_bins(who, m["n_bins"])
    pr = _monitor_bytes(who, m["records"], "records", epochs * val_record_bytes(n_bins))
    pb = pp = None
    if m["best_block"] is not None:
        pb = _monitor_bytes(who, m["best_block"], "best_block", _BEST_DTYPE.itemsize)
        _in_place(m["best_params"], torch.float32, f"{who}: best_params must be a contiguous fp32 tensor of {n_floats} elements on the GPU",
                  numel=n_floats)
        pp = m["best_params"].data_ptr()
    need = workspace_bytes(N, Cn, n_bins)
    if m.get("workspace") is None or m["workspace"].numel() < need:
        m["workspace"] = torch.empty(max(need, 256), dtype=torch.uint8, device=vf.device)
    m["_keep"] = (vf, vl)     # alive until the caller has waited for the run
    return (vf.data_ptr(), vf.stride(0), vl.data_ptr(), N, n_bins, pr, VAL_CRITERIA[m["criterion"]], pb, pp, m["workspace"].data_ptr(),
            m["workspace"].numel())


def fit_monitor_logits(m: dict, Cn: int) -> torch.Tensor:
    """The fp32 [N_val, C] logits of the last validated epoch of a monitored run, where its workspace holds them."""
    N = m["val_features"].shape[0]
    return m["workspace"][:4 * N * Cn].view(torch.float32).view(N, Cn)


PROMPT_MODES ={"coop": _lib.PROMPT_COOP, "kgcoop": _lib.PROMPT_KGCOOP, "prograd": _lib.PROMPT_PROGRAD}


def prompt_head(features: torch.Tensor, labels: torch.Tensor, text: torch.Tensor, scale: float, grad_scale: float = 1.0, method: str = "coop",
                teacher: Optional[torch.Tensor] = None, w: float = 8.0, T: float = 1.0, losses: Optional[torch.Tensor] = None):
    """The loss head of CoOp, KgCoOp or ProGrad (``method``): ``(losses fp32 [3], d_text fp32 [C, E], d_text_kl fp32 [C, E] or None)``,
    the gradients times ``grad_scale``.  Inputs as ``coop_head``'s; ``teacher`` fp32 [C, E]: the frozen zero-shot text features (the head
    normalises the rows).  ``losses``: [loss, 0, 0] for CoOp, [CE + w score, CE, score = 1 - mean cosine to the teacher] for KgCoOp,
    [xe, kl, 0] for ProGrad, whose two gradients are those of xe and of kl (``T``: the distillation temperature).  A caller's own
    ``losses`` (fp32 [3] on the GPU) is written where it lies instead -- the elements the method does not write keep what they held."""
    if method not in PROMPT_MODES:
        raise ValueError(f"prompt_head: method={method!r} (one of {sorted(PROMPT_MODES)})")
    labels, text, B, E, Cn = _head_inputs("prompt_head", features, labels, text)
    pt = None
    if method != "coop":
        if teacher is None:
            raise ValueError(f"prompt_head: method={method!r} needs the teacher")
        teacher = _dev(teacher, "teacher", (torch.float32,))
        if teacher.shape != text.shape:
            raise ValueError(f"prompt_head: teacher {tuple(teacher.shape)} must be {tuple(text.shape)}")
        pt = teacher.data_ptr()
    mode = PROMPT_MODES[method]
    if losses is None:
        losses = torch.zeros(3, dtype=torch.float32, device=text.device)
    else:
        _in_place(losses, torch.float32, "prompt_head: losses must be a contiguous fp32 tensor on the GPU", numel=3)
    d_text = torch.empty_like(text)
    d_kl = torch.empty_like(text) if method == "prograd" else None
    ws = torch.empty(max(lib.clipmi_prompt_head_workspace_bytes(B, E, Cn, mode), 8), dtype=torch.uint8, device=text.device)
    check(lib.clipmi_prompt_head(features.data_ptr(), features.stride(0), labels.data_ptr(), text.data_ptr(), B, E, Cn, float(scale),
                                 float(grad_scale), mode, pt, float(w), float(T), losses.data_ptr(), d_text.data_ptr(), None,
                                 None if d_kl is None else d_kl.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "clipmi_prompt_head")
    return losses, d_text, d_kl


def prograd_step(d_embed_xe: torch.Tensor, d_embed_kl: torch.Tensor, n_prompts: int, n_ctx: int, per_class: bool, grad_scale: float,
                 lam: float = 1.0, ctx: Optional[torch.Tensor] = None, buf: Optional[torch.Tensor] = None, lr: Optional[torch.Tensor] = None,
                 first_step: bool = False, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False,
                 want_report: bool = True):
    """ProGrad's projection and step from the two ``d_embed`` fp32 [C * L, D] (of xe and of kl): a and b are formed as ``ctx_step`` forms
    its gradient; the gradient applied is ``a - lam (a.b / b.b) b`` when ``a.b < 0`` (both norms non-zero, everything finite), else ``a``;
    with ``ctx`` torch.optim.SGD's step on it in place.  Returns ``(grad, projected int32 [1], dots float64 [3] = a.a, b.b, a.b)`` on
    the device when ``want_report``."""
    d_embed_xe, d_embed_kl = _dev(d_embed_xe, "d_embed_xe", (torch.float32,)), _dev(d_embed_kl, "d_embed_kl", (torch.float32,))
    if d_embed_kl.shape != d_embed_xe.shape:
        raise ValueError("prograd_step: the two d_embed differ in shape")
    L, D, shape, pc, pb, pl = _ctx_step_inputs("prograd_step", d_embed_xe, n_prompts, n_ctx, per_class, ctx, buf, lr)
    if ctx is None and not want_report:
        raise ValueError("prograd_step: nothing to do (no ctx and no report)")
    dev = d_embed_xe.device
    grad = proj = dots = None
    if want_report:
        grad = torch.empty(shape, dtype=torch.float32, device=dev)
        proj = torch.empty(1, dtype=torch.int32, device=dev)
        dots = torch.empty(3, dtype=torch.float64, device=dev)
    ws = torch.empty(max(lib.clipmi_prograd_step_workspace_bytes(n_prompts, D, int(n_ctx), int(bool(per_class))), 256), dtype=torch.uint8, device=dev)
    check(lib.clipmi_prograd_step(d_embed_xe.data_ptr(), d_embed_kl.data_ptr(), pc, pb, None if grad is None else grad.data_ptr(),
                                  None if proj is None else proj.data_ptr(), None if dots is None else dots.data_ptr(), n_prompts,
                                  L, D, int(n_ctx), int(bool(per_class)), float(grad_scale), float(lam), pl, int(bool(first_step)),
                                  float(momentum), float(dampening), float(weight_decay), int(bool(nesterov)), ws.data_ptr(), ws.numel(),
                                  _stream()), "clipmi_prograd_step")
    return (grad, proj, dots) if want_report else None


# ---- the class-sharded CoOp-family fit (csrc/shard_train.hip, DESIGN.md "Class-sharded CoOp fit")

def shard_compact(gathered: torch.Tensor, n_rows: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gathered, padded fp32 [G, ceil(n_rows / G), E] block -> fp32 [n_rows, E]: row c is the row of the rank that owns class c
    under the balanced split.  The padding rows are never read.  One launch."""
    gathered = _dev(gathered, "gathered", (torch.float32,))
    if gathered.dim() != 3 or not 1 <= gathered.shape[0] <= n_rows or gathered.shape[1] != -(-n_rows // gathered.shape[0]):
        raise ValueError(f"shard_compact: gathered {tuple(gathered.shape)} must be [G, ceil({n_rows} / G), E] with G <= {n_rows}")
    G, _, E = gathered.shape
    if out is None:
        out = torch.empty(n_rows, E, dtype=torch.float32, device=gathered.device)
    else:
        _in_place(out, torch.float32, "shard_compact: out must be a contiguous fp32 tensor on the GPU", numel=n_rows * E)
    check(lib.clipmi_shard_compact(gathered.data_ptr(), out.data_ptr(), int(n_rows), G, E, _stream()), "clipmi_shard_compact")
    return out


def ctx_partial(d_embed: torch.Tensor, n_prompts: int, n_ctx: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A rank's partial context gradient fp32 [n_ctx, D] from its own ``d_embed`` fp32 [n_prompts * L, D]: the classes' context rows
    added in ascending order, unscaled.  ``out``: where it is written (the rank's send block)."""
    d_embed = _dev(d_embed, "d_embed", (torch.float32,))
    M, D = d_embed.shape
    if n_prompts < 1 or M % n_prompts:
        raise ValueError(f"ctx_partial: {M} rows do not split into {n_prompts} prompts")
    if out is None:
        out = torch.empty(n_ctx, D, dtype=torch.float32, device=d_embed.device)
    else:
        _in_place(out, torch.float32, "ctx_partial: out must be a contiguous fp32 tensor on the GPU", numel=n_ctx * D)
    check(lib.clipmi_ctx_partial(d_embed.data_ptr(), out.data_ptr(), int(n_prompts), M // n_prompts, D, int(n_ctx), _stream()), "clipmi_ctx_partial")
    return out


def _step_targets(who: str, shape, ctx, buf, lr):
    """The pointers of ``ctx`` (of ``shape``), ``buf`` and ``lr``, or None each without a context, after the checks the sharded steps share."""
    if ctx is None:
        return None, None, None
    _in_place(ctx, torch.float32, f"{who}: ctx must be a contiguous fp32 tensor on the GPU")
    if tuple(ctx.shape) != tuple(shape):
        raise ValueError(f"{who}: ctx {tuple(ctx.shape)} must be {tuple(shape)}")
    if buf is not None:
        _in_place(buf, torch.float32, f"{who}: buf must be a contiguous fp32 tensor on the GPU", numel=ctx.numel())
    lr = _dev(lr, "lr", (torch.float32,))
    if lr.numel() != 1:
        raise ValueError(f"{who}: lr must hold one rate")
    return ctx.data_ptr(), None if buf is None else buf.data_ptr(), lr.data_ptr()


def ctx_step_gathered(partials: torch.Tensor, n_ctx: int, D: int, grad_scale: float, ctx: Optional[torch.Tensor] = None,
                      buf: Optional[torch.Tensor] = None, lr: Optional[torch.Tensor] = None, first_step: bool = False, momentum: float = 0.0,
                      dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False, want_grad: bool = True) -> Optional[torch.Tensor]:
    """``ctx_step`` from the gathered partials fp32 [G, >= n_ctx * D] (rank r's ``ctx_partial`` first in row r): the partials added in
    rank order, divided by ``grad_scale``, and with ``ctx`` [n_ctx, D] torch.optim.SGD's step on it in place.  A row wider than
    ``n_ctx * D`` is a padded rank stride: the elements behind a rank's partial are not read."""
    who = "ctx_step_gathered"
    _in_place(partials, torch.float32, f"{who}: partials must be a contiguous fp32 tensor on the GPU")
    n_ctx, D = int(n_ctx), int(D)
    if n_ctx < 1 or D < 1 or partials.dim() != 2 or partials.shape[0] < 1 or partials.shape[1] < n_ctx * D:
        raise ValueError(f"{who}: partials {tuple(partials.shape)} must be [G >= 1, >= n_ctx * D = {n_ctx} * {D}]")
    G, stride = partials.shape
    if ctx is None and not want_grad:
        raise ValueError(f"{who}: nothing to do (no ctx and no gradient wanted)")
    pc, pb, pl = _step_targets(who, (n_ctx, D), ctx, buf, lr)
    grad = torch.empty(n_ctx, D, dtype=torch.float32, device=partials.device) if want_grad else None
    check(lib.clipmi_ctx_step_gathered(partials.data_ptr(), G, stride, pc, pb, None if grad is None else grad.data_ptr(), int(D), int(n_ctx),
                                       float(grad_scale), pl, int(bool(first_step)), float(momentum), float(dampening), float(weight_decay),
                                       int(bool(nesterov)), _stream()), "clipmi_ctx_step_gathered")
    return grad


def shard_prograd_workspace(total: int, device) -> torch.Tensor:
    """The workspace ``shard_prograd_dots`` and ``shard_prograd_apply`` share for a context of ``total`` elements."""
    return torch.empty(max(lib.clipmi_shard_prograd_workspace_bytes(int(total)), 256), dtype=torch.uint8, device=device)


def shard_prograd_dots(src_a: torch.Tensor, src_b: torch.Tensor, n_prompts: int, n_ctx: int, per_class: bool, grad_scale: float,
                       workspace: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ProGrad's a and b into ``workspace`` and this rank's float64 dots [3] (a.a, b.b, a.b).  ``per_class``: from the rank's own two
    ``d_embed`` fp32 [n_prompts * L, D]; else from the gathered partials of the two losses, fp32 [G, >= n_ctx * D] views of equal strides
    (``n_prompts`` is not read)."""
    who = "shard_prograd_dots"
    if out is None:
        out = torch.empty(3, dtype=torch.float64, device=src_a.device)
    else:
        _in_place(out, torch.float64, f"{who}: out must be a contiguous float64 tensor on the GPU", numel=3)
    if per_class:
        src_a, src_b = _dev(src_a, "d_embed_xe", (torch.float32,)), _dev(src_b, "d_embed_kl", (torch.float32,))
        M, D = src_a.shape
        if src_b.shape != src_a.shape or n_prompts < 1 or M % n_prompts:
            raise ValueError(f"{who}: two d_embed of [{n_prompts} * L, D] expected, got {tuple(src_a.shape)} and {tuple(src_b.shape)}")
        G, stride, L, Cn = 1, 0, M // n_prompts, int(n_prompts)
    else:
        for t in (src_a, src_b):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.stride(2) == 1
                    and t.stride(1) == t.shape[2] and t.shape[1] == n_ctx):
                raise TypeError(f"{who}: the partials must be fp32 [G, n_ctx, D] views on the GPU with contiguous rows")
        if src_a.shape != src_b.shape or src_a.stride(0) != src_b.stride(0):
            raise ValueError(f"{who}: the two partials differ in shape or stride")
        G, stride, D, L, Cn = src_a.shape[0], src_a.stride(0), src_a.shape[2], 1 + n_ctx, 1
    check(lib.clipmi_shard_prograd_dots(src_a.data_ptr(), src_b.data_ptr(), G, stride, Cn, L, D, int(n_ctx), int(bool(per_class)), float(grad_scale),
                                        out.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream()), "clipmi_shard_prograd_dots")
    return out


def shard_prograd_apply(dots_ranks: torch.Tensor, lam: float, workspace: torch.Tensor, shape, ctx: Optional[torch.Tensor] = None,
                        buf: Optional[torch.Tensor] = None, lr: Optional[torch.Tensor] = None, first_step: bool = False, momentum: float = 0.0,
                        dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False, want_report: bool = True):
    """The ranks' dots float64 [G, 3] added in rank order, ProGrad's decision and the step on ``ctx`` (of ``shape``, the elements that
    ``shard_prograd_dots`` left a and b of in ``workspace``).  Returns ``(grad, projected, dots)`` as ``prograd_step`` when ``want_report``."""
    who = "shard_prograd_apply"
    _in_place(dots_ranks, torch.float64, f"{who}: dots_ranks must be a contiguous float64 tensor on the GPU")
    if dots_ranks.dim() != 2 or dots_ranks.shape[1] != 3:
        raise ValueError(f"{who}: dots_ranks {tuple(dots_ranks.shape)} must be [G, 3]")
    shape, dev = tuple(int(x) for x in shape), dots_ranks.device
    total = int(np.prod(shape))
    if ctx is None and not want_report:
        raise ValueError(f"{who}: nothing to do (no ctx and no report)")
    pc, pb, pl = _step_targets(who, shape, ctx, buf, lr)
    grad = proj = dots = None
    if want_report:
        grad = torch.empty(shape, dtype=torch.float32, device=dev)
        proj = torch.empty(1, dtype=torch.int32, device=dev)
        dots = torch.empty(3, dtype=torch.float64, device=dev)
    check(lib.clipmi_shard_prograd_apply(dots_ranks.data_ptr(), dots_ranks.shape[0], float(lam), pc, pb, None if grad is None else grad.data_ptr(),
                                         None if proj is None else proj.data_ptr(), None if dots is None else dots.data_ptr(), total, pl,
                                         int(bool(first_step)), float(momentum), float(dampening), float(weight_decay), int(bool(nesterov)),
                                         workspace.data_ptr(), workspace.numel(), _stream()), "clipmi_shard_prograd_apply")
    return (grad, proj, dots) if want_report else None


# ---- the batch-sharded fits through the image tower (csrc/shard_train.hip, DESIGN.md "Batch-sharded image-tower fits")

def _gathered_rows(who: str, gathered, total) -> Tuple[int, int, int]:
    """``(G, stride, total)`` of gathered blocks fp32 [G, >= total] on the GPU: rows of unit element stride, ``stride(0)`` floats apart (a
    column range of a wider receive block is taken where it lies)."""
    if not (isinstance(gathered, torch.Tensor) and gathered.is_cuda and gathered.dtype == torch.float32 and gathered.dim() == 2
            and gathered.shape[0] >= 1 and gathered.shape[1] >= 1 and (gathered.stride(1) == 1 or gathered.shape[1] == 1)):
        raise TypeError(f"{who}: gathered must be an fp32 [G >= 1, >= total] tensor on the GPU whose rows have unit element stride")
    if gathered.device.index != torch.cuda.current_device():
        raise RuntimeError(f"clipmi: `gathered` is on {gathered.device} but the current device is cuda:{torch.cuda.current_device()}")
    if isinstance(total, bool) or int(total) != total or not 1 <= int(total) <= gathered.shape[1]:
        raise ValueError(f"{who}: total={total} must be an integer in [1, {gathered.shape[1]}] (gathered {tuple(gathered.shape)})")
    G, stride = gathered.shape[0], gathered.stride(0) if gathered.shape[0] > 1 else gathered.shape[1]
    if stride < int(total):
        raise ValueError(f"{who}: the rows of gathered lie {stride} floats apart, fewer than total={total}")
    return G, stride, int(total)


def block_rank_mean(gathered: torch.Tensor, total: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """clipmi_block_rank_mean: the rank-ordered mean fp32 [total] of the first ``total`` floats of every row of ``gathered`` fp32
    [G, >= total] (rank r's block in row r; the floats of a row behind ``total`` are never read):
    ``(((p_0 + p_1) + p_2) + ..) * float32(1 / G)``, the same bits on every run; an inf or a NaN stays one; with G = 1 the row itself.
    ``out``: a contiguous fp32 tensor of ``total`` elements that does not overlap ``gathered``.  One launch."""
    who = "block_rank_mean"
    G, stride, total = _gathered_rows(who, gathered, total)
    if out is None:
        out = torch.empty(total, dtype=torch.float32, device=gathered.device)
    else:
        _in_place(out, torch.float32, f"{who}: out must be a contiguous fp32 tensor of {total} elements on the GPU", numel=total)
    check(lib.clipmi_block_rank_mean(gathered.data_ptr(), G, stride, total, out.data_ptr(), _stream()), "clipmi_block_rank_mean")
    return out


def block_step_gathered(gathered: torch.Tensor, total: int, grad_scale: float, params: Optional[torch.Tensor] = None, buf: Optional[torch.Tensor] = None,
                        lr: Optional[torch.Tensor] = None, first_step: bool = False, momentum: float = 0.0, dampening: float = 0.0,
                        weight_decay: float = 0.0, nesterov: bool = False, want_grad: bool = True) -> Optional[torch.Tensor]:
    """clipmi_block_step_gathered: ``block_rank_mean`` of ``gathered`` (rank r's ``grad_scale`` * gradient in row r), divided by
    ``grad_scale``, and with ``params`` (fp32, ``total`` elements) torch.optim.SGD's step on it in place -- one launch.  Returns the
    gradient fp32 [total] when ``want_grad``."""
    who = "block_step_gathered"
    G, stride, total = _gathered_rows(who, gathered, total)
    if params is None and not want_grad:
        raise ValueError(f"{who}: nothing to do (no params and no gradient wanted)")
    if params is not None and params.numel() != total:
        raise ValueError(f"{who}: params {tuple(params.shape)} must hold total={total} elements")
    pp, pb, pl = _step_targets(who, () if params is None else params.shape, params, buf, lr)
    grad = torch.empty(total, dtype=torch.float32, device=gathered.device) if want_grad else None
    check(lib.clipmi_block_step_gathered(gathered.data_ptr(), G, stride, total, float(grad_scale), pp, pb, None if grad is None else grad.data_ptr(), pl,
                                         int(bool(first_step)), float(momentum), float(dampening), float(weight_decay), int(bool(nesterov)), _stream()),
          "clipmi_block_step_gathered")
    return grad


PROMPT_POSITIONS = {"front": 0, "middle": 1, "end": 2}   # `position` of clipmi_prompt_place and clipmi_proda_embed's pos (plain integers there)


def _position_code(who: str, position) -> int:
    if position in PROMPT_POSITIONS:
        return PROMPT_POSITIONS[position]
    if isinstance(position, bool) or position not in PROMPT_POSITIONS.values():
        raise ValueError(f"{who}: position={position!r} must be one of {tuple(PROMPT_POSITIONS)} (or its code {PROMPT_POSITIONS})")
    return int(position)


def prompt_place(base: torch.Tensor, ctx: torch.Tensor, position, name_lens: torch.Tensor, rows: int = 0,
                 prompts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """CoOp's prompt assembly at a class-token position: ``prompts`` fp32 [C, Lc, D] from the class embeddings ``base`` [C, Lc, D] (fp16 or
    fp32, the tokens of ``"X .. X name."``), the fp32 master ``ctx`` ([n_ctx, D], or [C, n_ctx, D] class-specific), ``position``
    ("front", "middle", "end" or ProDA's code 0, 1, 2) and the int32 device vector ``name_lens`` [C].  Only the first ``rows`` token rows
    of each prompt are written (0: all of them).  A caller's own ``prompts`` is written where it lies.  One launch."""
    who = "prompt_place"
    ps = _position_code(who, position)
    base = _dev(base, "base", (torch.float16, torch.float32))
    ctx = _dev(ctx, "ctx", (torch.float32,))
    if base.dim() != 3 or ctx.dim() not in (2, 3) or ctx.shape[-1] != base.shape[2] or (ctx.dim() == 3 and ctx.shape[0] != base.shape[0]):
        raise ValueError(f"{who}: base {tuple(base.shape)} and ctx {tuple(ctx.shape)} do not agree")
    Cn, Lc, D = base.shape
    n_ctx = int(ctx.shape[-2])
    name_lens = _proda_index(name_lens, "name_lens", Cn)
    L = int(rows) if 0 < int(rows) < Lc else Lc
    if prompts is None:
        prompts = torch.empty(Cn, Lc, D, dtype=torch.float32, device=base.device)
    else:
        _in_place(prompts, torch.float32, f"{who}: prompts must be a contiguous fp32 tensor on the GPU", numel=Cn * Lc * D)
    check(lib.clipmi_prompt_place(base.data_ptr(), _DT[base.dtype], ctx.data_ptr(), int(ctx.dim() == 3), ps, name_lens.data_ptr(), prompts.data_ptr(),
                                  Cn, L, Lc, D, n_ctx, _stream()), "clipmi_prompt_place")
    return prompts


def prompt_unplace(d_embed: torch.Tensor, position, name_lens: torch.Tensor, n_ctx: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The inverse of ``prompt_place`` on the gradient stream: ``d_embed`` fp32 [C * L, D] as the backward wrote it -> fp32
    [C * (1 + n_ctx), D], row 1 + j of class c the row of prompt c that holds context vector j and row 0 zeros -- what ``ctx_step``,
    ``ctx_step_scaled`` and ``prograd_step`` read as a ``d_embed`` of 1 + n_ctx rows per prompt.  ``name_lens`` int32 [C] on the device.
    A caller's own ``out`` is written where it lies.  One launch."""
    who = "prompt_unplace"
    ps = _position_code(who, position)
    d_embed = _dev(d_embed, "d_embed", (torch.float32,))
    name_lens = _dev(name_lens, "name_lens", (torch.int32,))
    Cn, n_ctx = int(name_lens.numel()), int(n_ctx)
    if d_embed.dim() != 2 or name_lens.dim() != 1 or Cn < 1 or d_embed.shape[0] % Cn:
        raise ValueError(f"{who}: d_embed {tuple(d_embed.shape)} does not split into the {Cn} prompts of name_lens")
    L, D = d_embed.shape[0] // Cn, int(d_embed.shape[1])
    if out is None:
        out = torch.empty(Cn * (1 + n_ctx), D, dtype=torch.float32, device=d_embed.device)
    else:
        _in_place(out, torch.float32, f"{who}: out must be a contiguous fp32 tensor on the GPU", numel=Cn * (1 + n_ctx) * D)
    check(lib.clipmi_prompt_unplace(d_embed.data_ptr(), ps, name_lens.data_ptr(), out.data_ptr(), Cn, L, D, n_ctx, _stream()), "clipmi_prompt_unplace")
    return out


def _proda_index(t: torch.Tensor, name: str, n: int) -> torch.Tensor:
    t = _dev(t, name, (torch.int32,))
    if t.shape != (n,):
        raise ValueError(f"clipmi: `{name}` {tuple(t.shape)} must be int32 [{n}]")
    return t


def proda_embed(base: torch.Tensor, nc_base: torch.Tensor, ctx: torch.Tensor, sel: torch.Tensor, pos: torch.Tensor, name_lens: torch.Tensor,
                cls_eot: torch.Tensor, rows: int = 0, prompts: Optional[torch.Tensor] = None, eot: Optional[torch.Tensor] = None):
    """ProDA's prompt assembly: ``(prompts fp32 [C * Pb + P, Lc, D], eot int32 [C * Pb + P])`` from the class embeddings ``base``
    [C, Lc, D] and the no-class embedding ``nc_base`` [1, Lc, D] (fp16 or fp32), the fp32 master ``ctx`` [P, n_ctx, D] and the int32
    device vectors ``sel`` [Pb] (in the reference's end | middle | front order), ``pos`` [P] (0 front, 1 middle, 2 end), ``name_lens``
    [C] and ``cls_eot`` [C] (the classes' EOT rows, which every prompt of a class keeps): the class prompts class-major, then the P no-class prompts.  Only the first ``rows`` token rows of each prompt are written (0:
    all of them).  A caller's own ``prompts`` and ``eot`` are written where they lie."""
    base = _dev(base, "base", (torch.float16, torch.float32))
    nc_base = _dev(nc_base, "nc_base", (base.dtype,))
    ctx = _dev(ctx, "ctx", (torch.float32,))
    if base.dim() != 3 or ctx.dim() != 3 or nc_base.shape != (1,) + tuple(base.shape[1:]) or ctx.shape[2] != base.shape[2]:
        raise ValueError(f"proda_embed: base {tuple(base.shape)}, nc_base {tuple(nc_base.shape)} and ctx {tuple(ctx.shape)} do not agree")
    Cn, Lc, D = base.shape
    P, n_ctx = int(ctx.shape[0]), int(ctx.shape[1])
    sel = _dev(sel, "sel", (torch.int32,))
    Pb = int(sel.numel())
    sel, pos, name_lens = _proda_index(sel, "sel", Pb), _proda_index(pos, "pos", P), _proda_index(name_lens, "name_lens", Cn)
    cls_eot = _proda_index(cls_eot, "cls_eot", Cn)
    N = Cn * Pb + P
    L = int(rows) if 0 < int(rows) < Lc else Lc
    if prompts is None:
        prompts = torch.empty(N, Lc, D, dtype=torch.float32, device=base.device)
    else:
        _in_place(prompts, torch.float32, "proda_embed: prompts must be a contiguous fp32 tensor on the GPU", numel=N * Lc * D)
    if eot is None:
        eot = torch.empty(N, dtype=torch.int32, device=base.device)
    else:
        _in_place(eot, torch.int32, "proda_embed: eot must be a contiguous int32 tensor on the GPU", numel=N)
    check(lib.clipmi_proda_embed(base.data_ptr(), nc_base.data_ptr(), _DT[base.dtype], ctx.data_ptr(), sel.data_ptr(), pos.data_ptr(),
                                 name_lens.data_ptr(), cls_eot.data_ptr(), prompts.data_ptr(), eot.data_ptr(), Cn, Pb, P, L, Lc, D, n_ctx, _stream()), "clipmi_proda_embed")
    return prompts, eot


def proda_head(features: torch.Tensor, labels: torch.Tensor, text: torch.Tensor, n_cls: int, n_sel: int, scale: float, grad_scale: float = 1.0,
               alpha: float = 0.1, losses: Optional[torch.Tensor] = None):
    """ProDA's loss head: ``(losses fp32 [3] = [upper + alpha m, upper, m], d_text fp32 [N, E])``, the gradient times ``grad_scale``.
    ``text`` fp32 [N = n_cls * n_sel + P, E]: the raw features of the class prompts (class-major, ``n_sel`` per class) and of the P
    no-class prompts; ``features`` and ``labels`` as ``coop_head``'s.  upper is the cross-entropy of
    ``s x_b . m_c + 0.5 s^2 sigma[b, c]`` (include/clipmi.h), m the mean absolute cosine between two different no-class features."""
    labels, text, B, E, N = _head_inputs("proda_head", features, labels, text)
    Cn, Pb = int(n_cls), int(n_sel)
    P = N - Cn * Pb
    if Cn < 2 or Pb < 1 or P < 2 or Pb > P:
        raise ValueError(f"proda_head: {N} text rows do not split into {Cn} classes of {Pb} prompts and at least max(2, {Pb}) no-class prompts")
    if losses is None:
        losses = torch.empty(3, dtype=torch.float32, device=text.device)
    else:
        _in_place(losses, torch.float32, "proda_head: losses must be a contiguous fp32 tensor on the GPU", numel=3)
    d_text = torch.empty_like(text)
    ws = torch.empty(max(lib.clipmi_proda_head_workspace_bytes(B, E, Cn, Pb, P), 8), dtype=torch.uint8, device=text.device)
    check(lib.clipmi_proda_head(features.data_ptr(), features.stride(0), labels.data_ptr(), text.data_ptr(), B, E, Cn, Pb, P, float(scale),
                                float(grad_scale), float(alpha), losses.data_ptr(), d_text.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "clipmi_proda_head")
    return losses, d_text


def proda_ctx_step(d_embed: torch.Tensor, sel: torch.Tensor, pos: torch.Tensor, name_lens: torch.Tensor, n_ctx: int, grad_scale: float,
                   ctx: Optional[torch.Tensor] = None, buf: Optional[torch.Tensor] = None, lr: Optional[torch.Tensor] = None, first_step: bool = False,
                   momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False,
                   want_grad: bool = True) -> Optional[torch.Tensor]:
    """The gradient of ProDA's contexts [P, n_ctx, D] from ``d_embed`` fp32 [(C * Pb + P) * L, D]: for a selected context the classes'
    rows in ascending order, then -- for every context -- its no-class prompt's row, divided by ``grad_scale``; with ``ctx``,
    torch.optim.SGD's step on it in place as ``ctx_step`` takes it.  ``sel`` [Pb], ``pos`` [P], ``name_lens`` [C]: int32 on the device.
    Returns the gradient when ``want_grad``."""
    d_embed = _dev(d_embed, "d_embed", (torch.float32,))
    sel, pos, name_lens = (_dev(t, n, (torch.int32,)) for t, n in ((sel, "sel"), (pos, "pos"), (name_lens, "name_lens")))
    Pb, P, Cn = int(sel.numel()), int(pos.numel()), int(name_lens.numel())
    N = Cn * Pb + P
    if d_embed.dim() != 2 or d_embed.shape[0] % N:
        raise ValueError(f"proda_ctx_step: d_embed {tuple(d_embed.shape)} does not split into {N} prompts")
    L = d_embed.shape[0] // N
    # the no-class prompts are the last P of the N: to _ctx_step_inputs they are P prompts with one context each
    _, D, _, pc, pb, pl = _ctx_step_inputs("proda_ctx_step", d_embed[(N - P) * L:], P, n_ctx, True, ctx, buf, lr)
    grad = torch.empty(P, int(n_ctx), D, dtype=torch.float32, device=d_embed.device) if want_grad else None
    check(lib.clipmi_proda_ctx_step(d_embed.data_ptr(), pc, pb, None if grad is None else grad.data_ptr(), sel.data_ptr(), pos.data_ptr(),
                                    name_lens.data_ptr(), Cn, Pb, P, L, D, int(n_ctx), float(grad_scale), pl, int(bool(first_step)), float(momentum),
                                    float(dampening), float(weight_decay), int(bool(nesterov)), _stream()), "clipmi_proda_ctx_step")
    return grad


def proda_ctx_step_scaled(d_embed: torch.Tensor, sel: torch.Tensor, pos: torch.Tensor, name_lens: torch.Tensor, n_ctx: int, state: torch.Tensor,
                          ctx: torch.Tensor, buf: Optional[torch.Tensor], lr: torch.Tensor, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                          growth_interval: int = 2000, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                          nesterov: bool = False, want_grad: bool = True, workspace: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """``proda_ctx_step`` under the dynamic loss scale of ``state`` (``new_scaler_state``), as ``ctx_step_scaled`` is ``ctx_step``'s: the
    gather-reduce divided by the block's scale; a gradient with an inf or a NaN -- in a selected context's class rows or in any
    context's no-class row -- leaves ``ctx`` and ``buf`` as they are and backs the scale off, a clean one is applied (the momentum
    buffer starts on the first applied step) and counts towards the next growth.  Nothing is read back.  ``workspace``: a uint8 tensor
    to reuse between steps.  Returns the unscaled gradient [P, n_ctx, D] when ``want_grad``."""
    who = "proda_ctx_step_scaled"
    d_embed = _dev(d_embed, "d_embed", (torch.float32,))
    sel, pos, name_lens = (_dev(t, n, (torch.int32,)) for t, n in ((sel, "sel"), (pos, "pos"), (name_lens, "name_lens")))
    Pb, P, Cn = int(sel.numel()), int(pos.numel()), int(name_lens.numel())
    N = Cn * Pb + P
    if d_embed.dim() != 2 or d_embed.shape[0] % N:
        raise ValueError(f"{who}: d_embed {tuple(d_embed.shape)} does not split into {N} prompts")
    if ctx is None:
        raise ValueError(f"{who}: ctx is required (the step decides whether to write it)")
    L = d_embed.shape[0] // N
    _, D, _, pc, pb, pl = _ctx_step_inputs(who, d_embed[(N - P) * L:], P, n_ctx, True, ctx, buf, lr)
    ps = _scaler_state(who, state)
    grad = torch.empty(P, int(n_ctx), D, dtype=torch.float32, device=d_embed.device) if want_grad else None
    need = lib.clipmi_proda_ctx_step_scaled_workspace_bytes(P, D, int(n_ctx))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=d_embed.device)
    check(lib.clipmi_proda_ctx_step_scaled(d_embed.data_ptr(), pc, pb, None if grad is None else grad.data_ptr(), sel.data_ptr(), pos.data_ptr(),
                                           name_lens.data_ptr(), Cn, Pb, P, L, D, int(n_ctx), ps, float(growth_factor), float(backoff_factor),
                                           int(growth_interval), pl, float(momentum), float(dampening), float(weight_decay), int(bool(nesterov)),
                                           workspace.data_ptr(), workspace.numel(), _stream()), "clipmi_proda_ctx_step_scaled")
    return grad


# ---- the class-sharded ProDA fit (csrc/proda_train.hip, DESIGN.md "Class-sharded ProDA fit")

def proda_embed_shard(base: torch.Tensor, nc_base: torch.Tensor, ctx: torch.Tensor, sel: torch.Tensor, pos: torch.Tensor, name_lens: torch.Tensor,
                      cls_eot: torch.Tensor, nc_lo: int, nc_hi: int, rows: int = 0, prompts: Optional[torch.Tensor] = None,
                      eot: Optional[torch.Tensor] = None):
    """``proda_embed`` for one rank of the class-sharded fit: ``base`` [C_r, Lc, D], ``name_lens`` and ``cls_eot`` [C_r] are the rank's own
    classes' (one class is enough), ``ctx`` [P, n_ctx, D], ``sel`` and ``pos`` the whole collection's, and the no-class prompts written are
    those of the contexts ``nc_lo .. nc_hi - 1``: ``(prompts fp32 [C_r * Pb + P_r, Lc, D], eot int32 [C_r * Pb + P_r])``."""
    base = _dev(base, "base", (torch.float16, torch.float32))
    nc_base = _dev(nc_base, "nc_base", (base.dtype,))
    ctx = _dev(ctx, "ctx", (torch.float32,))
    if base.dim() != 3 or ctx.dim() != 3 or nc_base.shape != (1,) + tuple(base.shape[1:]) or ctx.shape[2] != base.shape[2]:
        raise ValueError(f"proda_embed_shard: base {tuple(base.shape)}, nc_base {tuple(nc_base.shape)} and ctx {tuple(ctx.shape)} do not agree")
    Cn, Lc, D = base.shape
    P, n_ctx = int(ctx.shape[0]), int(ctx.shape[1])
    nc_lo, nc_hi = int(nc_lo), int(nc_hi)
    if not 0 <= nc_lo < nc_hi <= P:
        raise ValueError(f"proda_embed_shard: the no-class prompts [{nc_lo}, {nc_hi}) must be a non-empty range of the {P} contexts")
    sel = _dev(sel, "sel", (torch.int32,))
    Pb = int(sel.numel())
    sel, pos, name_lens = _proda_index(sel, "sel", Pb), _proda_index(pos, "pos", P), _proda_index(name_lens, "name_lens", Cn)
    cls_eot = _proda_index(cls_eot, "cls_eot", Cn)
    N = Cn * Pb + nc_hi - nc_lo
    L = int(rows) if 0 < int(rows) < Lc else Lc
    if prompts is None:
        prompts = torch.empty(N, Lc, D, dtype=torch.float32, device=base.device)
    else:
        _in_place(prompts, torch.float32, "proda_embed_shard: prompts must be a contiguous fp32 tensor on the GPU", numel=N * Lc * D)
    if eot is None:
        eot = torch.empty(N, dtype=torch.int32, device=base.device)
    else:
        _in_place(eot, torch.int32, "proda_embed_shard: eot must be a contiguous int32 tensor on the GPU", numel=N)
    check(lib.clipmi_proda_embed_shard(base.data_ptr(), nc_base.data_ptr(), _DT[base.dtype], ctx.data_ptr(), sel.data_ptr(), pos.data_ptr(),
                                       name_lens.data_ptr(), cls_eot.data_ptr(), prompts.data_ptr(), eot.data_ptr(), Cn, Pb, P, nc_lo, nc_hi - nc_lo, L, Lc, D,
                                       n_ctx, _stream()), "clipmi_proda_embed_shard")
    return prompts, eot


def proda_shard_rows(n_cls: int, n_sel: int, n_prompt: int, world: int) -> int:
    """Rows of one rank's block of the gathered text features: ``ceil(C / G) * Pb + ceil(P / G)``."""
    return -(-int(n_cls) // int(world)) * int(n_sel) + -(-int(n_prompt) // int(world))


def proda_shard_compact(gathered: torch.Tensor, n_cls: int, n_sel: int, n_prompt: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gathered, padded fp32 [G, ``proda_shard_rows``, E] text features -> fp32 [n_cls * n_sel + n_prompt, E] in the unsharded order:
    block r holds rank r's ``C_r * Pb`` class rows, then its ``P_r`` no-class rows, then padding that is never read.  One launch."""
    gathered = _dev(gathered, "gathered", (torch.float32,))
    Cn, Pb, P = int(n_cls), int(n_sel), int(n_prompt)
    if gathered.dim() != 3 or not 1 <= gathered.shape[0] <= min(Cn, P) or Pb < 1 or gathered.shape[1] != proda_shard_rows(Cn, Pb, P, gathered.shape[0]):
        raise ValueError(f"proda_shard_compact: gathered {tuple(gathered.shape)} must be [G, ceil({Cn} / G) * {Pb} + ceil({P} / G), E] with G <= min({Cn}, {P})")
    G, _, E = gathered.shape
    N = Cn * Pb + P
    if out is None:
        out = torch.empty(N, E, dtype=torch.float32, device=gathered.device)
    else:
        _in_place(out, torch.float32, "proda_shard_compact: out must be a contiguous fp32 tensor on the GPU", numel=N * E)
    check(lib.clipmi_proda_shard_compact(gathered.data_ptr(), out.data_ptr(), Cn, Pb, P, G, E, _stream()), "clipmi_proda_shard_compact")
    return out


def proda_ctx_partial(d_embed: torch.Tensor, sel: torch.Tensor, pos: torch.Tensor, name_lens: torch.Tensor, n_own: int, n_ctx: int,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A rank's send block fp32 [Pb + n_own, n_ctx, D] from its own ``d_embed`` fp32 [(C_r * Pb + n_own) * L, D]: per selected slot the
    class rows of the rank's ``C_r`` classes (``name_lens`` [C_r], its own) added in ascending order, unscaled, then the rows of its
    ``n_own`` no-class prompts as they are.  ``sel`` [Pb], ``pos`` [P]: int32 on the device, the whole collection's.  ``out``: where it is
    written -- the first rows of the rank's padded send block."""
    who = "proda_ctx_partial"
    d_embed = _dev(d_embed, "d_embed", (torch.float32,))
    sel, pos, name_lens = (_dev(t, n, (torch.int32,)) for t, n in ((sel, "sel"), (pos, "pos"), (name_lens, "name_lens")))
    Pb, P, Cn, Pn, n_ctx = int(sel.numel()), int(pos.numel()), int(name_lens.numel()), int(n_own), int(n_ctx)
    N = Cn * Pb + Pn
    if d_embed.dim() != 2 or Pn < 1 or Pn > P or Cn < 1 or d_embed.shape[0] % N:
        raise ValueError(f"{who}: d_embed {tuple(d_embed.shape)} does not split into {Cn} * {Pb} class prompts and {Pn} (1 .. {P}) no-class prompts")
    L, D = d_embed.shape[0] // N, d_embed.shape[1]
    if out is None:
        out = torch.empty(Pb + Pn, n_ctx, D, dtype=torch.float32, device=d_embed.device)
    else:
        _in_place(out, torch.float32, f"{who}: out must be a contiguous fp32 tensor on the GPU", numel=(Pb + Pn) * n_ctx * D)
    check(lib.clipmi_proda_ctx_partial(d_embed.data_ptr(), out.data_ptr(), sel.data_ptr(), pos.data_ptr(), name_lens.data_ptr(), Cn, Pb, P, Pn, L, D, n_ctx,
                                       _stream()), "clipmi_proda_ctx_partial")
    return out


def _proda_gathered(who: str, gathered: torch.Tensor, sel: torch.Tensor, n_prompt: int, n_ctx: int, D: int):
    """(G, rank stride, Pb) of the gathered send blocks fp32 [G, >= (Pb + ceil(P / G)) * n_ctx * D] after their checks."""
    _in_place(gathered, torch.float32, f"{who}: gathered must be a contiguous fp32 tensor on the GPU")
    Pb = int(sel.numel())
    if gathered.dim() != 2 or not 1 <= gathered.shape[0] <= n_prompt or n_ctx < 1 or D < 1:
        raise ValueError(f"{who}: gathered {tuple(gathered.shape)} must be [G, elements per rank] with 1 <= G <= P = {n_prompt}")
    G, stride = gathered.shape
    need = (Pb + -(-n_prompt // G)) * n_ctx * D
    if stride < need:
        raise ValueError(f"{who}: gathered {tuple(gathered.shape)} holds fewer than (Pb + ceil(P / G)) * n_ctx * D = {need} elements per rank")
    return G, stride, Pb


def proda_ctx_step_gathered(gathered: torch.Tensor, sel: torch.Tensor, n_prompt: int, n_ctx: int, D: int, grad_scale: float,
                            ctx: Optional[torch.Tensor] = None, buf: Optional[torch.Tensor] = None, lr: Optional[torch.Tensor] = None,
                            first_step: bool = False, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False,
                            want_grad: bool = True) -> Optional[torch.Tensor]:
    """``proda_ctx_step`` from the gathered send blocks fp32 [G, >= (Pb + ceil(P / G)) * n_ctx * D] (rank r's ``proda_ctx_partial`` first
    in row r, padding behind it that is never read): for a context selected at slot q the G class sums of slot q added in rank order,
    then -- for every context -- its no-class row from the rank that owns it, divided by ``grad_scale``; with ``ctx`` [P, n_ctx, D]
    torch.optim.SGD's step on it in place."""
    who = "proda_ctx_step_gathered"
    sel = _dev(sel, "sel", (torch.int32,))
    P, n_ctx, D = int(n_prompt), int(n_ctx), int(D)
    G, stride, Pb = _proda_gathered(who, gathered, sel, P, n_ctx, D)
    if ctx is None and not want_grad:
        raise ValueError(f"{who}: nothing to do (no ctx and no gradient wanted)")
    pc, pb, pl = _step_targets(who, (P, n_ctx, D), ctx, buf, lr)
    grad = torch.empty(P, n_ctx, D, dtype=torch.float32, device=gathered.device) if want_grad else None
    check(lib.clipmi_proda_ctx_step_gathered(gathered.data_ptr(), G, stride, pc, pb, None if grad is None else grad.data_ptr(), sel.data_ptr(), Pb, P, D, n_ctx,
                                             float(grad_scale), pl, int(bool(first_step)), float(momentum), float(dampening), float(weight_decay),
                                             int(bool(nesterov)), _stream()), "clipmi_proda_ctx_step_gathered")
    return grad


def proda_ctx_reduce_gathered_scaled(gathered: torch.Tensor, sel: torch.Tensor, n_prompt: int, n_ctx: int, D: int, state: torch.Tensor, ctx: torch.Tensor,
                                     buf: Optional[torch.Tensor], lr: torch.Tensor, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                                     growth_interval: int = 2000, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                                     nesterov: bool = False, want_grad: bool = True, workspace: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """``proda_ctx_step_gathered`` under the dynamic loss scale of ``state``, as ``proda_ctx_step_scaled`` is ``proda_ctx_step``'s: the
    rank-ordered sum divided by the block's scale, the step skipped and the scale backed off when any element is an inf or a NaN.  Every
    rank reduces the same gathered bytes and so decides alike.  Returns the unscaled gradient [P, n_ctx, D] when ``want_grad``."""
    who = "proda_ctx_reduce_gathered_scaled"
    sel = _dev(sel, "sel", (torch.int32,))
    P, n_ctx, D = int(n_prompt), int(n_ctx), int(D)
    G, stride, Pb = _proda_gathered(who, gathered, sel, P, n_ctx, D)
    if ctx is None:
        raise ValueError(f"{who}: ctx is required (the step decides whether to write it)")
    pc, pb, pl = _step_targets(who, (P, n_ctx, D), ctx, buf, lr)
    ps = _scaler_state(who, state)
    grad = torch.empty(P, n_ctx, D, dtype=torch.float32, device=gathered.device) if want_grad else None
    need = lib.clipmi_proda_ctx_step_scaled_workspace_bytes(P, D, n_ctx)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=gathered.device)
    check(lib.clipmi_proda_ctx_reduce_gathered_scaled(gathered.data_ptr(), G, stride, pc, pb, None if grad is None else grad.data_ptr(), sel.data_ptr(), Pb, P,
                                                      D, n_ctx, ps, float(growth_factor), float(backoff_factor), int(growth_interval), pl, float(momentum),
                                                      float(dampening), float(weight_decay), int(bool(nesterov)), workspace.data_ptr(), workspace.numel(),
                                                      _stream()), "clipmi_proda_ctx_reduce_gathered_scaled")
    return grad


def cocoop_block_layout(n_ctx: int, D: int, E: int, H: int):
    """The offsets, in floats, of ``ctx | W1 | b1 | W2 | b2`` in CoCoOp's parameter block, and its size: a dict name -> (offset, shape),
    the names those of the reference's ``state_dict``, and the total (clipmi_cocoop_block_floats)."""
    n_ctx, D, E, H = int(n_ctx), int(D), int(E), int(H)
    total = lib.clipmi_cocoop_block_floats(n_ctx, D, E, H)
    if total == 0:
        raise ValueError(f"cocoop_block_layout: n_ctx={n_ctx} D={D} E={E} H={H} (all >= 1, H <= 4096)")
    out, off = collections.OrderedDict(), 0
    for name, shape in (("ctx", (n_ctx, D)), ("meta_net.linear1.weight", (H, E)), ("meta_net.linear1.bias", (H,)), ("meta_net.linear2.weight", (D, H)),
                        ("meta_net.linear2.bias", (D,))):
        out[name] = (off, shape)
        n = 1
        for s in shape:
            n *= s
        off += n
    assert off == total
    return out, total


def cocoop_block_views(block: torch.Tensor, n_ctx: int, D: int, E: int, H: int):
    """The five tensors of a parameter, momentum or gradient block fp32 [clipmi_cocoop_block_floats] as views of it."""
    layout, total = cocoop_block_layout(n_ctx, D, E, H)
    if block.numel() != total or block.dim() != 1:
        raise ValueError(f"cocoop_block_views: a block of {block.numel()} floats, {total} expected")
    return collections.OrderedDict((k, block[off:off + int(torch.Size(shape).numel())].view(shape)) for k, (off, shape) in layout.items())


def cocoop_meta(features: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, out=None):
    """CoCoOp's meta-net with what its backward needs kept: ``(x_n fp32 [B, E], hid fp32 [B, H], pi fp32 [B, D])`` for raw image
    ``features`` fp32 [B, E] (the rows may be a column slice): x = f / |f|, hid = relu(W1 x + b1), pi = W2 hid + b2.  ``out``: the
    caller's own three tensors, written where they lie."""
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.stride(1) != 1:
        raise ValueError("cocoop_meta: features must be a [B, E] tensor with unit column stride")
    if not features.is_cuda or features.dtype != torch.float32:
        raise TypeError("cocoop_meta: features must be fp32 on the GPU")
    w1, b1, w2, b2 = (_dev(t, n, (torch.float32,)) for t, n in ((w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2")))
    B, E = features.shape
    if w1.dim() != 2 or w2.dim() != 2 or w1.shape[1] != E or b1.shape != (w1.shape[0],) or w2.shape[1] != w1.shape[0] or b2.shape != (w2.shape[0],):
        raise ValueError(f"cocoop_meta: features {tuple(features.shape)}, W1 {tuple(w1.shape)}, b1 {tuple(b1.shape)}, W2 {tuple(w2.shape)}, b2 "
                         f"{tuple(b2.shape)} do not agree")
    H, D = int(w1.shape[0]), int(w2.shape[0])
    if out is None:
        out = tuple(torch.empty(B, n, dtype=torch.float32, device=features.device) for n in (E, H, D))
    else:
        for t, n in zip(out, (E, H, D)):
            _in_place(t, torch.float32, "cocoop_meta: x_n, hid and pi must be contiguous fp32 tensors on the GPU", numel=B * n)
    x_n, hid, pi = out
    check(lib.clipmi_cocoop_meta(features.data_ptr(), features.stride(0), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), x_n.data_ptr(),
                                 hid.data_ptr(), pi.data_ptr(), B, E, H, D, _stream()), "clipmi_cocoop_meta")
    return x_n, hid, pi


def cocoop_embed(base: torch.Tensor, ctx: torch.Tensor, pi: torch.Tensor, cls_eot: torch.Tensor, rows: int = 0, prompts: Optional[torch.Tensor] = None,
                 eot: Optional[torch.Tensor] = None):
    """CoCoOp's training prompts: ``(prompts fp32 [B * C, Lc, D], eot int32 [B * C])`` from the class embeddings ``base`` [C, Lc, D] (fp16
    or fp32), the fp32 master ``ctx`` [n_ctx, D], the images' shifts ``pi`` fp32 [B, D] and the classes' EOT rows ``cls_eot`` int32 [C]:
    image-major, context rows ``ctx[j] + pi[b]``.  Only the first ``rows`` token rows of each prompt are written (0: all of them).  A
    caller's own ``prompts`` and ``eot`` are written where they lie."""
    base = _dev(base, "base", (torch.float16, torch.float32))
    ctx, pi = _dev(ctx, "ctx", (torch.float32,)), _dev(pi, "pi", (torch.float32,))
    cls_eot = _dev(cls_eot, "cls_eot", (torch.int32,))
    if base.dim() != 3 or ctx.dim() != 2 or pi.dim() != 2 or ctx.shape[1] != base.shape[2] or pi.shape[1] != base.shape[2] or cls_eot.shape != (base.shape[0],):
        raise ValueError(f"cocoop_embed: base {tuple(base.shape)}, ctx {tuple(ctx.shape)}, pi {tuple(pi.shape)} and cls_eot {tuple(cls_eot.shape)} do not agree")
    Cn, Lc, D = base.shape
    B, n_ctx = int(pi.shape[0]), int(ctx.shape[0])
    N = B * Cn
    L = int(rows) if 0 < int(rows) < Lc else Lc
    if prompts is None:
        prompts = torch.empty(N, Lc, D, dtype=torch.float32, device=base.device)
    else:
        _in_place(prompts, torch.float32, "cocoop_embed: prompts must be a contiguous fp32 tensor on the GPU", numel=N * Lc * D)
    if eot is None:
        eot = torch.empty(N, dtype=torch.int32, device=base.device)
    else:
        _in_place(eot, torch.int32, "cocoop_embed: eot must be a contiguous int32 tensor on the GPU", numel=N)
    check(lib.clipmi_cocoop_embed(base.data_ptr(), _DT[base.dtype], ctx.data_ptr(), pi.data_ptr(), cls_eot.data_ptr(), prompts.data_ptr(), eot.data_ptr(),
                                  B, Cn, L, Lc, D, n_ctx, _stream()), "clipmi_cocoop_embed")
    return prompts, eot


def cocoop_head(features: torch.Tensor, labels: torch.Tensor, text: torch.Tensor, scale: float, grad_scale: float = 1.0,
                loss: Optional[torch.Tensor] = None, want_rows: bool = False):
    """CoCoOp's loss head: ``(loss fp32 [1], d_text fp32 [B * C, E])``, the gradient times ``grad_scale``; ``text`` fp32 [B * C, E] the
    raw features of the image-major prompts, ``features`` and ``labels`` as ``coop_head``'s.  ``want_rows`` adds the row losses fp32 [B]."""
    labels, text, B, E, N = _head_inputs("cocoop_head", features, labels, text)
    if N % B or N // B < 2:
        raise ValueError(f"cocoop_head: {N} text rows do not split into {B} images of at least 2 classes")
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=text.device)
    else:
        _in_place(loss, torch.float32, "cocoop_head: loss must be a contiguous fp32 tensor on the GPU", numel=1)
    rows = torch.empty(B, dtype=torch.float32, device=text.device) if want_rows else None
    d_text = torch.empty_like(text)
    ws = torch.empty(max(lib.clipmi_cocoop_head_workspace_bytes(B, N // B), 8), dtype=torch.uint8, device=text.device)
    check(lib.clipmi_cocoop_head(features.data_ptr(), features.stride(0), labels.data_ptr(), text.data_ptr(), B, E, N // B, float(scale), float(grad_scale),
                                 loss.data_ptr(), None if rows is None else rows.data_ptr(), d_text.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "clipmi_cocoop_head")
    return (loss, d_text, rows) if want_rows else (loss, d_text)


def cocoop_reduce(d_embed: torch.Tensor, x_n: torch.Tensor, hid: torch.Tensor, w2: torch.Tensor, n_cls: int, n_ctx: int, grad_scale: float,
                  grad: Optional[torch.Tensor] = None) -> torch.Tensor:
    """CoCoOp's five gradients from ``d_embed`` fp32 [B * C * L, D] as one block fp32 ``[ctx | W1 | b1 | W2 | b2]`` (``cocoop_block_views``
    splits it): the classes of an image in ascending order, divided by ``grad_scale``, then the meta-net's backward from ``x_n`` [B, E],
    ``hid`` [B, H] (its zeros are the ReLU's mask) and ``w2`` [D, H].  A caller's own ``grad`` is written where it lies."""
    d_embed, x_n, hid, w2 = (_dev(t, n, (torch.float32,)) for t, n in ((d_embed, "d_embed"), (x_n, "x_n"), (hid, "hid"), (w2, "w2")))
    if d_embed.dim() != 2 or x_n.dim() != 2 or hid.dim() != 2 or w2.dim() != 2 or hid.shape[0] != x_n.shape[0] or w2.shape != (d_embed.shape[1], hid.shape[1]):
        raise ValueError(f"cocoop_reduce: d_embed {tuple(d_embed.shape)}, x_n {tuple(x_n.shape)}, hid {tuple(hid.shape)}, w2 {tuple(w2.shape)} do not agree")
    (B, E), H, D, Cn = x_n.shape, int(hid.shape[1]), int(d_embed.shape[1]), int(n_cls)
    if Cn < 2 or d_embed.shape[0] % (B * Cn):
        raise ValueError(f"cocoop_reduce: {d_embed.shape[0]} rows do not split into {B} x {Cn} prompts")
    L = d_embed.shape[0] // (B * Cn)
    total = lib.clipmi_cocoop_block_floats(int(n_ctx), D, E, H)
    if grad is None:
        grad = torch.empty(max(total, 1), dtype=torch.float32, device=d_embed.device)
    else:
        _in_place(grad, torch.float32, "cocoop_reduce: grad must be a contiguous fp32 tensor on the GPU", numel=total)
    ws = torch.empty(max(lib.clipmi_cocoop_reduce_workspace_bytes(B, int(n_ctx), D, H), 8), dtype=torch.uint8, device=d_embed.device)
    check(lib.clipmi_cocoop_reduce(d_embed.data_ptr(), x_n.data_ptr(), hid.data_ptr(), w2.data_ptr(), grad.data_ptr(), B, Cn, L, D, E, H, int(n_ctx),
                                   float(grad_scale), ws.data_ptr(), ws.numel(), _stream()), "clipmi_cocoop_reduce")
    return grad


def cocoop_step(grad: torch.Tensor, params: torch.Tensor, buf: Optional[torch.Tensor], lr: torch.Tensor, n_ctx: int, D: int, E: int, H: int,
                first_step: bool = False, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False) -> None:
    """torch.optim.SGD's step on CoCoOp's parameter block ``params`` fp32 in place, with the gradient block ``grad`` and the momentum block
    ``buf`` (None without a momentum), at the rate ``lr`` fp32 [1] on the device: one rule and one set of hyper-parameters for the five
    tensors."""
    total = lib.clipmi_cocoop_block_floats(int(n_ctx), int(D), int(E), int(H))
    _in_place(params, torch.float32, "cocoop_step: params must be a contiguous fp32 tensor on the GPU", numel=total)
    _in_place(grad, torch.float32, "cocoop_step: grad must be a contiguous fp32 tensor on the GPU", numel=total)
    if buf is not None:
        _in_place(buf, torch.float32, "cocoop_step: buf must be a contiguous fp32 tensor on the GPU", numel=total)
    lr = _dev(lr, "lr", (torch.float32,))
    if lr.numel() != 1:
        raise ValueError("cocoop_step: lr must hold one rate")
    check(lib.clipmi_cocoop_step(grad.data_ptr(), params.data_ptr(), None if buf is None else buf.data_ptr(), int(n_ctx), int(D), int(E), int(H),
                                 lr.data_ptr(), int(bool(first_step)), float(momentum), float(dampening), float(weight_decay), int(bool(nesterov)),
                                 _stream()), "clipmi_cocoop_step")


# ---- the class-sharded CoCoOp fit (csrc/cocoop_train.hip, DESIGN.md "Class-sharded CoCoOp fit")

def cocoop_embed_classes(base: torch.Tensor, ctx: torch.Tensor, pi: torch.Tensor, cls_eot: torch.Tensor, lo: int, hi: int, rows: int = 0,
                         prompts: Optional[torch.Tensor] = None, eot: Optional[torch.Tensor] = None):
    """``cocoop_embed`` for the classes ``[lo, hi)`` of ``base`` [C, Lc, D] and ``cls_eot`` [C] (one class is enough): ``(prompts fp32
    [B * (hi - lo), Lc, D], eot int32 [B * (hi - lo)])``, image-major -- the slice ``[:, lo:hi]`` of ``cocoop_embed``'s [B, C, Lc, D]."""
    base = _dev(base, "base", (torch.float16, torch.float32))
    ctx, pi = _dev(ctx, "ctx", (torch.float32,)), _dev(pi, "pi", (torch.float32,))
    cls_eot = _dev(cls_eot, "cls_eot", (torch.int32,))
    if base.dim() != 3 or ctx.dim() != 2 or pi.dim() != 2 or ctx.shape[1] != base.shape[2] or pi.shape[1] != base.shape[2] or cls_eot.shape != (base.shape[0],):
        raise ValueError(f"cocoop_embed_classes: base {tuple(base.shape)}, ctx {tuple(ctx.shape)}, pi {tuple(pi.shape)} and cls_eot {tuple(cls_eot.shape)} "
                         "do not agree")
    Cn, Lc, D = base.shape
    lo, hi = int(lo), int(hi)
    if not 0 <= lo < hi <= Cn:
        raise ValueError(f"cocoop_embed_classes: the classes [{lo}, {hi}) must be a non-empty range of the {Cn} classes")
    B, n_ctx = int(pi.shape[0]), int(ctx.shape[0])
    N = B * (hi - lo)
    L = int(rows) if 0 < int(rows) < Lc else Lc
    if prompts is None:
        prompts = torch.empty(N, Lc, D, dtype=torch.float32, device=base.device)
    else:
        _in_place(prompts, torch.float32, "cocoop_embed_classes: prompts must be a contiguous fp32 tensor on the GPU", numel=N * Lc * D)
    if eot is None:
        eot = torch.empty(N, dtype=torch.int32, device=base.device)
    else:
        _in_place(eot, torch.int32, "cocoop_embed_classes: eot must be a contiguous int32 tensor on the GPU", numel=N)
    check(lib.clipmi_cocoop_embed_classes(base.data_ptr(), _DT[base.dtype], ctx.data_ptr(), pi.data_ptr(), cls_eot.data_ptr(), prompts.data_ptr(),
                                          eot.data_ptr(), B, Cn, lo, hi, L, Lc, D, n_ctx, _stream()), "clipmi_cocoop_embed_classes")
    return prompts, eot


def cocoop_shard_pad(n_cls: int, world: int) -> int:
    """Classes per rank of the gathered text features' blocks: ``ceil(C / G)``."""
    return -(-int(n_cls) // int(world))


def cocoop_shard_compact(gathered: torch.Tensor, B: int, n_cls: int, E: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gathered fp32 [G, elements per rank >= B * ceil(C / G) * E] text features -> fp32 [B * C, E] in the unsharded, image-major order:
    rank r's block starts with its own [B, C_r, E]; what lies behind it is never read.  One launch."""
    who = "cocoop_shard_compact"
    _in_place(gathered, torch.float32, f"{who}: gathered must be a contiguous fp32 tensor on the GPU")
    B, Cn, E = int(B), int(n_cls), int(E)
    if gathered.dim() != 2 or not 1 <= gathered.shape[0] <= Cn or B < 1 or E < 1:
        raise ValueError(f"{who}: gathered {tuple(gathered.shape)} must be [G, elements per rank] with 1 <= G <= C = {Cn}")
    G, stride = gathered.shape
    need = B * cocoop_shard_pad(Cn, G) * E
    if stride < need:
        raise ValueError(f"{who}: gathered {tuple(gathered.shape)} holds fewer than B * ceil(C / G) * E = {need} elements per rank")
    if out is None:
        out = torch.empty(B * Cn, E, dtype=torch.float32, device=gathered.device)
    else:
        _in_place(out, torch.float32, f"{who}: out must be a contiguous fp32 tensor on the GPU", numel=B * Cn * E)
    check(lib.clipmi_cocoop_shard_compact(gathered.data_ptr(), out.data_ptr(), B, Cn, G, E, stride, _stream()), "clipmi_cocoop_shard_compact")
    return out


def cocoop_shard_rows(d_text: torch.Tensor, B: int, lo: int, hi: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The rows ``{b * C + c : lo <= c < hi}`` of ``d_text`` fp32 [B * C, E] as a contiguous fp32 [B * (hi - lo), E].  One launch."""
    who = "cocoop_shard_rows"
    d_text = _dev(d_text, "d_text", (torch.float32,))
    B, lo, hi = int(B), int(lo), int(hi)
    if d_text.dim() != 2 or B < 1 or d_text.shape[0] % B:
        raise ValueError(f"{who}: d_text {tuple(d_text.shape)} does not split into {B} images")
    Cn, E = d_text.shape[0] // B, int(d_text.shape[1])
    if not 0 <= lo < hi <= Cn:
        raise ValueError(f"{who}: the classes [{lo}, {hi}) must be a non-empty range of the {Cn} classes")
    if out is None:
        out = torch.empty(B * (hi - lo), E, dtype=torch.float32, device=d_text.device)
    else:
        _in_place(out, torch.float32, f"{who}: out must be a contiguous fp32 tensor on the GPU", numel=B * (hi - lo) * E)
    check(lib.clipmi_cocoop_shard_rows(d_text.data_ptr(), out.data_ptr(), B, Cn, lo, hi, E, _stream()), "clipmi_cocoop_shard_rows")
    return out


def cocoop_dcs_partial(d_embed: torch.Tensor, B: int, n_cls: int, n_ctx: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A rank's send block fp32 [B, n_ctx, D] from its own ``d_embed`` fp32 [B * C_r * L, D] (``n_cls`` = C_r >= 1, its own classes):
    the context rows of an image's C_r prompts added in ascending class order from 0, unscaled.  One launch."""
    who = "cocoop_dcs_partial"
    d_embed = _dev(d_embed, "d_embed", (torch.float32,))
    B, Cn, n_ctx = int(B), int(n_cls), int(n_ctx)
    if d_embed.dim() != 2 or B < 1 or Cn < 1 or d_embed.shape[0] % (B * Cn):
        raise ValueError(f"{who}: d_embed {tuple(d_embed.shape)} does not split into {B} x {Cn} prompts")
    L, D = d_embed.shape[0] // (B * Cn), int(d_embed.shape[1])
    if out is None:
        out = torch.empty(B, n_ctx, D, dtype=torch.float32, device=d_embed.device)
    else:
        _in_place(out, torch.float32, f"{who}: out must be a contiguous fp32 tensor on the GPU", numel=B * n_ctx * D)
    check(lib.clipmi_cocoop_dcs_partial(d_embed.data_ptr(), out.data_ptr(), B, Cn, L, D, n_ctx, _stream()), "clipmi_cocoop_dcs_partial")
    return out


def cocoop_reduce_gathered(partials: torch.Tensor, x_n: torch.Tensor, hid: torch.Tensor, w2: torch.Tensor, n_ctx: int, grad_scale: float,
                           grad: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``cocoop_reduce`` from the gathered partials fp32 [G, elements per rank >= B * n_ctx * D] (rank r's ``cocoop_dcs_partial`` first in
    row r): the G partials added in rank order from 0, one multiplication by ``1 / grad_scale``, then the meta-net's backward as
    ``cocoop_reduce`` runs it.  Every rank given the same blocks writes the same gradient block."""
    who = "cocoop_reduce_gathered"
    _in_place(partials, torch.float32, f"{who}: partials must be a contiguous fp32 tensor on the GPU")
    x_n, hid, w2 = (_dev(t, n, (torch.float32,)) for t, n in ((x_n, "x_n"), (hid, "hid"), (w2, "w2")))
    if partials.dim() != 2 or x_n.dim() != 2 or hid.dim() != 2 or w2.dim() != 2 or hid.shape[0] != x_n.shape[0] or w2.shape[1] != hid.shape[1]:
        raise ValueError(f"{who}: partials {tuple(partials.shape)}, x_n {tuple(x_n.shape)}, hid {tuple(hid.shape)}, w2 {tuple(w2.shape)} do not agree")
    (B, E), H, D, n_ctx = x_n.shape, int(hid.shape[1]), int(w2.shape[0]), int(n_ctx)
    G, stride = partials.shape
    if G < 1 or n_ctx < 1 or stride < B * n_ctx * D:
        raise ValueError(f"{who}: partials {tuple(partials.shape)} holds fewer than B * n_ctx * D = {B * n_ctx * D} elements per rank")
    total = lib.clipmi_cocoop_block_floats(n_ctx, D, E, H)
    if grad is None:
        grad = torch.empty(max(total, 1), dtype=torch.float32, device=partials.device)
    else:
        _in_place(grad, torch.float32, f"{who}: grad must be a contiguous fp32 tensor on the GPU", numel=total)
    ws = torch.empty(max(lib.clipmi_cocoop_reduce_workspace_bytes(B, n_ctx, D, H), 8), dtype=torch.uint8, device=partials.device)
    check(lib.clipmi_cocoop_reduce_gathered(partials.data_ptr(), G, stride, x_n.data_ptr(), hid.data_ptr(), w2.data_ptr(), grad.data_ptr(), B, D, E, H, n_ctx,
                                            float(grad_scale), ws.data_ptr(), ws.numel(), _stream()), "clipmi_cocoop_reduce_gathered")
    return grad


# ---- per-epoch validation of the CoCoOp and ProDA fits (csrc/fit_monitor.hip, csrc/proda_train.hip; DESIGN.md "Fit monitor", "CoCoOp and ProDA")
COCOOP_VAL_MAX_C = 16384      # cocoop_val_rows_kernel keeps one image's C fp32 logits in LDS


def cocoop_val_rows(img_n: torch.Tensor, txt: torch.Tensor, scale: float, labels: torch.Tensor, n_bins: int,
                    row_results: Optional[torch.Tensor] = None, row0: int = 0) -> torch.Tensor:
    """clipmi_cocoop_val_rows: CoCoOp's per-pair tail fused into the row score.  ``img_n`` fp32 [Bv, E] unit image features, ``txt`` fp32
    [Bv, C, E] raw text-encoder outputs, ``labels`` int64 [Bv]: per image the C logits ``scale * <img_n[b], normalise(txt[b, c])>`` are
    formed in LDS (``logits_per_image``'s bits) and scored as ``val_score_rows`` scores a row, into ``row_results[row0 : row0 + Bv]``; the
    [Bv, C] logits never go to memory.  Returns ``row_results``."""
    who = "cocoop_val_rows"
    n_bins = _val_bins(who, n_bins)
    img_n = _dev(img_n, "img_n", (torch.float32,))
    txt = _dev(txt, "txt", (torch.float32,))
    labels = _dev(labels, "labels", (torch.int64,))
    if img_n.dim() != 2 or img_n.shape[0] < 1:
        raise ValueError(f"{who}: img_n {tuple(img_n.shape)} must be [Bv >= 1, E]")
    B, E = img_n.shape
    if txt.dim() != 3 or txt.shape[0] != B or txt.shape[2] != E or not 1 <= txt.shape[1] <= COCOOP_VAL_MAX_C:
        raise ValueError(f"{who}: txt must be [Bv={B}, 1 <= C <= {COCOOP_VAL_MAX_C}, E={E}], got {tuple(txt.shape)}")
    if labels.shape != (B,):
        raise ValueError(f"{who}: {B} rows need {B} labels, got {tuple(labels.shape)}")
    if row_results is None:
        row_results = new_val_row_results(row0 + B, img_n.device)
    pr = _row_results(who, row_results, B, row0)
    check(lib.clipmi_cocoop_val_rows(img_n.data_ptr(), txt.data_ptr(), float(scale), labels.data_ptr(), B, txt.shape[1], E, n_bins, pr, _stream()),
          "clipmi_cocoop_val_rows")
    return row_results


def proda_val_mean(text: torch.Tensor, group: int) -> torch.Tensor:
    """clipmi_proda_val_mean: raw text features fp32 [G * group, E] -> fp32 [G, E], the mean over a class's ``group`` L2-normalised rows
    (not renormalised): the bits of ``group_mean(l2_normalize(text), group)`` in one launch, without the normalised copy."""
    text = _dev(text, "text", (torch.float32,))
    rows, E = text.shape
    if group <= 0 or rows % group or rows == 0:
        raise ValueError(f"proda_val_mean: {rows} rows do not split into groups of {group}")
    out = torch.empty(rows // group, E, dtype=torch.float32, device=text.device)
    check(lib.clipmi_proda_val_mean(text.data_ptr(), out.data_ptr(), rows // group, int(group), E, _stream()), "clipmi_proda_val_mean")
    return out


ROW_SCORES_MAX_BINS = 1024     # clipmi_ece_accumulate's limit


def _row_score_bins(who: str, n_bins) -> int:
    if isinstance(n_bins, bool) or int(n_bins) != n_bins or not 1 <= int(n_bins) <= ROW_SCORES_MAX_BINS:
        raise ValueError(f"{who}: n_bins={n_bins} must be an integer in 1..{ROW_SCORES_MAX_BINS}")
    return int(n_bins)


def new_row_scores_acc(n_classes: int, n_bins: int, device) -> torch.Tensor:
    """The zeroed class-wise block of ``row_scores``: int64 [3, C, n_bins + 1] = count | conf_sum (32.32 fixed point) | hits on ``device``
    (``metrics.classwise_from_bins`` reads it)."""
    n_bins = _row_score_bins("new_row_scores_acc", n_bins)
    if int(n_classes) < 1:
        raise ValueError(f"new_row_scores_acc: n_classes={n_classes} (>= 1)")
    return torch.zeros(3, int(n_classes), n_bins + 1, dtype=torch.int64, device=device)


def row_scores(rows: torch.Tensor, labels: torch.Tensor, from_probs: bool = False, n_bins: int = 10, acc: Optional[torch.Tensor] = None,
               row_out: Optional[torch.Tensor] = None, row0: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """clipmi_row_scores: fp32 ``rows`` [N, C] (the rows may be a column slice) -- logits, or probabilities as given with ``from_probs`` --
    against ``labels`` int64 [N]: per row the negative log-likelihood and the Brier score into ``row_out[row0 : row0 + N]`` (fp32 [*, 2] on
    the GPU, made for this call alone when None), and every element into its class's confidence bin of ``acc`` (``new_row_scores_acc``,
    made when None), which is ADDED to: integer sums, so the block's bytes do not depend on how the rows were cut into calls.  A label
    outside [0, C) gives a NaN row score and no hit; a row without a softmax (a NaN, a +inf, nothing but -inf; any non-finite
    probability) gives a NaN row score and counts in the last bin only.  Nothing is read back; the inputs are not written.
    Returns ``(row_out, acc)``; ``row_scores_finish`` turns them into the scalars."""
    who = "row_scores"
    n_bins = _row_score_bins(who, n_bins)
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.shape[1] < 1:
        raise ValueError(f"{who}: rows {tuple(getattr(rows, 'shape', ()))} must be [N, C >= 1]")
    if not rows.is_cuda:
        raise RuntimeError(f"clipmi: `rows` must be a tensor on the GPU (got {rows.device}); the HIP path has no CPU fallback")
    if rows.dtype != torch.float32:
        raise TypeError(f"clipmi: `rows` has dtype {rows.dtype}, expected torch.float32")
    if rows.device.index != torch.cuda.current_device():
        raise RuntimeError(f"clipmi: `rows` is on {rows.device} but the current device is cuda:{torch.cuda.current_device()}")
    if rows.shape[0] and (rows.stride(1) != 1 or rows.stride(0) < rows.shape[1]):
        rows = rows.contiguous()
    labels = _dev(labels, "labels", (torch.int64,))
    N, Cn = rows.shape
    if labels.shape != (N,):
        raise ValueError(f"{who}: {N} rows need {N} labels, got {tuple(labels.shape)}")
    if acc is None:
        acc = new_row_scores_acc(Cn, n_bins, rows.device)
    _in_place(acc, torch.int64, f"{who}: acc must be a contiguous int64 [3, {Cn}, {n_bins + 1}] tensor on the GPU (new_row_scores_acc)",
              numel=3 * Cn * (n_bins + 1))
    if row_out is None:
        row_out = torch.empty(row0 + N, 2, dtype=torch.float32, device=rows.device)
    if not (isinstance(row_out, torch.Tensor) and row_out.is_cuda and row_out.dtype == torch.float32 and row_out.is_contiguous()
            and row_out.dim() == 2 and row_out.shape[1] == 2):
        raise TypeError(f"{who}: row_out must be a contiguous fp32 [rows, 2] tensor on the GPU")
    if isinstance(row0, bool) or int(row0) != row0 or row0 < 0 or row0 + N > row_out.shape[0]:
        raise ValueError(f"{who}: rows {row0} .. {row0 + N} lie outside the {row_out.shape[0]} row scores")
    if N == 0:
        return row_out, acc
    check(lib.clipmi_row_scores(rows.data_ptr(), rows.stride(0), labels.data_ptr(), N, Cn, int(bool(from_probs)), n_bins,
                                row_out.data_ptr() + 8 * int(row0), acc.data_ptr(), _stream()), "clipmi_row_scores")
    return row_out, acc


def row_scores_finish_device(row_out: torch.Tensor, acc: torch.Tensor, out: Optional[torch.Tensor] = None,
                             workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """clipmi_row_scores_finish without the read-back: float64 [4] on the GPU = mean nll, mean Brier, class-wise ECE (a fraction), N."""
    who = "row_scores_finish"
    if not (isinstance(row_out, torch.Tensor) and row_out.is_cuda and row_out.dtype == torch.float32 and row_out.is_contiguous()
            and row_out.dim() == 2 and row_out.shape[1] == 2 and row_out.shape[0] >= 1):
        raise TypeError(f"{who}: row_out must be a contiguous fp32 [N >= 1, 2] tensor on the GPU")
    if not (isinstance(acc, torch.Tensor) and acc.is_cuda and acc.dtype == torch.int64 and acc.is_contiguous() and acc.dim() == 3
            and acc.shape[0] == 3 and acc.shape[1] >= 1 and acc.shape[2] >= 2):
        raise TypeError(f"{who}: acc must be a contiguous int64 [3, C, n_bins + 1] tensor on the GPU (new_row_scores_acc)")
    N, Cn, n_bins = int(row_out.shape[0]), int(acc.shape[1]), int(acc.shape[2]) - 1
    if out is None:
        out = torch.empty(4, dtype=torch.float64, device=row_out.device)
    _in_place(out, torch.float64, f"{who}: out must be a contiguous float64 [4] tensor on the GPU", numel=4)
    need = lib.clipmi_row_scores_finish_workspace_bytes(N, Cn)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=row_out.device)
    check(lib.clipmi_row_scores_finish(row_out.data_ptr(), N, acc.data_ptr(), Cn, n_bins, out.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                       _stream()), "clipmi_row_scores_finish")
    return out


def row_scores_finish(row_out: torch.Tensor, acc: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> dict:
    """clipmi_row_scores_finish: ``dict(nll, brier, cw_ece, n)`` -- the mean negative log-likelihood, the mean Brier score, the class-wise
    ECE as a fraction and the row count -- from every row of ``row_out`` and the block ``acc``; the order of the additions depends on N
    and C alone, so the numbers are the same bits however the rows were chunked.  The one read-back of the path: it synchronises."""
    o = row_scores_finish_device(row_out, acc, workspace=workspace).cpu().numpy()
    return {"nll": float(o[0]), "brier": float(o[1]), "cw_ece": float(o[2]), "n": int(o[3])}
