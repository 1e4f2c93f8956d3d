"""One per-element bound and one fp32 emulation of a step of the three cached-feature fits: TaskRes (csrc/taskres_train.hip), CLIP-Adapter
(csrc/adapter_train.hip) and TempScaling (csrc/tempscale.hip), with the rules of csrc/train_rules.h.  It does not import the package's kernels.

The float64 formulas are the existing restatements -- ``taskresfit_ref.backward`` / ``adam_rule``, ``adapterfit_ref.backward``,
``tempscale_ref.batch_loss_grad`` / ``sgd_step`` -- called by the ``*_formulas`` functions; the bound functions evaluate the same expressions
once more, with the intermediate values the bound needs, and tests/test_cached_fit_ref_cpu.py holds the two equal.

The bound, u = 2^-24, derived from the kernels as written, one rounding point at a time.  Every term is evaluated on the float64 reference;
nothing the device returns enters it.  Shared pieces are head_ref's: ``_softmax_bound`` (__expf, the softmax sensitivities, xent_row's row
loss and dz with k = 1 / B), ``_mean_bound`` (the float64 mean rounded once).

TaskRes (``taskres_bound``), n16 = ceil(E / 16):
  t        t_e = fl(base_e + fl(alpha r_e)):  tt_e = u (|alpha r_e| + |t_e|).
  norms    ss = sum_e v_e^2 is a 16-strided fmaf chain of n16 terms and row16_sum's four levels over positive terms: relative (n16 + 4) u;
           sqrtf halves it and adds one rounding:  ef = ((n16 + 4) / 2 + 1) u on |f_b|;  en_c = ((n16 + 4) u + 2 sum_e |t_e| tt_e / n_c^2) / 2 + u.
  logit    acc = sum_e f_e t_e is ONE serial fmaf chain of depth E:  tacc = E u sum_e |f_e t_e| + sum_e |f_e| tt_e;
           z = fl(scale fl(fl(acc / nf) / n)):  tz = scale tacc / (nf n) + (3 u + ef + en_c) |z|.
  softmax  head_ref's, over 256 threads and four waves (nC + 10 roundings of S), k = fl(1 / rows).
  q_c      sum_b dz[b, c] z[b, c] in four serial fmaf ranges of span = ceil(rows / 4), added in order:
           tq = sum_b (tdz |z| + |dz| tz) + (span + 3) u sum_b |dz z|.
  du       acc2 = sum_b dz[b, c] x_be, x_be = fl(f_be / nf_b), a serial fmaf chain over the rows:
           tacc2 = sum_b tdz |x| + (ef + (1 + rows) u) sum_b |dz x|;  du = fl(scale acc2):  tdu = scale tacc2 + u |du|.
  dr       u_e = fl(t_e / n):  tu = tt / n + (en + u) |u|;  inner = fl(du - fl(u q)):  tinner = tdu + |u| tq + |q| tu + u |u q| + u |inner|;
           g = fl(alpha fl(inner / n)):  tg = |alpha| tinner / n + (en + 2 u) |g|.
  SGD      r' = fl(r - fl(lr g)):  lr tg + u |lr g| + u |r'|  (lr 1: u |r'| and tg alone; the momentum buffer of a first step is g itself).
  Adam     first step from zero moments, no weight decay: the update is lr g / (|g| + eps) in exact arithmetic; its derivative in g is
           lr eps / (|g| + eps)^2, taken at max(|g| - tg, 0); the rule's own roundings (1 - beta1 as fp32, m, v's three, step_size, sqrtf, the
           two divisions, + eps, the product) are below 12 u |update|, v below fp32's normal range adds 2^-62 lr |g| / (|g| + eps)^2; then u |r'|.

CLIP-Adapter (``adapter_bound``), n64(n) = ceil(n / 64); wave_dot is a lane-strided chain of n64 terms and the six-level tree: (n64 + 6) u sum |terms|:
  p1, h    tp1 = (n64(E) + 6) u sum_e |w1 f|;  relu is 1-Lipschitz: th = tp1.
  p2, a    tp2 = sum_k |w2_ek| th_k + (n64(H) + 6) u sum_k |w2 h|;  ta = tp2.
  g        fl(fl(ratio a) + fl(fl(1 - ratio) f)):  tg = ratio ta + u |ratio a| + 2 u |(1 - ratio) f| + u |g|.
  n, u     n = sqrtf(wave sum of g^2):  en = ((n64 + 6) u + 2 sum |g| tg / n^2) / 2 + u;  u = fl(g / n):  tu = tg / n + (en + u) |u|.
  logit    z_c = fl(scale wave_dot(T_c, u)):  tz = scale (sum_e |T_ce| tu_e + (n64 + 6) u sum_e |T u|) + u |z|.
  softmax  head_ref's with xent_row over 1024 threads and 16 waves: S carries ceil(C / 1024) + 6 + 15 roundings.
  columns_sum(mat, coef, depth, cols): parts = 1024 / cols (1 from 513 columns on), span = ceil(depth / parts), as the kernel computes them;
           `parts` serial ranges added in order:  sum_k tcoef_k |mat_kj| + (span + parts - 1) u sum_k |coef_k mat_kj|.
  du       fl(scale columns_sum(T, dz, C, E)):  tdu = scale traw + u |du|;  dot = u . du lane-strided:  tdot = sum (tu |du| + |u| tdu) + (n64 + 6) u sum |u du|.
  dg, da   dg = fl(fl(du - fl(u dot)) / n):  tdg = (tdu + tu |dot| + |u| tdot + u |u dot| + u |inner|) / n + (en + u) |dg|;  da = fl(ratio dg) [p2 > 0]:  ratio tdg + u |da|.
  dh       columns_sum(W2, da, E, H) [p1 > 0].
  dW2, dW1 sum_b da[b, e] h[b, k] and sum_b dh[b, k] f[b, e], serial over the rows:  sum_b (tda |h| + |da| th) + rows u sum_b |da h|, likewise dW1.
  ReLU     h is 0 on both sides where p1 < -tp1, so th = tp1 [p1 > -tp1], and likewise ta = tp2 [p2 > -tp2].  The masks [p > 0] are not
           continuous: a pre-activation with |p| <= tp may have the other sign on the device.  ``adapter_bound`` lists those (row, unit)
           pairs of the float64 reference; adapterfit_ref.excluded turns them into the entries of dW1 / dW2 that depend on them
           (``adapter_masks``), which are not compared: at most adapterfit_ref.EXCLUDED_CAP of either tensor, per case.
  cases    A worst-case bound grows with every L1 sum a value passes through, and f -> p1 -> p2 -> g -> z passes three.  ``adapter_case``
           therefore takes W1 and W2 at torch.nn.Linear's own initial spread (uniform of variance 1 / (3 fan_in): adapterfit_ref's
           draws times 1 / sqrt(3)) and W2 times W2_GAIN more, so that the adapter's branch is the small correction to f it is when a fit
           starts; at the LDS-limit shape, whose 7600 values of p2 cannot all stay clear of zero by a seed, every row of W2 has one sign,
           so p2_e = +- sum_k h_k |w2_ek| has no cancellation.
  SGD      w' = fl(w - fl(lr g)), as TaskRes'.

TempScaling: tempscale_ref.batch_error_bound is the derivation (S and T lane-strided, the float64 batch sums rounded once); ``tempscale_bound``
adds the step: the momentum buffer of a first step is the gradient itself, theta' = fl(theta - fl(lr g)):  lr tg + u |lr g| + u |theta'|.

The emulation (``emulate_*``) is numpy fp32 in the kernels' own summation orders; fmaf is evaluated in float64 and rounded once, __expf is
exp2 of the fp32 product.  ``corrupt`` seeds one defect (*_CORRUPTIONS)."""
import functools
import math

import numpy as np
import torch

import adapterfit_ref
import head_ref
import taskresfit_ref
import tempscale_ref
from head_ref import F, U, _expf, _fma, _lane_dot, _mean_f64, _tree, ceil_div, ratio  # noqa: F401  (ratio is the tests')

ALPHA = taskresfit_ref.ALPHA
S = taskresfit_ref.scale_of()
RATIO = float(np.float32(0.2))                 # clip_adapter.py's residual ratio, rounded to fp32 once as the host hands it over
ADAM = dict(betas=(0.9, 0.999), eps=1e-8)
ADAM_LR = float(np.float32(2e-3))
THETA = float(np.float32(taskresfit_ref.LOGIT_SCALE))
TEMP_LR = float(np.float32(0.01))

# (rows, E, C): a ragged last tile on every axis with E no multiple of 16; rows above 256 (strided mean, q_c ranges of 65, 65, 65, 62) at
# ImageNet's classes; fewer rows than q_c ranges at RN50's width
TASKRES_SHAPES = ((65, 70, 257), (257, 64, 1000), (3, 1024, 66))
# (rows, E, H, C): columns_sum with parts == 1 below 1024 columns (E = 768, E = 640); 1024 / 171 = 5 parts of an uneven span and 257 classes
# over 16 waves; rows above 256; the largest shape rows_lds_bytes accepts.  The value is the seed (tests/test_cached_fit_ref_cpu.py holds
# the excluded share of each below the cap)
ADAPTER_SHAPES = {(3, 768, 192, 1000): 1, (2, 640, 160, 17): 6, (5, 171, 48, 257): 25, (257, 64, 16, 3): 1, (2, 3800, 64, 3): 1}
TEMPSCALE_SHAPES = ((5, 65), (257, 1000), (1025, 3))


def _ro(c):
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def taskres_case(shape):
    """taskresfit_ref.make_case with the first row's label on the last class and the last row's on class 0."""
    c = taskresfit_ref.make_case(*shape, seed=11)
    c["y"][0], c["y"][-1] = shape[2] - 1, 0
    return _ro(c)


W2_GAIN = 0.125
LDS_LIMIT_SHAPE = (2, 3800, 64, 3)


@functools.lru_cache(maxsize=None)
def adapter_case(shape):
    """adapterfit_ref.make_case with the weights conditioned as the docstring says, the first row's label on the last class, the last on 0."""
    c = adapterfit_ref.make_case(*shape, seed=ADAPTER_SHAPES[shape])
    c["w1"] = (c["w1"] / math.sqrt(3.0)).astype(F)
    c["w2"] = (c["w2"] * (W2_GAIN / math.sqrt(3.0))).astype(F)
    if shape == LDS_LIMIT_SHAPE:
        sign = np.where(np.arange(shape[1]) % 2 == 0, 1.0, -1.0).astype(F)
        sign[-1] = 1.0                      # the last feature is active: the last term of dh's sum is not 0
        c["w2"] = (np.abs(c["w2"]) * sign[:, None]).astype(F)
    c["y"][0], c["y"][-1] = shape[3] - 1, 0
    return _ro(c)


@functools.lru_cache(maxsize=None)
def tempscale_case(shape):
    c, y = tempscale_ref.make_case(*shape, seed=3)
    y[0] = shape[1] - 1                           # the last class, raised as make_case raises a sharp row's label
    c[0, y[0]] = np.float32(0.5 * (float(c[0].max()) + 1.0))
    return _ro(dict(c=c, y=y))


def _t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _sgd_bound(w, g, tg, lr):
    new = w - lr * g
    return new, lr * tg + (U * (lr * g).abs() if lr != 1.0 else 0.0) + U * new.abs()


# ------------------------------------------------------------------------------------------------------------------------- TaskRes
@functools.lru_cache(maxsize=None)
def taskres_bound(shape, alpha=ALPHA, s=S, lr=1.0, adam_lr=ADAM_LR):
    """{name: (want float64, tol)}: rows [B], loss [1], dr [C, E], r_sgd (one SGD step at ``lr``), r_adam (a first Adam step at ``adam_lr``)."""
    c = taskres_case(shape)
    f, base, r, y = _t64(c["f"]), _t64(c["base"]), _t64(c["r"]), torch.from_numpy(np.array(c["y"]))
    B, E = f.shape
    C = base.shape[0]
    n16 = ceil_div(E, 16)
    t = base + alpha * r
    tt = U * ((alpha * r).abs() + t.abs())
    nf, n = f.norm(dim=1, keepdim=True), t.norm(dim=1, keepdim=True)
    ef = ((n16 + 4) / 2 + 1) * U
    en = ((n16 + 4) * U + 2 * (t.abs() * tt).sum(1, keepdim=True) / n ** 2) / 2 + U
    x, u = f / nf, t / n
    tacc = E * U * (f.abs() @ t.abs().t()) + f.abs() @ tt.t()
    z = s * (f @ t.t()) / nf / n.t()
    tz = abs(s) * tacc / nf / n.t() + (3 * U + ef + en.t()) * z.abs()
    _, _, dz, tdz, rows, trows = head_ref._softmax_bound(z, tz, y, 1.0 / B, C)
    loss, tloss = head_ref._mean_bound(rows, trows)
    span = ceil_div(B, 4)
    q = (dz * z).sum(0)[:, None]
    tq = ((tdz * z.abs() + dz.abs() * tz).sum(0) + (span + 3) * U * (dz * z).abs().sum(0))[:, None]
    du = s * (dz.t() @ x)
    tdu = abs(s) * (tdz.t() @ x.abs() + (ef + (1 + B) * U) * (dz.abs().t() @ x.abs())) + U * du.abs()
    tu = tt / n + (en + U) * u.abs()
    inner = du - u * q
    tinner = tdu + u.abs() * tq + q.abs() * tu + U * (u * q).abs() + U * inner.abs()
    g = alpha * inner / n
    tg = abs(alpha) * tinner / n + (en + 2 * U) * g.abs()
    r_sgd, tr_sgd = _sgd_bound(r, g, tg, lr)
    eps = ADAM["eps"]
    upd = adam_lr * g / (g.abs() + eps)
    low = (g.abs() - tg).clamp(min=0) + eps
    tupd = adam_lr * eps / low ** 2 * tg + 12 * U * upd.abs() + 2.0 ** -62 * adam_lr * g.abs() / (g.abs() + eps) ** 2
    r_adam = r - upd
    return {"rows": (rows, trows), "loss": (loss.reshape(1), tloss.reshape(1)), "dr": (g, tg), "r_sgd": (r_sgd, tr_sgd),
            "r_adam": (r_adam, tupd + U * r_adam.abs())}


def taskres_formulas(shape, alpha=ALPHA, s=S, adam_lr=ADAM_LR):
    c = taskres_case(shape)
    b = taskresfit_ref.backward(c, alpha, s)
    zero = np.zeros_like(b["dr"])
    r_adam, _, _ = taskresfit_ref.adam_rule(np.asarray(c["r"], np.float64), b["dr"], zero, zero, 1, adam_lr, **ADAM)
    return {"rows": _t64(b["row_loss"]), "loss": _t64(b["row_loss"].mean()).reshape(1), "dr": _t64(b["dr"]),
            "r_sgd": _t64(np.asarray(c["r"], np.float64) - b["dr"]), "r_adam": _t64(r_adam)}


TASKRES_CORRUPTIONS = ("tile_last_column", "q_fourth_range", "mean_first_256", "norm_E_minus_1", "alpha_missing", "skip_last_batch_row")


def _norm16(v, short=False):
    """sqrtf of the 16-strided fmaf chains' row16_sum over the last axis (taskres_logits_kernel's norms)."""
    if short:
        v = v[..., :-1]
    E = v.shape[-1]
    n = ceil_div(E, 16)
    v = np.pad(v, [(0, 0)] * (v.ndim - 1) + [(0, n * 16 - E)])
    ss = np.zeros(v.shape[:-1] + (16,), F)
    for i in range(n):
        ss = _fma(v[..., 16 * i:16 * i + 16], v[..., 16 * i:16 * i + 16], ss)
    return np.sqrt(_tree(ss)).astype(F)


def _sgd(w, g, lr):
    return (w - (F(lr) * g).astype(F)).astype(F)


def emulate_taskres(shape, alpha=ALPHA, s=S, lr=1.0, adam_lr=ADAM_LR, corrupt=None):
    """{rows, loss, dr, r_sgd, r_adam} of one clipmi_taskres_train_step, fp32 numpy in the kernels' order."""
    c = taskres_case(shape)
    f, base, r, y = c["f"], c["base"], c["r"], c["y"]
    B, E = f.shape
    C = base.shape[0]
    al, sc = F(alpha), F(s)
    t = (base + (al * r).astype(F)).astype(F)
    nf, nt = _norm16(f), _norm16(t, corrupt == "norm_E_minus_1")
    acc = np.zeros((B, C), F)
    for e in range(E):
        acc = _fma(f[:, e:e + 1], t[None, :, e], acc)
    z = (sc * ((acc / nf[:, None]).astype(F) / nt[None, :]).astype(F)).astype(F)
    if corrupt == "tile_last_column":
        z[:, C - 1] = 0
    dz, rows = head_ref._xent(z, y, F(1) / F(B))
    span = ceil_div(B, 4)
    parts = []
    for p in range(4):
        sp = np.zeros(C, F)
        for b in range(p * span, min(p * span + span, B)):
            sp = _fma(dz[b], z[b], sp)
        parts.append(sp)
    q = ((parts[0] + parts[1]) + parts[2]).astype(F)
    if corrupt != "q_fourth_range":
        q = (q + parts[3]).astype(F)
    x = (f / nf[:, None]).astype(F)
    acc2 = np.zeros((C, E), F)
    for b in range(B - 1 if corrupt == "skip_last_batch_row" else B):
        acc2 = _fma(dz[b][:, None], x[b][None, :], acc2)
    u = (t / nt[:, None]).astype(F)
    du = (sc * acc2).astype(F)
    g = ((du - (u * q[:, None]).astype(F)).astype(F) / nt[:, None]).astype(F)
    if corrupt != "alpha_missing":
        g = (al * g).astype(F)
    b1, b2 = ADAM["betas"]
    m1 = (g * F(1.0 - b1)).astype(F)
    v1 = ((F(1.0 - b2) * g).astype(F) * g).astype(F)
    step = F(adam_lr / (1.0 - b1))
    denom = ((np.sqrt(v1).astype(F) / F(math.sqrt(1.0 - b2))).astype(F) + F(ADAM["eps"])).astype(F)
    r_adam = (r - ((step * m1).astype(F) / denom).astype(F)).astype(F)
    return {"rows": torch.from_numpy(rows), "loss": torch.tensor([_mean_f64(rows, corrupt)]).float(), "dr": torch.from_numpy(g),
            "r_sgd": torch.from_numpy(_sgd(r, g, lr)), "r_adam": torch.from_numpy(r_adam)}


# -------------------------------------------------------------------------------------------------------------------- CLIP-Adapter
def columns_split(depth, cols):
    """(parts, span) as columns_sum computes them."""
    parts = 1024 // cols if cols < 1024 else 1
    return parts, ceil_div(depth, parts)


def _columns_bound(mat, coef, tcoef):
    """(out, tout) of out[b, j] = sum_k coef[b, k] mat[k, j]."""
    parts, span = columns_split(*mat.shape)
    return coef @ mat, tcoef @ mat.abs() + (span + parts - 1) * U * (coef.abs() @ mat.abs())


@functools.lru_cache(maxsize=None)
def adapter_bound(shape, ratio_=RATIO, s=S, lr=1.0):
    """{name: (want, tol)}: rows [B], loss [1], dw1 [H, E], dw2 [E, H], w1, w2 (after one SGD step at ``lr``), and "kinks": the (name, row,
    unit) list of the pre-activations within their own bound of zero, in adapterfit_ref.kinks' format."""
    c = adapter_case(shape)
    f, T, w1, w2, y = _t64(c["f"]), _t64(c["T"]), _t64(c["w1"]), _t64(c["w2"]), torch.from_numpy(np.array(c["y"]))
    B, E = f.shape
    H, C = w1.shape[0], T.shape[0]
    kE, kH = (ceil_div(E, 64) + 6) * U, (ceil_div(H, 64) + 6) * U
    p1 = f @ w1.t()
    tp1 = kE * (f.abs() @ w1.abs().t())
    h = p1.clamp(min=0)
    p2 = h @ w2.t()
    th = tp1 * (p1 > -tp1)                 # h is 0 on both sides where p1 < -tp1
    tp2 = th @ w2.abs().t() + kH * (h @ w2.abs().t())
    a = p2.clamp(min=0)
    ta = tp2 * (p2 > -tp2)
    om = float(np.float32(1.0) - np.float32(ratio_))
    g = ratio_ * a + (1 - ratio_) * f
    tg = ratio_ * ta + U * (ratio_ * a).abs() + 2 * U * (om * f).abs() + U * g.abs()
    n = g.norm(dim=1, keepdim=True)
    en = (kE + 2 * (g.abs() * tg).sum(1, keepdim=True) / n ** 2) / 2 + U
    u = g / n
    tu = tg / n + (en + U) * u.abs()
    z = s * (u @ T.t())
    tz = abs(s) * (tu @ T.abs().t() + kE * (u.abs() @ T.abs().t())) + U * z.abs()
    _, _, dz, tdz, rows, trows = head_ref._softmax_bound(z, tz, y, 1.0 / B, C, nsum=ceil_div(C, 1024) + 21)
    loss, tloss = head_ref._mean_bound(rows, trows)
    raw, traw = _columns_bound(T, dz, tdz)
    du = s * raw
    tdu = abs(s) * traw + U * du.abs()
    dot = (u * du).sum(1, keepdim=True)
    tdot = (tu * du.abs() + u.abs() * tdu).sum(1, keepdim=True) + kE * (u * du).abs().sum(1, keepdim=True)
    inner = du - u * dot
    dg = inner / n
    tdg = (tdu + tu * dot.abs() + u.abs() * tdot + U * (u * dot).abs() + U * inner.abs()) / n + (en + U) * dg.abs()
    on2, kink2 = (p2 > 0).double(), p2.abs() <= tp2
    full = ratio_ * dg
    da = full * on2
    tda = (ratio_ * tdg + U * da.abs()) * on2
    raw, traw = _columns_bound(w2, da, tda)
    on1, kink1 = (p1 > 0).double(), p1.abs() <= tp1
    dh, tdh = raw * on1, traw * on1
    dw2 = da.t() @ h
    tdw2 = tda.t() @ h + da.abs().t() @ th + B * U * (da.abs().t() @ h)
    dw1 = dh.t() @ f
    tdw1 = tdh.t() @ f.abs() + B * U * (dh.abs().t() @ f.abs())
    kink = [("p1", int(b), int(k)) for b, k in torch.nonzero(kink1)] + [("p2", int(b), int(k)) for b, k in torch.nonzero(kink2)]
    return {"rows": (rows, trows), "loss": (loss.reshape(1), tloss.reshape(1)), "dw1": (dw1, tdw1), "dw2": (dw2, tdw2),
            "w1": _sgd_bound(w1, dw1, tdw1, lr), "w2": _sgd_bound(w2, dw2, tdw2, lr), "kinks": kink}


def adapter_masks(shape):
    """(keep dW1 [H, E], keep dW2 [E, H]): adapterfit_ref.excluded on the float64 reference's pre-activations within their own bound of zero."""
    _, E, H, _ = shape
    x1, x2 = adapterfit_ref.excluded(adapter_bound(shape)["kinks"], E, H)
    return torch.from_numpy(~x1), torch.from_numpy(~x2)


def masked(bound, keep):
    """(want, tol) with the tolerance infinite where ``keep`` is False: those entries are not compared."""
    want, tol = bound
    return want, torch.where(keep, tol, torch.full_like(tol, float("inf")))


def adapter_formulas(shape, ratio_=RATIO, s=S):
    c = adapter_case(shape)
    b = adapterfit_ref.backward(c, ratio_, s)
    return {"rows": _t64(b["row_loss"]), "loss": _t64(b["row_loss"].mean()).reshape(1), "dw1": _t64(b["dw1"]), "dw2": _t64(b["dw2"]),
            "w1": _t64(np.asarray(c["w1"], np.float64) - b["dw1"]), "w2": _t64(np.asarray(c["w2"], np.float64) - b["dw2"])}


ADAPTER_CORRUPTIONS = ("columns_du_last_short", "columns_dh_last_short", "mean_first_256", "norm_E_minus_1", "class_wave_15_dropped", "skip_last_batch_row")


def _columns_sum(mat, coef, corrupt=None):
    depth, cols = mat.shape
    parts, span = columns_split(depth, cols)
    out = None
    for p in range(parts):
        k1 = min(p * span + span, depth)
        if corrupt == "last_short" and k1 == depth:
            k1 -= 1
        sp = np.zeros((coef.shape[0], cols), F)
        for k in range(p * span, k1):
            sp = _fma(coef[:, k:k + 1], mat[k][None, :], sp)
        out = sp if out is None else (out + sp).astype(F)
    return out


def _lane_sum_products(a, b):
    """sum_e fl(a_e b_e), lane-strided and the tree: the kernel body's own sums, compiled with contraction off."""
    E = a.shape[-1]
    n = ceil_div(E, 64)
    prod = np.pad((a * b).astype(F), [(0, 0)] * (a.ndim - 1) + [(0, n * 64 - E)])
    sp = np.zeros(a.shape[:-1] + (64,), F)
    for i in range(n):
        sp = (sp + prod[..., 64 * i:64 * i + 64]).astype(F)
    return _tree(sp)


def _xent1024(z, labels, k, corrupt=None):
    """xent_row<16>: S thread-strided over 1024 threads, sixteen wave trees added in ascending order."""
    R, C = z.shape
    ar = np.arange(R)
    m = z.max(axis=1, keepdims=True)
    e = _expf((z - m).astype(F))
    n = ceil_div(C, 1024)
    es = np.pad(e, [(0, 0), (0, n * 1024 - C)])
    if corrupt == "class_wave_15_dropped":
        es[:, 15 * 64:16 * 64] = 0
    sp = np.zeros((R, 1024), F)
    for i in range(n):
        sp = (sp + es[:, 1024 * i:1024 * i + 1024]).astype(F)
    w = _tree(sp.reshape(R, 16, 64))
    S_ = w[:, 0]
    for i in range(1, 16):
        S_ = (S_ + w[:, i]).astype(F)
    loss = (np.log(S_).astype(F) - (z[ar, labels] - m[:, 0]).astype(F)).astype(F)
    p = (e / S_[:, None]).astype(F)
    p[ar, labels] = p[ar, labels] - F(1)
    return (p * k).astype(F), loss


def emulate_adapter(shape, ratio_=RATIO, s=S, lr=1.0, corrupt=None):
    """{rows, loss, dw1, dw2, w1, w2} of one clipmi_adapter_train_step, fp32 numpy in the kernels' order."""
    c = adapter_case(shape)
    f, T, w1, w2, y = c["f"], c["T"], c["w1"], c["w2"], c["y"]
    B, E = f.shape
    rt, sc = F(ratio_), F(s)
    h = np.maximum(_lane_dot(np.broadcast_to(w1[None], (B,) + w1.shape), f[:, None, :]), F(0))
    a = np.maximum(_lane_dot(np.broadcast_to(w2[None], (B,) + w2.shape), h[:, None, :]), F(0))
    g = ((rt * a).astype(F) + (F(F(1) - rt) * f).astype(F)).astype(F)
    gn = g[:, :-1] if corrupt == "norm_E_minus_1" else g
    n = np.sqrt(_lane_sum_products(gn, gn)).astype(F)[:, None]
    u = (g / n).astype(F)
    z = np.stack([(sc * _lane_dot(T, u[b][None, :])).astype(F) for b in range(B)])
    dz, rows = _xent1024(z, y, F(1) / F(B), corrupt)
    du = (sc * _columns_sum(T, dz, "last_short" if corrupt == "columns_du_last_short" else None)).astype(F)
    dot = _lane_sum_products(u, du)[:, None]
    dg = ((du - (u * dot).astype(F)).astype(F) / n).astype(F)
    da = np.where(a > 0, (rt * dg).astype(F), F(0)).astype(F)
    dh = np.where(h > 0, _columns_sum(w2, da, "last_short" if corrupt == "columns_dh_last_short" else None), F(0)).astype(F)
    dw2, dw1 = np.zeros(w2.shape, F), np.zeros(w1.shape, F)
    for b in range(B - 1 if corrupt == "skip_last_batch_row" else B):
        dw2 = _fma(da[b][:, None], h[b][None, :], dw2)
        dw1 = _fma(dh[b][:, None], f[b][None, :], dw1)
    return {"rows": torch.from_numpy(rows), "loss": torch.tensor([_mean_f64(rows, corrupt)]).float(), "dw1": torch.from_numpy(dw1),
            "dw2": torch.from_numpy(dw2), "w1": torch.from_numpy(_sgd(w1, dw1, lr)), "w2": torch.from_numpy(_sgd(w2, dw2, lr))}


# --------------------------------------------------------------------------------------------------------------------- TempScaling
@functools.lru_cache(maxsize=None)
def tempscale_bound(shape, theta=THETA, lr=TEMP_LR, rows=None):
    """{name: (want, tol)}: pair [2] = (mean loss, mean d theta) of the batch (the first ``rows`` samples, or all), theta [1] after one SGD step."""
    c = tempscale_case(shape)
    cc, y = (c["c"], c["y"]) if rows is None else (c["c"][:rows], c["y"][:rows])
    loss, grad = tempscale_ref.batch_loss_grad(cc, y, theta)
    tl, tg = tempscale_ref.batch_error_bound(cc, y, theta)
    new, _ = tempscale_ref.sgd_step(theta, 0.0, 0, grad, lr)
    return {"pair": (torch.tensor([loss, grad], dtype=torch.float64), torch.tensor([tl, tg], dtype=torch.float64)),
            "theta": (torch.tensor([new], dtype=torch.float64), torch.tensor([lr * tg + U * abs(lr * grad) + U * abs(new)], dtype=torch.float64))}


TEMPSCALE_CORRUPTIONS = ("mean_first_256", "lane_second_term_dropped", "label_term_unscaled")


def emulate_tempscale(shape, theta=THETA, lr=TEMP_LR, corrupt=None):
    """{pair, theta} of clipmi_tempscale_batch and one step of clipmi_tempscale_fit, fp32 numpy in the kernels' order."""
    k = tempscale_case(shape)
    c, y = k["c"], k["y"]
    n, C = c.shape
    ar = np.arange(n)
    s = np.exp(F(theta)).astype(F)
    zz = (s * c).astype(F)
    m = zz.max(axis=1, keepdims=True)
    e = _expf((zz - m).astype(F))
    ev = (e * c).astype(F)
    nC = ceil_div(C, 64)
    pe, pv = (np.pad(v, [(0, 0), (0, nC * 64 - C)]) for v in (e, ev))
    if corrupt == "lane_second_term_dropped" and nC > 1:
        pe[:, 64], pv[:, 64] = 0, 0
    Sp, Tp = np.zeros((n, 64), F), np.zeros((n, 64), F)
    for i in range(nC):
        Sp = (Sp + pe[:, 64 * i:64 * i + 64]).astype(F)
        Tp = (Tp + pv[:, 64 * i:64 * i + 64]).astype(F)
    S_, T_ = _tree(Sp), _tree(Tp)
    cy = c[ar, y]
    zy = cy if corrupt == "label_term_unscaled" else (s * cy).astype(F)
    loss = (np.log(S_).astype(F) - (zy - m[:, 0]).astype(F)).astype(F)
    grad = (s * ((T_ / S_).astype(F) - cy).astype(F)).astype(F)
    ml, mg = F(_mean_f64(loss, corrupt)), F(_mean_f64(grad, corrupt))
    new = F(F(theta) - F(F(lr) * mg))
    return {"pair": torch.tensor([ml, mg]), "theta": torch.tensor([new])}
