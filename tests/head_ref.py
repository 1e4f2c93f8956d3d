"""One float64 reference, one per-element bound and one fp32 emulation of the training loss heads (csrc/prompt_train.hip, csrc/train_rules.h,
csrc/cocoop_train.hip, csrc/proda_train.hip).  It does not import the package's kernels.

The float64 formulas are the existing restatements -- ``coopfit_ref.head``, ``vptfit_ref.head_image``, ``maplefit_ref.joint_head``,
``promptfit_ref.kgcoop_head`` / ``prograd_head``, ``promptsrcfit_ref.head``, ``cocoopfit_ref.head``, ``prodafit_ref.head`` -- called by the
``*_formulas`` functions; the bound functions evaluate the same
expressions once more, with the intermediate values the bound needs, and tests/test_head_ref_cpu.py holds the two equal.  What this file adds:

The bound (``coop_bound``, ``kgcoop_bound``, ``cocoop_bound``), u = 2^-24, derived from the kernels as written, one rounding point at a time.
Every term is evaluated on the float64 reference; nothing the device returns enters it.
  norm     s = sum_e row_e^2 is a lane-strided fmaf chain of n64 = ceil(E / 64) terms and the six-level wave tree over positive terms:
           relative error (n64 + 6) u.  sqrtf halves it and adds one rounding, 1.f / x one more:  en = (n64 + 6) / 2 + 2  units on 1 / |row|.
  dot      the same chain and tree on f_e t_e:  (n64 + 6) u sum_e |x_e u_e|  after both normalisations (A below, <= 1).
  logit    z = scale ((s inf) intx): three roundings and two reciprocal norms:  tz = scale ((n64 + 6) u A + (3 + 2 en) u |cos|).
  exp      __expf(x) is exp2 of the rounded product x log2(e): the argument carries 2 u |x| (the constant and the product), the instruction
           itself two units, z - m one more rounding u |x| and a slack of one:  ee = (3 |x| + 4) u RELATIVE to the exponential -- a few hundred
           units at scale 100, hence every probability is held relative to itself.  Results below 2^-126 are flushed: an absolute 2^-126.
  softmax  the sensitivities of p_c = e_c / S to a perturbation w_j = tz_j + ee_j of the exponents are exact to first order:
           |dp_c| <= p_c ((1 - p_c) w_c + sum_{j != c} p_j w_j); the second order, w^2 <= 1e-7 of that, is covered by the factor 1 + 1e-6.
           S is a thread-strided sum of nC = ceil(C / 256) terms, the wave tree and three adds over the waves, and p one division:
           (nC + 10) u p_c, which does NOT cancel at the label: p_y - 1 carries (nC + 10) u absolutely, then one rounding of the subtraction.
  dz       k = grad_scale / (float)B is one rounding, the product one more, the subtraction one:  tdz = k tp + 3 u |dz|.
  row loss logf(S) - (z_y - m): sum_j p_j w_j + tz_y for the exponents, (nC + 10) u for S, two units on |log S|, two on |z_y - m|, two flat.
  mean     float64, then one rounding to fp32:  mean of the row bounds + u |mean|.
  du       CoOp: the serial fmaf chain over b of dz[b, c] (f_be inf_b):  sum_b tdz[b, c] |x_be| + (en + 1 + B) u sum_b |dz[b, c] x_be|.
           VPT: the same over c with C in place of B.  CoCoOp: no sum, v = (scale dz) (f_e inf):  scale tdz |x_e| + (en + 3) u |v|.
  project  q = sum_e (t_e itn) (scale du_e): thread-strided chain of n256 = ceil(E / 256) terms, the tree, the waves (CoCoOp: n64 and the tree):
           tq = sum_e |u_e| tg_e + (en + 2 + nred) u sum_e |u_e g_e|,  g = scale du, tg = scale tdu + u |g|;
           d = (g - u q) itn:  td = itn (tg + |u_e| tq + (en + 3) u |u_e q| + u |g|) + (en + 3) u |d|.
  fp16     d_text16 is the rounding of the device's own d_text: an identity, no tolerance.
  KgCoOp   uo = u . o as q is formed, both operands normalised:  tuo = (2 en + 2 + n256 + 9) u sum_e |u_e o_e|;  score = 1 - float64 mean;
           the gradient's term fmaf(kg itn, fmaf(-u_e, uo, o_e), d), kg = -(grad_scale w / C) two roundings.

The emulation (``emulate_*``) is numpy fp32 in the kernels' own summation orders (lane- and thread-strided chains, the adjacent-pair wave
tree the DPP steps amount to, ascending waves, serial b and c, float64 strided partials and the LDS tree for the mean).  fmaf is evaluated
in float64 and rounded once more; __expf is exp2 of the fp32 product.  ``corrupt`` seeds one defect (CORRUPTIONS).  tests/test_head_ref_cpu.py
holds the emulation to the bound and shows every corruption leaving it.

ProGrad's and PromptSRC's second softmax (``prograd_bound``, ``promptsrc_bound``).  Further rounding points, derived as above:
  temperature   x = (z - m) inv_t: the subtraction, inv_t = 1 / T and the product, then __expf's two on the argument:  w = tz / T + (5 |x| + 4) u.
  log-prob      a_c = log S - x_c (= -log p_c):  (W + tz_c / T)(1 + 1e-6) + 3 u |x_c| + (nC + 10) u + 2 u |log S| + 2 u + u |a_c|.
  dz_kl         (ps - pt) kt, kt = k T:  kt (tps + tpt) + 4 u |dz_kl|.
  kl row        T^2 sum_c pt_c a_c, thread-strided and the trees:  T^2 [sum_c (tpt_c a_c + pt_c ta_c) + (nC + 10) u sum_c pt_c a_c] + 2 u |row|.
  PromptSRC     kl row = sum_c pt_c (log pt_c - log ps_c): both log-prob bounds and one rounding per b_c; dz += (ps - pt) kk, kk five roundings.
  L1            d_e = u_e - o_e, both normalised:  td_e = (en + 1) u (|u_e| + |o_e|) + u |d_e|;  row = sum |d_e| + (n256 + 9) u sum |d_e|.
                sign(d_e) is not continuous: where 0 < |d_e| <= td_e the device may see another sign, tsgn_e = 2 there and 0 elsewhere
                (d_e = 0 exactly only where a row equals its teacher bit for bit; both sides then go through the same instructions).
                qs = sum_e u_e sign(d_e):  sum_e |u_e| (tsgn_e + (en + 1) u) + (n256 + 10) u sum_e |u_e|.
                add_e = (k ia)(sign(d_e) - u_e qs):  |k ia| (tsgn_e + |u_e| tqs + (en + 2) u |u_e qs| + u |sign - u qs|) + (en + 5) u |add_e|,
                and one rounding of the sum with the joint head's gradient.

ProDA (``proda_bound``).  (csrc/proda_train.hip; the values are prodafit_ref.head's.)  Rounding points beyond the shared ones, u_{c,q} = text_{c Pb + q} intx, tu = (en + 1) u |u|:
  mean      m_c = (sum_q u_{c,q}) / Pb, serial:  tm = sum_q tu / Pb + (Pb + 1) u sum_q |u| / Pb;   v = u - m:  tv = tu + tm + u |v|
  logit     dot = sum_e x_e m_e (lane chain and tree):  sum_e ((en + 1) u |x m| + |x| tm) + (n64 + 6) u sum_e |x m|
            d = v_y - v_c:  td = tv_y + tv_c + u |d|;   sq = sum_q d^2:  sum_q (2 |d| td + td^2) + (Pb + 1) u sq;   x^2:  (2 en + 3) u x^2
            sig = sum_e x_e^2 sq_e:  sum_e ((2 en + 3) u x^2 sq + x^2 tsq) + (n64 + 7) u sig
            z = fmaf(0.5 s s, sig / (Pb + 1), s dot):  0.5 s^2 / (Pb + 1) (tsig + 2 u sig) + s (tdot + u |dot|) + u |z|
  dm        s sum_b dz[b, k] x_b as CoOp's du, one more rounding for the product with s
  dv        w = (0.5 s s dz) x^2:  tw = 0.5 s^2 (x^2 tdz + (2 en + 3) u |dz| x^2) + 3 u |w|;  every term w (v_k - v_other) carries tw |dd| + |w| tdd;
            the serial chain of class k has L_k = B + C #{b: y_b = k} terms: L_k u sum |terms|; two roundings for 2 / (Pb + 1)
  du        (dv - mean_q dv) + dm / Pb: the mean as m above, then three roundings
  project   as CoOp's, with g = du and the thread-strided reduction
  no-class  G_pq = n_p . n_q:  tG = (2 en + 3 + n64 + 6) u sum_e |n_p n_q|;  sign(G_pq) may differ where 0 < |G_pq| <= tG (allowance 2);
            dn = k sum_{q != p} sign(G_pq) n_q:  sum_q (tsgn + (en + 1) u) |n_q| + P u sum_q |n_q|, two roundings for k; then the projection
  losses    upper as CoOp's loss; m = float64 mean of |G_pq|: mean tG + u m; total = upper + alpha m in fp32: two more roundings
"""
import functools

import numpy as np
import torch

import cocoopfit_ref
import coopfit_ref
import maplefit_ref
import promptfit_ref
import vptfit_ref

U = 2.0 ** -24
FLOOR = 2.0 ** -126
F = np.float32
LOG2E = F(1.4426950408889634)


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------------------- cases
# (B, C, E, strided, scale, labels or None): the smallest shapes at which a loop takes another trip (C, E, B across 64 / 256 / 257), a role
# boundary of the norm kernel falls inside a workgroup (B % 4 != 0, (B + C) % 4 != 0), the E = 768 / 1024 gradient kernels, and the
# 397 .. 1000-class sizes; scale 100 is the peaked, real setting, scale 1 the unsaturated one; a third of them with ld > E
SHARED_CASES = [
    (1, 2, 1, False, 100.0, None),
    (3, 3, 63, True, 1.0, None),
    (4, 63, 64, False, 100.0, None),
    (5, 64, 65, True, 100.0, None),
    (5, 65, 255, False, 1.0, None),
    (3, 255, 256, True, 100.0, None),
    (4, 256, 257, False, 100.0, None),
    (5, 257, 64, False, 100.0, (255, 256, 256, 0, 128)),
    (3, 257, 768, True, 1.0, (255, 256, 1)),
    (257, 3, 64, False, 100.0, None),
    (256, 2, 63, True, 1.0, None),
    (255, 5, 65, False, 100.0, None),
    (4, 1000, 512, False, 100.0, None),
    (33, 1000, 512, True, 100.0, None),
    (33, 511, 128, False, 1.0, None),
    (5, 513, 1024, True, 100.0, None),
    (1, 257, 256, False, 1.0, (256,)),
    (33, 37, 512, False, 100.0, None),
    (3, 2, 1024, False, 100.0, None),
    (4, 4, 512, False, 1.0, None),
]
# CoCoOp has B C text rows: B <= 5 at C >= 257
COCOOP_CASES = [
    (1, 2, 1, False, 100.0, None),
    (3, 3, 63, True, 1.0, None),
    (4, 64, 64, False, 100.0, None),
    (5, 257, 65, False, 100.0, (255, 256, 256, 0, 128)),
    (3, 65, 256, True, 100.0, None),
    (4, 255, 257, False, 1.0, None),
    (2, 513, 128, False, 100.0, None),
    (257, 3, 64, False, 100.0, None),
    (2, 1000, 512, True, 100.0, None),
    (5, 63, 1024, True, 1.0, None),
    (33, 5, 768, False, 100.0, None),
]
# two input regimes per shape: scale 100 (peaked, the real setting) and scale 1 (unsaturated: the low-probability classes carry weight)
SHARED_CASES = [c[:4] + (s, c[5]) for c in SHARED_CASES for s in (100.0, 1.0)]
COCOOP_CASES = [c[:4] + (s, c[5]) for c in COCOOP_CASES for s in (100.0, 1.0)]
KG_W = (0.0, 8.0)


@functools.lru_cache(maxsize=None)
def inputs(case, per_image=False):
    """dict of fp32 CPU tensors: feats [B, ld] (the head reads [:, :E]; the columns behind are NaN), text [C, E] or, per_image, [B C, E],
    teacher [C, E] (not normalised: its norms differ from the student's), labels int64 [B]."""
    B, C, E, strided, scale, labels = case
    g = torch.Generator().manual_seed(7000 + 131 * B + 17 * C + E)
    ld = E + 3 if strided else E
    feats = torch.full((B, ld), float("nan"))
    feats[:, :E] = torch.randn(B, E, generator=g) * 2.0
    rows = B * C if per_image else C
    text = torch.randn(rows, E, generator=g) * (0.5 + torch.rand(rows, 1, generator=g))
    teacher = (text[:C] + 0.5 * torch.randn(C, E, generator=g)) * (0.5 + 2.0 * torch.rand(C, 1, generator=g))
    if labels is None:
        y = torch.randint(0, C, (B,), generator=g)
        y[0], y[-1] = C - 1, 0 if B > 1 else C - 1
    else:
        y = torch.tensor(labels)
    return {"feats": feats, "ld": ld, "text": text, "teacher": teacher, "labels": y, "B": B, "C": C, "E": E, "scale": scale}


# ----------------------------------------------------------------------------------------------------------------------- the bound
def _unit(t):
    n = t.norm(dim=-1, keepdim=True)
    return t / n, 1.0 / n


def _en(E):
    return (ceil_div(E, 64) + 6) / 2 + 2


def _softmax_bound(z, tz, labels, k, C, nsum=None):
    """(p, tp, dz, tdz, rows, trows) of the cross-entropy rows of float64 logits z [R, C] with the bound tz on them; k = grad_scale / B.
    ``nsum``: the roundings of S's sum where it is not xent_row's over 256 threads and four waves (nC + 10)."""
    R = z.shape[0]
    ar = torch.arange(R)
    m = z.max(dim=-1, keepdim=True).values
    x = z - m
    p = torch.softmax(z, dim=-1)
    w = tz + (3 * x.abs() + 4) * U
    W = (p * w).sum(-1, keepdim=True)
    ns = ceil_div(C, 256) + 10 if nsum is None else nsum
    tp = (1 + 1e-6) * p * ((1 - p).clamp(min=0) * w + (W - p * w).clamp(min=0)) + ns * U * p + FLOOR
    dz = p.clone()
    dz[ar, labels] -= 1.0
    tdz = abs(k) * tp + 3 * U * (dz * k).abs()
    tdz[ar, labels] += abs(k) * U * (dz[ar, labels]).abs()
    lse = torch.logsumexp(z, dim=-1)
    rows = lse - z[ar, labels]
    log_s = lse - m[:, 0]
    trows = (1 + 1e-6) * (W[:, 0] + tz[ar, labels]) + ns * U + 2 * U * log_s.abs() + 2 * U * x[ar, labels].abs() + 2 * U
    return p, tp, dz * k, tdz, rows, trows


def _project_bound(g, tg, u, itn, en, nred):
    """(d, td) of d = (g - u (u . g)) itn for the float64 g with the bound tg; u the unit rows, itn [R, 1] their reciprocal norms."""
    q = (u * g).sum(-1, keepdim=True)
    tq = (u.abs() * tg).sum(-1, keepdim=True) + (en + 2 + nred) * U * (u * g).abs().sum(-1, keepdim=True)
    d = (g - u * q) * itn
    td = itn * (tg + u.abs() * tq + (en + 3) * U * (u * q).abs() + U * g.abs()) + (en + 3) * U * d.abs()
    return d, td


def _logit_bound(x, u, scale, E):
    n64, en = ceil_div(E, 64), _en(E)
    z = scale * x @ u.t()
    return z, abs(scale) * ((n64 + 6) * U * (x.abs() @ u.abs().t()) + (3 + 2 * en) * U * (x @ u.t()).abs())


def _mean_bound(rows, trows):
    mean = rows.mean()
    return mean, trows.mean() + U * mean.abs()


def coop_bound(inp, grad_scale=1.0):
    """{name: (want float64, tol)} of CoOp's, VPT's and MaPLe's outputs: loss [1], d_text [C, E], d_feats [B, E].  The float64 values are
    checked against coopfit_ref.head / vptfit_ref.head_image / maplefit_ref.joint_head in tests/test_head_ref_cpu.py."""
    B, C, E, scale = inp["B"], inp["C"], inp["E"], inp["scale"]
    f, t, y = inp["feats"][:, :E].double(), inp["text"].double(), inp["labels"]
    x, inf = _unit(f)
    u, itn = _unit(t)
    en = _en(E)
    z, tz = _logit_bound(x, u, scale, E)
    k = grad_scale / B
    _, _, dz, tdz, rows, trows = _softmax_bound(z, tz, y, k, C)
    loss, tloss = _mean_bound(rows, trows)
    nred = ceil_div(E, 256) + 9
    du = dz.t() @ x
    tdu = tdz.t() @ x.abs() + (en + 1 + B) * U * (dz.abs().t() @ x.abs())
    g = scale * du
    d_text, td_text = _project_bound(g, abs(scale) * tdu + U * g.abs(), u, itn, en, nred)
    dx = dz @ u
    tdx = tdz @ u.abs() + (en + 1 + C) * U * (dz.abs() @ u.abs())
    g = scale * dx
    d_feats, td_feats = _project_bound(g, abs(scale) * tdx + U * g.abs(), x, inf, en, nred)
    return {"loss": (loss.reshape(1), tloss.reshape(1)), "d_text": (d_text, td_text), "d_feats": (d_feats, td_feats)}


def kgcoop_bound(inp, w, grad_scale=1.0):
    """{name: (want, tol)} of KgCoOp's outputs: losses [3] = total, ce, score; d_text [C, E] (promptfit_ref.kgcoop_head's formulas)."""
    B, C, E = inp["B"], inp["C"], inp["E"]
    base = coop_bound(inp, grad_scale)
    u, itn = _unit(inp["text"].double())
    o, _ = _unit(inp["teacher"].double())
    en, n256 = _en(E), ceil_div(E, 256)
    uo = (u * o).sum(-1, keepdim=True)
    tuo = (2 * en + 2 + n256 + 9) * U * (u * o).abs().sum(-1, keepdim=True)
    score = 1.0 - uo.mean()
    tscore = tuo.mean() + U * score.abs()
    ce, tce = base["loss"]
    total = ce + w * score
    ttotal = tce + w * tscore + U * ((w * score).abs() + total.abs())
    kg = -(grad_scale * w / C)
    inner = o - u * uo
    tinner = (en + 1) * U * o.abs() + u.abs() * tuo + (en + 2) * U * (u * uo).abs() + U * inner.abs()
    add = kg * itn * inner
    d, td = base["d_text"]
    d_kg = d + add
    td_kg = td + abs(kg) * itn * tinner + (en + 5) * U * add.abs() + U * d_kg.abs()
    return {"losses": (torch.stack([total.reshape(()), ce.reshape(()), score]), torch.stack([ttotal.reshape(()), tce.reshape(()), tscore])),
            "d_text": (d_kg, td_kg)}


def cocoop_bound(inp, grad_scale=1.0):
    """{name: (want, tol)} of CoCoOp's outputs: loss [1], row_losses [B], d_text [B C, E] (cocoopfit_ref.head's formulas)."""
    B, C, E, scale = inp["B"], inp["C"], inp["E"], inp["scale"]
    f, t, y = inp["feats"][:, :E].double(), inp["text"].double().reshape(B, C, E), inp["labels"]
    x, _ = _unit(f)
    u, itn = _unit(t)
    n64, en = ceil_div(E, 64), _en(E)
    cos = (x[:, None] * u).sum(-1)
    z = scale * cos
    tz = abs(scale) * ((n64 + 6) * U * (x[:, None].abs() * u.abs()).sum(-1) + (3 + 2 * en) * U * cos.abs())
    _, _, dz, tdz, rows, trows = _softmax_bound(z, tz, y, grad_scale / B, C)
    loss, tloss = _mean_bound(rows, trows)
    v = scale * dz[:, :, None] * x[:, None]
    tv = (abs(scale) * tdz + U * (scale * dz).abs())[:, :, None] * x[:, None].abs() + (en + 3) * U * v.abs()
    d, td = _project_bound(v, tv, u, itn, en, n64 + 6)
    return {"loss": (loss.reshape(1), tloss.reshape(1)), "row_losses": (rows, trows), "d_text": (d.reshape(B * C, E), td.reshape(B * C, E))}


def ratio(got, want, tol):
    """max |got - want| / tol (inf for a NaN)."""
    diff = (torch.as_tensor(got).double().reshape(want.shape) - want).abs()
    r = diff / tol
    r[torch.isnan(r)] = float("inf")
    r[diff == 0] = 0.0
    return float(r.max())


# -------------------------------------------------------------------------------------------------------------------- the emulation
CORRUPTIONS = ("drop_class_256", "double_class_256", "max_first_256", "label_mod_256", "skip_last_batch_row", "mean_first_256", "k_over_C",
               "norm_role_off_by_one", "teacher_norms", "q_single_wave", "prograd_T2_dropped", "src_sign0_plus")


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _tree(v):
    """The wave tree over the last axis of 64 lanes: xor 1, xor 2, the two mirrors, the row and the half swaps = adjacent pairs, six times."""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _lane_dot(a, b, lanes=64):
    """sum_e a_e b_e over the last axis as `lanes` strided fmaf chains and the wave tree (lanes = 64) or the workgroup's (lanes = 256: four
    wave trees added in ascending order).  Idle lanes hold 0."""
    E = a.shape[-1]
    n = ceil_div(E, lanes)
    pad = [(0, 0)] * (a.ndim - 1) + [(0, n * lanes - E)]
    a, b = np.pad(a, pad), np.pad(np.broadcast_to(b, a.shape), pad)
    s = np.zeros(a.shape[:-1] + (lanes,), F)
    for i in range(n):
        s = _fma(a[..., i * lanes:(i + 1) * lanes], b[..., i * lanes:(i + 1) * lanes], s)
    return _block(s) if lanes == 256 else _tree(s)


def _block(s, single_wave=False):
    w = _tree(s.reshape(s.shape[:-1] + (4, 64)))
    if single_wave:
        return w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _strided_sum(v, op=np.add, init=0.0):
    """Thread-strided partials over the last axis (thread t takes t, t + 256, ..), returned per thread [.., 256]."""
    C = v.shape[-1]
    n = ceil_div(C, 256)
    v = np.pad(v, [(0, 0)] * (v.ndim - 1) + [(0, n * 256 - C)], constant_values=init)
    s = np.full(v.shape[:-1] + (256,), init, F)
    for i in range(n):
        s = op(s, v[..., i * 256:(i + 1) * 256]).astype(F)
    return s


def _block_max(s):
    return s.max(axis=-1)


def _expf(x):
    return np.exp2((x.astype(F) * LOG2E).astype(F)).astype(F)


def _inv_norm(rows):
    return (F(1) / np.sqrt(_lane_dot(rows, rows))).astype(F)


def _mean_f64(rows, corrupt=None):
    n = rows.shape[0]
    part = np.zeros(256, np.float64)
    for i in range(0, n, 256):
        if corrupt == "mean_first_256" and i >= 256:
            break
        chunk = rows[i:i + 256].astype(np.float64)
        part[:chunk.shape[0]] += chunk
    h = 128
    while h:
        part[:h] += part[h:2 * h]
        h //= 2
    return part[0] / n


def _xent(z, labels, k, corrupt=None):
    """(dz [R, C], row losses [R]) as coop_head_softmax_kernel and xent_row form them."""
    R, C = z.shape
    ar = np.arange(R)
    zm = z[:, :256] if corrupt == "max_first_256" else z
    m = _block_max(_strided_sum(zm, np.maximum, -np.inf))[:, None]
    e = _expf(z - m)
    es = e.copy()
    if corrupt == "drop_class_256" and C > 256:
        es[:, 256] = 0
    if corrupt == "double_class_256" and C > 256:
        es[:, 256] *= 2
    S = _block(_strided_sum(es))
    loss = (np.log(S).astype(F) - (z[ar, labels] - m[:, 0])).astype(F)
    p = (e / S[:, None]).astype(F)
    hot = labels % 256 if corrupt == "label_mod_256" else labels
    p[ar, hot] = p[ar, hot] - F(1)
    return (p * k).astype(F), loss


def _np(t):
    return t.numpy().astype(F)


def _norms(inp, teacher=None, corrupt=None):
    E = inp["E"]
    f, t = _np(inp["feats"][:, :E]), _np(inp["text"])
    inf, intx = _inv_norm(f), _inv_norm(t)
    if corrupt == "norm_role_off_by_one":
        intx = intx.copy()
        intx[0] = inf[-1]
    return f, t, inf, intx


def _logits(f, t, inf, intx, scale):
    z = np.empty((f.shape[0], t.shape[0]), F)
    for b in range(f.shape[0]):
        z[b] = F(scale) * ((_lane_dot(t, f[b][None, :]) * inf[b]) * intx)
    return z


def _coop_grad(f, t, inf, intx, dz, scale, corrupt=None):
    """(d_text, scale du, q) of coop_head_grad_kernel."""
    B = f.shape[0]
    du = np.zeros(t.shape, F)
    for b in range(B - 1 if corrupt == "skip_last_batch_row" else B):
        du = _fma(dz[b][:, None], (f[b] * inf[b]).astype(F)[None, :], du)
    u = (t * intx[:, None]).astype(F)
    g = (F(scale) * du).astype(F)
    E = t.shape[1]
    n = ceil_div(E, 256)
    pu, pg = np.pad(u, [(0, 0), (0, n * 256 - E)]), np.pad(g, [(0, 0), (0, n * 256 - E)])
    s = np.zeros((t.shape[0], 256), F)
    for i in range(n):
        s = _fma(pu[:, i * 256:(i + 1) * 256], pg[:, i * 256:(i + 1) * 256], s)
    q = _block(s, single_wave=corrupt == "q_single_wave")[:, None]
    return ((g - (u * q).astype(F)).astype(F) * intx[:, None]).astype(F)


def emulate_coop(inp, grad_scale=1.0, corrupt=None):
    """{loss, d_text, d_feats} of clipmi_maple_head (= clipmi_coop_head's and clipmi_vpt_head's) in the kernels' order, fp32 numpy."""
    B, C, scale = inp["B"], inp["C"], inp["scale"]
    f, t, inf, intx = _norms(inp, corrupt=corrupt)
    z = _logits(f, t, inf, intx, scale)
    k = F(grad_scale) / F(C if corrupt == "k_over_C" else B)
    dz, rows = _xent(z, inp["labels"].numpy(), k, corrupt)
    d_text = _coop_grad(f, t, inf, intx, dz, scale, corrupt)
    d_feats = _coop_grad(t, f, intx, inf, dz.T.copy(), scale, "q_single_wave" if corrupt == "q_single_wave" else None)   # VPT: the two sides exchanged
    return {"loss": torch.tensor([_mean_f64(rows, corrupt)]).float(), "d_text": torch.from_numpy(d_text), "d_feats": torch.from_numpy(d_feats),
            "rows": torch.from_numpy(rows)}


def emulate_kgcoop(inp, w, grad_scale=1.0, corrupt=None):
    """{losses [3], d_text} of clipmi_prompt_head, mode 1."""
    B, C, E, scale = inp["B"], inp["C"], inp["E"], inp["scale"]
    f, t, inf, intx = _norms(inp, corrupt=corrupt)
    o = _np(inp["teacher"])
    inty = _inv_norm(o)
    z = _logits(f, t, inf, inty if corrupt == "teacher_norms" else intx, scale)
    dz, rows = _xent(z, inp["labels"].numpy(), F(grad_scale) / F(B), corrupt)
    d = _coop_grad(f, t, inf, intx, dz, scale, corrupt)
    u, on = (t * intx[:, None]).astype(F), (o * inty[:, None]).astype(F)
    uo = _lane_dot(u, on, 256)[:, None]
    kg = -(F(grad_scale) * F(w) / F(C))
    d = _fma((kg * intx)[:, None], _fma(-u, uo, on), d)
    ce = F(_mean_f64(rows, corrupt))
    score = F(1.0 - _mean_f64(uo[:, 0]))
    total = F(ce + F(F(w) * score))
    return {"losses": torch.tensor([total, ce, score]), "d_text": torch.from_numpy(d)}


def emulate_cocoop(inp, grad_scale=1.0, corrupt=None):
    """{loss, row_losses, d_text} of clipmi_cocoop_head."""
    B, C, E, scale = inp["B"], inp["C"], inp["E"], inp["scale"]
    f, t = _np(inp["feats"][:, :E]), _np(inp["text"]).reshape(B, C, E)
    inf, intx = _inv_norm(f), _inv_norm(t)
    z = (F(scale) * ((_lane_dot(t, f[:, None, :]) * inf[:, None]) * intx)).astype(F)
    dz, rows = _xent(z, inp["labels"].numpy(), F(grad_scale) / F(C if corrupt == "k_over_C" else B), corrupt)
    k = (F(scale) * dz).astype(F)[:, :, None]
    v = (k * (f * inf[:, None]).astype(F)[:, None, :]).astype(F)
    u = (t * intx[:, :, None]).astype(F)
    q = _lane_dot(u, v)[:, :, None]
    d = ((v - (u * q).astype(F)).astype(F) * intx[:, :, None]).astype(F)
    return {"loss": torch.tensor([_mean_f64(rows, corrupt)]).float(), "row_losses": torch.from_numpy(rows), "d_text": torch.from_numpy(d.reshape(B * C, E))}


# ------------------------------------------------------------------------------------------------------------ constructed inputs
def uniform_inputs(B, C, E, seed=0):
    """Every text (and teacher) row equal: every logit of a row has the same bits, exp(z - m) = 1, S = C exactly; row loss = logf(C)."""
    g = torch.Generator().manual_seed(8100 + seed)
    row = torch.randn(1, E, generator=g)
    return {"feats": torch.randn(B, E, generator=g), "ld": E, "text": row.repeat(C, 1), "teacher": torch.randn(1, E, generator=g).repeat(C, 1),
            "labels": torch.tensor([(255, 256, C - 1, 0, 64)[b % 5] % C for b in range(B)]), "B": B, "C": C, "E": E, "scale": 100.0}


AXIS_SCALE = 128.0      # a power of two; exp(-128) is below fp32's denormals: __expf returns 0, the sum counts the maximal classes alone


def axis_inputs(B, C, E, first=0):
    """Signed powers of two on single coordinates: image b on coordinate (first + b) % min(E, C), class c on coordinate c % E with the sign (-1)^(c // E).
    Norms, cosines and scale * cos are exact: z[b, c] = +-128 where the coordinates meet, else 0.  The row's maximum 128 is taken by the
    n_b classes c = b % E + 2 j E < C; the label alternates between a class on another coordinate (row loss logf(n_b) + 128, even b: row 256
    is one of them) and the first of the maximal ones (logf(n_b)).  Returns (inputs, the float64 mean of those row losses with numpy's fp32 log)."""
    assert E >= 2
    feats, text = torch.zeros(B, E), torch.zeros(C, E)
    labels = torch.zeros(B, dtype=torch.int64)
    rows = np.zeros(B, np.float64)
    for c in range(C):
        text[c, c % E] = (-1.0) ** (c // E) * 2.0 ** (c % 5 - 2)
    for b in range(B):
        j = (first + b) % min(E, C)
        feats[b, j] = 2.0 ** (b % 7 - 3)
        n = len(range(j, C, 2 * E))
        other = (j + 1) % min(E, C)
        labels[b] = other if b % 2 == 0 else j
        rows[b] = float(np.log(F(n)) if b % 2 else F(np.log(F(n)) + F(128.0)))
    return ({"feats": feats, "ld": E, "text": text, "teacher": text.clone(), "labels": labels, "B": B, "C": C, "E": E, "scale": AXIS_SCALE},
            F(rows.sum() / B), bool(all(len(range((first + b) % min(E, C), C, 2 * E)) == 1 for b in range(B))))


def exact_dz_inputs(B, C, E, scale=64.0):
    """Uniform rows whose gradients are known bit for bit whatever the compiler contracts: every text row is 2^-1 e_0, every image 2^b e_1.
    x = e_1, u = e_0 and z = 0 exactly, so p = fl(1 / C), dz[b, c] = p k or (p - 1) k with k = fl(1 / B); du_c = (sum_b dz[b, c]) e_1 in the
    kernel's serial fp32 order, q = u . du = 0, and with scale and |t| powers of two d_text[c] = scale 2 (sum_b dz[b, c]) e_1 exactly;
    likewise d_feats[b] = scale 2^-b (sum_c dz[b, c], c ascending) e_0.  Returns (inputs, d_text [C, E], d_feats [B, E], loss = logf(C))."""
    feats, text = torch.zeros(B, E), torch.zeros(C, E)
    text[:, 0] = 0.5
    feats[:, 1] = 2.0 ** torch.arange(B).remainder(4)
    labels = torch.tensor([(255, 256, C - 1, 0, 64)[b % 5] % C for b in range(B)])
    k, p = F(1) / F(B), F(1) / F(C)
    dz = np.full((B, C), p * k, F)
    dz[np.arange(B), labels.numpy()] = F(p - F(1)) * k
    d_text, d_feats = np.zeros((C, E), F), np.zeros((B, E), F)
    acc = np.zeros(C, F)
    for b in range(B):
        acc = (acc + dz[b]).astype(F)
    d_text[:, 1] = F(scale) * F(2) * acc
    acc = np.zeros(B, F)
    for c in range(C):
        acc = (acc + dz[:, c]).astype(F)
    d_feats[:, 0] = F(scale) * acc / feats[:, 1].numpy()
    inp = {"feats": feats, "ld": E, "text": text, "teacher": text.clone(), "labels": labels, "B": B, "C": C, "E": E, "scale": scale}
    return inp, torch.from_numpy(d_text), torch.from_numpy(d_feats), np.log(F(C))


EXACT_DZ_CASES = [(1, 257, 64), (3, 257, 2), (5, 1000, 512), (4, 513, 768), (257, 3, 64)]
UNIFORM_CASES = [(3, 257, 64), (2, 1000, 512), (5, 64, 65), (4, 513, 768)]
# the third has a row whose only maximal class is 256: a maximum over the first 256 classes alone overflows its exponential
AXIS_CASES = [(257, 3, 64, 0), (256, 65, 65, 0), (3, 257, 512, 255), (5, 257, 64, 0), (33, 1000, 512, 0)]


# ------------------------------------------------------------------------------------------------------- the float64 formulas
def formulas(inp, w=8.0):
    """The existing restatements on the same inputs, float64: what the bound functions' values must equal."""
    E = inp["E"]
    f, t, o, y, s = inp["feats"][:, :E].double(), inp["text"].double(), inp["teacher"].double(), inp["labels"], inp["scale"]
    loss, d_text, _ = coopfit_ref.head(f, y, t, s)
    _, d_feats, _ = vptfit_ref.head_image(f, y, t, s)
    jl, jf, jt = maplefit_ref.joint_head(f, y, t, s)
    total, ce, score, d_kg = promptfit_ref.kgcoop_head(f, y, t, o, s, w)
    return {"loss": loss, "d_text": d_text, "d_feats": d_feats, "joint": (jl, jf, jt), "kg_losses": torch.stack([total, ce, score]), "kg_d_text": d_kg}


def cocoop_formulas(inp):
    E = inp["E"]
    loss, d, rows, _ = cocoopfit_ref.head(inp["feats"][:, :E].double(), inp["labels"], inp["text"].double(), inp["scale"])
    return {"loss": loss, "d_text": d, "row_losses": rows}



# ------------------------------------------------------------------------------------------- ProGrad's and PromptSRC's second softmax
def _p_bound(z, tz, C, T=1.0, xr=3):
    m = z.max(dim=-1, keepdim=True).values
    x = (z - m) / T
    p = torch.softmax(z / T, dim=-1)
    w = tz / T + (xr * x.abs() + 4) * U
    W = (p * w).sum(-1, keepdim=True)
    nC = ceil_div(C, 256)
    tp = (1 + 1e-6) * p * ((1 - p).clamp(min=0) * w + (W - p * w).clamp(min=0)) + (nC + 10) * U * p + FLOOR
    a = torch.logsumexp(z / T, dim=-1, keepdim=True) - z / T
    log_s = torch.logsumexp(z / T, dim=-1, keepdim=True) - m / T
    ta = (1 + 1e-6) * (W + tz / T) + 3 * U * x.abs() + (nC + 10) * U + 2 * U * log_s.abs() + 2 * U + U * a.abs()
    return p, tp, a, ta


def _text_grad_bound(dz, tdz, x, u, itn, scale, E, B):
    en, nred = _en(E), ceil_div(E, 256) + 9
    du = dz.t() @ x
    tdu = tdz.t() @ x.abs() + (en + 1 + B) * U * (dz.abs().t() @ x.abs())
    g = scale * du
    return _project_bound(g, abs(scale) * tdu + U * g.abs(), u, itn, en, nred)


def prograd_bound(inp, T, grad_scale=1.0):
    """{losses [2] = xe, kl; d_text; d_text_kl}: (want, tol), the values promptfit_ref.prograd_head's."""
    B, C, E, scale = inp["B"], inp["C"], inp["E"], inp["scale"]
    base = coop_bound(inp, grad_scale)
    x, _ = _unit(inp["feats"][:, :E].double())
    u, itn = _unit(inp["text"].double())
    o, _ = _unit(inp["teacher"].double())
    z, tz = _logit_bound(x, u, scale, E)
    zt, tzt = _logit_bound(x, o, scale, E)
    ps, tps, a, ta = _p_bound(z, tz, C, T, 5)
    pt, tpt, _, _ = _p_bound(zt, tzt, C, T, 5)
    nC, kt = ceil_div(C, 256), grad_scale / B * T
    dzk = (ps - pt) * kt
    tdzk = abs(kt) * (tps + tpt) + 4 * U * dzk.abs()
    rows = T * T * (pt * a).sum(-1)
    trows = T * T * ((tpt * a + pt * ta).sum(-1) + (nC + 10) * U * (pt * a).sum(-1)) + 2 * U * rows.abs()
    kl, tkl = _mean_bound(rows, trows)
    d_kl, td_kl = _text_grad_bound(dzk, tdzk, x, u, itn, scale, E, B)
    xe, txe = base["loss"]
    return {"losses": (torch.stack([xe.reshape(()), kl]), torch.stack([txe.reshape(()), tkl])), "d_text": base["d_text"], "d_text_kl": (d_kl, td_kl)}


def _l1_bound(a, o, k, E):
    """(row sums, their bound, the gradient's addend, its bound) of one side of promptsrc_l1_kernel: a the raw rows, o the teacher's."""
    u, ia = _unit(a)
    on, _ = _unit(o)
    en, n256 = _en(E), ceil_div(E, 256)
    d = u - on
    td = (en + 1) * U * (u.abs() + on.abs()) + U * d.abs()
    rows = d.abs().sum(-1)
    trows = td.sum(-1) + (n256 + 9) * U * rows
    s = torch.sign(d)
    tsgn = 2.0 * ((d.abs() <= td) & (d != 0)).double()
    qs = (u * s).sum(-1, keepdim=True)
    tqs = (u.abs() * (tsgn + (en + 1) * U)).sum(-1, keepdim=True) + (n256 + 10) * U * u.abs().sum(-1, keepdim=True)
    inner = s - u * qs
    add = k * ia * inner
    tadd = abs(k) * ia * (tsgn + u.abs() * tqs + (en + 2) * U * (u * qs).abs() + U * inner.abs()) + (en + 5) * U * add.abs()
    return rows, trows, add, tadd


def promptsrc_bound(inp, weights, grad_scale=1.0):
    """{losses [5]; d_feats; d_text}: (want, tol), the values promptsrcfit_ref.head's."""
    B, C, E, scale = inp["B"], inp["C"], inp["E"], inp["scale"]
    wt, wi, wl = weights
    f, t, y = inp["feats"][:, :E].double(), inp["text"].double(), inp["labels"]
    zs, tea = inp["zs"].double(), inp["teacher"].double()
    x, inf = _unit(f)
    u, itn = _unit(t)
    yy, _ = _unit(zs)
    o, _ = _unit(tea)
    en, nC, nred = _en(E), ceil_div(C, 256), ceil_div(E, 256) + 9
    z, tz = _logit_bound(x, u, scale, E)
    _, _, dz, tdz, rows, trows = _softmax_bound(z, tz, y, grad_scale / B, C)
    ce, tce = _mean_bound(rows, trows)
    kl = tkl = torch.zeros((), dtype=torch.float64)
    if wl != 0:
        zz, tzz = _logit_bound(yy, o, scale, E)
        ps, tps, a, ta = _p_bound(z, tz, C)
        pt, tpt, at, tat = _p_bound(zz, tzz, C)
        kk = grad_scale * wl / (B * C)
        add = (ps - pt) * kk
        dz = dz + add
        tdz = tdz + abs(kk) * (tps + tpt) + 5 * U * add.abs() + U * dz.abs()
        b = a - at
        tb = ta + tat + U * b.abs()
        krow = (pt * b).sum(-1)
        tkrow = (tpt * b.abs() + pt * tb).sum(-1) + (nC + 10) * U * (pt * b.abs()).sum(-1)
        kl = krow.sum() / (B * C)
        tkl = tkrow.sum() / (B * C) + U * kl.abs()
    d_text, td_text = _text_grad_bound(dz, tdz, x, u, itn, scale, E, B)
    d_feats, td_feats = _text_grad_bound(dz.t(), tdz.t(), u, x, inf, scale, E, C)
    lt = tlt = li = tli = torch.zeros((), dtype=torch.float64)
    if wt != 0:
        r, tr, add, tadd = _l1_bound(t, tea, grad_scale * wt / (C * E), E)
        lt = r.sum() / (C * E)
        tlt = tr.sum() / (C * E) + U * lt.abs()
        d_text = d_text + add
        td_text = td_text + tadd + U * d_text.abs()
    if wi != 0:
        r, tr, add, tadd = _l1_bound(f, zs, grad_scale * wi / (B * E), E)
        li = r.sum() / (B * E)
        tli = tr.sum() / (B * E) + U * li.abs()
        d_feats = d_feats + add
        td_feats = td_feats + tadd + U * d_feats.abs()
    total = ce + wt * lt + wi * li + wl * kl
    ttotal = tce + wt * tlt + wi * tli + wl * tkl + U * total.abs()
    return {"losses": (torch.stack([total, ce, lt, li, kl]), torch.stack([ttotal, tce, tlt, tli, tkl])), "d_feats": (d_feats, td_feats),
            "d_text": (d_text, td_text)}


SRC_WEIGHTS = (25.0, 10.0, 25.0)               # promptsrc.py's TEXT / IMAGE / LOGIT loss weights
SRC_WEIGHT_SETS = (SRC_WEIGHTS, (25.0, 0.0, 25.0))
PROGRAD_T = (1.0, 2.0)


def src_inputs(inp, same=False):
    """``inp`` with the frozen image features zs [B, E]; text row 0 and feature row 0 EQUAL their teachers (sign(0) = 0 is exercised).
    ``same``: every row equals its teacher."""
    g = torch.Generator().manual_seed(9100 + inp["B"] + inp["C"])
    E = inp["E"]
    out = dict(inp)
    if same:
        out["zs"], out["teacher"] = inp["feats"][:, :E].clone(), inp["text"].clone()
        return out
    out["zs"] = inp["feats"][:, :E] + 0.3 * torch.randn(inp["B"], E, generator=g)
    out["zs"][0] = inp["feats"][0, :E]
    out["teacher"] = inp["teacher"].clone()
    out["teacher"][0] = inp["text"][0]
    return out


def _soft(z, inv_t=None):
    m = _block_max(_strided_sum(z, np.maximum, -np.inf))[:, None]
    x = (z - m).astype(F) if inv_t is None else ((z - m).astype(F) * F(inv_t)).astype(F)
    e = _expf(x)
    S = _block(_strided_sum(e))
    return x, e, S, (e / S[:, None]).astype(F)


def _row_sum(v):
    return _block(_strided_sum(v))


def emulate_prograd(inp, T, grad_scale=1.0, corrupt=None):
    """{losses [2] = xe, kl; d_text; d_text_kl} of clipmi_prompt_head, mode 2."""
    B, scale = inp["B"], inp["scale"]
    f, t, inf, intx = _norms(inp)
    o = _np(inp["teacher"])
    inty = _inv_norm(o)
    z, zt = _logits(f, t, inf, intx, scale), _logits(f, o, inf, inty, scale)
    k = F(grad_scale) / F(B)
    dz, rows = _xent(z, inp["labels"].numpy(), k)
    inv_t = F(1) / F(T)
    x, _, Ss, ps = _soft(z, inv_t)
    _, _, _, pt = _soft(zt, inv_t)
    dzk = ((ps - pt).astype(F) * F(k * F(T))).astype(F)
    log_ss = np.log(Ss).astype(F)[:, None]
    kl = _row_sum((pt * (log_ss - x).astype(F)).astype(F))
    if corrupt != "prograd_T2_dropped":
        kl = (kl * F(F(T) * F(T))).astype(F)
    return {"losses": torch.tensor([F(_mean_f64(rows)), F(_mean_f64(kl))]), "d_text": torch.from_numpy(_coop_grad(f, t, inf, intx, dz, scale)),
            "d_text_kl": torch.from_numpy(_coop_grad(f, t, inf, intx, dzk, scale))}


def _emulate_l1(a, ia, o, io, k, out, corrupt):
    u = (a * ia[:, None]).astype(F)
    d = (u - (o * io[:, None]).astype(F)).astype(F)
    s = np.sign(d).astype(F)
    if corrupt == "src_sign0_plus":
        s[d == 0] = 1
    l1 = _row_sum(np.abs(d))
    qs = _row_sum((u * s).astype(F))[:, None]
    add = ((F(k) * ia)[:, None].astype(F) * (s - (u * qs).astype(F)).astype(F)).astype(F)
    return l1, np.where(add != 0, (out + add).astype(F), out)


def emulate_promptsrc(inp, weights, grad_scale=1.0, corrupt=None):
    """{losses [5]; d_feats; d_text} of clipmi_promptsrc_head."""
    B, C, E, scale = inp["B"], inp["C"], inp["E"], inp["scale"]
    wt, wi, wl = weights
    f, t, inf, intx = _norms(inp)
    zs, o = _np(inp["zs"]), _np(inp["teacher"])
    inzs, inty = _inv_norm(zs), _inv_norm(o)
    z = _logits(f, t, inf, intx, scale)
    dz, rows = _xent(z, inp["labels"].numpy(), F(grad_scale) / F(B))
    kl_rows = np.zeros(B, F)
    if wl != 0:
        zz = _logits(zs, o, inzs, inty, scale)
        x, _, Ss, ps = _soft(z)
        xt, _, St, pt = _soft(zz)
        kk = F(F(grad_scale) * F(wl)) / F(F(B) * F(C))
        dz = (dz + ((ps - pt).astype(F) * kk).astype(F)).astype(F)
        ls, lt_ = np.log(Ss).astype(F)[:, None], np.log(St).astype(F)[:, None]
        kl_rows = _row_sum((pt * ((xt - lt_).astype(F) - (x - ls).astype(F)).astype(F)).astype(F))
    d_text = _coop_grad(f, t, inf, intx, dz, scale)
    d_feats = _coop_grad(t, f, intx, inf, dz.T.copy(), scale)
    l1t, l1i = np.zeros(C, F), np.zeros(B, F)
    if wt != 0:
        l1t, d_text = _emulate_l1(t, intx, o, inty, F(F(grad_scale) * F(wt)) / F(F(C) * F(E)), d_text, corrupt)
    if wi != 0:
        l1i, d_feats = _emulate_l1(f, inf, zs, inzs, F(F(grad_scale) * F(wi)) / F(F(B) * F(E)), d_feats, corrupt)
    ce = _mean_f64(rows)
    lt = _mean_f64(l1t) / E if wt != 0 else 0.0
    li = _mean_f64(l1i) / E if wi != 0 else 0.0
    kl = _mean_f64(kl_rows) / C if wl != 0 else 0.0
    total = ce + float(F(wt)) * lt + float(F(wi)) * li + float(F(wl)) * kl
    return {"losses": torch.tensor([F(total), F(ce), F(lt), F(li), F(kl)]), "d_feats": torch.from_numpy(d_feats), "d_text": torch.from_numpy(d_text)}


def prograd_formulas(inp, T):
    E = inp["E"]
    xe, kl, d_xe, d_kl = promptfit_ref.prograd_head(inp["feats"][:, :E].double(), inp["labels"], inp["text"].double(), inp["teacher"].double(), inp["scale"], T)
    return {"losses": torch.stack([xe, kl]), "d_text": d_xe, "d_text_kl": d_kl}


def promptsrc_formulas(inp, weights):
    import promptsrcfit_ref
    E = inp["E"]
    losses, d_feats, d_text = promptsrcfit_ref.head(inp["feats"][:, :E].double(), inp["zs"].double(), inp["text"].double(), inp["teacher"].double(),
                                                    inp["labels"], inp["scale"], weights)
    return {"losses": losses, "d_feats": d_feats, "d_text": d_text}


# ------------------------------------------------------------------------------------------------------------------------- ProDA
PRODA_SCALES = (100.0, 10.0)        # the real setting and prodafit_ref.HEAD_SCALE, at which prodafit_ref.head_case's softmax is not saturated
# (B, C, E, Pb, P, strided): (Pb, P) from prodafit_ref.HEAD_CASES on a reduced shape list -- C across 256 / 257 / 1000, E across 64 .. 1024, B = 257
PRODA_SHAPES = [(3, 257, 64, 2, 8, False), (2, 257, 512, 1, 4, True), (5, 65, 1024, 4, 4, False), (257, 3, 64, 2, 8, False), (4, 513, 128, 2, 8, True),
                (2, 1000, 65, 1, 4, False), (5, 4, 257, 4, 4, True), (1, 2, 1, 1, 4, False)]
PRODA_CASES = [c + (s,) for c in PRODA_SHAPES for s in PRODA_SCALES]
PRODA_ALPHA = 0.1


@functools.lru_cache(maxsize=None)
def proda_inputs(case):
    import prodafit_ref
    B, C, E, Pb, P, strided, scale = case
    wide, text, y = prodafit_ref.head_case(B, C, E, Pb, P)
    ld = E + 3 if strided else E
    feats = torch.full((B, ld), float("nan"))
    feats[:, :E] = wide[:, :E]
    y = y.clone()
    y[0] = C - 1
    if C > 256 and B > 1:
        y[1] = 256 if C > 257 else 255
    return {"feats": feats, "ld": ld, "text": text, "labels": y, "B": B, "C": C, "E": E, "Pb": Pb, "P": P, "scale": scale}


def proda_formulas(inp, alpha=PRODA_ALPHA):
    import prodafit_ref
    E = inp["E"]
    total, upper, lm, d, _ = prodafit_ref.head(inp["feats"][:, :E].double(), inp["labels"], inp["text"].double(), inp["C"], inp["Pb"], inp["scale"], alpha)
    return {"losses": torch.stack([total, upper, lm]), "d_text": d}


def proda_bound(inp, alpha=PRODA_ALPHA, grad_scale=1.0):
    """{losses [3] = total, upper, m; d_text [C Pb + P, E]}: (want, tol)."""
    B, C, E, Pb, P, s = inp["B"], inp["C"], inp["E"], inp["Pb"], inp["P"], inp["scale"]
    f, text, y = inp["feats"][:, :E].double(), inp["text"].double(), inp["labels"]
    en, n64, n256 = _en(E), ceil_div(E, 64), ceil_div(E, 256)
    x, _ = _unit(f)
    tc = text[:C * Pb].reshape(C, Pb, E)
    u, itn = _unit(tc)
    tu = (en + 1) * U * u.abs()
    m = u.mean(1)
    tm = tu.sum(1) / Pb + (Pb + 1) * U * u.abs().sum(1) / Pb
    v = u - m[:, None]
    tv = tu + tm[:, None] + U * v.abs()
    x2 = x * x
    tx2 = (2 * en + 3) * U * x2
    dot = x @ m.t()
    tdot = (en + 1) * U * (x.abs() @ m.abs().t()) + x.abs() @ tm.t() + (n64 + 6) * U * (x.abs() @ m.abs().t())
    diff = v[y][:, None] - v[None]                                        # [B, C, Pb, E]: v_y - v_c
    tdiff = tv[y][:, None] + tv[None] + U * diff.abs()
    sq = (diff ** 2).sum(2)
    tsq = (2 * diff.abs() * tdiff + tdiff ** 2).sum(2) + (Pb + 1) * U * sq
    sig = (x2[:, None] * sq).sum(-1)
    tsig = (tx2[:, None] * sq + x2[:, None] * tsq).sum(-1) + (n64 + 7) * U * sig
    hs2 = 0.5 * s * s
    z = s * dot + hs2 * sig / (Pb + 1)
    tz = hs2 / (Pb + 1) * (tsig + 2 * U * sig) + abs(s) * (tdot + U * dot.abs()) + U * z.abs()
    _, _, dz, tdz, rows, trows = _softmax_bound(z, tz, y, grad_scale / B, C)
    upper, tupper = _mean_bound(rows, trows)
    dm = s * (dz.t() @ x)
    tdm = abs(s) * (tdz.t() @ x.abs() + (en + 1 + B) * U * (dz.abs().t() @ x.abs())) + U * dm.abs()
    w = hs2 * dz[:, :, None] * x2[:, None]                                # [B, C, E]
    tw = hs2 * (tdz[:, :, None] * x2[:, None] + dz.abs()[:, :, None] * tx2[:, None]) + 3 * U * w.abs()
    terms = w[:, :, None] * diff                                          # [B, C, Pb, E]
    tterms = tw[:, :, None] * diff.abs() + w.abs()[:, :, None] * tdiff
    zero = torch.zeros(C, Pb, E, dtype=torch.float64)
    a = -terms.sum(0) + zero.clone().index_add_(0, y, terms.sum(1))
    sabs = terms.abs().sum(0) + zero.clone().index_add_(0, y, terms.abs().sum(1))
    ta = tterms.sum(0) + zero.clone().index_add_(0, y, tterms.sum(1))
    Lk = (B + C * torch.bincount(y, minlength=C)).double()[:, None, None]
    two_over = 2.0 / (Pb + 1)
    dv = two_over * a
    tdv = two_over * (ta + Lk * U * sabs) + 2 * U * dv.abs()
    mean = dv.mean(1, keepdim=True)
    tmean = tdv.sum(1, keepdim=True) / Pb + (Pb + 1) * U * dv.abs().sum(1, keepdim=True) / Pb
    du = dv - mean + dm[:, None] / Pb
    tdu = tdv + tmean + U * (dv - mean).abs() + (tdm[:, None] / Pb + 2 * U * dm.abs()[:, None] / Pb) + U * du.abs()
    d_cls, td_cls = _project_bound(du, tdu, u, itn, en, n256 + 9)
    n, inn = _unit(text[C * Pb:])
    G = n @ n.t()
    tG = (2 * en + 3 + n64 + 6) * U * (n.abs() @ n.abs().t())
    off = (~torch.eye(P, dtype=torch.bool)).double()
    lm = (G.abs() * off).sum() / (P * (P - 1))
    tlm = (tG * off).sum() / (P * (P - 1)) + U * lm.abs()
    k = grad_scale * alpha * 2.0 / (P * (P - 1))
    sg = torch.sign(G) * off
    tsg = 2.0 * ((G.abs() <= tG) & (G != 0)).double() * off
    g = k * (sg @ n)
    tg = abs(k) * ((tsg + (en + 1) * U * off) @ n.abs() + P * U * (off @ n.abs())) + 2 * U * g.abs()
    d_nc, td_nc = _project_bound(g, tg, n, inn, en, n256 + 9)
    total = upper + alpha * lm
    ttotal = tupper + alpha * tlm + U * ((alpha * lm).abs() + total.abs())
    return {"losses": (torch.stack([total, upper, lm]), torch.stack([ttotal, tupper, tlm])),
            "d_text": (torch.cat([d_cls.reshape(C * Pb, E), d_nc]), torch.cat([td_cls.reshape(C * Pb, E), td_nc]))}


def _thread_dot(a, b):
    """sum_e a_e b_e as proda's `e += THREADS` loops form it: 256 strided fmaf chains, four wave trees, the waves in ascending order."""
    return _lane_dot(a, b, 256)


def emulate_proda(inp, alpha=PRODA_ALPHA, grad_scale=1.0, corrupt=None):
    """{losses [3], d_text} of clipmi_proda_head in the kernels' order, fp32 numpy (the sums that carry no pragma are taken unfused)."""
    B, C, E, Pb, P, s = inp["B"], inp["C"], inp["E"], inp["Pb"], inp["P"], F(inp["scale"])
    f, text, y = _np(inp["feats"][:, :E]), _np(inp["text"]), inp["labels"].numpy()
    inf, intx = _inv_norm(f), _inv_norm(text)
    tc, itc = text[:C * Pb].reshape(C, Pb, E), intx[:C * Pb].reshape(C, Pb)
    u = (tc * itc[:, :, None]).astype(F)
    m = np.zeros((C, E), F)
    for q in range(Pb):
        m = (m + u[:, q]).astype(F)
    m = (m / F(Pb)).astype(F)
    v = (u - m[:, None]).astype(F)
    x = (f * inf[:, None]).astype(F)
    x2 = (x * x).astype(F)
    z = np.empty((B, C), F)
    hs2 = F(F(0.5) * s) * s
    for b in range(B):
        dot = _lane_dot(m, x[b][None, :])
        sq = np.zeros((C, E), F)
        for q in range(Pb):
            d = (v[y[b], q][None, :] - v[:, q]).astype(F)
            sq = _fma(d, d, sq)
        sig = _lane_dot(sq, x2[b][None, :])
        z[b] = _fma(hs2, (sig / F(Pb + 1)).astype(F), (s * dot).astype(F))
    dz, rows = _xent(z, y, F(grad_scale) / F(B), corrupt)
    dm = np.zeros((C, E), F)
    for b in range(B):
        dm = _fma(dz[b][:, None], x[b][None, :], dm)
    dm = (dm * s).astype(F)
    a = np.zeros((C, Pb, E), F)
    for b in range(B):
        coef = ((hs2 * dz[b]).astype(F)[:, None] * x2[b][None, :]).astype(F)          # [C, E]
        a = _fma(coef[:, None, :], (v - v[y[b]][None]).astype(F), a)
        k = y[b]
        for c in range(C):
            a[k] = _fma(coef[c][None, :], (v[k] - v[c]).astype(F), a[k])
    a = (a * F(F(2) / F(Pb + 1))).astype(F)
    mean = np.zeros((C, E), F)
    for q in range(Pb):
        mean = (mean + a[:, q]).astype(F)
    mean = (mean * F(F(1) / F(Pb))).astype(F)
    du = ((a - mean[:, None]).astype(F) + (dm * F(F(1) / F(Pb))).astype(F)[:, None]).astype(F)
    dot = _thread_dot(u, du)[:, :, None]
    if corrupt == "q_single_wave":
        pad = np.pad((u * du).astype(F), [(0, 0), (0, 0), (0, ceil_div(E, 256) * 256 - E)])
        dot = _block(pad.reshape(C, Pb, -1, 256).sum(2).astype(F), single_wave=True)[:, :, None]
    d_cls = ((du - (u * dot).astype(F)).astype(F) * itc[:, :, None]).astype(F)
    nc, inn = text[C * Pb:], intx[C * Pb:]
    n = (nc * inn[:, None]).astype(F)
    G = np.stack([_lane_dot(n, n[p][None, :]) for p in range(P)])
    kk = F(float(grad_scale) * 2.0 * float(alpha) / (P * (P - 1.0)))
    dn = np.zeros((P, E), F)
    for q in range(P):
        sg = np.sign(G[:, q]).astype(F)
        sg[q] = 0
        dn = np.where((np.arange(P) != q)[:, None], _fma(sg[:, None], n[q][None, :], dn), dn)
    g = (kk * dn).astype(F)
    dd = _thread_dot(n, g)[:, None]
    d_nc = ((g - (n * dd).astype(F)).astype(F) * inn[:, None]).astype(F)
    upper = F(_mean_f64(rows, corrupt))
    part = np.zeros(256, np.float64)
    flat = np.abs(G).reshape(-1).astype(np.float64) * (1 - np.eye(P)).reshape(-1)
    for i in range(0, P * P, 256):
        part[:min(256, P * P - i)] += flat[i:i + 256]
    h = 128
    while h:
        part[:h] += part[h:2 * h]
        h //= 2
    lm = F(part[0] / (P * (P - 1.0)))
    total = F(upper + F(F(alpha) * lm))
    return {"losses": torch.tensor([total, upper, lm]), "d_text": torch.from_numpy(np.concatenate([d_cls.reshape(C * Pb, E), d_nc]))}
