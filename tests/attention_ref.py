"""Plain reference of the attention entry points clipmi_attention (csrc/attention.hip) and clipmi_attention_cls (csrc/attention_cls.hip) --
the oracle of tests/test_attention_ref_cpu.py and tests/test_gpu_attention_ops.py.  Written from clip/model.py:181-183 (nn.MultiheadAttention
on the packed in-projection: head_dim 64, softmax(q k^T / 8 + mask) v, the text tower's mask of :585-591) and include/clipmi.h, not from the
kernels: float64 on the exact values of the fp16 inputs.

``attention`` returns ``(out, tol)``, both float64: ``tol`` is the forward error bound PER OUTPUT ELEMENT of the arithmetic the kernels
document (fp32 scores from exact fp16 products, P rounded to fp16 before the PV product, the row sum from the same rounded P, fp32
accumulation, one fp16 rounding of the output); every term is stated with its source in ``_tolerance``.  ``emulate`` is that arithmetic on the
CPU (and three deliberately wrong variants of it); the constructed inputs (selection, uniform) need no tolerance at all; the case lists at
the end are shared by the CPU test and the GPU test: same seeds, same tensors.

The second half is the same for the two backward entry points, clipmi_attention_backward and clipmi_attention_backward_full:
``attention_backward`` (reference and per-element tolerance), ``emulate_backward`` (and seven wrong variants), the backward selection and
uniform inputs and the case lists of tests/test_gpu_attention_backward_ops.py.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

U16 = 2.0 ** -11      # unit roundoff of fp16
U32 = 2.0 ** -24      # unit roundoff of fp32
C_EXP = 0.125 * math.log2(math.e)     # softmax(s / 8) = 2^(C s - C max)
LN2 = math.log(2.0)


def _f64(t):
    return t.detach().cpu().to(torch.float64)


def _allowed(R, L, causal):
    """[R, L] bool: query q may attend to key k."""
    if not causal:
        return torch.ones(R, L, dtype=torch.bool)
    return torch.arange(L)[None, :] <= torch.arange(R)[:, None]


# ------------------------------------------------------------------------------------------------------------- reference and tolerance
def _tolerance(o, p, v, raw, sabs, allowed, p_fp16, updates):
    """Forward error bound of one (sequence, head): o [R,64], p [R,L] (exact probabilities), v [L,64], raw = q k^T, sabs = |q| |k|^T.

    Notation: with exact probabilities P and an approximation P_k (1 + e_k) in numerator and row sum alike,
        o' - o = sum_k P_k e_k (v_k - o) / (1 + sum_k P_k e_k),    so    |o' - o| <~ max|e| * sum_k P_k |v_k - o|.
    ``spread`` bounds that sum twice over: by A + |o| with A = sum_k P_k |v_k| (the triangle inequality; A >= |o|, so this is the
    2 A of the usual statement) and by the standard deviation sqrt(sum_k P_k v_k^2 - o^2) of v under P (Cauchy-Schwarz); the smaller holds.

    Terms (u16 = 2^-11, u32 = 2^-24):
      1. u16 |o| + 2^-25                the one fp16 rounding of the output (2^-25: half a subnormal step);
      2. u16 * spread                   P rounded to fp16, in the PV product and in the row sum (fp16 P only);
      3. 2^-25 (sum_k |v_k| + n |o|)    probabilities under fp16's normal range 2^-14 are rounded with an ABSOLUTE error of half a
                                        subnormal step, 2^-25, each, in the numerator and (n allowed keys) in the row sum; a probability is
                                        formed relative to the running maximum, so the row sum is at least 1 (fp16 P only);
      4. e_exp * spread                 the fp32 exponent.  The exponent of key k is t = C (s_k - m) with C = log2(e) / 8:
           * the score s_k is an fp32 sum of 64 exact products in some order: |error| <= 64 u32 sum_i |q_i k_i|       (Higham, gamma_64);
           * C is rounded to fp32 (|s - m| <= 2 S, S = max_k |s_k|), the product m C is rounded (<= S C u32) and so is the fused
             multiply-add that forms t (|t| <= 2 S C): 5 S C u32 together;
           * a running maximum may move once per 32-key tile (per key of a lane's row group in the class-row kernel): ``updates`` rescales by
             2^(C (m_old - m_new)), each with a rounded difference, a rounded product and the rounded C (6 S C u32) and one exp2;
           * exp2 itself (v_exp_f32, 1 ulp by the ISA manual; 2 ulp allowed): 2^-22 per evaluation;
         an absolute error d of t is a relative error ln(2) d of 2^t;
      5. 2 (n + updates) u32 A          fp32 accumulation of n terms and ``updates`` rescales, in the numerator and, relative to |o| <= A, in the
                                        row sum (Higham, gamma_n);
      6. 3 u32 |o|                      the reciprocal of the row sum and the product with it.
    Second-order products of these are covered by the factor 1.01."""
    ab = o.abs()
    vab = v.abs()
    pa = p @ vab
    spread = torch.minimum(torch.sqrt((p @ (v * v) - o * o).clamp_min(0.0)), pa + ab)
    n = allowed.sum(dim=1, keepdim=True).to(torch.float64)
    smax = raw.abs().masked_fill(~allowed, 0.0).amax(dim=1, keepdim=True)
    sacc = sabs.masked_fill(~allowed, 0.0).amax(dim=1, keepdim=True)
    e_exp = LN2 * C_EXP * U32 * (64.0 * sacc + (5.0 + 6.0 * updates) * smax) + (1.0 + updates) * 2.0 ** -22
    tol = U16 * ab + 2.0 ** -25 + e_exp * spread + 2.0 * (n + updates) * U32 * pa + 3.0 * U32 * ab
    if p_fp16:
        vsum = allowed.to(torch.float64) @ vab
        tol = tol + U16 * spread + 2.0 ** -25 * (vsum + n * ab)
    return 1.01 * tol


def attention(qkv, N, L, H, causal, rows=None, p_fp16=True):
    """qkv fp16 [N*L, 3*64*H] (q | k | v) -> (out, tol) float64 [N, R, 64*H] with R = L, or the first ``rows`` queries of every sequence.
    p_fp16 False: the bound of a kernel that keeps P in fp32 (clipmi_attention_cls)."""
    R = L if rows is None else rows
    x = _f64(qkv).reshape(N, L, 3, H, 64)
    allowed = _allowed(R, L, causal)
    updates = float((L + 31) // 32 if p_fp16 else (L + 7) // 8 + 3)
    out = torch.empty(N, R, H, 64, dtype=torch.float64)
    tol = torch.empty_like(out)
    for n in range(N):
        for h in range(H):
            q, k, v = x[n, :R, 0, h], x[n, :, 1, h], x[n, :, 2, h]
            raw = q @ k.t()
            p = torch.softmax((raw / 8.0).masked_fill(~allowed, float("-inf")), dim=-1)
            o = p @ v
            out[n, :, h] = o
            tol[n, :, h] = _tolerance(o, p, v, raw, q.abs() @ k.abs().t(), allowed, p_fp16, updates)
    return out.reshape(N, R, 64 * H), tol.reshape(N, R, 64 * H)


def attention_cls(qkv, N, L, H):
    """clipmi_attention_cls: row 0 of every sequence, never masked, P in fp32 -> (out, tol) float64 [N, 64*H]."""
    out, tol = attention(qkv, N, L, H, False, rows=1, p_fp16=False)
    return out[:, 0], tol[:, 0]


# ------------------------------------------------------------------------------------------------------------------------ CPU emulation
WRONG = ("drop_last", "admit_next", "next_seq")


def emulate(qkv, N, L, H, causal, rows=None, p_fp16=True, wrong=None):
    """The documented arithmetic in torch on the CPU: float32 scores, exp2 in float32, .half() on P, float32 PV and row sum, .half() on the
    quotient -> fp16 [N, R, 64*H].  ``wrong`` makes it wrong in one way:
      drop_last   the last key a row may see is dropped: key L-1 (non-causal), key q of row q >= 1 (causal);
      admit_next  the causal mask admits key q + 1;
      next_seq    row 0 of the next sequence of the batch (cyclically) is one more key."""
    R = L if rows is None else rows
    x = qkv.detach().cpu().reshape(N, L, 3, H, 64).float()
    allowed = _allowed(R, L, causal)
    if wrong == "drop_last":
        if causal:
            i = torch.arange(1, R)
            allowed[i, i] = False
        else:
            allowed[:, L - 1] = False
    elif wrong == "admit_next":
        i = torch.arange(0, min(R, L - 1))
        allowed[i, i + 1] = True
    elif wrong == "next_seq":
        allowed = torch.cat([allowed, torch.ones(R, 1, dtype=torch.bool)], dim=1)
    c = torch.tensor(C_EXP, dtype=torch.float32)
    out = torch.empty(N, R, H, 64, dtype=torch.float16)
    for n in range(N):
        for h in range(H):
            q, k, v = x[n, :R, 0, h], x[n, :, 1, h], x[n, :, 2, h]
            if wrong == "next_seq":
                k = torch.cat([k, x[(n + 1) % N, :1, 1, h]])
                v = torch.cat([v, x[(n + 1) % N, :1, 2, h]])
            s = (q @ k.t()).masked_fill(~allowed, float("-inf"))
            m = s.amax(dim=1, keepdim=True)
            p = torch.exp2(s * c - m * c)
            if p_fp16:
                p = p.half().float()
            out[n, :, h] = ((p @ v) / p.sum(dim=1, keepdim=True)).half()
    return out.reshape(N, R, 64 * H)


def worst_ratio(got, want, tol):
    """max |got - want| / tol over all elements (inf where got is not finite)."""
    r = (got.double().reshape(want.shape) - want).abs() / tol
    r[torch.isnan(r)] = float("inf")
    return float(r.max())


# ---------------------------------------------------------------------------------------------------------------- random inputs
def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 1000003 ** i * int(k) for i, k in enumerate(key)) % (2 ** 63 - 1)))


def random_batch(N, L, H, causal, distinct, scale=1.5):
    """N sequences built from ``distinct`` different ones, N(0, scale^2), placed in a shuffled order (every distinct one at least once).
    -> (qkv fp16 [N*L, 3*64*H], order: the distinct sequence behind every batch slot, seqs fp16 [distinct, L, 3*64*H])."""
    g = _gen(N, L, H, int(causal), distinct)
    seqs = (torch.randn(distinct, L, 3 * 64 * H, generator=g) * scale).half()
    order = torch.cat([torch.arange(distinct), torch.randint(0, distinct, (N - distinct,), generator=g)])
    order = order[torch.randperm(N, generator=g)]
    return seqs[order].reshape(N * L, 3 * 64 * H), order.tolist(), seqs


def legacy_qkv(n, l, h, scale=1.5):
    """The input of the attention tests of tests/test_gpu_ops.py: seed n*1000 + l + h, N(0, 1.5^2)."""
    g = torch.Generator().manual_seed(n * 1000 + l + h)
    return (torch.randn(n * l, 3 * 64 * h, generator=g) * scale).half()


def peaked_qkv(which):
    """The two peaked-row inputs of tests/test_gpu_ops.py (large queries, a dominant key late in the sequence) -> (qkv, N, L, H)."""
    if which == "ring":
        n, l, h = 1, 577, 2
        qkv = torch.randn(n * l, 3 * 64 * h, generator=torch.Generator().manual_seed(7))
        qkv[:, :128] *= 5.0
        qkv[570, 128:256] *= 5.0
        qkv[3, 128:256] *= 4.0
    else:
        n, l, h = 1, 197, 2
        qkv = torch.randn(n * l, 3 * 64 * h, generator=torch.Generator().manual_seed(5))
        qkv[:, :128] *= 6.0
        qkv[150, 128:256] *= 5.0
    return qkv.half(), n, l, h


# ---------------------------------------------------------------------------------------------------------- constructed: selection
SELECT_KINDS = {False: ("perm", "last", "first"), True: ("diag", "below", "decoy")}
CODE_BITS = 12          # 4096 key indices


def _bits_pm(idx):
    """[n] int -> [n, 12] of -1 / +1: the bits of the index."""
    return (((idx[:, None] >> torch.arange(CODE_BITS)[None, :]) & 1) * 2 - 1).to(torch.float64)


def selection_target(L, kind, g):
    """pi: the key every query selects."""
    q = torch.arange(L)
    if kind == "perm":
        return torch.randperm(L, generator=g)
    if kind == "last":
        return torch.full((L,), L - 1)
    if kind == "first":
        return torch.zeros(L, dtype=torch.long)
    if kind == "diag":
        return q
    if kind == "below":
        return (torch.rand(L, generator=g) * (q + 1).double()).long().clamp_max(q)
    if kind == "decoy":
        return (q + 1) & q          # q + 1 with its lowest set bit cleared: <= q
    raise ValueError(kind)


def selection_batch(N, L, H, kind, pi0=None):
    """-> (qkv fp16 [N*L, 3*64*H], want fp16 [N*L, 64*H], pi [N, H, L]): out of query q comes the V row of key pi(q), bit for bit.

    Twelve of the 64 dimensions (at positions drawn per item) hold the code of an index, +-16 per bit: key j carries code(j), query q carries
    code(pi(q)), so q . k = 256 (12 - 2 hamming(pi(q), j)): 3072 for the target, at most 2560 for any other key -- 512 / 8 = 64 natural units
    behind, a probability below e^-64 = 1.7e-28: 0 in fp16, and in fp32 far under half an ulp of any normal fp16 V.  The other 52 dimensions
    hold small integers in pairs that cancel: (a, a) in the key against (b, -b) in the query.  Every score is an exact integer in fp32.
    kind "decoy" (causal): the query carries code(q + 1) and key j carries code(j) with bit i weighted (i + 1): q . k = 256 sum_i (i + 1) [bits
    agree].  Key q + 1 agrees everywhere and leads; among the keys 0..q the best is q + 1 with its cheapest set bit cleared, pi(q) = (q + 1) & q
    (any other key <= q differs in a dearer set bit, or in more), and it leads the rest by at least 2 * 256 = 64 natural units.  A mask that
    admits key q + 1 changes the row completely.
    V: random sign, exponent 1..30 and mantissa: normal, non-zero, finite, over fp16's whole exponent range.
    pi0: optional target of query 0 of every item (the class-row tests), else drawn by ``kind``."""
    g = _gen(N, L, H, sorted(sum(SELECT_KINDS.values(), ())).index(kind), 77)
    D = 64 * H
    qkv = torch.zeros(N, L, 3, H, 64, dtype=torch.float64)
    vb = (torch.randint(0, 2, (N, L, H, 64), generator=g) << 15) | (torch.randint(1, 31, (N, L, H, 64), generator=g) << 10) | \
        torch.randint(0, 1024, (N, L, H, 64), generator=g)
    v = torch.from_numpy(vb.numpy().astype(np.uint16).view(np.float16).copy())
    pis = torch.empty(N, H, L, dtype=torch.long)
    idx = torch.arange(L)
    for n in range(N):
        for h in range(H):
            pi = selection_target(L, kind, g)
            if pi0 is not None:
                pi[0] = pi0
            pis[n, h] = pi
            dims = torch.randperm(64, generator=g)
            code, rest = dims[:CODE_BITS], dims[CODE_BITS:]
            if kind == "decoy":
                qkv[n, :, 0, h, code] = 16.0 * _bits_pm(idx + 1)
                qkv[n, :, 1, h, code] = 16.0 * _bits_pm(idx) * torch.arange(1, CODE_BITS + 1, dtype=torch.float64)[None, :]
            else:
                qkv[n, :, 0, h, code] = 16.0 * _bits_pm(pi)
                qkv[n, :, 1, h, code] = 16.0 * _bits_pm(idx)
            a = torch.randint(-2, 3, (L, 26), generator=g).double()
            b = torch.randint(-2, 3, (L, 26), generator=g).double()
            qkv[n, :, 1, h, rest[0::2]] = a
            qkv[n, :, 1, h, rest[1::2]] = a
            qkv[n, :, 0, h, rest[0::2]] = b
            qkv[n, :, 0, h, rest[1::2]] = -b
    qkv = qkv.half()
    qkv[:, :, 2] = v
    want = torch.stack([torch.stack([v[n, pis[n, h], h] for h in range(H)], dim=1) for n in range(N)])      # [N, L, H, 64]
    return qkv.reshape(N * L, 3 * D), want.reshape(N * L, D), pis


# ------------------------------------------------------------------------------------------------------------ constructed: uniform
def uniform_batch(N, L, H, causal):
    """q == 0: every allowed key has probability exactly 1 and the row sum is the key count; V holds integers of magnitude 8..15 with random
    signs (sums exact in fp32); k is random and must not matter.  -> (qkv fp16, exact float64 [N*L, 64*H]: the mean over the allowed keys)."""
    g = _gen(N, L, H, int(causal), 99)
    D = 64 * H
    qkv = torch.zeros(N, L, 3, D, dtype=torch.float64)
    qkv[:, :, 1] = torch.randn(N, L, D, generator=g) * 1.5
    v = torch.randint(8, 16, (N, L, D), generator=g).double() * (torch.randint(0, 2, (N, L, D), generator=g) * 2 - 1).double()
    qkv[:, :, 2] = v
    exact = v.cumsum(dim=1) / torch.arange(1, L + 1, dtype=torch.float64)[None, :, None] if causal else v.mean(dim=1, keepdim=True).expand(N, L, D)
    return qkv.half().reshape(N * L, 3 * D), exact.reshape(N * L, D).clone()


def _ordered(h16):
    """fp16 -> int32 that counts representable values along the real line (-0 and +0 both 0)."""
    b = h16.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7FFF))


def fp16_steps_from_nearest(got16, exact):
    """How many fp16 values ``got16`` lies from the fp16 value nearest to ``exact`` (float64): [.] int32; NaN counts as far."""
    d = (_ordered(got16.cpu().reshape(exact.shape)) - _ordered(exact.half())).abs()
    d[torch.isnan(got16.cpu().reshape(exact.shape).float())] = 1 << 20
    return d


UNIFORM_STEPS = 1       # the output is the fp16 value nearest to the exact mean, or its neighbour (fp32 sum exact; reciprocal, product: ~1.5 ulp of fp32)


# --------------------------------------------------------------------------------------------------------------------------- cases
LENGTHS = (1, 2, 8, 31, 32, 33, 50, 64, 65, 77, 96, 97, 128, 129, 160, 192, 193, 197, 200, 201, 224, 225, 256, 257, 320, 321, 352, 353, 448,
           449, 577, 1025, 2816, 2817)
HEADS = (1, 2, 12, 16)
KERNELS = ("small", "persist<3,3,0>", "persist<3,3,2>", "persist<7,4,0>", "persist<7,4,1>", "vision", "vision_nt", "stream<4>", "stream<7>",
           "ring")
CAUSAL_ONLY = ("persist<3,3,2>",)
NONCAUSAL_ONLY = ("persist<7,4,1>", "vision", "vision_nt", "ring")
SEAMS = (32, 64, 96, 192, 200, 224, 320)            # a kernel family changes between L and L + 1
RING_MAX = 2816
DEFAULTS = {"attn_small": 1, "attn_loader": 2, "attn_ring": 1}


def kernel_for(L, causal, opts=None):
    """The dispatch of launch_attention (csrc/attention.hip) as a table: which instantiation a call reaches."""
    o = dict(DEFAULTS, **(opts or {}))
    if L <= 32 and o["attn_small"]:
        return "small"
    if L <= 96:
        return "persist<3,3,2>" if causal and L > 64 else "persist<3,3,0>"
    if L <= 224:
        if not causal and L > 192:
            if L <= 200 and o["attn_loader"]:
                return "vision_nt" if o["attn_loader"] == 2 else "vision"
            return "persist<7,4,1>"
        return "persist<7,4,0>"
    if not causal and o["attn_ring"] and L <= RING_MAX:
        return "ring"
    return "stream<4>" if L <= 320 else "stream<7>"


def option_settings(L, causal):
    """Every setting of the three options that changes the kernel at (L, causal); the default first."""
    if L <= 32:
        return [{"attn_small": 1}, {"attn_small": 0}]
    if not causal and 193 <= L <= 200:
        return [{"attn_loader": 2}, {"attn_loader": 1}, {"attn_loader": 0}]
    if not causal and 224 < L <= RING_MAX:
        return [{"attn_ring": 1}, {"attn_ring": 0}]
    return [{}]


def same_bits(a, b):
    """The bit-identity claims of include/clipmi.h: attn_loader 0 / 1 / 2 "all three: same bits", attn_small 0 "same bits"."""
    fam = lambda k: "p73" if k in ("vision", "vision_nt", "persist<7,4,1>") else "p33" if k in ("small", "persist<3,3,0>") else k
    return fam(a) == fam(b)


Case = namedtuple("Case", "N L H causal distinct")


def _sweep():
    out = []
    for i, L in enumerate(LENGTHS):
        for causal in (False, True):
            H = HEADS[(i + int(causal)) % 4] if L <= 577 else (2 if L == 1025 else 1)
            N = 1 + (i + int(causal)) % 3 if L <= 1025 else 1 + int(causal)
            out.append(Case(N, L, H, causal, min(N, 2)))
    return out


SWEEP = _sweep()
# the many-item cases: several items per workgroup (or per wave), every one of them under the reference of its distinct sequence
MANY = [Case(40, 197, 12, False, 3), Case(70, 257, 16, False, 3), Case(40, 577, 16, False, 2), Case(300, 577, 1, False, 3),
        Case(500, 24, 8, True, 3), Case(4100, 24, 1, True, 3)]
RANDOM_CASES = SWEEP + MANY
PEAKED = ("persist", "ring")

# tests/test_gpu_ops.py, the attention tests: (n, l, h, causal) and the scalar bound used there
LEGACY = ([(c, 4e-3) for c in [(2, 197, 12, False), (3, 77, 8, True), (2, 17, 2, False), (1, 10, 3, False), (2, 199, 12, False), (1, 257, 16, False),
                               (1, 577, 4, False), (2, 77, 1, True), (1, 32, 1, True), (1, 1, 1, False), (1, 225, 2, True)]] +
          [((n, l, h, False), 4e-3) for n, l, h in [(3, 197, 12), (2, 199, 12), (1, 193, 2), (5, 200, 1), (40, 197, 12)]] +
          [((n, l, h, False), 4e-3) for n, l, h in [(1, 577, 4), (2, 257, 16), (3, 225, 2), (1, 256, 1), (2, 300, 3), (1, 384, 2), (1, 512, 1), (2, 545, 2),
                                                    (1, 576, 2), (1, 640, 1), (1, 1025, 1), (70, 257, 16), (40, 577, 16), (1, 352, 2), (1, 448, 1),
                                                    (2, 480, 2), (1, 2560, 1), (2, 416, 2), (1, 2816, 1), (300, 577, 1)]] +
          [(c, 4e-3) for c in [(500, 24, 8, True), (1000, 16, 8, True), (3, 32, 2, False), (7, 31, 3, True), (5, 1, 2, False), (2, 9, 1, True),
                               (260, 8, 12, False), (4100, 24, 1, True)]])
PEAKED_BOUND = 8e-3
# where the derived bound exceeds the scalar at some element (tests/test_attention_ref_cpu.py::test_tolerance_against_the_scalar_bound says why)
LEGACY_OVER = {(2, 197, 12, False), (3, 77, 8, True), (40, 197, 12, False), (2, 300, 3, False), (1, 576, 2, False), (70, 257, 16, False),
               (40, 577, 16, False), (300, 577, 1, False), (1000, 16, 8, True), (7, 31, 3, True), (1, 2560, 1, False), (1, 2816, 1, False)}

# one (L, causal, options) per kernel instantiation, for the isolation test
ISOLATION = {"small": (24, True, {}), "persist<3,3,0>": (50, False, {}), "persist<3,3,2>": (77, True, {}), "persist<7,4,0>": (129, True, {}),
             "persist<7,4,1>": (201, False, {}), "vision": (197, False, {"attn_loader": 1}), "vision_nt": (197, False, {}),
             "stream<4>": (257, True, {}), "stream<7>": (353, True, {}), "ring": (577, False, {})}

CLS_LENGTHS = (1, 7, 8, 9, 50, 197, 257, 577)
CLS_CASES = [(N, L, 1) for L in CLS_LENGTHS for N in (1, 2, 3, 4)] + [(3, L, 12) for L in CLS_LENGTHS] + [(2, L, 16) for L in CLS_LENGTHS]


def constructed_shape(L):
    """(N, H) of the selection and uniform batches at length L."""
    return (3, 2) if L <= 577 else (1, 1)


def poison_like(t, g):
    """A tensor of t's shape filled with NaN and +-inf fp16 patterns."""
    pat = np.array([0x7E00, 0x7C00, 0xFC00, 0x7C01, 0xFE00], dtype=np.uint16)
    return torch.from_numpy(pat[torch.randint(0, len(pat), tuple(t.shape), generator=g).numpy()].view(np.float16).copy())


# ====================================================================================================================== the backward
# clipmi_attention_backward (causal, L <= 80) and clipmi_attention_backward_full (no mask, L <= 224) of csrc/attention.hip: d_out [N L, 64 H]
# -> dqkv [N L, 3 * 64 H] (dq | dk | dv).  The oracle of the backward half of tests/test_attention_ref_cpu.py, of
# tests/test_gpu_attention_backward_ops.py and of the attention test of tests/test_gpu_text_backward.py.
AB_MAX_L = {True: 80, False: 224}


def _heads(t, N, L, H):
    return t.reshape(N, L, H, 64).transpose(1, 2)          # [N, H, L, 64]


def _rows(t, N, L, H):
    return t.transpose(1, 2).reshape(N * L, 64 * H)


def attention_backward(qkv, d_out, N, L, H, causal, fp32_terms=True):
    """-> (want, tol), float64 [N L, 3 * 64 H], per element.  ``want`` is the restatement of tests/coopfit_ref.py (causal) or
    tests/vptfit_ref.py (no mask) on the exact values of the fp16 inputs.  ``tol``: P and dS reach the matrix cores rounded to fp16 (u16
    relative each, 2^-25 absolute -- half a subnormal step -- where they are subnormal), the products are accumulated in fp32 and the result
    is rounded to fp16 once.  Per element of a product sum_t a_t b_t with a rounded:
        u16 sum |a| |b|      the rounded operand (P in dV = P^T dO; dS in dQ = dS K / 8 and dK = dS^T Q / 8),
        2^-25 sum |b|        the flushed tail of that operand,
        u16 |want|           the output rounding;
    dS itself is formed in fp32 from fp32 P and dP (errors of order u32).  The project's factor 2 for the fast exponential and the fp32 sums,
    and 2^-24 (a subnormal step of the output).  The tail term runs over every (query, key) pair under either mask: a masked pair is an exact
    zero on the device, so under the causal mask the term is up to twice what the kernel can use.

    ``fp32_terms`` (False: the bound as tests/test_gpu_text_backward.py has always asserted it, sufficient where every softmax row is flat)
    adds what fp32 leaves on P and dS before they are rounded, which is what carries the error of a peaked row: there
    dP_t - rowsum = sum_j p_j (dP_t - dP_j) is a small difference of two numbers of the size of dP, and one fp32 rounding of the row sum is
    an error u32 |dP| of it -- relative u32 / (1 - p_t), beyond u16 once 1 - p_t < 2^-13.  With n allowed keys of row q, written per row:
      eps   relative error of an unnormalised probability: the exponent s / 8 - max carries the fp32 score (64 products in some order,
            64 u32 sum_i |q_i k_i| / 8, Higham gamma_64), its own rounding and that of the product with log2(e) in the fast exponential
            (2 u32 |s / 8 - max|), and the hardware exp2 (2^-22, as in ``_tolerance``); the maximum over the row's allowed keys;
      eta   (n + 2) u32: the sum of n terms in any order, its reciprocal and the product -- common to the row;
      T     sum_j p_j |dP_j| >= |rowsum|;      B_qk = sum_i |dO_qi| |V_ki|, so that 64 u32 B_qk bounds the error of dP_qk.
    Probabilities p_k (1 + e_k) renormalise to p_k (1 + e_k - sum_j p_j e_j): |dp_k| <= 2 eps p_k, and because these changes sum to zero,
    the row sum moves by sum_j dp_j (dP_j - rowsum), at most 2 eps sum_j |dS_j|.  The common factor eta does not cancel: P no longer sums to
    one, dS_k moves by eta (|dS_k| + p_k |rowsum|).  The row sum is n fused multiply-adds and a tree in any order, (n + 1) u32 T, of inexact
    dP; the error d_k of dP_k enters dS_k as p_k ((1 - p_k) d_k - sum_{j != k} p_j d_j): where p_k is one, it cancels.  Together
        |d dS_qk| <= (2 eps + eta + 2 u32) |dS_qk| + p_qk (2 eps sum_j |dS_qj| + (2 n + 3) u32 T_q + 64 u32 ((1 - 2 p_qk) B_qk + sum_j p_qj B_qj)),
        |d P_qk|  <= (2 eps + eta) p_qk,
    carried through |K| / 8, |Q| / 8 and |dO| like the fp16 roundings and under the same factor 2."""
    import coopfit_ref as cref
    import vptfit_ref as vref
    D = 64 * H
    x, g = _f64(qkv).reshape(N * L, 3 * D), _f64(d_out).reshape(N * L, D)
    want = cref.attention_backward(x, g, N, L, H) if causal else vref.attention_backward_full(x, g, N, L, H)
    q, k, v = (_heads(t, N, L, H) for t in x.split(D, dim=-1))
    d = _heads(g, N, L, H)
    p = cref.attention_probs(q, k) if causal else vref.attention_probs_full(q, k)
    dp = d @ v.transpose(-1, -2)
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    ones = torch.ones_like(p)
    bq = (ds.abs() @ k.abs()) / 8 * U16 + 2.0 ** -25 * (ones @ k.abs()) / 8
    bk = (ds.abs().transpose(-1, -2) @ q.abs()) / 8 * U16 + 2.0 ** -25 * (ones @ q.abs()) / 8
    bv = (p.transpose(-1, -2) @ d.abs()) * U16 + 2.0 ** -25 * (ones @ d.abs())
    if fp32_terms:
        ok = _allowed(L, L, causal)
        n = ok.sum(dim=1, keepdim=True).to(torch.float64)
        x8 = (q @ k.transpose(-1, -2) / 8).masked_fill(~ok, float("-inf"))
        spread = (x8.amax(-1, keepdim=True) - x8.masked_fill(~ok, float("inf")).amin(-1, keepdim=True))
        sacc = (q.abs() @ k.abs().transpose(-1, -2)).masked_fill(~ok, 0.0).amax(-1, keepdim=True)
        eps = U32 * (64.0 * sacc / 8 + 2.0 * spread) + 2.0 ** -22
        eta = (n + 2) * U32
        B = d.abs() @ v.abs().transpose(-1, -2)
        T = (p * dp.abs()).sum(-1, keepdim=True)
        row = 2 * eps * ds.abs().sum(-1, keepdim=True) + (2 * n + 3) * U32 * T + 64 * U32 * (p * B).sum(-1, keepdim=True)
        dds = (2 * eps + eta + 2 * U32) * ds.abs() + p * (row + 64 * U32 * (1 - 2 * p) * B)
        bq = bq + (dds @ k.abs()) / 8
        bk = bk + (dds.transpose(-1, -2) @ q.abs()) / 8
        bv = bv + ((2 * eps + eta) * p).transpose(-1, -2) @ d.abs()
    bound = torch.cat([_rows(t, N, L, H) for t in (bq, bk, bv)], dim=-1)
    return want, 2 * (bound + U16 * want.abs()) + 2.0 ** -24


WRONG_BACKWARD = ("drop_last", "admit_next", "next_seq", "no_rowsum", "dk_unscaled", "stale_stats", "swap_pair")


def wrong_backward_applies(wrong, N, L, causal):
    if wrong == "drop_last":
        return L >= 2
    if wrong == "admit_next":
        return causal and L >= 2
    if wrong == "next_seq":
        return N >= 2
    if wrong == "stale_stats":
        return not causal and L >= 17          # only the kernel without a mask recomputes P and dS from saved statistics
    if wrong == "swap_pair":
        return L >= 17
    return L >= 2                              # no_rowsum, dk_unscaled: with one key dS, dq and dk are zero either way


def _swap16(t, L):
    """Rows q <-> q ^ 16 (the two 16-row tiles of a 32-row pair); the partner of a row past L is a zero row."""
    idx = torch.arange(L) ^ 16
    out = torch.zeros_like(t)
    ok = idx < L
    out[ok] = t[idx[ok]]
    return out


def emulate_backward(qkv, d_out, N, L, H, causal, wrong=None):
    """The kernels' arithmetic in torch on the CPU: float32 throughout, P = exp(s / 8 - max) * (1 / sum), dS = P (dP - rowsum(dP P)),
    .half() on P and dS in front of their products, one .half() on dqkv -> fp16 [N L, 3 * 64 H].  ``wrong`` makes it wrong in one way, each a
    mistake these kernels could make:
      drop_last    the last key a row may see is dropped: key L-1 (no mask), key q of row q >= 1 (causal);
      admit_next   the causal mask admits key q + 1;
      next_seq     query row 0 of the next sequence of the batch (cyclically) is one more query row in dK and dV (a padding row not zeroed);
      no_rowsum    dS = P dP, without the row-sum term;
      dk_unscaled  the 1 / 8 is missing from dK;
      stale_stats  dK and dV recompute P and dS of query q from the maximum, 1 / sum and row sum of query q + 16 (where that exists);
      swap_pair    the token-row operand of every product is gathered with the two tiles of a 32-row pair swapped (row q ^ 16)."""
    D = 64 * H
    x = qkv.detach().cpu().reshape(N, L, 3, H, 64).float()
    g = d_out.detach().cpu().reshape(N, L, H, 64).float()
    allowed = _allowed(L, L, causal)
    if wrong == "drop_last":
        if causal:
            i = torch.arange(1, L)
            allowed[i, i] = False
        else:
            allowed[:, L - 1] = False
    elif wrong == "admit_next":
        i = torch.arange(0, L - 1)
        allowed[i, i + 1] = True
    out = torch.empty(N, L, 3, H, 64, dtype=torch.float16)
    r16 = lambda t: t.half().float()
    for n in range(N):
        for h in range(H):
            q, k, v, do = x[n, :, 0, h], x[n, :, 1, h], x[n, :, 2, h], g[n, :, h]
            ok = allowed
            if wrong == "next_seq":
                q = torch.cat([q, x[(n + 1) % N, :1, 0, h]])
                do = torch.cat([do, g[(n + 1) % N, :1, h]])
                ok = torch.cat([allowed, torch.ones(1, L, dtype=torch.bool)])
            s = ((q @ k.t()) * 0.125).masked_fill(~ok, float("-inf"))
            m = s.amax(dim=1, keepdim=True)
            e = torch.exp(s - m)
            inv = 1.0 / e.sum(dim=1, keepdim=True)
            p = e * inv
            dp = do @ v.t()
            rs = (p * dp).sum(dim=1, keepdim=True)
            ds = p * dp if wrong == "no_rowsum" else p * (dp - rs)
            p2, ds2 = p, ds
            if wrong == "stale_stats":
                j = torch.arange(L) + 16
                j = torch.where(j < L, j, torch.arange(L))
                p2 = torch.exp(s - m[j]) * inv[j]
                ds2 = p2 * (dp - rs[j])
            kb, qb, dob = k, q, do
            if wrong == "swap_pair":
                kb, qb, dob = _swap16(k, L), _swap16(q, L), _swap16(do, L)
            dq = (r16(ds) @ kb) * 0.125
            dk = r16(ds2).t() @ qb
            if wrong != "dk_unscaled":
                dk = dk * 0.125
            dv = r16(p2).t() @ dob
            out[n, :, 0, h], out[n, :, 1, h], out[n, :, 2, h] = dq[:L].half(), dk.half(), dv.half()
    return out.reshape(N * L, 3 * D)


# ---- random and peaked inputs
# d_out: N(0, 0.5^2) as in the trainers' operator tests; that scaled by 2^-10 (dS moves into fp16's subnormals and the 2^-25 terms carry the
# bound); N(0, 2^-6 ^2) scaled by 2^10 (the larger base would take dS = P (dP - rowsum) past 65504 at qkv scale 3: dP is a sum of 64 products)
DOUT_SCALES = {"1": 0.5, "2^-10": 0.5 * 2.0 ** -10, "2^10": 2.0 ** -6 * 2.0 ** 10}
BCase = namedtuple("BCase", "N L H causal distinct scale dout late")


def backward_batch(case):
    """N sequences built from ``distinct`` different ones in a shuffled order, qkv ~ N(0, scale^2), d_out ~ N(0, DOUT_SCALES[dout]^2);
    ``late``: a common offset on every query and on the keys of the last 16-row tile, so that the rows that see them have their maximum there.
    -> (qkv [N L, 3 D], d_out [N L, D], order, seq_qkv [distinct L, 3 D], seq_d_out [distinct L, D]), fp16."""
    N, L, H, causal, S, scale, dout, late = case
    D = 64 * H
    g = _gen(N, L, H, int(causal), S, int(scale * 10), sorted(DOUT_SCALES).index(dout), int(late), 4242)
    seqs = torch.randn(S, L, 3 * D, generator=g) * scale
    if late:
        seqs[:, :, :D] += 0.75
        seqs[:, (L - 1) // 16 * 16:, D:2 * D] += 1.5          # 64 * 0.75 * 1.5 / 8 = 9 on the score, four of its standard deviations
    seqs = seqs.half()
    do = (torch.randn(S, L, D, generator=g) * DOUT_SCALES[dout]).half()
    order = torch.cat([torch.arange(S), torch.randint(0, S, (N - S,), generator=g)])
    order = order[torch.randperm(N, generator=g)]
    return seqs[order].reshape(N * L, 3 * D), do[order].reshape(N * L, D), order.tolist(), seqs.reshape(S * L, 3 * D), do.reshape(S * L, D)


# both sides of every seam: 16-row tiles, the 32-row k-steps of the causal kernel's phase B and its 96 zeroed rows behind L = 80; without a
# mask NT odd against even (the padding tile of NTP live at 33..48, 65..80, 97..112, 193..208) and NT no multiple of the four waves
BACKWARD_LENGTHS = {True: (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 77, 79, 80),
                    False: (1, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 96, 97, 112, 113, 197, 205, 207, 208, 209, 223, 224)}
BACKWARD_SEAMS = {True: (17, 33, 64, 77, 80), False: (17, 49, 113, 197, 224)}          # the H and N sweep, the d_out scales
BACKWARD_ISOLATION = {True: (17, 33, 77, 80), False: (17, 33, 197, 209, 224)}
BACKWARD_SHAPES = ((1, 1), (1, 8), (3, 1), (3, 12))                                     # (N, H) of the sweep; (3, 2) is the shape of every length
BACKWARD_WIDE = {True: (37, 8, 77), False: (37, 8, 197)}                                 # N H = 296 items: wider than the device once


def _backward_cases():
    flat, peaked = [], []
    for causal in (True, False):
        for L in BACKWARD_LENGTHS[causal]:
            flat.append(BCase(3, L, 2, causal, 2, 0.7, "1", False))
            peaked += [BCase(3, L, 2, causal, 2, 1.5, "1", False), BCase(3, L, 2, causal, 2, 3.0, "1", False), BCase(3, L, 2, causal, 2, 1.5, "1", True)]
        for L in BACKWARD_SEAMS[causal]:
            flat += [BCase(N, L, H, causal, min(N, 2), 0.7, "1", False) for N, H in BACKWARD_SHAPES]
            peaked += [BCase(1, L, 2, causal, 1, s, d, s == 1.5) for s in (1.5, 3.0) for d in ("2^10", "2^-10")]
        N, H, L = BACKWARD_WIDE[causal]
        flat.append(BCase(N, L, H, causal, 3, 0.7, "1", False))
    return flat, peaked


BACKWARD_RANDOM, BACKWARD_PEAKED = _backward_cases()


# ---- constructed: selection
def selection_backward_batch(N, L, H, kind):
    """Q and K of ``selection_batch``: the target pi(q) leads every other key of row q by 64 natural units, so P16 is exactly one-hot.
    V holds integers of -3..3 and d_out integers of -8..8, so every dP is an exact integer in fp32: at the target rowsum(dP o P) == dP and dS
    is exactly zero; everywhere else p < e^-64 and |dP - rowsum| < 2^25, so dS < 2^-67 flushes to zero in fp16.  Hence dq == 0 and dk == 0 in
    every element, and dv[j] = sum over the queries with pi(q) = j of d_out[q]: at most 224 integers of magnitude <= 8, exact in fp32 and,
    below 2048, in fp16.  kind "perm": pi is a permutation, dv is a row permutation of d_out bit for bit, and d_out instead holds fp16 values
    with random sign, exponent 1..30 and mantissa (dP is then no integer, but the target's dS is the difference of a value and itself, and
    the others' |dP - rowsum| < 2^25 still).  -> (qkv fp16 [N L, 3 D], d_out fp16 [N L, D], dv fp16 [N L, D], pi [N, H, L])."""
    qkv, _, pis = selection_batch(N, L, H, kind)
    g = _gen(N, L, H, sorted(sum(SELECT_KINDS.values(), ())).index(kind), 78)
    D = 64 * H
    qkv = qkv.reshape(N, L, 3, H, 64).clone()
    qkv[:, :, 2] = torch.randint(-3, 4, (N, L, H, 64), generator=g).half()
    if kind == "perm":
        b = (torch.randint(0, 2, (N, L, H, 64), generator=g) << 15) | (torch.randint(1, 31, (N, L, H, 64), generator=g) << 10) | \
            torch.randint(0, 1024, (N, L, H, 64), generator=g)
        do = torch.from_numpy(b.numpy().astype(np.uint16).view(np.float16).copy())
    else:
        do = torch.randint(-8, 9, (N, L, H, 64), generator=g).half()
    dv = torch.zeros(N, L, H, 64, dtype=torch.float64)
    for n in range(N):
        for h in range(H):
            dv[n, :, h].index_add_(0, pis[n, h], do[n, :, h].double())
    assert dv.abs().max() <= (65504 if kind == "perm" else 2048)
    return qkv.reshape(N * L, 3 * D), do.reshape(N * L, D), dv.half().reshape(N * L, D), pis


# ---- constructed: uniform
def uniform_backward_batch(N, L, H, causal):
    """q == 0: every allowed key of row q has the probability fp32(1 / n_q), n_q the number of its allowed keys (q + 1 under the causal mask);
    K and V are random, d_out holds integers of -8..8.  dk = dS^T q is exactly zero; dv[j] = sum over the queries that may see key j of
    fp16(fp32(1 / n_q)) d_out[q], every (query, key) pair counted once; dq is an ordinary result (``attention_backward``).
    -> (qkv fp16, d_out fp16, dv float64 [N L, D], dv_tol float64).  dv_tol per element:
        u16 |dv|                    the one rounding of the output to fp16,
        2^-20 sum_q P16 |d_out|     the fp32 sum: at most 224 terms summed in k-steps of 32 and a chain of 7, < 16 roundings of 2^-24 each,
        2^-25                       half a subnormal step of the output."""
    g = _gen(N, L, H, int(causal), 98)
    D = 64 * H
    qkv = torch.zeros(N, L, 3, D)
    qkv[:, :, 1] = torch.randn(N, L, D, generator=g) * 1.5
    qkv[:, :, 2] = torch.randn(N, L, D, generator=g)
    do = torch.randint(-8, 9, (N, L, D), generator=g).double()
    allowed = _allowed(L, L, causal).double()
    n_q = allowed.sum(dim=1)
    p16 = (1.0 / n_q.float()).half().double()[:, None] * allowed                      # [q, key]
    dv = torch.einsum("qk,nqd->nkd", p16, do)
    tol = U16 * dv.abs() + 2.0 ** -20 * torch.einsum("qk,nqd->nkd", p16, do.abs()) + 2.0 ** -25
    return qkv.half().reshape(N * L, 3 * D), do.half().reshape(N * L, D), dv.reshape(N * L, D), tol.reshape(N * L, D)


BACKWARD_CONSTRUCTED_SHAPE = (3, 2)          # (N, H) of the selection and uniform batches


def poison_one(d_out, N, L, H, n, r, h, value):
    """d_out with ``value`` in one element of row r, head h of item n."""
    out = d_out.clone().reshape(N, L, H, 64)
    out[n, r, h, 5] = value
    return out.reshape(N * L, 64 * H)
