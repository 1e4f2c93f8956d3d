"""Plain references for the calibration tail (csrc/logits.hip, csrc/knn.hip, l2norm_kernel of csrc/elementwise.hip): float64 evaluations
that return (want, tol) with a PER-ELEMENT tolerance derived from the arithmetic the kernel headers document, a CPU emulation of that
arithmetic in torch float32 / float16 (tests/test_tail_ref_cpu.py holds it inside the same tolerances, and against every constructed
expectation exactly), and the case lists the CPU and the GPU tests share.  No GPU, no project kernel, nothing taken from a GPU output.

Notation: u = 2^-24, the unit roundoff of fp32.  Every bound is first order in u; MARGIN covers the second-order terms."""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
MARGIN = 1.0 + 2.0 ** -4        # over the first-order terms: products of two roundings (< E u^2 relative) and the float64 reference's own error
                                # (< E 2^-53) are below 2^-10 of any bound here; 1/16 is taken so that nothing hangs on that estimate
F16_SUB = 2.0 ** -24            # spacing of fp16 subnormals; 2^-14 is the smallest normal


def _gen(*key):
    seed = 17
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ---- L2 normalisation ------------------------------------------------------------------------------------------------------------------------
def _norm_rel(E):
    """Relative error of one normalised component, in units of u.  l2norm_kernel (and phase 0 of the fused tail, same order): a lane adds
    n squares with fused multiply-adds (n = 8 ceil(E / 512) for E % 8 == 0, else ceil(E / 64)), then 6 butterfly additions: all terms
    positive, so ss carries at most (n + 6) u relative, its square root half of that; sqrtf, the division and the product x * inv add one
    correctly rounded operation each (1 u); 2 u more are allowed for a sqrtf / division that is within 1 ulp instead of 1/2."""
    n = 8 * math.ceil(E / 512) if E % 8 == 0 else math.ceil(E / 64)
    return (n + 6) / 2 + 3 + 2


def l2_normalize(x, out_dtype=torch.float32):
    """x [rows, E] fp32 or fp16 -> (x / ||x|| in float64, tol).  fp16 output: one more rounding, 2^-11 relative or half a subnormal step."""
    x64 = x.double()
    want = x64 / x64.norm(dim=-1, keepdim=True)
    tol = _norm_rel(x.shape[1]) * U * want.abs()
    if out_dtype == torch.float16:
        tol = tol + torch.maximum(2.0 ** -11 * want.abs(), torch.tensor(F16_SUB / 2, dtype=torch.float64))
    return want, tol * MARGIN


# ---- scaled cosine logits --------------------------------------------------------------------------------------------------------------------
def _split_residual(x):
    """|x - hi - lo| of split8 for |x| <= 1: hi = fp16(x) leaves |x - hi| <= 2^-11 |x| (exact in fp32), lo = fp16(x - hi) leaves 2^-11 of that
    where lo is a normal fp16 number -- 2^-22 |x| -- and half a subnormal step, 2^-25, where it is not.  |x - hi| < 2^-14 is the rule for
    unit-norm features (every |x| < 2^-3), so the floor applies to nearly every operand, not only to those below 2^-14: for those hi is itself
    subnormal and the same 2^-25 holds.  x == 0 splits exactly.  This assumes fp16 subnormals are honoured by the conversions and by the matrix
    instruction; the small-component cases are there to find out."""
    a = x.abs()
    return torch.where(a == 0, a, torch.maximum(2.0 ** -22 * a, torch.tensor(2.0 ** -25, dtype=a.dtype)))


def n_mfma(E):
    return 3 * (E // 32) + (4 if E % 32 else 0)     # three 16x16x32 f16 per 32-wide step; E % 32 == 16: four exact 16x16x4 f32


def cosine_logits(img, txt_n, scale, normalize):
    """float64 scale32 * normalise(img) . txt_n (the text rows as given) -> (want [B, C], tol [B, C], img_n64).  With a = img_n, b = txt_n,
    S = sum |a_i b_i|:
      normalisation   _norm_rel(E) u S                          (normalize only; an fp16 row converts to fp32 exactly)
      split           sum_i r(a_i) |b_i| + |a_i| r(b_i) + |lo_a lo_b|,  r = _split_residual, |lo| <= 2^-11 |x| + 2^-25 (the dropped term)
      accumulation    (n_mfma + 5) 2^-23 S: every matrix instruction rounds acc + its block once, and its 32 products are summed inside by
                      a tree of depth 5; 2^-23 instead of u because the matrix pipe is not documented to round to nearest
      scale * acc     u |want|
    all times |scale|, times MARGIN."""
    s32 = float(np.float32(scale))
    a = img.double()
    if normalize:
        a = a / a.norm(dim=-1, keepdim=True)
    b = txt_n.double()
    E = a.shape[1]
    dot = a @ b.t()
    aa, ab = a.abs(), b.abs()
    S = aa @ ab.t()
    ra, rb = _split_residual(a), _split_residual(b)
    la, lb = 2.0 ** -11 * aa + 2.0 ** -25 * (aa != 0), 2.0 ** -11 * ab + 2.0 ** -25 * (ab != 0)
    err = ra @ ab.t() + aa @ rb.t() + la @ lb.t() + (n_mfma(E) + 5) * 2.0 ** -23 * S
    if normalize:
        err = err + _norm_rel(E) * U * S
    want = s32 * dot
    return want, (abs(s32) * err + U * want.abs()) * MARGIN, a


def top2_gap(want):
    """float64 logits -> (argmax with the lowest index, top-1 minus top-2 per row; inf for one class)."""
    if want.shape[1] == 1:
        return torch.zeros(want.shape[0], dtype=torch.int64), torch.full((want.shape[0],), float("inf"), dtype=torch.float64)
    v, i = torch.topk(want, 2, dim=1)
    return want.argmax(dim=1), v[:, 0] - v[:, 1]


def dac_scale(want, tol, dac, pred):
    """DAC row scale x * f, f = dac[pred] > 0: the bound scales with f and takes one more rounding, u |x f|."""
    f = dac.double()[pred.long()][:, None]
    return want * f, (tol * f + U * (want * f).abs()) * MARGIN


# ---- softmax top-1 ---------------------------------------------------------------------------------------------------------------------------
def softmax_top1(logits):
    """The float64 softmax of the logits THE KERNEL RETURNED (logit error and row-pass error are judged apart) ->
    (conf [B], pred [B] lowest-index argmax, tol_conf [B], probs [B, C], tol_probs [B, C]).
    conf = 1 / sum_c e_c, e_c = exp(x_c - M).  Relative error of a term, d = |x_c - M|: the subtraction rounds once (u d absolute in the
    exponent = u d relative in e_c), __expf is exp2(x log2 e): the product rounds once (u d), log2 e is off by <= u / 2 relative (u d / 2,
    taken as u d), v_exp_f32 is within 1 ulp (2 u): (2 + 3 d) u.  The blockwise form writes e_c = exp(x_c - m_t) exp(m_t - M): the d of the
    two factors add up to the same d, and the second exponential and the product add 2 u + 1 u: (5 + 3 d) u covers both forms.  The relative
    error of the sum is the p-weighted mean of the terms' plus the additions: 6 (wave tree) + ceil(C / 64) (a lane's column loop or the
    block merge) roundings of positive terms, 1 u each; the division 1 / sum: 1 u, 2 u allowed.  A term may be flushed to zero below 2^-126:
    C 2^-126 absolute.  probs: one more exponential and product, (3 + 3 d) u."""
    x = logits.double()
    M, pred = x.max(dim=1, keepdim=True).values, x.argmax(dim=1)
    d = (M - x)
    e = torch.exp(-d)
    s = e.sum(dim=1, keepdim=True)
    p = e / s
    C = x.shape[1]
    rel = ((p * (5 + 3 * d)).sum(dim=1) + 6 + math.ceil(C / 64) + 2) * U
    conf = 1.0 / s[:, 0]
    tol_conf = (rel * conf + C * 2.0 ** -126) * MARGIN
    tol_probs = ((rel[:, None] + (3 + 3 * d) * U) * p + 2.0 ** -126) * MARGIN
    return conf, pred, tol_conf, p, tol_probs


# ---- ECE bins --------------------------------------------------------------------------------------------------------------------------------
def bin_statistics(conf, pred, labels, n_bins):
    """float64 [3, n_bins + 1] = count | sum conf | sum correct per bin np.digitize(conf, linspace(0, 1, n_bins + 1)) - 1 (tools/metrics.py:90-130):
    conf == 1.0 and NaN land in bin n_bins."""
    conf = np.asarray(conf, dtype=np.float64)
    which = np.digitize(conf, np.linspace(0, 1, n_bins + 1)) - 1
    which = np.clip(which, 0, n_bins)            # conf < 0 does not occur (a softmax maximum); the kernel clamps it into bin 0
    out = np.zeros((3, n_bins + 1))
    np.add.at(out[0], which, 1.0)
    np.add.at(out[1], which, conf)
    np.add.at(out[2], which, (np.asarray(pred).astype(np.int64) == np.asarray(labels).astype(np.int64)).astype(np.float64))
    return out


def bin_sum_rtol(n):
    """The confidence sums are n double additions of non-negative numbers in whatever order the atomics land, against np.add.at's order:
    each side is within (n - 1) 2^-53 relative of the exact sum."""
    return 2.0 * max(n, 1) * 2.0 ** -53


def assert_bins(got, want, n, what):
    got, want = np.asarray(got).reshape(3, -1), np.asarray(want).reshape(3, -1)
    assert np.array_equal(got[0], want[0]), f"{what}: counts {got[0].tolist()} != {want[0].tolist()}"
    assert np.array_equal(got[2], want[2]), f"{what}: hits {got[2].tolist()} != {want[2].tolist()}"
    fin = np.isfinite(want[1])
    assert np.array_equal(np.isnan(got[1]), np.isnan(want[1])), f"{what}: NaN confidence sums in other bins than the reference's"
    assert (np.abs(got[1][fin] - want[1][fin]) <= bin_sum_rtol(n) * np.abs(want[1][fin])).all(), f"{what}: confidence sums {got[1].tolist()} != {want[1].tolist()}"


# ---- kNN -------------------------------------------------------------------------------------------------------------------------------------
def knn(q, refs, K):
    """Brute force in float64: the K smallest L2 distances per query, ascending, NaN last (a reference row with a NaN is never a neighbour),
    multiplicities kept -> (want [Nq, K], tol).  Kernel: a = q_e - r_e rounds once (u relative), fmaf(a, a, d) over E terms: a^2 carries 2 u and
    the chain of E additions of positive terms E u, so d^2 is within (E + 2) u relative, its root within half of that, sqrtf 1 u (2 u
    allowed): every distance is within rel = ((E + 2) / 2 + 2) u of its float64 value.  Order statistics: if every d_i moves by at most
    rel d_i, the k-th smallest of the moved values lies within rel of the k-th smallest of the true ones (at least k moved values are
    <= (1 + rel) want_k, and at most k - 1 are < (1 - rel) want_k), so the bound holds for the sorted output whatever rows swap places."""
    d = (q.double()[:, None, :] - refs.double()[None, :, :]).norm(dim=2)
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    want = torch.sort(d, dim=1).values[:, :K]
    return want, ((refs.shape[1] + 2) / 2 + 2) * U * want * MARGIN


# ---- CPU emulation of the documented arithmetic -------------------------------------------------------------------------------------------------
WRONG = ("skip_kstep", "tie_high", "edge_low", "drop_dup")     # one deliberate fault per class (tests/test_tail_ref_cpu.py docstring)


def f32(t):
    return t.double().float()


def split8(x):
    """x fp32 -> (hi, lo) fp16: hi = fp16(x), lo = fp16(x - hi)."""
    hi = x.half()
    return hi, (x - hi.float()).half()


def emulate_normalize(x):
    """l2norm_kernel / phase 0: per-lane fused multiply-adds over its chunks in ascending order, xor butterfly 32..1, 1 / sqrtf, x * inv (fp32)."""
    x = x.float()
    rows, E = x.shape
    if E % 8 == 0:
        nch = E // 8
        pad = (-nch) % 64
        xc = torch.cat([x.reshape(rows, nch, 8), torch.zeros(rows, pad, 8)], dim=1).reshape(rows, -1, 64, 8)     # [rows, stripe, lane, e]
        seq = xc.permute(0, 2, 1, 3).reshape(rows, 64, -1)                                                         # a lane's elements in its order
    else:
        pad = (-E) % 64
        seq = torch.cat([x, torch.zeros(rows, pad)], dim=1).reshape(rows, -1, 64).permute(0, 2, 1)
    ss = torch.zeros(rows, 64)
    for i in range(seq.shape[2]):
        v = seq[:, :, i].double()
        ss = (v * v + ss.double()).float()                # fmaf: v * v is exact in float64
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        ss = ss + ss[:, lanes ^ o]
    inv = 1.0 / torch.sqrt(ss[:, :1])
    return x * inv


def emulate_logits(img_n, txt_n, scale, wrong=None):
    """acc += hi_a . hi_b; acc += hi_a . lo_b; acc += lo_a . hi_b per 32-wide k-step, every matrix instruction = one fp32 rounding of acc + its
    exact block sum; E % 32 == 16: four exact-f32 16x16x4 steps, instruction e taking k = k0 + 4 g + e, g = 0..3; logits = scale * acc."""
    a, b = img_n.float(), txt_n.float()
    E = a.shape[1]
    ah, al = (t.double() for t in split8(a))
    bh, bl = (t.double() for t in split8(b))
    acc = torch.zeros(a.shape[0], b.shape[0])
    steps = E // 32
    for s in range(steps):
        if wrong == "skip_kstep" and s == steps - 1:
            continue
        k = slice(32 * s, 32 * s + 32)
        for x, y in ((ah, bh), (ah, bl), (al, bh)):
            acc = (acc.double() + x[:, k] @ y[:, k].t()).float()
    if E % 32:
        k0 = 32 * steps
        for e in range(4):
            idx = torch.tensor([k0 + 4 * g + e for g in range(4)])
            acc = (acc.double() + a.double()[:, idx] @ b.double()[:, idx].t()).float()
    return torch.tensor(float(np.float32(scale))) * acc


def _tree_sum(v):
    """wave_sum: quad_perm xor 1, xor 2, row_half_mirror, row_mirror, row swap, half swap = a binary tree over adjacent lanes; v [..., 64] fp32."""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _first_max(v, idx, wrong):
    """(value, index) pairs along the last axis -> the largest value and the LOWEST index that holds it (wave_argmax)."""
    m = v.max(dim=-1, keepdim=True).values
    cand = torch.where(v == m, idx, torch.full_like(idx, -1 if wrong == "tie_high" else 0x7FFFFFFF))
    return m[..., 0], (cand.max(dim=-1).values if wrong == "tie_high" else cand.min(dim=-1).values)


def emulate_rows(logits, dac=None, wrong=None):
    """calibrate_row in fp32 -> (logits after the DAC scale, conf, pred, probs).  No DAC: per 64-column block (max, lowest argmax, tree sum of
    exp(x - m_t)), merged in ascending block order: the first maximum wins, sum = fmaf(s_t, exp(m_t - M), sum).  DAC: lane-strided argmax
    (first occurrence inside a lane, lowest index across lanes), f = dac[pred], lane-strided sum of exp(x f - M f), tree."""
    x = logits.float()
    B, C = x.shape
    nt = (C + 63) // 64
    pad = nt * 64 - C
    xp = torch.cat([x, torch.full((B, pad), float("-inf"))], dim=1).reshape(B, nt, 64)
    col = torch.arange(nt * 64, dtype=torch.int64).reshape(1, nt, 64).expand(B, nt, 64)
    col = torch.where(col < C, col, torch.full_like(col, 0x7FFFFFFF))
    if dac is None:
        m_t, a_t = _first_max(xp, col, wrong)                                   # [B, nt]
        live = (col != 0x7FFFFFFF) & (m_t[..., None] != float("-inf"))
        s_t = _tree_sum(torch.where(live, torch.exp(xp - m_t[..., None]), torch.zeros(())))
        M = torch.full((B,), float("-inf"))
        arg = torch.full((B,), 0x7FFFFFFF, dtype=torch.int64)
        for t in range(nt):
            take = (m_t[:, t] >= M) if wrong == "tie_high" else (m_t[:, t] > M)
            M, arg = torch.where(take, m_t[:, t], M), torch.where(take, a_t[:, t], arg)
        arg = torch.where(arg == 0x7FFFFFFF, torch.zeros_like(arg), arg)
        s = torch.zeros(B)
        for t in range(nt):
            s = (s_t[:, t].double() * torch.exp(m_t[:, t] - M).double() + s.double()).float()
        probs = torch.exp(x - M[:, None]) * (1.0 / s)[:, None]
        return x, 1.0 / s, arg.int(), probs
    lane_v = xp.permute(0, 2, 1)                                                # [B, lane, t]: a lane's columns in ascending order
    lane_c = col.permute(0, 2, 1)
    best, bi = _first_max(lane_v, lane_c, wrong)                                # inside a lane
    M, arg = _first_max(best, bi, wrong)                                        # across lanes
    arg = torch.where(arg == 0x7FFFFFFF, torch.zeros_like(arg), arg)
    f = dac.float()[arg]
    v = x * f[:, None]
    mx = M * f
    e = torch.cat([torch.exp(v - mx[:, None]), torch.zeros(B, pad)], dim=1).reshape(B, nt, 64)
    se = torch.zeros(B, 64)
    for t in range(nt):
        se = se + e[:, t]
    s = _tree_sum(se)
    probs = torch.exp(v - mx[:, None]) * (1.0 / s)[:, None]
    return v, 1.0 / s, arg.int(), probs


def emulate_ece_bin(conf, n_bins, wrong=None):
    """ece_bin of logits.hip in float64: floor(x n) clamped, moved until edge(b) <= x < edge(b + 1) with edge(k) = k (1 / n) and edge(n) = 1.0;
    x >= 1.0 or NaN -> bin n_bins."""
    x = np.asarray(conf, dtype=np.float64)
    step = 1.0 / n_bins
    edge = lambda k: np.where(k >= n_bins, 1.0, k * step)     # noqa: E731
    with np.errstate(invalid="ignore"):
        b = np.clip(np.nan_to_num(np.floor(x * n_bins), nan=0.0), 0, n_bins).astype(np.int64)
        for _ in range(3):
            if wrong == "edge_low":
                b = np.where((b < n_bins) & (edge(b + 1) < x), b + 1, b)
                b = np.where((b > 0) & (edge(b) >= x), b - 1, b)
            else:
                b = np.where((b < n_bins) & (edge(b + 1) <= x), b + 1, b)
                b = np.where((b > 0) & (edge(b) > x), b - 1, b)
        b = np.where(~(x < 1.0), n_bins, b)
    return b


def emulate_bins(conf, pred, labels, n_bins, wrong=None):
    b = emulate_ece_bin(conf, n_bins, wrong)
    out = np.zeros((3, n_bins + 1))
    np.add.at(out[0], b, 1.0)
    np.add.at(out[1], b, np.asarray(conf, dtype=np.float64))
    np.add.at(out[2], b, (np.asarray(labels).astype(np.int64) == np.asarray(pred).astype(np.int64)).astype(np.float64))
    return out


def emulate_knn(q, refs, K, wrong=None):
    """knn_kernel: d = fmaf(q_e - r_e, q_e - r_e, d) over e ascending (fp32); lane r & 63 keeps a sorted list of its K smallest (a NaN distance
    enters as +inf), rows in ascending order; K rounds of "take the smallest head, lowest lane on ties" over the 64 lists; sqrtf."""
    q, refs = q.float(), refs.float()
    Nq, Nr = q.shape[0], refs.shape[0]
    d = torch.zeros(Nq, Nr)
    for e in range(q.shape[1]):
        a = (q[:, e, None] - refs[None, :, e]).double()
        d = (a * a + d.double()).float()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d).numpy()
    out = np.empty((Nq, K), dtype=np.float32)
    for i in range(Nq):
        lists = [[] for _ in range(64)]
        for r in range(Nr):                                   # sorted insertion, depth K
            lst = lists[r & 63]
            v = d[i, r]
            for k in range(len(lst)):
                if v < lst[k]:
                    lst[k], v = v, lst[k]
            if len(lst) < K:
                lst.append(v)
        head = [0] * 64
        for k in range(K):
            m, ml = np.float32(np.inf), 0
            for lane in range(64):
                v = lists[lane][head[lane]] if head[lane] < len(lists[lane]) else np.float32(np.inf)
                if v < m:
                    m, ml = v, lane
            if wrong == "drop_dup":
                for lane in range(64):
                    while head[lane] < len(lists[lane]) and lists[lane][head[lane]] == m:
                        head[lane] += 1
            else:
                head[ml] += 1
            out[i, k] = np.sqrt(np.float32(m))
    return torch.from_numpy(out)


def worst_ratio(got, want, tol):
    r = (got.reshape(want.shape).double() - want).abs() / tol
    r[torch.isnan(r)] = float("inf")
    return float(r.max()) if r.numel() else 0.0


def fp32_steps_from_nearest(got, exact):
    """How many fp32 values lie between got and the fp32 value nearest to the float64 `exact` (0 = the nearest itself)."""
    near = exact.double().float()
    o = lambda t: torch.where(t.view(torch.int32) < 0, -(t.view(torch.int32) & 0x7FFFFFFF), t.view(torch.int32)).long()   # noqa: E731
    return (o(got.float().contiguous().reshape(near.shape)) - o(near.contiguous())).abs()


# ---- cases: random -----------------------------------------------------------------------------------------------------------------------------
# (B, C, E, seed): the seed is CHOSEN so that no row's float64 top-2 gap is under twice the logit tolerance at either scale, with and without
# normalisation and for fp32 and fp16 image features (tests/test_tail_ref_cpu.py::test_seeds_leave_no_ambiguous_argmax asserts it): the GPU tests
# can then ask for pred == the reference argmax at every row.
FUSED_SHAPES = [
    (1, 1, 64, 0),
    (17, 65, 64, 0),          # two column blocks, the second with one live column
    (16, 199, 128, 0),        # C % 4 != 0: 4-byte stores, the release fence with DAC
    (513, 65, 64, 0),         # RB = 32, last row block of one row
    (33, 1025, 64, 0),        # 17 partials per row: the 16-partial chunking; the DAC pass with C > 1024
    (5, 2049, 64, 0),         # 33 partials
    (9, 70, 1088, 0),         # E > 1024: the nch > 128 branch of phase 0
    (256, 1000, 512, 0),      # workload-like
]
LOGITS_SHAPES = [(20, 40, 48, 0), (20, 40, 80, 0), (5, 3, 16, 0)]      # clipmi_logits: split steps + the exact-f32 tail step; the tail step alone
SCALES = (100.0, 1.0)                                                # exp(logit_scale) of CLIP; TempScaling's base models use 1.0
DTYPES = (torch.float32, torch.float16)
N_BINS = 15


@functools.lru_cache(maxsize=None)
def random_inputs(B, C, E, seed, dtype, normalize):
    """-> (img [B, E] dtype, txt_n [C, E] fp32 unit rows, dac [C] fp32 in [0.5, 1.5], labels [B] int64).  normalize: raw features of norm ~ 3 sqrt(E);
    otherwise rows normalised in float64 and rounded once to dtype."""
    g = _gen(B, C, E, seed, 7)
    img = torch.randn(B, E, generator=g, dtype=torch.float64) * 3.0
    txt = torch.randn(C, E, generator=g, dtype=torch.float64)
    if not normalize:
        img = img / img.norm(dim=1, keepdim=True)
    txt_n = (txt / txt.norm(dim=1, keepdim=True)).float()
    dac = (torch.rand(C, generator=g) + 0.5).float()
    labels = torch.randint(0, C, (B,), generator=g)
    return img.to(dtype), txt_n, dac, labels


@functools.lru_cache(maxsize=None)
def random_reference(B, C, E, seed, dtype, normalize, scale):
    img, txt_n, dac, labels = random_inputs(B, C, E, seed, dtype, normalize)
    want, tol, img_n = cosine_logits(img, txt_n, scale, normalize)
    pred, gap = top2_gap(want)
    return want, tol, img_n, pred, gap


# ---- cases: small components -------------------------------------------------------------------------------------------------------------------
SMALL_E, SMALL_ROWS, SMALL_BLOCK = 64, 24, 16


def small_component_rows(mirror):
    """-> (img_n [24, 64], txt_n [24, 64]) fp32, unit rows up to rounding.  Components 0..15 of every row of the SMALL side lie in [2^-27, 2^-14):
    exact fp16 subnormals k 2^-24, values between two of them, values below 2^-24 and below 2^-25 (hi = 0: they survive only through lo, or not
    at all: that is inside the 2^-25 floor), and the largest fp16 subnormal; the FACING side has one component of 0.7 among its first 16
    (row c: component c % 16) and nothing else there; components 16..63 carry the rest of both norms.  If a subnormal operand half were flushed,
    logit[b, c] would lose up to 100 * 0.7 * 2^-14 = 4e-3 where its tolerance is ~1e-4."""
    g = _gen(64, 24, int(mirror))
    n, E, k = SMALL_ROWS, SMALL_E, SMALL_BLOCK
    small = torch.zeros(n, E, dtype=torch.float64)
    mant = torch.rand(n, k, generator=g, dtype=torch.float64) + 1.0
    expo = torch.randint(-24, -14, (n, k), generator=g).double()
    small[:, :k] = mant * 2.0 ** expo * (torch.randint(0, 2, (n, k), generator=g) * 2 - 1)
    small[0, :k] = torch.arange(1, k + 1).double() * 2.0 ** -24                       # exact subnormals
    small[1, :k] = (torch.arange(1, k + 1).double() + 0.5) * 2.0 ** -24               # ties between two subnormals
    small[2, :k] = 2.0 ** -24 * torch.tensor([0.25, 0.49, 0.5, 0.51, 0.75, 0.99, 1.01, 1.49] * 2).double()
    small[3, :k] = 1023 * 2.0 ** -24                                                  # the largest subnormal
    small[4, :k] = 2.0 ** -14 * (1 - 2.0 ** -12)                                      # rounds up to the smallest normal
    rest = torch.randn(n, E - k, generator=g, dtype=torch.float64)
    small[:, k:] = rest / rest.norm(dim=1, keepdim=True)                              # the block adds < 2^-24 to the squared norm
    facing = torch.zeros(n, E, dtype=torch.float64)
    facing[torch.arange(n), torch.arange(n) % k] = 0.7
    rest = torch.randn(n, E - k, generator=g, dtype=torch.float64)
    facing[:, k:] = rest / rest.norm(dim=1, keepdim=True) * math.sqrt(1 - 0.49)
    return (facing.float(), small.float()) if mirror else (small.float(), facing.float())


# ---- cases: exact ------------------------------------------------------------------------------------------------------------------------------
ONE_HOT = [(64, 65, True), (1088, 65, True), (80, 65, False)]        # (E, C, fused entry); B = E: j walks every column once


def one_hot_case(E, C, normalize):
    """img[b] = 4 e_b (norm 4, inverse 0.25: exact) or e_b; txt[c, j] = small integers / 64, exact in fp16 (lo = 0) -> logits[b, c] ==
    fp32(scale) * txt[c, b], every other product of the sum being an exact zero."""
    g = _gen(E, C, 11)
    txt = torch.randint(-63, 64, (C, E), generator=g).float() / 64.0
    txt = torch.where(txt == 0, torch.full_like(txt, 1.0 / 64), txt)          # no zeros: a dropped product always shows
    img = torch.eye(E) * (4.0 if normalize else 1.0)
    return img, txt


def one_hot_want(txt, scale):
    return (torch.tensor(float(np.float32(scale))) * txt.float()).t().contiguous()


# (B, C, columns that hold the row maximum): inside one 64-block, blocks 0 and 1, three-fold, blocks 0 and 17 (two chunks of 16 partials)
TIES = [(20, 130, (3, 40)), (20, 130, (7, 64 + 7)), (20, 130, (5, 60, 129)), (7, 1100, (9, 17 * 64 + 9)), (7, 1100, (64, 128, 1099)),
        (530, 70, (2, 66))]                                                    # B > 512: RB = 32
TIES_E = 64


def ties_case(B, C, cols):
    """Text row `cols[0]` is copied to the other columns of `cols` and every image row is pulled towards it, so the row maximum (by a wide
    margin) sits at exactly those columns with identical bits."""
    g = _gen(B, C, *cols)
    txt = torch.randn(C, TIES_E, generator=g, dtype=torch.float64)
    txt = (txt / txt.norm(dim=1, keepdim=True)).float()
    for c in cols[1:]:
        txt[c] = txt[cols[0]]
    img = torch.randn(B, TIES_E, generator=g, dtype=torch.float64) * 0.5 + 4.0 * txt[cols[0]].double()
    return img.float(), txt


UNIFORM_C = (2, 5, 10, 64, 65, 1025)


def uniform_case(C, B=5, E=64):
    g = _gen(C, 13)
    row = torch.randn(E, generator=g, dtype=torch.float64)
    txt = (row / row.norm()).float().repeat(C, 1)
    img = torch.randn(B, E, generator=g).float()
    return img, txt


def poison_rows(t, g):
    """t filled with NaN, +inf and -inf."""
    sel = torch.randint(0, 3, t.shape, generator=g)
    vals = torch.tensor([float("nan"), float("inf"), float("-inf")])
    return vals[sel].to(t.dtype)


# ---- cases: ECE ----------------------------------------------------------------------------------------------------------------------------------
ECE_N_BINS = (1, 2, 3, 7, 10, 15, 16, 100, 1024)
ECE_SIZES = (1, 255, 256, 257, 262144 + 257)            # one block more or less; the grid-stride second lap (1024 blocks of 256)


def ece_edge_conf(n_bins):
    """fp32 confidences just below, at and just above every fp32-rounded edge of linspace(0, 1, n_bins + 1), and 0.0, -0.0, the smallest
    subnormal, nextafter(1, 0), 1.0."""
    e = np.linspace(0, 1, n_bins + 1).astype(np.float32)
    lo, hi = np.nextafter(e, np.float32(-1)), np.nextafter(e, np.float32(2))
    v = np.concatenate([lo[1:], e, hi[:-1], np.array([0.0, -0.0, 1e-45, np.nextafter(np.float32(1), np.float32(0)), 1.0], dtype=np.float32)])
    return v.astype(np.float32)


def ece_case(n_bins, n=None):
    """-> conf fp32 [n], pred int32 [n], labels int64 [n]: a third hits, the others -1, 2^32 + pred (equal in the low 32 bits) and pred + 1."""
    v = ece_edge_conf(n_bins)
    n = n or v.size
    g = np.random.default_rng(n_bins * 7 + n)
    conf = v[g.permutation(max(n, v.size))[:n] % v.size] if n >= v.size else v[g.permutation(v.size)[:n]]
    pred = g.integers(0, 1000, size=n).astype(np.int32)
    kind = g.integers(0, 4, size=n)
    labels = np.where(kind == 0, pred.astype(np.int64), np.where(kind == 1, -1, np.where(kind == 2, (1 << 32) + pred.astype(np.int64), pred.astype(np.int64) + 1)))
    return conf, pred, labels.astype(np.int64)


# ---- cases: kNN ----------------------------------------------------------------------------------------------------------------------------------
KNN_NR, KNN_NQ, KNN_E = (1, 16, 63, 64, 65, 130), (1, 7, 8, 9), (64, 128)
KNN_PLACEMENTS = ("one_lane", "one_per_lane", "last_tile", "seams", "duplicates")
KNN_DEEP = (64 * 16 + 1, 9, 16, 64)                     # 17 rows in lane 0: "one_lane" at the full list depth KMAX = 16


def knn_ks(Nr):
    return sorted({k for k in (1, 5, 16, Nr) if k <= min(16, Nr)})


def knn_lattice(Nr, Nq, K, E, placement):
    """Integer coordinates: query i = i e_1, K chosen reference rows m e_2 at distances m = 1, 2, 3, ... from query 0 (perfect squares
    1, 4, 9, ...; sqrt(i^2 + m^2) from query i), every other row 40 away or more; every squared distance is an exact fp32 integer -> (q, refs, want [Nq, K] exact) or None
    where the placement does not fit Nr.  Placements of the chosen rows: "one_lane" indices congruent mod 64 (one lane's list, full depth),
    "one_per_lane" consecutive indices of the first tile, "last_tile" the highest indices, "seams" 63, 64 and Nr - 1 first,
    "duplicates" the nearest row repeated (multiplicity kept)."""
    if placement == "one_lane":
        idx = list(range((Nr - 1) % 64, Nr, 64))[:K]              # the lane of the last row: its list holds rows of every tile, the ragged one too
    elif placement == "one_per_lane":
        idx = list(range(min(K, Nr)))
    elif placement == "last_tile":
        idx = list(range(Nr - K, Nr))
    elif placement == "seams":
        idx = [i for i in dict.fromkeys((63, 64, Nr - 1, 0, Nr // 2)) if 0 <= i < Nr]
        idx = (idx + [i for i in range(Nr) if i not in idx])[:K]
    else:
        idx = list(range(Nr - 1, -1, -max(1, Nr // K)))[:K]
        idx = (idx + [i for i in range(Nr) if i not in idx])[:K]
    if len(idx) < K:
        return None
    g = _gen(Nr, Nq, K, E, len(placement))
    q = torch.zeros(Nq, E)
    q[:, 1] = torch.arange(Nq).float()                             # query i = i e_1: distances differ per query, still integers
    far = torch.randint(40, 60, (Nr, E), generator=g).float() * (torch.randint(0, 2, (Nr, E), generator=g) * 2 - 1).float()
    refs = far.clone()                                             # |far - q|^2 >= 39^2 E: never among the K nearest
    dist = list(range(1, K + 1))
    if placement == "duplicates" and K >= 2:
        dist = [1] + [1] + list(range(2, K))                       # the nearest row twice (three times from K = 5 on)
        if K >= 5:
            dist = [1, 1, 1] + list(range(2, K - 1))
    order = torch.randperm(K, generator=g).tolist()                # which chosen row gets which distance
    for slot, i in enumerate(idx):
        refs[i] = 0.0
        refs[i, 2] = float(dist[order[slot]])                      # m e_2: |q_i - r|^2 = i^2 + m^2
    want = torch.sqrt((torch.arange(Nq).double()[:, None] ** 2) + torch.tensor(sorted(dist)).double()[None, :] ** 2)
    return q, refs, want


def knn_random(Nr=130, Nq=9, K=16, E=128):
    g = _gen(Nr, Nq, K, E)
    return torch.randn(Nq, E, generator=g), torch.randn(Nr, E, generator=g)


KNN_GRID = [(Nr, Nq, K, E, p) for Nr in KNN_NR for Nq in KNN_NQ for E in KNN_E for K in knn_ks(Nr) for p in KNN_PLACEMENTS
            if knn_lattice(Nr, Nq, K, E, p) is not None] + [KNN_DEEP + ("one_lane",)]


# ---- checks the CPU emulation and the GPU kernels both have to pass ------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def check_one_hot(logits, txt, scale, what):
    want = one_hot_want(txt, scale)
    bad = torch.nonzero(_bits(logits.reshape(want.shape).float()) != _bits(want))
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {want.numel()} logits differ from scale * txt[c, j(b)], first at [b, c] = {bad[0].tolist()}"


def check_ties(logits, pred, cols, what):
    lg = logits.float()
    for c in cols[1:]:
        assert torch.equal(_bits(lg[:, c]), _bits(lg[:, cols[0]])), f"{what}: column {c} differs from its duplicate {cols[0]}"
    other = lg.clone()
    other[:, list(cols)] = float("-inf")
    assert (lg[:, cols[0]] > other.max(dim=1).values).all(), f"{what}: the duplicated class is not the row maximum (the case is broken)"
    assert (pred.long() == min(cols)).all(), f"{what}: pred {sorted(set(pred.tolist()))}, want the lowest tied column {min(cols)}"


def check_uniform(logits, conf, pred, C, what):
    lg = logits.float()
    assert (_bits(lg) == _bits(lg[:, :1].expand_as(lg).contiguous())).all(), f"{what}: the logits of a row differ"
    assert (pred.long() == 0).all(), f"{what}: pred {pred.tolist()}, want 0"
    steps = fp32_steps_from_nearest(conf, torch.full(conf.shape, 1.0 / C, dtype=torch.float64))
    assert (steps <= 1).all(), f"{what}: conf {conf.tolist()} is not 1 / {C} to the nearest fp32 value or its neighbour"


def check_knn_lattice(got, want, what):
    steps = fp32_steps_from_nearest(got, want)
    assert (steps <= 1).all(), f"{what}: got {got.tolist()}, want {want.tolist()}"


def check_tail(img_n, raw, out, conf, pred, case, scale, dac, labels, note=None, probs=None):
    """What the GPU tests assert of a random case, on (normalised features or None, logits before DAC or None, logits returned, conf, pred)."""
    (B, C, E, seed), dt, nz = case
    want, tol, n64, wpred, _ = random_reference(B, C, E, seed, dt, nz, scale)
    worst = {}
    if img_n is not None and nz:
        nw, ntol = l2_normalize(random_inputs(B, C, E, seed, dt, nz)[0])
        worst["l2norm"] = worst_ratio(img_n, nw, ntol)
    if raw is not None:
        worst["logits"] = worst_ratio(raw, want, tol)
    if dac is not None:
        want, tol = dac_scale(want, tol, dac, wpred)
    worst["logits_dac" if dac is not None else "logits"] = max(worst_ratio(out, want, tol), worst.get("logits", 0.0) if dac is None else 0.0)
    assert torch.equal(pred.long(), wpred), f"{case}: pred differs from the float64 argmax at rows {torch.nonzero(pred.long() != wpred).flatten().tolist()[:8]}"
    c64, p64, ctol, pr64, ptol = softmax_top1(out)
    worst["conf_dac" if dac is not None else "conf"] = worst_ratio(conf, c64, ctol)
    if probs is not None:
        worst["probs"] = worst_ratio(probs, pr64, ptol)
    for k, v in worst.items():
        if note:
            note(k, v)
        assert v <= 1.0, f"{case} scale {scale} dac {dac is not None}: {k} worst |err| / tol = {v:.3f}"
    return worst
