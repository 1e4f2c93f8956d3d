"""Reference, tolerance, operands, emulation and dispatch mirror for clipmi_gemm_ln_fold (csrc/gemm.hip "LayerNorm folded into the GEMMs": in-proj and
c_fc behind a fold producer) -- the oracle of tests/test_ln_fold_ref_cpu.py and tests/test_gpu_ln_fold_matrix.py.  torch only, float64 wherever the
reference does arithmetic; every function works on the device its operands are on.

The operation is exactly what the entry point is given -- the reference is of the KERNEL, not of LayerNorm (tests/test_gpu_ln_fold.py holds the fold
against a true LayerNorm, statistically):

    out[m, n] = epi( rstd_m * (a[m, :] . w_f[n, :])  -  mean_m * rstd_m * g[n]  +  c[n] )          epi: bias (identity) or gelu (QuickGELU)

    s_m  = sum_p stats[p, m].sum,  ss_m = sum_p stats[p, m].sumsq      float64, the partials added in order
    mean = s / ln_dim,   var = max(ss / ln_dim - mean^2, 0),   rstd = 1 / sqrt(var + eps)

Partial p of row m is the float pair at ``2 * (p * plane + m * row_stride)`` of ``stats`` (``row_params``).

Tolerance (``tolerance``), per element, in the shape of gemm_ref.tolerance with one more term:

    FACTOR * ( C_ACC * reach + rho_m * (|t1| + |t2|) + u_out * |want| [+ U16 * GELU_SLOPE * |pre|] ) + FLOOR

* ``t1`` = rstd * acc and ``t2`` = mean * rstd * g: the two terms that carry the row parameters;
* ``reach`` = rstd * (|a| @ |w_f|^T) + |t2| + |c|: what an fp32 accumulation and the two fp32 multiply-adds of the combination are relative to;
* ``u_out``, the bracketed gelu-to-fp16 term, FACTOR, C_ACC and FLOOR are gemm_ref's (the project's): no new constant;
* ``rho_m``: the relative error of the row parameters computed as the kernels compute them -- float64 sums of the fp32 partials (exact to 2^-53),
  then, with u = 2^-24,
      mean = s * (double) fp32(1 / ln_dim)        ln_inv_d carries one fp32 rounding: relative u in mean, and in ss * ln_inv_d
      var  = ss * ln_inv_d - mean^2               |d var| <= u * ss / ln_dim + 2 u * mean^2
      (float) var                                  + u * var
  => dvar = u * (ss / ln_dim + 2 mean^2) + u * var.  rstd = (var + eps)^-1/2 moves by 0.5 * dvar / (var + eps) relative; the fp32 sum
  ``var + eps``, ``rsqrtf`` (1 ulp), the cast ``(float) mean`` and the product ``(float) mean * rstd`` add at most u each:
      rho = 0.5 * dvar / (var + eps) + 4 u.
  t1 carries rstd's error, t2 that of mean * rstd: rho * (|t1| + |t2|).  The operands keep |mean| / sigma <= 10, where rho stays near 1.3e-5; the
  degenerate end (|mean| / sigma in the hundreds, constant rows, var ~ eps), where rho grows past usefulness, belongs to tests/test_gpu_ln_fold.py.

Operands (``operands``): fp16 ``a`` whose row m belongs to class (m // 2) % 3 of mean / sigma in {0, +3, -10} (the offset added before the scale),
every odd row -- mean included -- scaled by 1 / 64: neighbouring rows differ 64 x in rstd and in sign and size of mean * rstd, so a row parameter taken
from a neighbour cannot pass, and on the scaled rows eps = 1e-5 is about 4 % of var.  ``w`` is fp16 ~ N(0, 1 / K) with a seeded quarter of its rows
scaled by 1 / 64 (gemm_ref.operands' column classes), gamma = 1 + 0.2 N(0, 1), beta = 0.1 N(0, 1), bias = 0.1 N(0, 1), folded by the formula of
ops.fold_layernorm_linear.  The partials are fp32 sums of the fp16 row over ``parts`` column slices of UNEQUAL width, laid out as [8][plane] float pairs,
plane = row_stride * M + plane_pad, row m at pair m * row_stride; every float the call must not read is NaN: planes p >= parts, the pairs between the
rows of a strided plane and the rows behind the last one.

``emulate`` is the reference's arithmetic in fp32, never the device's: fp32(1 / ln_dim), float64 sums, rstd in fp32, a torch fp32 matmul, the
three-term combination in fp32, one rounding to the output type (gelu to fp16: also the twice-rounded form).

``exact_case``: constructed inputs that need no tolerance.  ln_dim = 1024 (a power of two: fp32(1 / ln_dim) is exact; it is NOT K), eps = 0; ``a``
in {-1, 0, 1}, ``w_f`` in {-1, 0, 1}, g = the integer row sums of w_f, c in [-4, 4]; per row an integer mean in [-2, 2] that differs between
neighbouring rows and var = 1: s = ln_dim * mean and ss = ln_dim * (1 + mean^2) are split across the partials as integers (below 2^24: exact in fp32
and in any order), a different split per row.  rstd = rsqrtf(1) = 1 (tests/test_gpu_ln_fold.py already relies on it), so
out = acc - mean * g + c exactly: |acc| <= K, |mean * g| <= 2 K, integers of magnitude <= 3 K + 4 <= 2048 for K <= 576 and exact in fp16 and fp32 on
every kernel.  ``var4=True`` is the separate power-of-four case: rows of var = 1 / 4, 1, 4 in turn (rstd = 2, 1, 1 / 2 if the hardware's reciprocal square root
is exact there), ``a`` and the means doubled so that every term stays an integer.

Dispatch mirror (``expected_kernel``) -- CHANGE TOGETHER with launch_one / pick_variant / launch_stream in csrc/gemm.hip; no test can observe which
kernel ran, so "the streamed kernel ran" rests on this mirror, as on residual_gemm_ref.rstream_plan in the residual tests.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from gemm_ref import C_ACC, FACTOR, FLOOR, GELU_SLOPE, U16, U32, check, m_star, quickgelu  # noqa: F401  (re-exported: one bound for the suites)
from residual_gemm_ref import cdiv, default_variant

U = 2.0 ** -24
EPS = 1e-5
SMALL = 1.0 / 64.0
LN_MAX_PARTS = 8
STREAM_RAW_PARTS = 4
BK = 64
CLASS_MEANS = (0.0, 3.0, -10.0)
EXACT_LN_DIM = 1024

# (M, N, K) -> partials (and whether the scratch row ``ln_rows`` is given) of the one statistics layout the full variant x epilogue x output cross
# runs with; M = None is M* (gemm_ref.m_star).  48 K-steps run with the maximum of 8 partials, which reach the streamed kernel only through
# ln_finalize_kernel: that shape passes ln_rows.
SHAPES = [((1, 8, 64), 1, False), ((7, 4, 64), 2, False), ((300, 260, 128), 2, False), ((321, 264, 64), 1, False), ((600, 520, 576), 3, False),
          ((None, 1672, 512), 4, False), ((333, 512, 3072), 8, True)]
EXACT_SHAPES = [(300, 264, 128), (600, 520, 576), (None, 1672, 512)]


# ------------------------------------------------------------------------------------------------------------------ row parameters
def _pairs(stats, M, parts, plane, row_stride):
    """float64 [parts, M, 2]: partial p of row m, the float pair at 2 * (p * plane + m * row_stride)."""
    flat = stats.reshape(-1)
    rows = torch.arange(M, device=flat.device) * row_stride
    idx = (torch.arange(parts, device=flat.device)[:, None] * plane + rows[None, :]) * 2
    return torch.stack([flat[idx], flat[idx + 1]], -1).double()


def sums(stats, M, parts, plane=None, row_stride=1):
    """(s, ss) float64 [M]: the partials added in order."""
    p = _pairs(stats, M, parts, M if plane is None else plane, row_stride)
    s = torch.zeros(M, dtype=torch.float64, device=p.device)
    ss = torch.zeros_like(s)
    for i in range(parts):
        s = s + p[i, :, 0]
        ss = ss + p[i, :, 1]
    return s, ss


def row_params(stats, M, parts, ln_dim, eps, plane=None, row_stride=1):
    """(mean, rstd, rho) float64 [M] of the module docstring."""
    s, ss = sums(stats, M, parts, plane, row_stride)
    mean = s / ln_dim
    ex2 = ss / ln_dim
    var = (ex2 - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    dvar = U * (ex2 + 2.0 * mean * mean) + U * var
    rho = 0.5 * dvar / (var + eps) + 4.0 * U
    return mean, rstd, rho


# ------------------------------------------------------------------------------------------------------------------ reference and tolerance
def products(a, w_f):
    """(a @ w_f^T, |a| @ |w_f|^T) in float64: the part of the reference that does not depend on the statistics."""
    a64, w64 = a.double(), w_f.double()
    return a64 @ w64.t(), a64.abs() @ w64.abs().t()


def reference(a, w_f, g, c, mean, rstd, epi, prod=None):
    """(want, pre, reach, t1, t2), float64 [M, N].  ``prod`` = products(a, w_f) where the caller keeps it."""
    assert epi in ("bias", "gelu"), epi
    acc, mag = products(a, w_f) if prod is None else prod
    t1 = rstd[:, None] * acc
    t2 = (mean * rstd)[:, None] * g.double()[None, :]
    pre = t1 - t2 + c.double()[None, :]
    reach = rstd[:, None] * mag + t2.abs() + c.double().abs()[None, :]
    want = quickgelu(pre) if epi == "gelu" else pre
    return want, pre, reach, t1, t2


def non_rounding(reach, t1, t2, rho):
    """The part of the tolerance in front of the output rounding, unfactored: accumulation and row parameters."""
    return C_ACC * reach + rho[:, None] * (t1.abs() + t2.abs())


def tolerance(want, pre, reach, t1, t2, rho, epi, f16_out, factor=FACTOR):
    t = non_rounding(reach, t1, t2, rho) + (U16 if f16_out else U32) * want.abs()
    if epi == "gelu" and f16_out:
        t = t + U16 * GELU_SLOPE * pre.abs()
    return factor * t + FLOOR


# ------------------------------------------------------------------------------------------------------------------ operands
def fold(w, b, gamma, beta):
    """(w_f, g, c) by the formula of ops.fold_layernorm_linear."""
    w32 = w.float()
    wf = (w32 * gamma.float()[None, :]).to(torch.float16).contiguous()
    return wf, wf.float().sum(dim=1).contiguous(), (w32 @ beta.float() + b.float()).contiguous()


def slice_bounds(K, parts):
    """Column slices of unequal width: slice i ends at round(K * i (i + 1) / (parts (parts + 1)))."""
    b = [int(round(K * i * (i + 1) / (parts * (parts + 1)))) for i in range(parts + 1)]
    assert b[0] == 0 and b[-1] == K and all(hi > lo for lo, hi in zip(b, b[1:])), f"{parts} slices of K = {K}: {b}"
    assert parts == 1 or len({hi - lo for lo, hi in zip(b, b[1:])}) > 1
    return b


def layout(partials, M, plane_pad=0, row_stride=1):
    """fp32 [8 * plane * 2] from partials [parts, M, 2]: NaN wherever the call must not read.  Returns (stats, plane)."""
    parts = partials.shape[0]
    plane = row_stride * M + plane_pad
    stats = torch.full((LN_MAX_PARTS, plane, 2), float("nan"), dtype=torch.float32)
    stats[:parts, torch.arange(M) * row_stride] = partials.float()
    return stats.reshape(-1), plane


def row_partials(a, parts):
    """fp32 [parts, M, 2]: (sum, sum of squares) of the fp16 row over ``parts`` unequal column slices, as fp32 sums."""
    b = slice_bounds(a.shape[1], parts)
    x = a.float()
    return torch.stack([torch.stack([x[:, lo:hi].sum(1), (x[:, lo:hi] * x[:, lo:hi]).sum(1)], -1) for lo, hi in zip(b, b[1:])])


def operands(M, N, K, parts, plane_pad=0, seed=None, row_stride=1):
    """The case on the CPU: a fp16 [M, K], w_f fp16 [N, K], g, c fp32 [N], stats fp32 [8 * plane * 2], plane, parts, row_stride, ln_dim = K,
    eps = 1e-5, small_cols bool [N].  ``a``, ``w_f``, ``g`` and ``c`` depend on (M, N, K, seed) alone, not on the statistics layout."""
    gen = torch.Generator().manual_seed(M * 7 + N + K if seed is None else seed)
    z = torch.randn(M, K, generator=gen)
    w = torch.randn(N, K, generator=gen) * K ** -0.5
    b = torch.randn(N, generator=gen) * 0.1
    gamma = 1.0 + 0.2 * torch.randn(K, generator=gen)
    beta = 0.1 * torch.randn(K, generator=gen)
    small_cols = torch.zeros(N, dtype=torch.bool)
    small_cols[torch.randperm(N, generator=gen)[:(N + 2) // 4]] = True
    w[small_cols] *= SMALL
    m = torch.arange(M)
    x = z + torch.tensor(CLASS_MEANS)[(m // 2) % 3][:, None]      # the offset before the scale
    x[m % 2 == 1] *= SMALL
    a = x.half()
    w_f, g, c = fold(w.half(), b, gamma, beta)
    stats, plane = layout(row_partials(a, parts), M, plane_pad, row_stride)
    return SimpleNamespace(a=a, w_f=w_f, g=g, c=c, stats=stats, plane=plane, parts=parts, row_stride=row_stride, ln_dim=K, eps=EPS,
                           small_cols=small_cols)


# ------------------------------------------------------------------------------------------------------------------ the exact case
def exact_case(M, N, K, parts, var4=False):
    """Constructed inputs whose outputs are integers (module docstring).  Returns the case (as ``operands``) with ``mean`` and ``rstd`` (float64
    [M], the stated values) and ``want`` = rstd * acc - mean * rstd * g + c (float64 integers) added."""
    assert K % BK == 0 and 1 <= parts <= LN_MAX_PARTS
    D = EXACT_LN_DIM
    gen = torch.Generator().manual_seed(M + 3 * N + 5 * K + 7 * parts + (11 if var4 else 0))
    a = torch.randint(-1, 2, (M, K), generator=gen).double()
    w_f = torch.randint(-1, 2, (N, K), generator=gen).double()
    c = torch.randint(-4, 5, (N,), generator=gen).double()
    g = w_f.sum(1)
    m = torch.arange(M)
    mean = ((m * 3) % 5 - 2).double()                     # -2 .. 2, neighbours differ (3 is a unit modulo 5)
    var = torch.ones(M, dtype=torch.float64)
    if var4:
        a, mean = 2.0 * a, 2.0 * mean                      # rstd = 1 / 2 leaves integers
        var = torch.tensor([0.25, 1.0, 4.0], dtype=torch.float64)[(m // 3) % 3]
    rstd = 1.0 / torch.sqrt(var)
    s, ss = D * mean, D * (var + mean * mean)
    cuts = torch.randint(-1000, 1001, (parts - 1, M, 2), generator=gen).double()      # a different integer split per row
    last = torch.stack([s, ss], -1) - cuts.sum(0)
    partials = torch.cat([cuts, last[None]])
    assert float(partials.abs().max()) < 2.0 ** 24 and bool((partials == partials.round()).all())
    stats, plane = layout(partials, M)
    want = rstd[:, None] * (a @ w_f.t()) - (mean * rstd)[:, None] * g[None, :] + c[None, :]
    assert bool((want == want.round()).all()) and float(want.abs().max()) <= 2048.0, f"exact case: outputs up to {float(want.abs().max())}"
    assert var4 or 3 * K + 4 <= 2048
    return SimpleNamespace(a=a.half(), w_f=w_f.half(), g=g.float(), c=c.float(), stats=stats, plane=plane, parts=parts, row_stride=1, ln_dim=D,
                           eps=0.0, mean=mean, rstd=rstd, want=want)


def quickgelu_f16_bits(want):
    """Bits (int32, 0 .. 65535) of the correctly rounded fp16 of h sigmoid(1.702 h) for the integers ``want`` (|h| <= 2048): float64, one rounding
    (numpy rounds float64 -> float16 once; a torch cast would go through fp32)."""
    import numpy as np
    h = np.arange(-2048, 2049, dtype=np.float64)
    with np.errstate(over="ignore"):
        y = h / (1.0 + np.exp(-1.702 * h))
    lut = torch.from_numpy(y.astype(np.float16).view(np.int16).astype(np.int32) & 0xFFFF).to(want.device)
    return lut[(want + 2048.0).long()]


def f16_ordinal(bits):
    """fp16 bits (int32) -> ordinal: neighbouring values differ by one, +-0 -> 0."""
    return torch.where(bits >= 0x8000, -(bits & 0x7FFF), bits)


# ------------------------------------------------------------------------------------------------------------------ emulation
def emulate_rows(stats, M, parts, ln_dim, eps, plane=None, row_stride=1):
    """(rstd, mean * rstd) fp32 [M]: float64 sums, fp32(1 / ln_dim), the variance in float64, rstd and the product in fp32."""
    s, ss = sums(stats, M, parts, plane, row_stride)
    inv_d = torch.tensor(1.0 / ln_dim, dtype=torch.float32).double().to(s.device)
    mean = s * inv_d
    var = (ss * inv_d - mean * mean).clamp_min(0.0)
    rstd = torch.rsqrt(var.float() + torch.tensor(eps, dtype=torch.float32, device=s.device))
    return rstd, mean.float() * rstd


def acc32(a, w_f):
    return a.float() @ w_f.float().t()


def emulate_pre(acc, g, c, rstd, mrs):
    """The three-term combination in fp32."""
    return acc * rstd[:, None] - mrs[:, None] * g.float()[None, :] + c.float()[None, :]


def finish(pre, epi, f16_out, twice=False):
    """The epilogue in fp32 and one rounding to the output type.  ``twice`` (gelu to fp16): the pre-activation rounded to fp16 first."""
    if twice:
        assert epi == "gelu" and f16_out
        pre = pre.half().float()
    out = quickgelu(pre) if epi == "gelu" else pre
    return out.half() if f16_out else out


def emulate(case, M, epi, f16_out, twice=False):
    rstd, mrs = emulate_rows(case.stats, M, case.parts, case.ln_dim, case.eps, case.plane, case.row_stride)
    return finish(emulate_pre(acc32(case.a, case.w_f), case.g, case.c, rstd, mrs), epi, f16_out, twice)


# ------------------------------------------------------------------------------------------------------------------ dispatch mirror (change both together)
TILE_NAME = {0: "128x128", 1: "256x256", 10: "320x256"}


def _tile_variant(variant, cus, M, N, K):
    """pick_variant with the two persistent kernels sent to the 256 x 256 tiles."""
    if variant is None:
        return default_variant(cus, M, N, K)
    if variant == 10:
        return 10 if K >= 2 * BK else 1
    return 1 if variant in (13, 16) else variant


def split_head(M, N, variant, cus):
    """Rows of the streamed head when launch_one cuts a ragged last tile row off as a launch of its own (gemm_split_rows 1, the default), else None."""
    n_cu = cus & ~7
    tm, tn, rem = cdiv(M, 256), cdiv(N, 256), M % 256
    split = variant is None and rem != 0 and rem <= 128 and tm > 2 and n_cu > 0 and cdiv((tm - 1) * tn, n_cu) < cdiv(tm * tn, n_cu)
    return M - rem if split else None


def expected_kernel(M, N, K, ldo, f16_out, parts, has_ln_rows, row_stride, variant, cus, lda=None, ldw=None, plane=None):
    """The rule of launch_one for a folded call: "stream-raw" (gemm_stream_kernel finalising up to 4 partials itself), "stream-finalised"
    (ln_finalize_kernel, then gemm_stream_kernel), or the tile kernel "128x128" / "256x256" / "320x256" -- with "+direct" where an fp16 output leaves
    through the direct epilogue (N % 8 or ldo % 8) and "+f32" for an fp32 output.  A split launch is "<head kernel>[0:head] | <tail kernel>[head:M]
    stats+2*head"."""
    lda, ldw, plane = (K if lda is None else lda), (K if ldw is None else ldw), (M if plane is None else plane)

    def tile(rows):
        name = TILE_NAME[_tile_variant(variant, cus, rows, N, K)]
        return name + ("+f32" if not f16_out else "+direct" if N % 8 or ldo % 8 else "")

    lim = (1 << 31) // (2 * 257)                                   # stream_offsets_ok
    whole = (1 << 31) - (1 << 24)                                  # stream_whole_matrix_ok
    tiles = cdiv(M, 256) * cdiv(N, 256)
    fits = (f16_out and N % 8 == 0 and ldo % 8 == 0 and K >= 8 * BK and row_stride == 1 and (parts <= STREAM_RAW_PARTS or has_ln_rows)
            and max(lda, ldw, ldo) < lim and (cus & ~7) >= 8
            and (M + 256) * lda * 2 < whole and (N + 256) * ldw * 2 < whole and (M + 256) * ldo * 2 < whole and (parts * plane + 256) * 8 < whole
            and tiles * tiles < (1 << 32))
    wanted = variant == 13 or (variant is None and 5 * tiles >= 7 * cus)      # 1.4 rounds of tiles
    if not (fits and wanted):
        return tile(M)
    stream = "stream-raw" if parts <= STREAM_RAW_PARTS else "stream-finalised"
    head = split_head(M, N, variant, cus)
    if head is None:
        return stream
    return f"{stream}[0:{head}] | {tile(M - head)}[{head}:{M}] stats+2*{head}"
