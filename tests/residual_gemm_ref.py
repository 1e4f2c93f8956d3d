"""Reference, tolerance, emulation and dispatch mirror for the two residual producers of a transformer block -- clipmi_gemm_residual_f16 (out-proj /
c_proj on the fp16 stream; the entry point that reaches gemm_rstream_kernel) and clipmi_gemm_residual_fold (the same pair on the fp32 stream) -- the
oracle of tests/test_residual_gemm_ref_cpu.py and tests/test_gpu_residual_gemm.py.  torch only, float64 wherever the module does arithmetic; every
function works on the device its operands are on.

    x[m, n] <- x_old[m, n] + a[m, :] . w[n, :] + bias[n]       in place, ONE rounding of the fp32 sum to the stream type (fp16 or fp32)
    x16     =  fp16(x)                                          fp32 stream only, bit for bit of the kernel's own x
    stats[t, m] = (sum, sum of squares) of row m of the STORED x over column tile t; `parts` tiles of w_part = 256 (128-column kernel: 128) columns

Operands (``operands``): gemm_ref.operands -- seeded, round(M / 4) rows of ``a`` and round(N / 4) rows of ``w`` scaled by 1 / 64 -- and the old stream
value follows the same classes: ``x_old`` ~ N(0, 1) scaled by 1 / 64 on the small rows and again on the small columns, fp16-valued for the fp16
stream.  Outputs of size 1, 1 / 64 and 1 / 4096 then sit side by side in every tile, and the output's own rounding cannot hide an error in the small
ones (with an O(1) residual everywhere, 2^-11 of the residual is far more than a lost K-step of a 1 / 64-scaled row).

Outputs (``expected``): want = x_old + a @ w^T + bias in float64, reach = |a| @ |w|^T + |bias| + |x_old|, and gemm_ref.tolerance(.., "residual", f16_out):
FACTOR * (C_ACC * reach + u_out |want|) + 2^-24 with FACTOR = 2, C_ACC = 2^-20 -- the project's bound.  It allows any order of the fp32 sum, so also the
row-range kernel's (bias, a few K-steps, the residual, the other K-steps).  C_ACC is kept on the same condition as in gemm_ref: the emulation stays
within 2^-21 * reach of float64 in front of the output rounding (tests/test_residual_gemm_ref_cpu.py asserts it per shape and prints the figure).

Row partials (``check_partials``) are held against the kernel's OWN stored row ``got`` (the rounded fp16 row, or the fp32 row), in float64:

    |stats[t, m, 0] - sum(got)|   <= 2^-19 * sum|got|         |stats[t, m, 1] - sum(got^2)| <= 2^-19 * sum(got^2)

2^-19 = 32 * 2^-24: an fp32 sum of at most 256 terms in a tree of depth < 32 (the error model of tests/test_gpu_ln_fold.py).  A partial formed from the
unrounded fp32 sums of an fp16 row is off by the sum of up to 256 rounding errors of 2^-12 |x| each -- some 2^-9 of sum|got| / 16 -- and fails.

``emulate`` is the reference's arithmetic, never the device's: fp32 matmul + bias + residual, one rounding to the stream type, partials as fp32 sums
of that result.

``exact_case``: constructed inputs that need no tolerance.  Small integers everywhere (a, bias, x_old in [-4, 4]); row n of w holds exactly two
entries of +-1, at k1(n) = n % (K / 2) and k2(n) = K / 2 + (n + 64) % (K / 2) -- 64 or K / 2 + 64 columns apart, so always in different 64-wide K-steps,
and with N >= K / 2 every one of the K columns is used.  Every output is an integer of magnitude <= 16 (exact in fp16), every partial at most
256 * 256 (exact in fp32 under any order): outputs and partials must equal the float64 result bit for bit under every kernel; a dropped, doubled or
misplaced K-step, LDS stage, row, column, bias element or residual slice changes whole integers.

Dispatch mirrors -- CHANGE BOTH TOGETHER with csrc/gemm_rstream.hip (rstream_fits, the kernel's range / tile split) and csrc/gemm.hip (pick_variant,
launch_one); no test can observe which kernel ran, so "gemm_rstream_kernel ran" rests on these mirrors:

* ``rstream_plan(cus, M, N, K, ldx)``: None where the row-range kernel does not take the shape, else the set of tile structures that occur -- one tuple
  per distinct range, the pairs (32 rows) of its tiles in order, e.g. (10, 9).  groups = (cus & ~7) // tiles_n ranges of pairs, range g =
  [g * pairs // groups, (g + 1) * pairs // groups), each cut into ceil(len / 10) tiles equal to within one pair, the taller first.
* ``rstream_shape(cus, N, len, extra, cut)``: M = (groups * len + extra) * 32 - cut: ``extra`` ranges of len + 1 pairs, a last pair ``cut`` rows short.
* ``expected_parts``: the number of partials the launcher reports.  (N + 255) / 256 from the row-range kernel and the 256- and 320-row tile kernels;
  (N + 127) / 128 from the 128 x 128 kernel while that is at most 8, else the launcher takes the 256 x 256 tiles.  The 128 x 128 kernel runs when
  variant 0 is forced AND when the unforced cost model (``default_variant``) picks it for a small problem.
"""
from __future__ import annotations

import torch

import gemm_ref
from gemm_ref import C_ACC, FACTOR, SMALL, check, reference, tolerance  # noqa: F401  (re-exported: one bound for both suites)

PART_BOUND = 2.0 ** -19
LN_MAX_PARTS = 8
BK = 64

# (M, N, K)
SMALL_SHAPES = [(1, 8, 64), (7, 8, 64), (300, 264, 128), (321, 264, 64), (600, 520, 576), (333, 512, 3072), (300, 1672, 128)]
# (N, K, len, extra, cut) -> the tile structures that must occur on any device, and what the shape pins
ROW_RANGE = [
    ((2048, 448, 8, 0, 13), {(8,)}),                        # the smallest shape taken; 7 K-steps (the plain loop is empty); 8 partials; ragged last pair
    ((2048, 512, 9, 5, 13), {(9,), (10,)}),                 # h0 = 5, h1 = 4: the fifth-block branch on one half only; 8 K-steps
    ((520, 576, 19, 3, 5), {(10, 9), (10, 10)}),            # a tile change with residual and stores in flight; last column tile of 8; 9 K-steps (odd)
    ((2048, 448, 25, 1, 13), {(9, 8, 8), (9, 9, 8)}),       # two tile changes, the LDS buffer parity flipping at each (odd K-step count)
]
ONE_PAIR_SHORT = (2048, 448, 8, -1, 13)                     # groups * 8 - 1 pairs: refused by the row-range kernel, correct through the fall-back


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------------------------ operands, reference, emulation
def operands(M: int, N: int, K: int, f16_stream: bool, seed: int | None = None):
    """(a fp16 [M,K], w fp16 [N,K], bias fp32 [N], x_old [M,N] fp16 / fp32, small_rows bool [M], small_cols bool [N]) on the CPU."""
    a, w, bias, res, small_rows, small_cols = gemm_ref.operands(M, N, K, seed)
    x_old = res.clone()
    x_old[small_rows] *= SMALL
    x_old[:, small_cols] *= SMALL
    return a, w, bias, (x_old.half() if f16_stream else x_old), small_rows, small_cols


def expected(a, w, bias, x_old, f16_stream: bool):
    """(want, reach, tol), float64."""
    want, reach, pre = reference(a, w, bias, x_old, "residual")
    return want, reach, tolerance(want, reach, pre, "residual", f16_stream)


def tile_sums(got, w_part: int):
    """float64 (sum, sum of squares, sum of magnitudes) of ``got`` [M, N] over column tiles of ``w_part``: three [parts, M] tensors."""
    M, N = got.shape
    parts = cdiv(N, w_part)
    g = got.double().contiguous()
    if parts * w_part != N:
        g = torch.cat([g, g.new_zeros(M, parts * w_part - N)], 1)
    g = g.view(M, parts, w_part).transpose(0, 1)
    return g.sum(-1), (g * g).sum(-1), g.abs().sum(-1)


def partials32(out, w_part: int):
    """fp32 [parts, M, 2]: (sum, sum of squares) of the stored row over each column tile, as fp32 sums -- the reference's arithmetic."""
    M, N = out.shape
    o = out.float()
    cols = [o[:, c:min(c + w_part, N)] for c in range(0, N, w_part)]
    return torch.stack([torch.stack([c.sum(1), (c * c).sum(1)], -1) for c in cols])


def emulate(a, w, bias, x_old, f16_stream: bool, w_part: int = 256):
    """(x, x16, stats): fp32 matmul + bias + residual, one rounding to the stream type, x16 = fp16(x), partials as fp32 sums of x."""
    x = gemm_ref.emulate(a, w, bias, x_old.float(), "residual", f16_stream)
    return x, x.half(), partials32(x, w_part)


def accumulation_error(a, w, bias, x_old, want, reach):
    """max |fp32 evaluation - float64| / reach in front of the output rounding: <= 2^-21 keeps C_ACC = 2^-20."""
    return gemm_ref.accumulation_error(a, w, bias, x_old.float(), want, reach, "residual")


def part_width(parts: int, N: int) -> int:
    """The column-tile width that a returned ``*parts`` implies."""
    for w_part in (256, 128):
        if parts == cdiv(N, w_part):
            return w_part
    raise AssertionError(f"{parts} partials fit neither 256- nor 128-column tiles of N = {N}")


def check_partials(stats, got, w_part: int, what=""):
    """``stats`` [parts, M, 2] against float64 sums of the stored row ``got`` [M, N].  Returns (worst error / bound, (t, m, which))."""
    s, q, mag = tile_sums(got, w_part)
    assert tuple(stats.shape) == (s.shape[0], s.shape[1], 2), f"{what}: stats {tuple(stats.shape)} for {s.shape[0]} tiles of {s.shape[1]} rows"
    st = stats.double()
    assert bool(torch.isfinite(st).all()), f"{what}: non-finite partials"
    err = torch.stack([(st[..., 0] - s).abs(), (st[..., 1] - q).abs()], -1)
    bound = PART_BOUND * torch.stack([mag, q], -1)
    # an all-zero tile has a bound of zero: exact or beyond every ratio
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")).double())
    flat = int(ratio.argmax())
    at = (flat // (ratio.shape[1] * 2), flat // 2 % ratio.shape[1], flat % 2)
    worst = float(ratio.flatten()[flat])
    assert worst <= 1.0, (f"{what}: {int((ratio > 1.0).sum())} of {ratio.numel()} partials beyond 2^-19, worst {worst:.3f} x at tile {at[0]} row {at[1]} "
                          f"{'sum' if at[2] == 0 else 'sum of squares'}: got {float(st[at]):.9g} want {float((s if at[2] == 0 else q)[at[:2]]):.9g}")
    return worst, at


# ------------------------------------------------------------------------------------------------------------------ the exact case
def exact_case(M: int, N: int, K: int, seed: int, f16_stream: bool = True):
    """(a fp16, w fp16, bias fp32, x_old fp16 / fp32) of small integers, on the CPU; see the module docstring."""
    H = K // 2
    assert K % BK == 0 and K >= 2 * BK and N >= H, f"exact_case needs two K-steps and N >= K / 2 (N = {N}, K = {K})"
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-4, 5, (M, K), generator=g).half()
    bias = torch.randint(-4, 5, (N,), generator=g).float()
    x_old = torch.randint(-4, 5, (M, N), generator=g).float()
    sign = (torch.randint(0, 2, (N, 2), generator=g) * 2 - 1).half()
    n = torch.arange(N)
    k1, k2 = n % H, H + (n + BK) % H
    assert bool((k1 // BK != k2 // BK).all())
    w = torch.zeros(N, K, dtype=torch.float16)
    w[n, k1] = sign[:, 0]
    w[n, k2] = sign[:, 1]
    return a, w, bias, (x_old.half() if f16_stream else x_old)


def exact_result(a, w, bias, x_old):
    """float64 x_old + a @ w^T + bias: integers."""
    return x_old.double() + a.double() @ w.double().t() + bias.double()


# ------------------------------------------------------------------------------------------------------------------ dispatch mirrors (change both together)
def rstream_groups(cus: int, N: int) -> int:
    return (cus & ~7) // cdiv(N, 256)


def rstream_shape(cus: int, N: int, length: int, extra: int, cut: int) -> int:
    return (rstream_groups(cus, N) * length + extra) * 32 - cut


def rstream_plan(cus: int, M: int, N: int, K: int, ldx: int | None = None, lda: int | None = None, ldw: int | None = None):
    """Mirror of rstream_fits and of gemm_rstream_kernel's range / tile split.  None = not taken."""
    ldx, lda, ldw = (N if ldx is None else ldx), (K if lda is None else lda), (K if ldw is None else ldw)
    n_cu = cus & ~7
    tiles_n = cdiv(N, 256)
    if n_cu < 8 or tiles_n > n_cu or tiles_n > LN_MAX_PARTS:
        return None
    groups = n_cu // tiles_n
    pairs = cdiv(M, 32)
    lim = (1 << 31) // (2 * 257)                      # stream_offsets_ok
    if not (K >= 7 * BK and N % 8 == 0 and ldx % 8 == 0 and max(lda, ldw, ldx) < lim):
        return None
    for length in range(pairs // groups, cdiv(pairs, groups) + 1):
        if length < 8 or length // cdiv(length, 10) < 8:
            return None
    plan = set()
    for g in range(groups):
        length = (g + 1) * pairs // groups - g * pairs // groups
        n_tiles = cdiv(length, 10)
        base, rem = divmod(length, n_tiles)
        plan.add(tuple(base + (1 if k < rem else 0) for k in range(n_tiles)))
    return plan


def default_variant(cus: int, M: int, N: int, K: int) -> int:
    """Mirror of pick_variant's unforced cost model: rounds x tile area x workgroups per CU x penalty over the three tile kernels."""
    best, best_cost = 1, float("inf")
    for vid, bm, bn, per_cu, penalty in ((1, 256, 256, 1, 1.00), (10, 320, 256, 1, 1.03), (0, 128, 128, 2, 1.12)):
        if vid == 10 and K < 2 * BK:
            continue
        rounds = cdiv(cdiv(M, bm) * cdiv(N, bn), cus * per_cu)
        cost = float(rounds) * bm * bn * per_cu * penalty
        if vid == 10 and K <= 512:
            cost *= 0.93
        if cost < best_cost:
            best, best_cost = vid, cost
    return best


def expected_parts(variant: int | None, cus: int, M: int, N: int, K: int, f16_stream: bool, ldx: int | None = None,
                   lda: int | None = None, ldw: int | None = None) -> int:
    """Mirror of launch_one for the two producers: the ``*parts`` the launcher reports under forced ``variant`` (None = the default dispatch)."""
    if f16_stream and (variant == 16 or (variant is None and K <= 1536)) and rstream_plan(cus, M, N, K, ldx, lda, ldw) is not None:
        return cdiv(N, 256)
    v = default_variant(cus, M, N, K) if variant is None else variant
    if v == 0 and cdiv(N, 128) <= LN_MAX_PARTS:
        return cdiv(N, 128)
    return cdiv(N, 256)
