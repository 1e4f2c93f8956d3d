"""Reference, tolerance and emulation for clipmi_gemm_f16's plain entry point (csrc/gemm.hip) -- the oracle of tests/test_gemm_ref_cpu.py and
tests/test_gpu_gemm_matrix.py.  torch only, float64 wherever the reference does arithmetic; every function works on the device its operands are on.

``out = epi(a[M,K] @ w[N,K]^T)`` with fp16 operands, fp32 bias / residual and an fp16 or fp32 output.  The epilogues: none, bias, gelu (bias, then QuickGELU
``x * sigmoid(1.702 x)``, clip/model.py:162-164), residual (bias + an fp32 residual, the towers' in-place form) and relu.

Operands (``operands``): seeded fp16-valued ``a`` ~ N(0, 1) and ``w`` ~ N(0, 1 / K); round(M / 4) seeded rows of ``a`` and round(N / 4) seeded columns of the
output (rows of ``w``) are scaled by 1 / 64, so outputs of size 1, 1 / 64 and 1 / 4096 sit beside one another in every tile -- what a bound on the
matrix's largest element cannot see.  ``bias`` ~ 0.1 N(0, 1) and ``res`` ~ N(0, 1) are fp32.

Tolerance (``tolerance``), per element, in the shape of linear_tol in tests/test_gpu_vision_train.py:

    FACTOR * (C_ACC * reach + u_out * |want| [+ 1.1 * 2^-11 * |pre|]) + 2^-24

* ``reach`` = |a| @ |w|^T + |bias| + |res|: what an fp32 accumulation error is relative to, whatever the order of the sum;
* ``u_out`` = 2^-11 (fp16) or 2^-23 (fp32): the output's rounding;
* the bracketed term, gelu to fp16 only: every kernel rounds the pre-activation to fp16 before the activation (gemm.hip "QuickGELU", the reference's own
  rounding point) and QuickGELU's slope is at most 1.1 -- a second rounding term beside the first, under the same factor;
* FACTOR = 2 is the project's factor over the reference's own arithmetic; 2^-24 is the smallest fp16 subnormal.

C_ACC = 2^-20, the project's value.  It is kept because the emulation -- the REFERENCE's arithmetic (``emulate``: a torch fp32 matmul of the same operands,
the epilogue in fp32, one rounding to the output type; for gelu to fp16 also the twice-rounded form), never the device's -- stays within 2^-21 * reach
of float64 at every element of every shape of the matrix, in front of the output rounding (``accumulation_error``).  Largest measured
|fp32 product + bias + residual - float64| / reach on the CPU, full shapes (M* = 9256, the 256-CU value), per K:

    K =   64   2^-21.74  (321 x 264 x 64; 1 x 8 x 64: 2^-24.63, 7 x 4 x 64: 2^-23.51)
    K =  128   2^-21.67  (300 x 260 x 128)
    K =  512   2^-22.13  (9256 x 1672 x 512)
    K =  576   2^-22.46  (600 x 520 x 576)
    K =  768   2^-22.11  (16448 x 3072 x 768, the checked rows)
    K = 3072   2^-23.59  (333 x 512 x 3072)

(the largest of some 10^5 .. 10^7 elements: a sum whose partial sums run at several times its standard deviation, 2^-24 of them per addition)
against the 2^-21 that keeping C_ACC asks for (the worst case (K + 2) * 2^-24 is not needed for any shape).  tests/test_gemm_ref_cpu.py asserts the
2^-21 at every shape it runs and prints the figure.

``check(got, want, tol)`` holds every element: finite, and |got - want| <= tol; it returns the worst error / tolerance and where it is.
"""
from __future__ import annotations

import torch

FACTOR = 2.0
C_ACC = 2.0 ** -20
U16 = 2.0 ** -11
U32 = 2.0 ** -23      # the spacing-relative figure linear_tol uses for fp32 outputs
FLOOR = 2.0 ** -24
GELU_SLOPE = 1.1
SMALL = 1.0 / 64.0

EPILOGUES = ("none", "bias", "gelu", "residual", "relu")
# the matrix: {none, bias, gelu} x {fp16, fp32} and the fp32 residual
PAIRS = [("none", True), ("none", False), ("bias", True), ("bias", False), ("gelu", True), ("gelu", False), ("residual", False)]
# (M, N, K); M = None is M*, which depends on the device (m_star)
SHAPES = [(1, 8, 64), (7, 4, 64), (300, 260, 128), (321, 264, 64), (600, 520, 576), (None, 1672, 512), (333, 512, 3072)]
SPLIT_SHAPE = (16448, 3072, 768)


def m_star(cus: int) -> tuple[int, int, int]:
    """(M*, tiles, grid) of the persistent kernel on a device of ``cus`` compute units: the smallest count of 256-row tiles with tiles_m * 7 column
    tiles beyond the grid (cus & ~7), the last row tile holding 40 rows.  256 CUs: 37 x 7 = 259 tiles, M* = 9256."""
    grid = cus & ~7
    tiles_m = grid // 7 + 1
    return (tiles_m - 1) * 256 + 40, tiles_m * 7, grid


def split_rows(M: int) -> torch.Tensor:
    """Rows of the split case that are checked: both ends and the rows around the cut at head = M // 256 * 256."""
    head = M // 256 * 256
    return torch.cat([torch.arange(0, 300), torch.arange(head - 300, head + 64), torch.arange(M - 300, M)]).unique()


def operands(M: int, N: int, K: int, seed: int | None = None):
    """(a fp16 [M,K], w fp16 [N,K], bias fp32 [N], res fp32 [M,N], small_rows bool [M], small_cols bool [N]) on the CPU."""
    g = torch.Generator().manual_seed(M * 7 + N + K if seed is None else seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    bias = torch.randn(N, generator=g) * 0.1
    res = torch.randn(M, N, generator=g)
    small_rows = torch.zeros(M, dtype=torch.bool)
    small_rows[torch.randperm(M, generator=g)[:(M + 2) // 4]] = True
    small_cols = torch.zeros(N, dtype=torch.bool)
    small_cols[torch.randperm(N, generator=g)[:(N + 2) // 4]] = True
    a[small_rows] *= SMALL
    w[small_cols] *= SMALL
    return a.half(), w.half(), bias, res, small_rows, small_cols


def quickgelu(x):
    return x * torch.sigmoid(1.702 * x)


def _epi_terms(epi, bias, res):
    assert epi in EPILOGUES, epi
    return (bias if epi != "none" else None), (res if epi == "residual" else None)


def reference(a, w, bias, res, epi):
    """(want, reach, pre), float64: the exact result, what accumulation errors are relative to, and the value in front of the activation."""
    b, r = _epi_terms(epi, bias, res)
    a64, w64 = a.double(), w.double()
    pre = a64 @ w64.t()
    reach = a64.abs() @ w64.abs().t()
    if b is not None:
        pre = pre + b.double()
        reach = reach + b.double().abs()
    if r is not None:
        pre = pre + r.double()
        reach = reach + r.double().abs()
    want = quickgelu(pre) if epi == "gelu" else pre.clamp_min(0.0) if epi == "relu" else pre
    return want, reach, pre


def tolerance(want, reach, pre, epi, f16_out, c_acc=C_ACC):
    t = c_acc * reach + (U16 if f16_out else U32) * want.abs()
    if epi == "gelu" and f16_out:
        t = t + U16 * GELU_SLOPE * pre.abs()
    return FACTOR * t + FLOOR


def _pre32(a, w, bias, res, epi):
    b, r = _epi_terms(epi, bias, res)
    pre = a.float() @ w.float().t()
    if b is not None:
        pre = pre + b.float()
    if r is not None:
        pre = pre + r.float()
    return pre


def emulate(a, w, bias, res, epi, f16_out, twice=False):
    """The reference's arithmetic: fp32 matmul, fp32 epilogue, one rounding to the output type.  ``twice`` (gelu to fp16): the pre-activation rounded to
    fp16 first, as an fp16 Linear followed by QuickGELU rounds it (clip/model.py:174-177)."""
    pre = _pre32(a, w, bias, res, epi)
    if twice:
        assert epi == "gelu" and f16_out
        pre = pre.half().float()
    out = quickgelu(pre) if epi == "gelu" else pre.clamp_min(0.0) if epi == "relu" else pre
    return out.half() if f16_out else out


def accumulation_error(a, w, bias, res, pre, reach, epi="residual"):
    """max |fp32 evaluation - float64| / reach in front of the activation and the output rounding: what decides C_ACC (<= 2^-21 keeps 2^-20)."""
    return float(((_pre32(a, w, bias, res, epi).double() - pre).abs() / reach.clamp_min(1e-300)).max())


def check(got, want, tol, what=""):
    """Every element finite and within its tolerance.  Returns (worst error / tolerance, (m, n) of that element)."""
    assert got.shape == want.shape == tol.shape, f"{what}: shapes {tuple(got.shape)} {tuple(want.shape)} {tuple(tol.shape)}"
    g = got.double()
    finite = torch.isfinite(g)
    assert bool(finite.all()), f"{what}: {int((~finite).sum())} non-finite elements, first at {tuple(int(i) for i in torch.nonzero(~finite)[0])}"
    ratio = (g - want).abs() / tol
    flat = int(ratio.argmax())
    at = (flat // ratio.shape[1], flat % ratio.shape[1])
    worst = float(ratio.flatten()[flat])
    assert worst <= 1.0, (f"{what}: {int((ratio > 1.0).sum())} of {ratio.numel()} elements beyond their tolerance, worst {worst:.3f} x at {at}: "
                          f"got {float(g[at]):.9g} want {float(want[at]):.9g} tol {float(tol[at]):.3g}")
    return worst, at
