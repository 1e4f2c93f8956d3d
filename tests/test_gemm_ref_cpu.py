"""The checker of tests/test_gpu_gemm_matrix.py has teeth (tests/gemm_ref.py; CPU only).

For every shape of the GPU matrix and every (epilogue, output type) pair -- every K whole; M* is that of a 64-CU device (2344 rows: the element-wise
float64 work on 9256 x 1672 is what would take seconds here, not K), the split case is its checked rows --

* the emulation (the reference's fp32 arithmetic, gemm_ref.emulate; for gelu to fp16 also its twice-rounded form) passes ``check`` with a worst
  error / tolerance <= 0.5, so the reference alone stays well inside and a failure on the GPU means the kernel;
* its accumulation error in front of the output rounding is <= 2^-21 * reach, which is what keeps C_ACC = 2^-20 (printed per K);
* each seeded corruption of the emulation's output makes ``check`` fail:
    bias      the bias left out on the last 4 columns (epilogues with a bias);
    swap      rows M - 2 and M - 1, inside the last ragged row tile, swapped (M >= 2);
    colgroup  the last 16-column group [g0, N), g0 = (N - 1) // 16 * 16, taken from the group in front of it (N >= 32);
    shift     the rows from M // 256 * 256 on computed from ``a`` one row further on -- the off-by-one of a sliced launch (two such rows or more);
    ulp4      one element of a 1/64-scaled row moved by 4 ulp of the output type, away from the exact value (M >= 2: one row has no scaled row).
  ulp4 and the bound: the element is the seeded pick among the scaled rows' elements whose tolerance is below 4 ulp, and with an fp16 output the
  test asserts that there are such elements (cancelled sums, whose tolerance is the accumulation term, and mantissas at the top of a binade, where
  FACTOR * 2^-11 |want| is 4 ulp itself, are not among them).  With an fp32 output there are none, by arithmetic and not by measurement: 4 ulp <=
  2^-21 |want| <= 2^-21 reach, below the FACTOR * C_ACC * reach = 2^-19 reach that any order of an fp32 sum is allowed -- the test asserts exactly
  that, and that the move stays inside the bound.
"""
import functools

import pytest
import torch

import gemm_ref as ref

def cpu_shape(shape):
    M, N, K = shape
    if M is None:
        M = ref.m_star(64)[0]
    return M, N, K, (ref.split_rows(M) if shape == ref.SPLIT_SHAPE else None)


SHAPES = ref.SHAPES + [ref.SPLIT_SHAPE]
IDS = ["x".join("M*" if v is None else str(v) for v in s) for s in SHAPES]


@functools.lru_cache(maxsize=2)
def problem(shape):
    M, N, K, rows = cpu_shape(shape)
    a, w, bias, res, small_rows, small_cols = ref.operands(M, N, K)
    if rows is not None:            # the split case is checked on row ranges only
        a, res, small_rows = a[rows], res[rows], small_rows[rows]
    return a, w, bias, res, small_rows, small_cols


@functools.lru_cache(maxsize=8)
def exact(shape, epi):
    a, w, bias, res = problem(shape)[:4]
    return ref.reference(a, w, bias, res, epi)


def ulp(x, f16_out):
    """Spacing of the output type at |x| (subnormals: the smallest spacing)."""
    e = torch.floor(torch.log2(x.double().abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, (e.clamp_min(-14.0) - 10.0) if f16_out else (e.clamp_min(-126.0) - 23.0))


def corruptions(shape, epi, f16_out, emu, want, tol):
    """name -> corrupted copy of ``emu`` (or None where the corruption does not exist at this shape / epilogue)."""
    a, w, bias, res, small_rows, _ = problem(shape)
    M, N = emu.shape
    out = {}

    c = None
    if epi != "none":
        b = bias.clone()
        b[-4:] = 0.0
        c = ref.emulate(a, w, b, res, epi, f16_out)
    out["bias"] = c

    c = None
    if M >= 2:
        c = emu.clone()
        c[M - 2], c[M - 1] = emu[M - 1], emu[M - 2]
    out["swap"] = c

    c = None
    g0 = (N - 1) // 16 * 16
    if g0 >= 16:
        c = emu.clone()
        c[:, g0:N] = emu[:, g0 - 16:g0 - 16 + (N - g0)]
    out["colgroup"] = c

    c = None
    r0 = M // 256 * 256
    if shape == ref.SPLIT_SHAPE:
        r0 = 300 + 300          # the cut of the real launch, in the checked rows' numbering
    if M - r0 >= 2:
        c = emu.clone()
        shifted = torch.roll(a[r0:], -1, dims=0)
        c[r0:] = ref.emulate(shifted, w, bias, res[r0:], epi, f16_out)
    out["shift"] = c

    four = 4.0 * ulp(emu, f16_out)
    eligible = (four > tol * (1.0 + 2.0 ** -20)) & small_rows[:, None] & (emu != 0)
    if not bool(small_rows.any()):          # M = 1: no scaled row
        out["ulp4"] = None
    elif not f16_out:
        assert not bool(eligible.any()), "4 ulp of fp32 cannot exceed FACTOR * C_ACC * reach"
        assert bool((four <= 2.0 ** -21 * exact(shape, epi)[1] * (1.0 + 2.0 ** -20)).all())
        out["ulp4"] = None
    else:
        idx = torch.nonzero(eligible)
        assert idx.shape[0] > 0, "no element of a 1/64-scaled row has a tolerance below 4 ulp"
        g = torch.Generator().manual_seed(M + N)
        m, n = (int(v) for v in idx[int(torch.randint(idx.shape[0], (1,), generator=g))])
        away = 1.0 if float(emu[m, n]) >= float(want[m, n]) else -1.0
        c = emu.clone()
        c[m, n] = float(emu[m, n]) + away * float(four[m, n])       # exact: a multiple of the spacing, inside the format's range
        assert float(c[m, n]) == float(emu[m, n]) + away * float(four[m, n])
        out["ulp4"] = c
    return out


@pytest.mark.parametrize("epi,f16_out", ref.PAIRS, ids=[f"{e}-{'f16' if h else 'f32'}" for e, h in ref.PAIRS])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_emulation_passes_and_corruptions_fail(shape, epi, f16_out):
    a, w, bias, res, small_rows, small_cols = problem(shape)
    want, reach, pre = exact(shape, epi)
    tol = ref.tolerance(want, reach, pre, epi, f16_out)
    K = a.shape[1]
    acc = ref.accumulation_error(a, w, bias, res, pre, reach, epi)
    print(f"gemm-ref: {a.shape[0]}x{w.shape[0]}x{K} {epi}: fp32 evaluation within 2^{torch.log2(torch.tensor(max(acc, 1e-300))).item():.2f} * reach of float64")
    assert acc <= 2.0 ** -21, "the reference's own accumulation no longer justifies C_ACC = 2^-20"
    emu = ref.emulate(a, w, bias, res, epi, f16_out)
    worst, at = ref.check(emu, want, tol, "emulation")
    print(f"gemm-ref: {a.shape[0]}x{w.shape[0]}x{K} {epi} {'f16' if f16_out else 'f32'}: emulation worst error / tolerance {worst:.3f} at {at}")
    assert worst <= 0.5
    if epi == "gelu" and f16_out:
        twice, at2 = ref.check(ref.emulate(a, w, bias, res, epi, True, twice=True), want, tol, "twice-rounded emulation")
        print(f"gemm-ref: {a.shape[0]}x{w.shape[0]}x{K} gelu f16: twice-rounded emulation {twice:.3f} at {at2}")
        # <= 0.5 by construction above the subnormal range; inside it both roundings are absolute, 2^-25 each, the first through a slope of 1/2
        # at zero: (1/2 + 1) * 2^-25 against the floor of 2^-24
        assert twice <= 0.75
    applied = []
    for name, bad in corruptions(shape, epi, f16_out, emu, want, tol).items():
        if bad is None:
            continue
        with pytest.raises(AssertionError):
            ref.check(bad, want, tol, name)
        applied.append(name)
    M, N = emu.shape
    expected = [n for n, there in (("bias", epi != "none"), ("swap", M >= 2), ("colgroup", N >= 32), ("shift", M >= 2), ("ulp4", f16_out and M >= 2)) if there]
    assert applied == expected, f"corruptions applied {applied}, expected {expected}"


def test_ulp4_within_fp32_bound_is_accepted():
    """The other side of ulp4: a move the bound allows is not refused (the checker is a bound, not a bitwise comparison)."""
    shape = (300, 260, 128)
    a, w, bias, res, small_rows, _ = problem(shape)
    want, reach, pre = exact(shape, "none")
    tol = ref.tolerance(want, reach, pre, "none", False)
    emu = ref.emulate(a, w, bias, res, "none", False)
    m = int(torch.nonzero(small_rows)[0])
    moved = emu.clone()
    moved[m, 0] = float(emu[m, 0]) + 4.0 * float(ulp(emu, False)[m, 0])
    ref.check(moved, want, tol, "4 ulp of fp32")


def test_check_refuses_non_finite_and_reports_the_element():
    want = torch.zeros(3, 4, dtype=torch.float64)
    tol = torch.full((3, 4), 1e-3, dtype=torch.float64)
    got = torch.zeros(3, 4)
    assert ref.check(got, want, tol) == (0.0, (0, 0))
    got[2, 1] = 5e-4
    assert ref.check(got, want, tol)[1] == (2, 1)
    got[1, 3] = 2e-3
    with pytest.raises(AssertionError, match=r"\(1, 3\)"):
        ref.check(got, want, tol)
    got[1, 3] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        ref.check(got, want, tol)


def test_m_star():
    assert ref.m_star(256) == (9256, 259, 256)
    for cus in (8, 64, 228, 256, 304):
        M, tiles, grid = ref.m_star(cus)
        assert tiles > grid and tiles - 7 <= grid and (M + 255) // 256 * 7 == tiles and M % 256 == 40
