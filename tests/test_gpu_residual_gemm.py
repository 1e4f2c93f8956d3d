"""The two residual producers of a transformer block held element by element: clipmi_gemm_residual_f16 (fp16 stream; the entry point that reaches
gemm_rstream_kernel, csrc/gemm_rstream.hip) and clipmi_gemm_residual_fold (fp32 stream), through the C entry points, under every dispatch, against the
float64 reference, the per-element tolerance and the 2^-19 partial bound of tests/residual_gemm_ref.py (whose teeth tests/test_residual_gemm_ref_cpu.py
shows).  Needs a real MI355X.

  1 x 8 x 64, 7 x 8 x 64    fewer rows than one MFMA row group, one 8-column store
  300 x 264 x 128           ragged M inside 128-, 256- and 320-row tiles; a last column tile of 8; two K-steps, the ping-pong loop's minimum
  321 x 264 x 64            one K-step (variant 10 falls back to 1); one row beyond a 320-row tile
  600 x 520 x 576           nine K-steps (odd), 3 x 3 tiles, a last column tile of 8
  333 x 512 x 3072          48 K-steps: the shape that decides C_ACC
  300 x 1672 x 128          7 partials of 256 columns; 14 of 128 would be beyond the 8 that `stats` holds: forced 0 must report 7
  the four row-range shapes (residual_gemm_ref.ROW_RANGE at this device's CU count), fp16 stream under the default dispatch and forced 16: the tile
  structures where gemm_rstream_kernel's uniform branches differ -- 8, 9 and 10 pairs; one, two and three tiles per range; 7 K-steps; odd and even
  K-step counts.  The test asserts that the mirrored dispatch rule (rstream_plan) says the shape is taken with the named structures.  No test can
  observe which kernel ran: that rests on the mirror.

Every case runs twice into fresh buffers and must give the same bits, outputs and partials alike; checks every element and every partial; prints the
worst error / tolerance and where it is.  `stats` is always its full 8 * M * 2 floats plus a guard, patterned: nothing beyond parts * M * 2 floats may
be written.  `*parts` must be what residual_gemm_ref.expected_parts mirrors from the launcher: (N + 255) / 256, except from the 128 x 128 kernel
((N + 127) / 128 while that is at most 8) -- which runs under forced variant 0 and where the unforced cost model picks it for a small problem.

The strided cases use lda = K + 8, ldw = K + 16, ldx = N + 8: NaN in the operands' padding columns poisons any product that touches them; the padding
columns of x / x16 and one guard row behind them carry a finite pattern that must keep its bits.  The exact cases (residual_gemm_ref.exact_case) need
no tolerance: outputs and partials are the float64 integers bit for bit, so every dispatch agrees with every other.  The refused calls return
CLIPMI_ERR_ARG or CLIPMI_ERR_SHAPE and write nothing.
"""
import ctypes

import pytest
import torch

import residual_gemm_ref as ref
from clip_calibration_amd import _lib

pytestmark = pytest.mark.gpu

DISPATCH = [("f16", v) for v in (None, 0, 1, 10, 16)] + [("fold", v) for v in (None, 0, 1, 10)]
PATTERN = {torch.float16: 0x5A3C, torch.float32: 0x5A3C1E0F}     # finite, unlike anything the operands produce
INT = {torch.float16: torch.int16, torch.float32: torch.int32}
STATS_GUARD = 64

_cache = {}      # one shape at a time: operands and references on the device, per stream type and kind


def did(entry, variant):
    return f"{entry}-{'default' if variant is None else f'v{variant}'}"


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def row_range(i):
    """(M, N, K) of row-range shape i on this device, and the tile structures it must produce."""
    (N, K, ln, extra, cut), named = ref.ROW_RANGE[i]
    return (ref.rstream_shape(cus(), N, ln, extra, cut), N, K), named


def problem(shape, f16_stream, kind="plain"):
    if _cache.get("shape") != shape:
        _cache.clear()
        torch.cuda.empty_cache()
        _cache["shape"] = shape
    key = (kind, f16_stream)
    if key not in _cache:
        M, N, K = shape
        if kind == "plain":
            a, w, bias, x_old = (t.cuda() for t in ref.operands(M, N, K, f16_stream)[:4])
            want, _, tol = ref.expected(a, w, bias, x_old, f16_stream)
        else:
            a, w, bias, x_old = (t.cuda() for t in ref.exact_case(M, N, K, M + K, f16_stream))
            want, tol = ref.exact_result(a, w, bias, x_old), None
        _cache[key] = dict(a=a, w=w, bias=bias, x_old=x_old, want=want, tol=tol)
    return _cache[key]


def patterned(shape, dtype):
    return torch.full(shape, PATTERN[dtype], dtype=INT[dtype], device="cuda").view(dtype)


def bits(t):
    return t.view(INT[t.dtype])


def untouched(t):
    return bool((bits(t) == PATTERN[t.dtype]).all())


def padded(t, ld):
    p = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device=t.device)
    p[:, :t.shape[1]] = t
    return p


def call(entry, a, lda, w, ldw, bias, x, x16, ldx, stats, parts, M, N, K):
    s = torch.cuda.current_stream().cuda_stream
    pp = None if parts is None else ctypes.byref(parts)
    if entry == "f16":
        return _lib.lib.clipmi_gemm_residual_f16(a.data_ptr(), lda, w.data_ptr(), ldw, bias.data_ptr(), x16.data_ptr(), ldx, stats.data_ptr(), pp, M, N, K, s)
    return _lib.lib.clipmi_gemm_residual_fold(a.data_ptr(), lda, w.data_ptr(), ldw, bias.data_ptr(), x.data_ptr(), ldx, x16.data_ptr(), stats.data_ptr(),
                                              pp, M, N, K, s)


def launch(entry, p, shape, strided):
    """One launch into fresh buffers.  Returns (stream buffer, x16 buffer or None, stats buffer, parts, (lda, ldw, ldx))."""
    M, N, K = shape
    fold = entry == "fold"
    lda, ldw, ldx = (K + 8, K + 16, N + 8) if strided else (K, K, N)
    a, w = (padded(p["a"], lda), padded(p["w"], ldw)) if strided else (p["a"], p["w"])
    dtype = torch.float32 if fold else torch.float16
    if strided:       # padding columns and one guard row of the pattern
        xbuf = patterned((M + 1, ldx), dtype)
        xbuf[:M, :N] = p["x_old"]
        x16buf = patterned((M + 1, ldx), torch.float16) if fold else None
    else:             # x16 of the fp32 stream starts from NaN: an element that no workgroup writes has to show
        xbuf = p["x_old"].clone()
        x16buf = torch.full((M, N), float("nan"), dtype=torch.float16, device="cuda") if fold else None
    stats = patterned((8 * M * 2 + STATS_GUARD,), torch.float32)
    parts = ctypes.c_int(-1)
    rc = call(entry, a, lda, w, ldw, p["bias"], xbuf, x16buf if fold else xbuf, ldx, stats, parts, M, N, K)
    assert rc == _lib.OK, _lib.last_error()
    return xbuf, x16buf, stats, parts.value, (lda, ldw, ldx)


def run_case(entry, variant, shape, clipmi_option, kind="plain", strided=False, named=None):
    M, N, K = shape
    fold = entry == "fold"
    p = problem(shape, not fold, kind)
    if variant is not None:
        clipmi_option("gemm_variant", variant)
    runs = [launch(entry, p, shape, strided) for _ in range(2)]
    torch.cuda.synchronize()
    xbuf, x16buf, stats, parts, (lda, ldw, ldx) = runs[0]
    tag = (f"residual-matrix: {M}x{N}x{K} {entry} {'default' if variant is None else variant}"
           f"{' exact' if kind == 'exact' else ''}{' lda+8 ldw+16 ldx+8' if strided else ''}")

    if named is not None and not fold and variant in (None, 16):      # the row-range kernel must be the one that ran
        plan = ref.rstream_plan(cus(), M, N, K, ldx, lda, ldw)
        print(f"{tag}: {cus()} CUs, M = {M}: row-range tile structures {sorted(plan) if plan else plan}")
        assert plan == named, f"the mirrored dispatch rule gives {plan}, not {named}"
    want_parts = ref.expected_parts(variant, cus(), M, N, K, not fold, ldx, lda, ldw)
    assert parts == want_parts, f"*parts = {parts}, the launcher's rule gives {want_parts}"
    if variant in (1, 10, 16):
        assert parts == ref.cdiv(N, 256)
    if variant == 0:
        assert parts == (ref.cdiv(N, 128) if ref.cdiv(N, 128) <= 8 else ref.cdiv(N, 256))
    w_part = ref.part_width(parts, N)

    got = xbuf[:M, :N]
    if kind == "exact":
        assert torch.equal(got.double(), p["want"]), f"{tag}: {int((got.double() != p['want']).sum())} outputs are not the exact integers"
        s, q, _ = ref.tile_sums(p["want"], w_part)
        st = stats[:parts * M * 2].view(parts, M, 2).double()
        assert torch.equal(st[..., 0], s) and torch.equal(st[..., 1], q), f"{tag}: partials are not the exact integers"
        print(f"{tag}: {parts} partials of {w_part}: outputs and partials exact")
    else:
        worst, at = ref.check(got, p["want"], p["tol"], tag)
        pworst, pat = ref.check_partials(stats[:parts * M * 2].view(parts, M, 2), got, w_part, tag)
        print(f"{tag}: worst error / tolerance {worst:.3f} at {at}; {parts} partials of {w_part}: worst error / bound {pworst:.3f} at {pat}")
    if fold:
        assert torch.equal(bits(x16buf[:M, :N]), bits(got.half())), f"{tag}: x16 is not fp16(x) of the kernel's own x"
    assert untouched(stats[parts * M * 2:]), f"{tag}: `stats` written beyond parts * M * 2 floats"
    if strided:
        for buf in (xbuf, x16buf) if fold else (xbuf,):
            assert untouched(buf[:M, N:]) and untouched(buf[M:]), f"{tag}: padding columns or the guard row were written"
    for b0, b1 in zip(runs[0][:3], runs[1][:3]):
        if b0 is not None:
            assert torch.equal(bits(b0), bits(b1)), f"{tag}: a second launch gives other bits"
    assert runs[1][3] == parts


@pytest.mark.parametrize("entry,variant", DISPATCH, ids=[did(*d) for d in DISPATCH])
@pytest.mark.parametrize("shape", ref.SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matrix(clipmi_option, shape, entry, variant):
    assert ref.rstream_plan(cus(), *shape) is None      # small shapes: the tile kernels, under forced 16 through the fall-back
    run_case(entry, variant, shape, clipmi_option)


@pytest.mark.parametrize("variant", [None, 16], ids=["default", "v16"])
@pytest.mark.parametrize("i", range(len(ref.ROW_RANGE)), ids=[f"N{s[0]}-K{s[1]}-len{s[2]}+{s[3]}" for s, _ in ref.ROW_RANGE])
def test_row_range_shapes(clipmi_option, i, variant):
    shape, named = row_range(i)
    run_case("f16", variant, shape, clipmi_option, named=named)


@pytest.mark.parametrize("variant", [None, 16], ids=["default", "v16"])
def test_one_pair_short_falls_back(clipmi_option, variant):
    """groups * 8 - 1 pairs: some range would hold 7 pairs, the row-range kernel is not taken, and the call is correct through the tile kernels."""
    N, K, ln, extra, cut = ref.ONE_PAIR_SHORT
    M = ref.rstream_shape(cus(), N, ln, extra, cut)
    assert ref.rstream_plan(cus(), M, N, K, N) is None
    run_case("f16", variant, (M, N, K), clipmi_option)


STRIDED = [(300, 264, 128), (600, 520, 576), 0, 2]


@pytest.mark.parametrize("entry,variant", DISPATCH, ids=[did(*d) for d in DISPATCH])
@pytest.mark.parametrize("which", STRIDED, ids=["300x264x128", "600x520x576", "row-range-1", "row-range-3"])
def test_strides_and_guards(clipmi_option, which, entry, variant):
    shape, named = row_range(which) if isinstance(which, int) else (which, None)
    run_case(entry, variant, shape, clipmi_option, strided=True, named=named)


EXACT = [((600, 520, 576), e, v) for e, v in DISPATCH] + [(i, e, v) for i in (1, 3) for e, v in DISPATCH if v in (None, 16, 10)]


@pytest.mark.parametrize("which,entry,variant", EXACT,
                         ids=[f"{'x'.join(map(str, w)) if isinstance(w, tuple) else f'row-range-{w + 1}'}-{did(e, v)}" for w, e, v in EXACT])
def test_exact_case(clipmi_option, which, entry, variant):
    shape, named = row_range(which) if isinstance(which, int) else (which, None)
    run_case(entry, variant, shape, clipmi_option, kind="exact", named=named)


@pytest.mark.parametrize("entry", ["f16", "fold"])
@pytest.mark.parametrize("what", ["N % 8", "ldx % 8", "bias", "parts"])
def test_refusals(entry, what):
    M, N, K = 300, 264, 128
    fold = entry == "fold"
    p = problem((M, N, K), not fold)
    ldx, bias, parts = N, p["bias"], ctypes.c_int(-1)
    if what == "N % 8":
        N = 260                                    # ldx stays 264: only N is wrong
    elif what == "ldx % 8":
        ldx = N + 4
    elif what == "bias":
        bias = torch.zeros(N + 4, device="cuda")[1:N + 1]      # 4 bytes off the 16-byte alignment the f32x4 loads need
        bias.copy_(p["bias"])
        assert bias.data_ptr() % 16 == 4
    else:
        parts = None
    dtype = torch.float32 if fold else torch.float16
    xbuf = patterned((M + 1, ldx), dtype)
    x16buf = patterned((M + 1, ldx), torch.float16) if fold else None
    stats = patterned((8 * M * 2 + STATS_GUARD,), torch.float32)
    rc = call(entry, p["a"], K, p["w"], K, bias, xbuf, x16buf if fold else xbuf, ldx, stats, parts, M, N, K)
    torch.cuda.synchronize()
    assert rc in (_lib.ERR_ARG, _lib.ERR_SHAPE), f"rc = {rc}"
    assert parts is None or parts.value in (-1, 0)
    assert untouched(xbuf) and untouched(stats) and (x16buf is None or untouched(x16buf)), "a refused call wrote a buffer"
