"""clipmi_gemm_f16's plain entry point held element by element (csrc/gemm.hip): every epilogue of the base call with both output types, under every
dispatch, at the smallest shapes at which each mechanism is live, against the float64 reference and the per-element tolerance of tests/gemm_ref.py
(whose teeth tests/test_gemm_ref_cpu.py shows).  Needs a real MI355X.

  1 x 8 x 64, 7 x 4 x 64   fewer rows than one MFMA row group; N = 4 is one f16x4 store of the direct fp16 epilogue
  300 x 260 x 128          N % 8 == 4: the direct fp16 epilogue (quick_gelu_h_tile there) on every tile kernel; ragged M inside 128-, 256- and 320-row
                           tiles; two K-steps, the ping-pong loop's minimum
  321 x 264 x 64           one K-step (variant 10 falls back to 1); one row beyond a 320-row tile; a last column tile of 8 on the staged path
  600 x 520 x 576          nine K-steps (odd, for the two-buffer parity), 3 x 3 tiles, a last column tile of 8; forced 13 runs gemm_stream_kernel with one
                           tile per workgroup
  M* x 1672 x 512          gemm_stream_kernel's minimum of eight K-steps; seven column tiles = a band of 4 and a narrower last band of 3 (mg_gw_last), a
                           ragged last column tile of 136; M* (gemm_ref.m_star) is the smallest M with more tiles than the persistent grid, so some
                           workgroups change tile with outputs held across the change
  333 x 512 x 3072         48 K-steps: the shape that decides C_ACC

Forced variant 13 takes the persistent kernel only with an fp16 output, N % 8 == 0, ldo % 8 == 0 and K >= 512 (launch_one); everything else it sends to
the 256 x 256 tiles, as the default dispatch does below 1.4 rounds of tiles.  Every case starts from an ``out`` of NaN (or of the guard pattern), checks every element,
prints the worst error / tolerance and its (m, n), and asserts that a second launch gives the same bits.  The strided cases call the C entry point with lda = K + 8, ldw = K + 16, ldo = N + 8 or
N + 4: NaN in the operands' padding columns poisons any product that touches them, and the padding columns of ``out`` and a guard row behind it must
keep their bit pattern.
"""
import pytest
import torch

import gemm_ref as ref
from clip_calibration_amd import _lib

pytestmark = pytest.mark.gpu

EPI = {"none": _lib.EPI_NONE, "bias": _lib.EPI_BIAS, "gelu": _lib.EPI_BIAS_QUICKGELU, "residual": _lib.EPI_BIAS_RESIDUAL}
VARIANTS = [None, 0, 1, 10, 13]
# (epilogue, fp16 output, residual in place): the matrix, the residual once in place as the towers run it and once out of place
CASES = [(e, h, False) for e, h in ref.PAIRS] + [("residual", False, True)]
CASE_IDS = [f"{e}-{'f16' if h else 'f32'}{'-inplace' if ip else ''}" for e, h, ip in CASES]
SHAPE_IDS = ["x".join("M*" if v is None else str(v) for v in s) for s in ref.SHAPES]
PATTERN = {torch.float16: 0x5A3C, torch.float32: 0x5A3C1E0F}     # finite, unlike anything the operands produce
INT = {torch.float16: torch.int16, torch.float32: torch.int32}

_problem = {}      # one shape at a time: operands on the device and the references of the epilogues asked for so far


def resolve(shape):
    M, N, K = shape
    if M is None:
        M, tiles, grid = ref.m_star(torch.cuda.get_device_properties(0).multi_processor_count)
        # more 256 x 256 tiles than persistent workgroups: some workgroup changes tile
        assert tiles > grid and (M + 255) // 256 * ((N + 255) // 256) == tiles
    return M, N, K


def problem(shape, rows=None):
    key = (shape, None if rows is None else rows.numel())
    if _problem.get("key") != key:
        _problem.clear()
        torch.cuda.empty_cache()
        M, N, K = resolve(shape)
        a, w, bias, res, _, _ = ref.operands(M, N, K)
        _problem.update(key=key, M=M, N=N, K=K, a=a.cuda(), w=w.cuda(), bias=bias.cuda(), res=None if rows is not None else res.cuda(), ref={})
    return _problem


def expected(p, epi, f16_out, rows=None):
    """(want, tol) float64 on the device, computed once per shape and epilogue."""
    if (epi, f16_out) not in p["ref"]:
        a = p["a"] if rows is None else p["a"][rows.cuda()]
        want, reach, pre = ref.reference(a, p["w"], p["bias"], p["res"], epi)
        p["ref"][(epi, f16_out)] = (want, ref.tolerance(want, reach, pre, epi, f16_out))
    return p["ref"][(epi, f16_out)]


def gemm(a, lda, w, ldw, bias, residual, out, ldo, M, N, K, epi):
    return _lib.lib.clipmi_gemm_f16(a.data_ptr(), lda, w.data_ptr(), ldw, None if bias is None else bias.data_ptr(),
                                    None if residual is None else residual.data_ptr(), out.data_ptr(), ldo,
                                    _lib.F16 if out.dtype == torch.float16 else _lib.F32, M, N, K, EPI[epi], torch.cuda.current_stream().cuda_stream)


def padded(t, ld, fill=float("nan"), guard_rows=0):
    """[rows + guard_rows, ld] with ``t`` in the leading columns and ``fill`` everywhere else."""
    p = torch.full((t.shape[0] + guard_rows, ld), fill, dtype=t.dtype, device=t.device)
    p[:t.shape[0], :t.shape[1]] = t
    return p


def patterned(M, N, ldo, dtype):
    """[M + 1, ldo] of the guard pattern: M rows of ``out`` with their padding columns, and one guard row behind them."""
    return torch.full((M + 1, ldo), PATTERN[dtype], dtype=INT[dtype], device="cuda").view(dtype)


def guard_intact(buf, M, N):
    bits = buf.view(INT[buf.dtype])
    return bool((bits[:M, N:] == PATTERN[buf.dtype]).all()) and bool((bits[M:] == PATTERN[buf.dtype]).all())


def set_variant(clipmi_option, variant):
    if variant is not None:
        clipmi_option("gemm_variant", variant)


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "default" if v is None else f"v{v}")
@pytest.mark.parametrize("epi,f16_out,in_place", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=SHAPE_IDS)
def test_matrix(clipmi_option, shape, epi, f16_out, in_place, variant):
    p = problem(shape)
    M, N, K = p["M"], p["N"], p["K"]
    want, tol = expected(p, epi, f16_out)
    set_variant(clipmi_option, variant)
    dtype = torch.float16 if f16_out else torch.float32
    outs = []
    for _ in range(2):
        # NaN, not torch.empty: the allocator hands back the block of the previous case, which holds that case's (correct) result -- an
        # element that no workgroup writes has to show
        out = p["res"].clone() if in_place else torch.full((M, N), float("nan"), dtype=dtype, device="cuda")
        residual = None if epi != "residual" else out if in_place else p["res"]
        rc = gemm(p["a"], K, p["w"], K, None if epi == "none" else p["bias"], residual, out, N, M, N, K, epi)
        assert rc == _lib.OK, _lib.last_error()
        outs.append(out)
    torch.cuda.synchronize()
    worst, at = ref.check(outs[0], want, tol, f"{M}x{N}x{K} {epi}")
    print(f"gemm-matrix: {M}x{N}x{K} {CASE_IDS[CASES.index((epi, f16_out, in_place))]} {'default' if variant is None else variant}: "
          f"worst error / tolerance {worst:.3f} at {at}")
    assert torch.equal(outs[0], outs[1]), "a second launch gives other bits"


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "default" if v is None else f"v{v}")
@pytest.mark.parametrize("epi,f16_out,in_place,ldo_pad", [(e, h, ip, pad) for e, h, ip in CASES for pad in ((8, 4) if h else (4,))],
                         ids=[f"{i}-ldo+{pad}" for i, (e, h, ip) in zip(CASE_IDS, CASES) for pad in ((8, 4) if h else (4,))])
@pytest.mark.parametrize("shape", [(300, 260, 128), (600, 520, 576)], ids=["300x260x128", "600x520x576"])
def test_strides_and_padding(clipmi_option, shape, epi, f16_out, in_place, ldo_pad, variant):
    """lda, ldw and ldo beyond the row length; fp16 output with ldo = N + 4 takes the direct epilogue through ``ldo & 7`` also where N % 8 == 0."""
    p = problem(shape)
    M, N, K = p["M"], p["N"], p["K"]
    want, tol = expected(p, epi, f16_out)
    set_variant(clipmi_option, variant)
    dtype = torch.float16 if f16_out else torch.float32
    lda, ldw, ldo = K + 8, K + 16, N + ldo_pad
    a, w = padded(p["a"], lda), padded(p["w"], ldw)
    outs = []
    for _ in range(2):
        out = patterned(M, N, ldo, dtype)
        residual = None
        if epi == "residual":                      # the residual shares ldo: the kernels read residual + row * ldo
            if in_place:
                out[:M, :N] = p["res"]
                residual = out
            else:
                residual = padded(p["res"], ldo)
        rc = gemm(a, lda, w, ldw, None if epi == "none" else p["bias"], residual, out, ldo, M, N, K, epi)
        assert rc == _lib.OK, _lib.last_error()
        outs.append(out)
    torch.cuda.synchronize()
    worst, at = ref.check(outs[0][:M, :N], want, tol, f"{M}x{N}x{K} {epi} strided")
    print(f"gemm-matrix: {M}x{N}x{K} lda+8 ldw+16 ldo+{ldo_pad} {CASE_IDS[CASES.index((epi, f16_out, in_place))]} "
          f"{'default' if variant is None else variant}: worst error / tolerance {worst:.3f} at {at}")
    assert guard_intact(outs[0], M, N), "padding columns or the guard row of `out` were written"
    assert torch.equal(outs[0].view(INT[dtype]), outs[1].view(INT[dtype])), "a second launch gives other bits"


@pytest.mark.parametrize("epi", ["none", "gelu"])
def test_split_tail_launch_with_strides(epi):
    """16448 x 3072 x 768 to fp16 under the default dispatch: 65 x 12 tiles, the last tile row 64 rows high -- on 256 CUs gemm_split_rows cuts a tail
    launch at A + head * lda and out + head * ldo (launch_one), head = 16384.  lda = K + 8, ldw = K + 16, ldo = N + 8; checked on rows 0..299, head - 300 ..
    head + 64 and the last 300, and on every padding column and the guard row."""
    M, N, K = ref.SPLIT_SHAPE
    rows = ref.split_rows(M)
    p = problem(ref.SPLIT_SHAPE, rows)
    want, tol = expected(p, epi, True, rows)
    lda, ldw, ldo = K + 8, K + 16, N + 8
    a, w = padded(p["a"], lda), padded(p["w"], ldw)
    outs = []
    for _ in range(2):
        out = patterned(M, N, ldo, torch.float16)
        rc = gemm(a, lda, w, ldw, None if epi == "none" else p["bias"], None, out, ldo, M, N, K, epi)
        assert rc == _lib.OK, _lib.last_error()
        outs.append(out)
    torch.cuda.synchronize()
    worst, at = ref.check(outs[0][rows.cuda(), :N], want, tol, f"{M}x{N}x{K} {epi} split")
    print(f"gemm-matrix: {M}x{N}x{K} lda+8 ldw+16 ldo+8 {epi}-f16 default: worst error / tolerance {worst:.3f} at row {int(rows[at[0]])} column {at[1]}")
    assert bool(torch.isfinite(outs[0][:M, :N]).all())
    assert guard_intact(outs[0], M, N), "padding columns or the guard row of `out` were written"
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "a second launch gives other bits"


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "default" if v is None else f"v{v}")
def test_residual_to_fp16_is_refused(clipmi_option, variant):
    p = problem((300, 260, 128))
    M, N, K = p["M"], p["N"], p["K"]
    set_variant(clipmi_option, variant)
    out = patterned(M, N, N, torch.float16)
    rc = gemm(p["a"], K, p["w"], K, p["bias"], p["res"], out, N, M, N, K, "residual")
    torch.cuda.synchronize()
    assert rc == _lib.ERR_ARG
    assert bool((out.view(torch.int16) == PATTERN[torch.float16]).all()), "a refused call wrote `out`"


@pytest.mark.parametrize("epi,f16_out", [(e, h) for e, h in ref.PAIRS if e != "none"], ids=[f"{e}-{'f16' if h else 'f32'}" for e, h in ref.PAIRS if e != "none"])
def test_unaligned_bias_is_refused(epi, f16_out):
    p = problem((300, 260, 128))
    M, N, K = p["M"], p["N"], p["K"]
    dtype = torch.float16 if f16_out else torch.float32
    shifted = torch.zeros(N + 4, device="cuda")[1:N + 1]      # 4 bytes off the 16-byte alignment the f32x4 loads need
    shifted.copy_(p["bias"])
    assert shifted.data_ptr() % 16 == 4
    out = patterned(M, N, N, dtype)
    rc = gemm(p["a"], K, p["w"], K, shifted, p["res"] if epi == "residual" else None, out, N, M, N, K, epi)
    torch.cuda.synchronize()
    assert rc == _lib.ERR_ARG
    assert bool((out.view(INT[dtype]) == PATTERN[dtype]).all()), "a refused call wrote `out`"
