"""clipmi_gemm_ln_fold -- the LayerNorm-folded consumer GEMM (in-proj / c_fc behind a fold producer; csrc/gemm.hip) -- held element by element: both
epilogues with both output types under every dispatch, at the smallest shapes at which each mechanism is live, against the float64 reference of the
operation the entry point is given and the per-element tolerance of tests/ln_fold_ref.py (whose teeth tests/test_ln_fold_ref_cpu.py shows).  The
degenerate row classes, the consumer beyond one descriptor and the every-pattern QuickGELU table stay in tests/test_gpu_ln_fold.py.  Needs a real MI355X.

  1 x 8 x 64, 7 x 4 x 64   fewer rows than one MFMA row group; N = 4 is one f16x4 store of the direct fp16 epilogue
  300 x 260 x 128          N % 8 == 4: the direct fp16 epilogue with the fold on every tile kernel; ragged M inside 128-, 256- and 320-row tiles; two K-steps
  321 x 264 x 64           one K-step (variant 10 falls back to 1); one row beyond a 320-row tile; a last column tile of 8
  600 x 520 x 576          nine K-steps; forced 13 runs gemm_stream_kernel with one tile per workgroup, whose ragged last row tile reads row partials
                           past row M
  M* x 1672 x 512          gemm_stream_kernel's minimum of eight K-steps; a band of 4 and a last band of 3, a ragged column tile of 136; M*
                           (gemm_ref.m_star) has more tiles than the persistent grid: folded outputs are held across a tile change while the next
                           tile's row and column parameters arrive by DMA
  333 x 512 x 3072         48 K-steps; 8 partials with the scratch row: ln_finalize_kernel in front of the streamed kernel

test_matrix is the full {bias, gelu} x {fp16, fp32} x gemm_variant {default, 0, 1, 10, 13} cross with one statistics layout per shape
(ln_fold_ref.SHAPES).  test_layouts runs the other layouts at 300 x 260 x 128, 600 x 520 x 576 and M* x 1672 x 512: 1, 4 (RAW), 5 with and without
ln_rows and 8 partials, a plane of M + 64, a row stride of 2 and the towers' window form (the statistics pointer offset by 2 r0 floats,
ln_plane = the producer's rows) -- to fp16 under the default dispatch and forced 13 with both epilogues, and the four that matter to the tile
kernels (8 partials, plane, stride, window) under forced 0 / 1 / 10 with the bias epilogue to both types.  Every float of ``stats`` that the call
must not read is NaN.

Every case starts from an ``out`` of NaN (or of the guard pattern), runs twice into fresh buffers and asserts the same bits, checks EVERY element,
prints the worst error / tolerance with its (m, n) and the kernel the dispatch mirror (ln_fold_ref.expected_kernel) names, and asserts on that name:
no test can observe which kernel ran.  The strided cases use lda = K + 8, ldw = K + 16, ldo = N + 8 or N + 4 with NaN in the operands' padding columns;
the padding columns of ``out``, one guard row behind it and the guard behind ``ln_rows`` must keep their bits.  The exact cases
(ln_fold_ref.exact_case) need no tolerance.  The refused calls return CLIPMI_ERR_ARG and write nothing.
"""
import pytest
import torch

import gemm_ref
import ln_fold_ref as ref
from clip_calibration_amd import _lib

pytestmark = pytest.mark.gpu

EPI = {"bias": _lib.EPI_BIAS, "gelu": _lib.EPI_BIAS_QUICKGELU}
VARIANTS = [None, 0, 1, 10, 13]
PAIRS = [("bias", True), ("bias", False), ("gelu", True), ("gelu", False)]
PAIR_IDS = [f"{e}-{'f16' if h else 'f32'}" for e, h in PAIRS]
PATTERN = {torch.float16: 0x5A3C, torch.float32: 0x5A3C1E0F}     # finite, unlike anything the operands produce
INT = {torch.float16: torch.int16, torch.float32: torch.int32}
ROWS_GUARD = 64
WINDOW_R0, WINDOW_BEHIND = 37, 27

# name -> (parts, ln_rows given, plane_pad, row_stride, window)
LAYOUTS = {"p1": (1, False, 0, 1, False), "p4": (4, False, 0, 1, False), "p5-rows": (5, True, 0, 1, False), "p5": (5, False, 0, 1, False),
           "p8": (8, False, 0, 1, False), "plane+64": (4, False, 64, 1, False), "stride2": (3, False, 0, 2, False), "window": (4, False, 0, 1, True)}
LAYOUT_SHAPES = [(300, 260, 128), (600, 520, 576), (None, 1672, 512)]

_cache = {}      # one shape at a time: operands and the float64 products on the device, the cases and references asked for so far


def sid(shape):
    return "x".join("M*" if v is None else str(v) for v in shape)


def vid(v):
    return "default" if v is None else f"v{v}"


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def resolve(shape):
    M, N, K = shape
    if M is None:
        M, tiles, grid = ref.m_star(cus())
        assert tiles > grid and (M + 255) // 256 * ((N + 255) // 256) == tiles      # some workgroup of the persistent grid changes tile
    return M, N, K


def to_cuda(case):
    for k, v in vars(case).items():
        if torch.is_tensor(v):
            setattr(case, k, v.cuda())
    return case


def problem(shape, kind="plain"):
    """The cache of one (shape, kind): cleared when another is asked for."""
    key = (shape, kind)
    if _cache.get("key") != key:
        _cache.clear()
        torch.cuda.empty_cache()
        _cache.update(key=key, dims=resolve(shape), cases={}, refs={}, prod=None)
    return _cache


def plain_case(shape, layout):
    """(case on the device, window offset r0) of a statistics layout; the float64 products a @ w_f^T are computed once per shape."""
    p = problem(shape)
    M, N, K = p["dims"]
    parts, _, pad, rs, window = LAYOUTS[layout] if isinstance(layout, str) else layout
    key = (parts, pad, rs, window)
    if key not in p["cases"]:
        case = ref.operands(M, N, K, parts, plane_pad=pad, row_stride=rs)
        r0 = 0
        if window:      # the rows r0 .. r0 + M of a producer of r0 + M + WINDOW_BEHIND rows: NaN in front of and behind the window's rows
            r0, plane = WINDOW_R0, WINDOW_R0 + M + WINDOW_BEHIND
            stats = torch.full((ref.LN_MAX_PARTS, plane, 2), float("nan"))
            stats[:, r0:r0 + M] = case.stats.view(ref.LN_MAX_PARTS, M, 2)
            case.stats, case.plane = stats.reshape(-1), plane
        to_cuda(case)
        if p["prod"] is None:
            p["prod"] = ref.products(case.a, case.w_f)
        view = case.stats[2 * r0:]
        case.rows = ref.row_params(view, M, parts, case.ln_dim, case.eps, case.plane, rs)
        p["cases"][key] = (case, r0)
    return p["cases"][key]


def expected(shape, layout, epi, f16_out):
    """(want, tol) float64 on the device, once per shape, layout, epilogue and output type."""
    p = problem(shape)
    case, r0 = plain_case(shape, layout)
    parts, _, pad, rs, window = LAYOUTS[layout] if isinstance(layout, str) else layout
    key = (parts, pad, rs, window, epi, f16_out)
    if key not in p["refs"]:
        if len(p["refs"]) >= 4:      # float64 [M, N] pairs: keep a handful
            p["refs"].pop(next(iter(p["refs"])))
        mean, rstd, rho = case.rows
        want, pre, reach, t1, t2 = ref.reference(case.a, case.w_f, case.g, case.c, mean, rstd, epi, p["prod"])
        p["refs"][key] = (want, ref.tolerance(want, pre, reach, t1, t2, rho, epi, f16_out))
    return p["refs"][key]


def fold(case, r0, a, lda, w, ldw, ln_rows, out, ldo, M, N, K, epi, **kw):
    """The C entry point; ``kw`` overrides single arguments (the refusals)."""
    a_ = dict(c=case.c.data_ptr(), g=case.g.data_ptr(), stats=case.stats.data_ptr() + 8 * r0, parts=case.parts,
              plane=0 if case.plane == M else case.plane, stride=case.row_stride, ln_dim=case.ln_dim, epilogue=EPI[epi])
    a_.update(kw)
    return _lib.lib.clipmi_gemm_ln_fold(a.data_ptr(), lda, w.data_ptr(), ldw, a_["c"], a_["g"], a_["stats"], a_["parts"], a_["plane"], a_["stride"],
                                        a_["ln_dim"], case.eps, None if ln_rows is None else ln_rows.data_ptr(), out.data_ptr(), ldo,
                                        _lib.F16 if out.dtype == torch.float16 else _lib.F32, M, N, K, a_["epilogue"], torch.cuda.current_stream().cuda_stream)


def patterned(shape, dtype):
    return torch.full(shape, PATTERN[dtype], dtype=INT[dtype], device="cuda").view(dtype)


def untouched(t):
    return bool((t.view(INT[t.dtype]) == PATTERN[t.dtype]).all())


def padded(t, ld):
    p = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device=t.device)
    p[:, :t.shape[1]] = t
    return p


def scratch_rows(M):
    """[M, 2] for ln_finalize_kernel, NaN, and a patterned guard behind it."""
    buf = patterned((M * 2 + ROWS_GUARD,), torch.float32)
    buf[:M * 2] = float("nan")
    return buf


def launch_twice(case, r0, dims, epi, f16_out, with_rows, strides=None):
    """Two launches into fresh buffers.  Returns (out [M, N] view of the first, kernel-independent guard checks done)."""
    M, N, K = dims
    dtype = torch.float16 if f16_out else torch.float32
    lda, ldw, ldo = (K, K, N) if strides is None else strides
    a, w = (case.a, case.w_f) if strides is None else (padded(case.a, lda), padded(case.w_f, ldw))
    outs = []
    for _ in range(2):
        # NaN, not torch.empty: the allocator hands back the block of the previous case, which holds that case's (correct) result
        out = torch.full((M, N), float("nan"), dtype=dtype, device="cuda") if strides is None else patterned((M + 1, ldo), dtype)
        rows = scratch_rows(M) if with_rows else None
        rc = fold(case, r0, a, lda, w, ldw, rows, out, ldo, M, N, K, epi)
        assert rc == _lib.OK, _lib.last_error()
        outs.append((out, rows))
    torch.cuda.synchronize()
    (o0, r0_), (o1, r1_) = outs
    assert torch.equal(o0.view(INT[dtype]), o1.view(INT[dtype])), "a second launch gives other bits"
    if strides is not None:
        assert untouched(o0[:M, N:]) and untouched(o0[M:]), "padding columns or the guard row of `out` were written"
    if with_rows:
        assert untouched(r0_[M * 2:]), "the guard behind `ln_rows` was written"
        assert torch.equal(r0_.view(torch.int32), r1_.view(torch.int32))
    return o0[:M, :N]


def run_case(clipmi_option, shape, layout, epi, f16_out, variant, strides=None, must=None):
    case, r0 = plain_case(shape, layout)
    M, N, K = dims = problem(shape)["dims"]
    with_rows = LAYOUTS[layout][1] if isinstance(layout, str) else layout[1]
    want, tol = expected(shape, layout, epi, f16_out)
    if variant is not None:
        clipmi_option("gemm_variant", variant)
    lda, ldw, ldo = (K, K, N) if strides is None else strides
    kernel = ref.expected_kernel(M, N, K, ldo, f16_out, case.parts, with_rows, case.row_stride, variant, cus(), lda, ldw, case.plane)
    got = launch_twice(case, r0, dims, epi, f16_out, with_rows, strides)
    tag = (f"ln-fold-matrix: {M}x{N}x{K} {layout if isinstance(layout, str) else f'p{layout[0]}'}{'' if strides is None else f' lda+8 ldw+16 ldo+{ldo - N}'} "
           f"{epi}-{'f16' if f16_out else 'f32'} {vid(variant)} [{kernel}]")
    worst, at = ref.check(got, want, tol, tag)
    print(f"{tag}: worst error / tolerance {worst:.3f} at {at}")
    if must is not None:
        assert must(kernel), f"{tag}: the mirrored dispatch rule names {kernel}"
    return kernel


def streams(M, N, K, ldo, f16_out, parts, with_rows, rs, variant):
    """Whether the case must reach gemm_stream_kernel, stated from the issue's rule and this file's shapes alone (not from the mirror): forced 13, or
    the default dispatch from 1.4 rounds of tiles on; fp16 out, 8-aligned, eight K-steps, unit row stride, up to four partials or the scratch row."""
    tiles = -(-M // 256) * -(-N // 256)
    return (f16_out and N % 8 == 0 and ldo % 8 == 0 and K >= 512 and rs == 1 and (parts <= 4 or with_rows)
            and (variant == 13 or (variant is None and 5 * tiles >= 7 * cus())))


def must_be(dims, ldo, f16_out, layout, variant):
    M, N, K = dims
    parts, with_rows, _, rs, _ = LAYOUTS[layout] if isinstance(layout, str) else layout
    if streams(M, N, K, ldo, f16_out, parts, with_rows, rs, variant):
        return lambda k: k == ("stream-raw" if parts <= 4 else "stream-finalised")
    forced_tile = {0: "128x128", 1: "256x256", 13: "256x256", 10: "320x256" if K >= 128 else "256x256"}.get(variant)
    suffix = "f32" if not f16_out else "direct" if N % 8 or ldo % 8 else ""
    return lambda k: not k.startswith("stream") and k.partition("+")[2] == suffix and (forced_tile is None or k.partition("+")[0] == forced_tile)


MATRIX = [(s, (p, rows, 0, 1, False)) for s, p, rows in ref.SHAPES]


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
@pytest.mark.parametrize("epi,f16_out", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("shape,layout", MATRIX, ids=[f"{sid(s)}-p{l[0]}{'-rows' if l[1] else ''}" for s, l in MATRIX])
def test_matrix(clipmi_option, shape, layout, epi, f16_out, variant):
    dims = resolve(shape)
    kernel = run_case(clipmi_option, shape, layout, epi, f16_out, variant, must=must_be(dims, dims[1], f16_out, layout, variant))
    if variant == 13 and f16_out and dims[2] >= 512:      # the three shapes of the streamed kernel: one tile per workgroup, a tile change, 48 K-steps
        assert kernel == ("stream-finalised" if layout[0] > 4 else "stream-raw")


LAYOUT_CASES = ([(s, l, e, True, v) for s in LAYOUT_SHAPES for l in LAYOUTS for e in ("bias", "gelu") for v in (None, 13)] +
                [(s, l, "bias", h, v) for s in LAYOUT_SHAPES for l in ("p8", "plane+64", "stride2", "window") for h in (True, False) for v in (0, 1, 10)])
LAYOUT_CASES.sort(key=lambda c: LAYOUT_SHAPES.index(c[0]))      # one shape at a time: the cache holds one


@pytest.mark.parametrize("shape,layout,epi,f16_out,variant", LAYOUT_CASES,
                         ids=[f"{sid(s)}-{l}-{e}-{'f16' if h else 'f32'}-{vid(v)}" for s, l, e, h, v in LAYOUT_CASES])
def test_layouts(clipmi_option, shape, layout, epi, f16_out, variant):
    dims = resolve(shape)
    kernel = run_case(clipmi_option, shape, layout, epi, f16_out, variant, must=must_be(dims, dims[1], f16_out, layout, variant))
    if layout in ("p5", "p8", "stride2"):
        assert not kernel.startswith("stream"), "more than four partials without ln_rows, or a row stride, must leave the streamed kernel"
    if variant == 13 and f16_out and dims[2] >= 512 and layout in ("p1", "p4", "plane+64", "window"):
        assert kernel == "stream-raw"
    if variant == 13 and f16_out and dims[2] >= 512 and layout == "p5-rows":
        assert kernel == "stream-finalised"


STRIDED = [(s, l, e, h, pad, v) for s, l in (((300, 260, 128), "p4"), ((600, 520, 576), "p5-rows")) for e, h in PAIRS
           for pad in ((8, 4) if h else (4,)) for v in VARIANTS]


@pytest.mark.parametrize("shape,layout,epi,f16_out,ldo_pad,variant", STRIDED,
                         ids=[f"{sid(s)}-{l}-{e}-{'f16' if h else 'f32'}-ldo+{pad}-{vid(v)}" for s, l, e, h, pad, v in STRIDED])
def test_strides_and_guards(clipmi_option, shape, layout, epi, f16_out, ldo_pad, variant):
    """lda, ldw and ldo beyond the row length; fp16 output with ldo = N + 4 takes the direct epilogue through ``ldo & 7`` also where N % 8 == 0, and
    leaves the streamed kernel.  600 x 520 x 576 passes 5 partials and a guarded ln_rows: ln_finalize_kernel under forced 13 with ldo = N + 8."""
    M, N, K = dims = resolve(shape)
    strides = (K + 8, K + 16, N + ldo_pad)
    kernel = run_case(clipmi_option, shape, layout, epi, f16_out, variant, strides=strides, must=must_be(dims, N + ldo_pad, f16_out, layout, variant))
    if shape == (600, 520, 576) and variant == 13 and f16_out:
        assert kernel == ("stream-finalised" if ldo_pad == 8 else "256x256+direct")


@pytest.mark.parametrize("epi", ["bias", "gelu"])
def test_split_tail_launch_with_the_fold(epi):
    """16448 x 3072 x 768 to fp16 under the default dispatch with 3 partials: 65 x 12 tiles, the last tile row 64 rows high -- on 256 CUs
    gemm_split_rows cuts a tail launch at A + head * lda, out + head * ldo and stats + 2 * head (launch_one), head = 16384.  lda = K + 8,
    ldw = K + 16, ldo = N + 8; checked element-wise on rows 0..299, head - 300 .. head + 64 and the last 300, finite everywhere, guards intact."""
    shape = gemm_ref.SPLIT_SHAPE
    M, N, K = shape
    layout = (3, False, 0, 1, False)
    rows = gemm_ref.split_rows(M).cuda()
    p = problem(shape, "split")
    if not p["cases"]:
        case = to_cuda(ref.operands(M, N, K, 3))
        mean, rstd, rho = ref.row_params(case.stats, M, 3, K, case.eps)
        case.rows = (mean[rows], rstd[rows], rho[rows])
        p["cases"][0] = case
    case = p["cases"][0]
    mean, rstd, rho = case.rows
    want, pre, reach, t1, t2 = ref.reference(case.a[rows], case.w_f, case.g, case.c, mean, rstd, epi)
    tol = ref.tolerance(want, pre, reach, t1, t2, rho, epi, True)
    strides = (K + 8, K + 16, N + 8)
    kernel = ref.expected_kernel(M, N, K, N + 8, True, 3, False, 1, None, cus(), *strides[:2])
    got = launch_twice(case, 0, shape, epi, True, False, strides)
    worst, at = ref.check(got[rows], want, tol, f"{M}x{N}x{K} {epi} split")
    print(f"ln-fold-matrix: {M}x{N}x{K} p3 lda+8 ldw+16 ldo+8 {epi}-f16 default [{kernel}]: worst error / tolerance {worst:.3f} at row {int(rows[at[0]])} "
          f"column {at[1]}")
    assert bool(torch.isfinite(got).all())
    if cus() == 256:
        head = M // 256 * 256
        assert ref.split_head(M, N, None, cus()) == head
        assert kernel == f"stream-raw[0:{head}] | 128x128[{head}:{M}] stats+2*{head}", kernel
    else:
        assert kernel.startswith("stream-raw"), kernel


def exact(shape, parts, var4=False):
    p = problem(shape, "exact")
    key = (parts, var4)
    if key not in p["cases"]:
        case = to_cuda(ref.exact_case(*p["dims"], parts, var4=var4))
        case.lut = ref.quickgelu_f16_bits(case.want)
        p["cases"][key] = case
    return p["cases"][key]


def check_exact(case, got, epi, tag):
    if epi == "bias":
        bad = got.double() != case.want
        assert not bool(bad.any()), (f"{tag}: {int(bad.sum())} outputs are not the exact integers, first at {tuple(int(i) for i in torch.nonzero(bad)[0])}: "
                                     f"got {float(got[tuple(torch.nonzero(bad)[0])])} want {float(case.want[tuple(torch.nonzero(bad)[0])])}")
        return "exact"
    # gelu: against the correctly rounded fp16 activation of the integers: at most one fp16 ulp, zeros of the right sign (the criterion of
    # test_quick_gelu_every_finite_fp16_preactivation); an fp32 output is rounded to fp16 once first
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite outputs"
    bits = got.half().view(torch.int16).to(torch.int32) & 0xFFFF
    far = (ref.f16_ordinal(bits) - ref.f16_ordinal(case.lut)).abs() > 1
    assert not bool(far.any()), f"{tag}: {int(far.sum())} outputs more than one fp16 ulp from the correctly rounded activation"
    zero = ((bits & 0x7FFF) == 0) | ((case.lut & 0x7FFF) == 0)
    wrong = int((zero & (((bits ^ case.lut) & 0x8000) != 0)).sum())
    assert wrong == 0, f"{tag}: {wrong} zeros of the wrong sign"
    return f"{int((bits != case.lut).sum())} of {bits.numel()} outputs 1 ulp from the correctly rounded activation"


EXACT = [(s, parts, rows, h, v) for s in ref.EXACT_SHAPES for parts, rows in ((1, False), (4, False), (5, True), (8, False)) for h in (True, False)
         for v in VARIANTS]


@pytest.mark.parametrize("shape,parts,with_rows,f16_out,variant", EXACT,
                         ids=[f"{sid(s)}-p{p}{'-rows' if r else ''}-{'f16' if h else 'f32'}-{vid(v)}" for s, p, r, h, v in EXACT])
def test_exact_case(clipmi_option, shape, parts, with_rows, f16_out, variant):
    """Integers in, integers out: bias bit for bit under every dispatch, gelu within one fp16 ulp of the correctly rounded activation."""
    case = exact(shape, parts)
    M, N, K = dims = problem(shape, "exact")["dims"]
    if variant is not None:
        clipmi_option("gemm_variant", variant)
    kernel = ref.expected_kernel(M, N, K, N, f16_out, parts, with_rows, 1, variant, cus())
    assert must_be(dims, N, f16_out, (parts, with_rows, 0, 1, False), variant)(kernel), kernel
    for epi in ("bias", "gelu"):
        got = launch_twice(case, 0, dims, epi, f16_out, with_rows)
        tag = f"ln-fold-matrix: exact {M}x{N}x{K} p{parts} {epi}-{'f16' if f16_out else 'f32'} {vid(variant)} [{kernel}]"
        print(f"{tag}: {check_exact(case, got, epi, tag)}")


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_exact_case_power_of_four_variances(clipmi_option, variant):
    """The separate case: rows of var = 1 / 4, 1 and 4, rstd = 2, 1 and 1 / 2 -- exact only if the hardware's reciprocal square root is exact at powers of four."""
    shape = (600, 520, 576)
    case = exact(shape, 4, var4=True)
    dims = problem(shape, "exact")["dims"]
    if variant is not None:
        clipmi_option("gemm_variant", variant)
    for f16_out in (True, False):
        got = launch_twice(case, 0, dims, "bias", f16_out, False)
        tag = f"ln-fold-matrix: exact var 4^j {'x'.join(map(str, dims))} p4 bias-{'f16' if f16_out else 'f32'} {vid(variant)}"
        print(f"{tag}: {check_exact(case, got, 'bias', tag)}")


REFUSALS = {"parts 0": dict(parts=0), "parts 9": dict(parts=9), "epilogue none": dict(epilogue=_lib.EPI_NONE), "epilogue residual": dict(epilogue=_lib.EPI_BIAS_RESIDUAL),
            "null stats": dict(stats=None), "null g": dict(g=None), "null c": dict(c=None), "ln_dim 0": dict(ln_dim=0), "ln_row_stride 0": dict(stride=0),
            "negative ln_plane": dict(plane=-1), "stats off 8-byte alignment": "stats", "g off 16-byte alignment": "g"}


@pytest.mark.parametrize("f16_out", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals(what, f16_out):
    shape = (300, 260, 128)
    case, r0 = plain_case(shape, "p4")
    M, N, K = problem(shape)["dims"]
    kw = REFUSALS[what]
    if kw == "stats":
        kw = dict(stats=case.stats.data_ptr() + 4)
        assert kw["stats"] % 8 == 4
    elif kw == "g":
        shifted = torch.zeros(N + 4, device="cuda")[1:N + 1]      # 4 bytes off the 16-byte alignment the f32x4 loads need
        shifted.copy_(case.g)
        kw = dict(g=shifted.data_ptr())
        assert kw["g"] % 16 == 4
    out = patterned((M + 1, N), torch.float16 if f16_out else torch.float32)
    rc = fold(case, r0, case.a, K, case.w_f, K, None, out, N, M, N, K, "bias", **kw)
    torch.cuda.synchronize()
    assert rc == _lib.ERR_ARG, f"{what}: rc = {rc}"
    assert untouched(out), f"{what}: a refused call wrote `out`"
