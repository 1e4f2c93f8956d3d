"""The checker of tests/test_gpu_ln_fold_matrix.py has teeth (tests/ln_fold_ref.py; CPU only).

For every shape of the GPU matrix with its statistics layout, and the further layouts (8 partials, 5 partials, a plane of M + 64, a row stride of
2) -- every K whole; M* is that of a 32-CU device (1064 rows = 5 row tiles x 7 column tiles on 32 persistent workgroups, a last row tile of 40:
the structure of the 256-CU value 9256, whose element-wise float64 work is what would take seconds here) --

* in front of the output rounding the emulation (the reference's fp32 arithmetic, ln_fold_ref.emulate) stays within HALF of the unfactored
  non-rounding part of the tolerance, C_ACC * reach + rho * (|t1| + |t2|): the condition on which C_ACC and rho are kept;
* after the rounding it stays within the full unfactored tolerance (gelu to fp16: also the twice-rounded form), so under FACTOR = 2 the
  reference alone uses at most half of what a kernel is allowed; both figures and the largest rho are printed per shape;
* each mutant of the emulation puts at least one element beyond its (factored) tolerance, or makes it non-finite, wherever it applies; its worst
  error / tolerance is printed:
    row+1, row-1   the row parameters (rstd, mean * rstd) of row m + 1 / m - 1 (M >= 2)
    g+1, g-1       g taken from column n + 1 / n - 1
    c+1, c-1       c taken from column n + 1 / n - 1
    last-partial   the last partial dropped (two partials or more)
    plane          the partials read with plane M where it is M + 64 (two partials or more)
    stride         the partials read with row stride 1 where it is 2 (M >= 2)
    eps            eps left out (M >= 2: the 1 / 64-scaled rows, where eps is 4 % of var, are the odd ones)
    sign           mean * rstd * g added instead of subtracted
    gelu-of-t1     gelu only: the activation taken of acc * rstd alone
  and, in the exact case, ln_dim replaced by K (the two differ only there).

Then the exact case on the reference and, bit for bit, on the emulation; the dispatch mirror against values worked out by hand for 256 CUs; and
the refusals of clipmi_gemm_ln_fold that return before any device call.
"""
import ctypes
import functools

import pytest
import torch

import ln_fold_ref as ref
from clip_calibration_amd import _lib

CPU_CUS = 32
PAIRS = [("bias", True), ("bias", False), ("gelu", True), ("gelu", False)]
# (shape, parts, plane_pad, row_stride): the matrix' own layout per shape, then the layouts of the GPU file's second axis
CASES = [(s, p, 0, 1) for s, p, _ in ref.SHAPES] + [((300, 264, 128), 2, 0, 1)] + [
    ((300, 260, 128), 8, 0, 1), ((600, 520, 576), 5, 0, 1), ((600, 520, 576), 4, 64, 1), ((600, 520, 576), 3, 0, 2), ((None, 1672, 512), 4, 64, 1)]
IDS = ["x".join("M*" if v is None else str(v) for v in s) + f"-p{p}" + (f"-plane+{pad}" if pad else "") + (f"-stride{rs}" if rs > 1 else "")
       for s, p, pad, rs in CASES]


def resolve(shape):
    M, N, K = shape
    return (ref.m_star(CPU_CUS)[0] if M is None else M), N, K


@functools.lru_cache(maxsize=2)
def problem(shape, parts, pad, rs):
    M, N, K = resolve(shape)
    case = ref.operands(M, N, K, parts, plane_pad=pad, row_stride=rs)
    mean, rstd, rho = ref.row_params(case.stats, M, parts, case.ln_dim, case.eps, case.plane, rs)
    return case, mean, rstd, rho, ref.products(case.a, case.w_f), ref.acc32(case.a, case.w_f)


def ratio(got, want, tol):
    g = got.double()
    return float("inf") if not bool(torch.isfinite(g).all()) else float(((g - want).abs() / tol).max())


def mutants(case, M, acc, epi, f16_out):
    """name -> mutated emulation output (None where the mutant does not apply)."""
    rows = lambda **kw: ref.emulate_rows(case.stats, M, kw.pop("parts", case.parts), case.ln_dim, kw.pop("eps", case.eps),
                                         kw.pop("plane", case.plane), kw.pop("row_stride", case.row_stride))
    rstd, mrs = rows()
    out = lambda r, q, g=case.g, c=case.c: ref.finish(ref.emulate_pre(acc, g, c, r, q), epi, f16_out)
    m = {}
    for name, sh in (("row+1", -1), ("row-1", 1)):
        m[name] = out(torch.roll(rstd, sh), torch.roll(mrs, sh)) if M >= 2 else None
    for name, sh in (("g+1", -1), ("g-1", 1)):
        m[name] = out(rstd, mrs, g=torch.roll(case.g, sh))
    for name, sh in (("c+1", -1), ("c-1", 1)):
        m[name] = out(rstd, mrs, c=torch.roll(case.c, sh))
    m["last-partial"] = out(*rows(parts=case.parts - 1)) if case.parts >= 2 else None
    m["plane"] = out(*rows(plane=M)) if case.plane == M + 64 and case.parts >= 2 else None
    m["stride"] = out(*rows(row_stride=1)) if case.row_stride == 2 and M >= 2 else None
    m["eps"] = out(*rows(eps=0.0)) if M >= 2 else None
    m["sign"] = out(rstd, -mrs)
    m["gelu-of-t1"] = None
    if epi == "gelu":
        bad = ref.quickgelu(acc * rstd[:, None]) - mrs[:, None] * case.g[None, :] + case.c[None, :]
        m["gelu-of-t1"] = bad.half() if f16_out else bad
    return m


@pytest.mark.parametrize("epi,f16_out", PAIRS, ids=[f"{e}-{'f16' if h else 'f32'}" for e, h in PAIRS])
@pytest.mark.parametrize("shape,parts,pad,rs", CASES, ids=IDS)
def test_emulation_within_bounds_and_mutants_fail(shape, parts, pad, rs, epi, f16_out):
    case, mean, rstd, rho, prod, acc = problem(shape, parts, pad, rs)
    M, N, K = resolve(shape)
    tag = f"ln-fold-ref: {M}x{N}x{K} p{parts}{f' plane+{pad}' if pad else ''}{f' stride {rs}' if rs > 1 else ''} {epi} {'f16' if f16_out else 'f32'}"
    assert bool(torch.isnan(case.stats.view(8, case.plane, 2)[parts:]).all()) and int(torch.isfinite(case.stats).sum()) == parts * M * 2
    want, pre, reach, t1, t2 = ref.reference(case.a, case.w_f, case.g, case.c, mean, rstd, epi, prod)
    e_rstd, e_mrs = ref.emulate_rows(case.stats, M, parts, case.ln_dim, case.eps, case.plane, rs)
    e_pre = ref.emulate_pre(acc, case.g, case.c, e_rstd, e_mrs)
    share = float(((e_pre.double() - pre).abs() / ref.non_rounding(reach, t1, t2, rho)).max())
    unfactored = ref.tolerance(want, pre, reach, t1, t2, rho, epi, f16_out, factor=1.0)
    emu = ref.emulate(case, M, epi, f16_out)
    assert torch.equal(emu, ref.finish(e_pre, epi, f16_out))
    full = ratio(emu, want, unfactored)
    print(f"{tag}: emulation at {share:.3f} of the non-rounding part, {full:.3f} of the unfactored tolerance; largest rho {float(rho.max()):.2e}")
    assert share <= 0.5, "the reference's own arithmetic no longer justifies C_ACC and rho"
    assert full <= 1.0
    # |mean| / sigma <= 10 by construction: rho = (1 + 1.5 mean^2 / var + 4) u, 1.3e-5 at mean^2 / var = 140 (the -10 class after the fp16 rounding and the
    # sampling of var); a 64-element row can sample half the variance: at most 2^-15
    assert float(rho.max()) <= 2.0 ** -15
    tol = ref.tolerance(want, pre, reach, t1, t2, rho, epi, f16_out)
    assert ref.check(emu, want, tol, "emulation")[0] <= 0.5 + 2.0 ** -20
    if epi == "gelu" and f16_out:
        twice = ratio(ref.emulate(case, M, epi, True, twice=True), want, unfactored)
        print(f"{tag}: twice-rounded emulation at {twice:.3f} of the unfactored tolerance")
        assert twice <= 1.0
    applied = []
    for name, bad in mutants(case, M, acc, epi, f16_out).items():
        if bad is None:
            continue
        worst = ratio(bad, want, tol)
        print(f"{tag}: mutant {name}: worst error / tolerance {'non-finite' if worst == float('inf') else f'{worst:.3g}'}")
        with pytest.raises(AssertionError):
            ref.check(bad, want, tol, name)
        assert worst > 1.0
        applied.append(name)
    expected = [n for n, there in (("row+1", M >= 2), ("row-1", M >= 2), ("g+1", True), ("g-1", True), ("c+1", True), ("c-1", True),
                                   ("last-partial", parts >= 2), ("plane", pad == 64 and parts >= 2), ("stride", rs == 2 and M >= 2),
                                   ("eps", M >= 2), ("sign", True), ("gelu-of-t1", epi == "gelu")) if there]
    assert applied == expected, f"mutants applied {applied}, expected {expected}"


def test_operands_are_what_the_docstring_says():
    M, N, K = 600, 520, 576
    case = ref.operands(M, N, K, 3)
    assert case.a.dtype == case.w_f.dtype == torch.float16 and case.ln_dim == K and case.plane == M
    other = ref.operands(M, N, K, 8, plane_pad=64)
    assert torch.equal(case.a, other.a) and torch.equal(case.w_f, other.w_f) and torch.equal(case.g, other.g) and torch.equal(case.c, other.c)
    x = case.a.double()
    mu, sd = x.mean(1), x.std(1)
    m = torch.arange(M)
    scale = torch.where(m % 2 == 1, ref.SMALL, 1.0).double()
    assert bool(((sd / scale - 1.0).abs() < 0.15).all())
    assert bool(((mu / scale - torch.tensor(ref.CLASS_MEANS, dtype=torch.float64)[(m // 2) % 3]).abs() < 0.2).all())
    mean, rstd, rho = ref.row_params(case.stats, M, 3, K, case.eps)
    assert bool(((mean - mu).abs() <= 1e-5 * (1 + mu.abs())).all())
    odd = rstd[1::2] / rstd[0::2]
    assert 50.0 < float(odd.min()) and float(odd.max()) < 80.0          # neighbours differ 64 x in rstd (less what eps takes)
    var_small = 1.0 / rstd[1::2] ** 2 - case.eps
    assert 0.03 < float((case.eps / var_small).median()) < 0.05           # eps is about 4 % of var on the scaled rows
    assert int(case.small_cols.sum()) == (N + 2) // 4
    b = ref.slice_bounds(K, 3)
    assert b == [0, 96, 288, 576]
    # the folding formula is ops.fold_layernorm_linear's, bit for bit
    from clip_calibration_amd import ops
    gen = torch.Generator().manual_seed(5)
    w, bias = (torch.randn(24, 64, generator=gen) * 0.1).half(), torch.randn(24, generator=gen)
    gamma, beta = 1 + 0.2 * torch.randn(64, generator=gen), 0.1 * torch.randn(64, generator=gen)
    for got, want in zip(ref.fold(w, bias, gamma, beta), ops.fold_layernorm_linear(w, bias, gamma, beta)):
        assert torch.equal(got, want)
    # the strided and padded layouts put the same partials where the call reads them and NaN everywhere else
    st = ref.operands(M, N, K, 3, plane_pad=64, row_stride=2)
    assert st.plane == 2 * M + 64
    v = st.stats.view(8, st.plane, 2)
    assert torch.equal(v[:3, 0:2 * M:2], case.stats.view(8, M, 2)[:3]) and bool(torch.isnan(v[:3, 1:2 * M:2]).all()) and bool(torch.isnan(v[:, 2 * M:]).all())
    for a, b in zip(ref.row_params(st.stats, M, 3, K, st.eps, st.plane, 2), (mean, rstd, rho)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("parts", [1, 4, 5, 8])
@pytest.mark.parametrize("shape", ref.EXACT_SHAPES, ids=lambda s: "x".join("M*" if v is None else str(v) for v in s))
def test_exact_case_is_integers_on_reference_and_emulation(shape, parts):
    M, N, K = resolve(shape)
    case = ref.exact_case(M, N, K, parts)
    assert case.ln_dim == ref.EXACT_LN_DIM != K and case.eps == 0.0
    for t, lim in ((case.a, 1), (case.w_f, 1), (case.c, 4), (case.g, K)):
        assert bool((t.double() == t.double().round()).all()) and float(t.abs().max()) <= lim
    assert torch.equal(case.g.double(), case.w_f.double().sum(1))
    assert bool((case.mean[1:] != case.mean[:-1]).all()) and float(case.mean.abs().max()) == 2.0
    st = case.stats.view(8, M, 2)[:parts]
    assert bool((st == st.round()).all())
    assert parts == 1 or not torch.equal(st[0, 0], st[0, 1])                      # a different split per row
    mean, rstd, rho = ref.row_params(case.stats, M, parts, case.ln_dim, 0.0)
    assert torch.equal(mean, case.mean) and torch.equal(rstd, torch.ones_like(rstd))
    for epi in ("bias", "gelu"):
        want, pre, _, _, _ = ref.reference(case.a, case.w_f, case.g, case.c, mean, rstd, epi)
        assert torch.equal(pre, case.want) and float(pre.abs().max()) <= 2048.0
        if epi == "bias":
            assert torch.equal(want, case.want)
    for f16_out in (True, False):
        emu = ref.emulate(case, M, "bias", f16_out)
        assert torch.equal(emu.double(), case.want), "the emulation does not return the integers bit for bit"
    # ln_dim replaced by K: whole integers change
    rstd_k, mrs_k = ref.emulate_rows(case.stats, M, parts, K, 0.0)
    bad = ref.finish(ref.emulate_pre(ref.acc32(case.a, case.w_f), case.g, case.c, rstd_k, mrs_k), "bias", False)
    wrong = int((bad.double() != case.want).sum())
    print(f"ln-fold-ref: exact {M}x{N}x{K} p{parts}: ln_dim = K changes {wrong} of {bad.numel()} outputs")
    assert wrong > bad.numel() // 2
    # gelu of the integers: the emulation's fp16 result is within one ulp of the correctly rounded table, zeros of the right sign
    lut = ref.quickgelu_f16_bits(case.want)
    got = ref.emulate(case, M, "gelu", True).view(torch.int16).to(torch.int32) & 0xFFFF
    assert int((ref.f16_ordinal(got) - ref.f16_ordinal(lut)).abs().max()) <= 1
    zero = ((got & 0x7FFF) == 0) | ((lut & 0x7FFF) == 0)
    assert not bool((zero & (((got ^ lut) & 0x8000) != 0)).any())


def test_exact_case_with_power_of_four_variances():
    M, N, K = 600, 520, 576
    case = ref.exact_case(M, N, K, 4, var4=True)
    mean, rstd, _ = ref.row_params(case.stats, M, 4, case.ln_dim, 0.0)
    assert torch.equal(mean, case.mean) and torch.equal(rstd, case.rstd) and set(rstd.tolist()) == {0.5, 1.0, 2.0}
    assert torch.equal(ref.reference(case.a, case.w_f, case.g, case.c, mean, rstd, "bias")[0], case.want)
    for f16_out in (True, False):      # torch.rsqrt of 0.25, 1 and 4 in fp32 on the CPU is exact; the device's is what the GPU test measures
        assert torch.equal(ref.emulate(case, M, "bias", f16_out).double(), case.want)


def test_quickgelu_table():
    h = torch.tensor([-2048.0, -60.0, -1.0, 0.0, 1.0, 3.0, 2048.0], dtype=torch.float64)
    bits = ref.quickgelu_f16_bits(h)
    val = bits.to(torch.int16).view(torch.float16).double()
    assert bits[0] == 0x8000 and bits[1] == 0x8000 and bits[3] == 0 and float(val[-1]) == 2048.0
    assert bool(((val - ref.quickgelu(h)).abs() <= 2.0 ** -11 * ref.quickgelu(h).abs() + 2.0 ** -25).all())
    assert ref.f16_ordinal(torch.tensor([0x8001, 0x8000, 0, 1])).tolist() == [-1, 0, 0, 1]


def test_expected_kernel_reproduces_the_rule_for_256_cus():
    k = lambda M, N, K, variant, f16=True, parts=4, rows=False, rs=1, ldo=None, **kw: ref.expected_kernel(
        M, N, K, N if ldo is None else ldo, f16, parts, rows, rs, variant, 256, **kw)
    Ms = ref.m_star(256)[0]
    assert Ms == 9256
    # M* x 1672 x 512: 259 tiles = 1.01 rounds: the default dispatch stays with the tile kernels (cost model: 2 rounds of 128 x 128 pairs, 73 400,
    # against one round of 320 x 256 at 0.93 x 84 378 = 78 471 and two of 256 x 256), forced 13 streams
    assert k(Ms, 1672, 512, None) == "128x128" and k(Ms, 1672, 512, 13) == "stream-raw"
    assert k(Ms, 1672, 512, 13, parts=5, rows=True) == "stream-finalised"
    assert k(Ms, 1672, 512, 13, parts=5) == "256x256", "more than four partials without ln_rows leave the streamed kernel"
    assert k(Ms, 1672, 512, 13, parts=4, rows=True) == "stream-raw", "up to four partials are finalised in the kernel, ln_rows or not"
    assert k(Ms, 1672, 512, 13, parts=8) == "256x256" and k(Ms, 1672, 512, 13, parts=8, rows=True) == "stream-finalised"
    assert k(Ms, 1672, 512, 13, rs=2) == "256x256" and k(Ms, 1672, 512, 13, f16=False) == "256x256+f32"
    assert k(Ms, 1672, 512, 13, ldo=1676) == "256x256+direct" and k(Ms, 1672, 512, 13, ldo=1680) == "stream-raw"
    assert k(Ms, 1672, 448, 13) == "256x256", "seven K-steps"
    assert [k(Ms, 1672, 512, v) for v in (0, 1, 10)] == ["128x128", "256x256", "320x256"]
    # the small shapes
    assert k(600, 520, 576, 13, parts=3) == "stream-raw" and k(600, 520, 576, None, parts=3) == "128x128"
    assert k(333, 512, 3072, 13, parts=8, rows=True) == "stream-finalised" and k(333, 512, 3072, 13, parts=8) == "256x256"
    assert k(300, 260, 128, 13, parts=2) == "256x256+direct" and k(300, 260, 128, 0, parts=2, f16=False) == "128x128+f32"
    assert k(321, 264, 64, 10, parts=1) == "256x256", "one K-step: the ping-pong loop hands over"
    assert k(300, 264, 128, 10, parts=1) == "320x256"
    # c_fc of a width-768 tower at 10240 rows: 480 tiles = 1.9 rounds streams by default; no ragged last tile row
    assert k(10240, 3072, 768, None) == "stream-raw" and k(10240, 3072, 768, None, parts=5) == "256x256"
    # 16448 x 3072 x 768: 65 x 12 tiles, the last tile row of 64 rows opens a fourth round: a tail launch on the rows from 16384
    assert ref.split_head(16448, 3072, None, 256) == 16384 and ref.split_head(16448, 3072, 13, 256) is None
    assert k(16448, 3072, 768, None, parts=3) == "stream-raw[0:16384] | 128x128[16384:16448] stats+2*16384"
    assert k(16448, 3072, 768, 13, parts=3) == "stream-raw"
    assert ref.split_head(16384 + 200, 3072, None, 256) is None, "more than 128 rows stay in the persistent launch"
    # fewer than 8 CUs: no persistent grid
    assert ref.expected_kernel(Ms, 1672, 512, 1672, True, 4, False, 1, 13, 7) == "256x256"


def test_ln_fold_entry_validates_arguments_without_a_gpu():
    """The refusals of clipmi_gemm_ln_fold that return before any device call: each leaves a patterned ``out`` untouched."""
    M, N, K = 4, 8, 64
    out = (ctypes.c_uint16 * (M * N))(*([0x5A3C] * (M * N)))
    p = ctypes.c_void_p(4096)
    ok = dict(c=p, g=p, stats=p, parts=3, plane=0, stride=1, ln_dim=K, epi=_lib.EPI_BIAS)

    def fold(**kw):
        a = dict(ok, **kw)
        rc = _lib.lib.clipmi_gemm_ln_fold(p, K, p, K, a["c"], a["g"], a["stats"], a["parts"], a["plane"], a["stride"], a["ln_dim"], 1e-5, None,
                                          ctypes.addressof(out), N, _lib.F16, M, N, K, a["epi"], None)
        assert all(v == 0x5A3C for v in out), f"a refused call wrote `out`: {kw}"
        return rc

    for kw in (dict(parts=0), dict(parts=9), dict(epi=_lib.EPI_NONE), dict(epi=_lib.EPI_BIAS_RESIDUAL), dict(stats=None), dict(g=None),
               dict(c=None), dict(ln_dim=0), dict(stride=0), dict(plane=-1), dict(stats=ctypes.c_void_p(4100)), dict(g=ctypes.c_void_p(4100))):
        assert fold(**kw) == _lib.ERR_ARG, kw
        assert "gemm_ln_fold" in _lib.last_error(), (kw, _lib.last_error())
    assert fold(g=ctypes.c_void_p(4104)) == _lib.ERR_ARG       # 8-byte aligned g: the f32x4 loads need 16
