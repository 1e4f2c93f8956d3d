"""The checker of tests/test_gpu_residual_gemm.py has teeth (tests/residual_gemm_ref.py; CPU only).

For every shape of the GPU matrix and both stream types -- every K whole; the row-range shapes at the M of a 64-CU device (2035 .. 12859 rows: the
element-wise float64 work is what would take seconds here, not K) --

* the emulation (the reference's fp32 arithmetic, residual_gemm_ref.emulate) passes the output check with a worst error / tolerance <= 0.5 and its
  partials pass theirs with a worst error / bound <= 0.5, at 256- and at 128-column tiles: the reference alone stays well inside, and a failure on
  the GPU means the kernel;
* its accumulation error in front of the output rounding is <= 2^-21 * reach, which is what keeps C_ACC = 2^-20 (printed per shape and K);
* each seeded corruption makes the matching check fail:
    kstep     one 64-wide K-step left out on one 1/64-scaled row (M >= 2: one row has no scaled row);
    resblock  the residual of one 16-row block taken from the block 16 rows further on (M >= 32);
    coltile   the last 8 columns' outputs taken from the 8 columns before them (N >= 16);
    bias      the bias left out on the last 4 columns;
    shifted   the partials of tile t stored at tile t + 1 (two tiles or more);
    unrounded fp16 stream only: the partials formed from the unrounded fp32 sums;
    nudged    one partial of a 1/64-scaled row moved by 2^-17 of its sum of magnitudes (M >= 2).

Then the constructed exact case, and the Python mirror of the row-range kernel's dispatch rule and tile split against the table of values worked out
by hand for 256 CUs (and the named structures at 64, 228 and 304 CUs).
"""
import functools

import pytest
import torch

import residual_gemm_ref as ref

CPU_CUS = 64
SHAPES = list(ref.SMALL_SHAPES) + [(ref.rstream_shape(CPU_CUS, N, ln, extra, cut), N, K) for (N, K, ln, extra, cut), _ in ref.ROW_RANGE]
IDS = ["x".join(str(v) for v in s) for s in SHAPES]


@functools.lru_cache(maxsize=2)
def problem(shape, f16_stream):
    a, w, bias, x_old, small_rows, small_cols = ref.operands(*shape, f16_stream)
    want, reach, tol = ref.expected(a, w, bias, x_old, f16_stream)
    return a, w, bias, x_old, small_rows, small_cols, want, reach, tol


def output_corruptions(shape, f16_stream):
    """name -> corrupted output (or None where the corruption does not exist at this shape)."""
    a, w, bias, x_old, small_rows, _ = problem(shape, f16_stream)[:6]
    M, N, K = shape
    g = torch.Generator().manual_seed(M + N + K)
    emu = ref.emulate(a, w, bias, x_old, f16_stream)[0]
    out = {}

    c = None
    if bool(small_rows.any()):
        rows = torch.nonzero(small_rows).flatten()
        m = int(rows[int(torch.randint(rows.numel(), (1,), generator=g))])
        k0 = int(torch.randint(K // 64, (1,), generator=g)) * 64
        a_bad = a[m:m + 1].clone()
        a_bad[:, k0:k0 + 64] = 0
        c = emu.clone()
        c[m:m + 1] = ref.emulate(a_bad, w, bias, x_old[m:m + 1], f16_stream)[0]
    out["kstep"] = c

    c = None
    if M >= 32:
        r0 = int(torch.randint(M // 16 - 1, (1,), generator=g)) * 16
        c = emu.clone()
        c[r0:r0 + 16] = ref.emulate(a[r0:r0 + 16], w, bias, x_old[r0 + 16:r0 + 32], f16_stream)[0]
    out["resblock"] = c

    c = None
    if N >= 16:
        c = emu.clone()
        c[:, N - 8:] = emu[:, N - 16:N - 8]
    out["coltile"] = c

    b = bias.clone()
    b[-4:] = 0.0
    out["bias"] = ref.emulate(a, w, b, x_old, f16_stream)[0]
    return emu, out


@pytest.mark.parametrize("f16_stream", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_emulation_passes_and_corruptions_fail(shape, f16_stream):
    a, w, bias, x_old, small_rows, small_cols, want, reach, tol = problem(shape, f16_stream)
    M, N, K = shape
    tag = f"residual-ref: {M}x{N}x{K} {'f16' if f16_stream else 'f32'}"
    acc = ref.accumulation_error(a, w, bias, x_old, want, reach)
    print(f"{tag}: K = {K}: fp32 evaluation within 2^{torch.log2(torch.tensor(max(acc, 1e-300))).item():.2f} * reach of float64")
    assert acc <= 2.0 ** -21, "the reference's own accumulation no longer justifies C_ACC = 2^-20"

    emu, bad_outputs = output_corruptions(shape, f16_stream)
    worst, at = ref.check(emu, want, tol, "emulation")
    print(f"{tag}: emulation worst error / tolerance {worst:.3f} at {at}")
    assert worst <= 0.5
    applied = []
    for name, bad in bad_outputs.items():
        if bad is None:
            continue
        with pytest.raises(AssertionError):
            ref.check(bad, want, tol, name)
        applied.append(name)
    assert applied == [n for n, there in (("kstep", M >= 2), ("resblock", M >= 32), ("coltile", N >= 16), ("bias", True)) if there]

    g = torch.Generator().manual_seed(M * 3 + N + K)
    for w_part in (256, 128):
        x, x16, stats = ref.emulate(a, w, bias, x_old, f16_stream, w_part)
        assert torch.equal(x16, x.half()) and x.dtype == (torch.float16 if f16_stream else torch.float32)
        parts = ref.cdiv(N, w_part)
        assert ref.part_width(parts, N) in ((w_part,) if N > 128 else (128, 256))
        worst, at = ref.check_partials(stats, x, w_part, "emulation")
        print(f"{tag}: emulation partials of {w_part} columns: worst error / bound {worst:.3f} at {at}")
        assert worst <= 0.5
        applied = []
        if parts >= 2:
            with pytest.raises(AssertionError):
                ref.check_partials(torch.roll(stats, 1, 0), x, w_part, "shifted")
            applied.append("shifted")
        if f16_stream:
            pre = ref.gemm_ref.emulate(a, w, bias, x_old.float(), "residual", False)      # the fp32 sums in front of the rounding
            with pytest.raises(AssertionError):
                ref.check_partials(ref.partials32(pre, w_part), x, w_part, "unrounded")
            applied.append("unrounded")
        if bool(small_rows.any()):
            rows = torch.nonzero(small_rows).flatten()
            m = int(rows[int(torch.randint(rows.numel(), (1,), generator=g))])
            t = int(torch.randint(parts, (1,), generator=g))
            mag = float(ref.tile_sums(x, w_part)[2][t, m])
            nudged = stats.clone()
            nudged[t, m, 0] += 2.0 ** -17 * mag
            with pytest.raises(AssertionError):
                ref.check_partials(nudged, x, w_part, "nudged")
            applied.append("nudged")
        assert applied == [n for n, there in (("shifted", parts >= 2), ("unrounded", f16_stream), ("nudged", M >= 2)) if there]


@pytest.mark.parametrize("f16_stream", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("shape", [(600, 520, 576), (2451, 2048, 512), (6419, 2048, 448)], ids=lambda s: "x".join(map(str, s)))
def test_exact_case_is_integers_and_uses_every_column(shape, f16_stream):
    M, N, K = shape
    a, w, bias, x_old = ref.exact_case(M, N, K, seed=M + K, f16_stream=f16_stream)
    assert x_old.dtype == (torch.float16 if f16_stream else torch.float32)
    for t, lim in ((a, 4), (bias, 4), (x_old, 4), (w, 1)):
        assert bool((t.double() == t.double().round()).all()) and float(t.abs().max()) <= lim
    nz = w != 0
    assert bool((nz.sum(1) == 2).all()), "two entries per row of w"
    cols = torch.nonzero(nz)[:, 1].view(N, 2)
    assert bool((cols[:, 0] // 64 != cols[:, 1] // 64).all()), "the two entries of a row sit in different K-steps"
    assert bool(nz.any(0).all()), "every K column is used"
    want = ref.exact_result(a, w, bias, x_old)
    assert bool((want == want.round()).all()) and float(want.abs().max()) <= 16
    assert torch.equal(want.half().double(), want)
    for w_part in (256, 128):
        s, q, _ = ref.tile_sums(want, w_part)
        assert float(q.max()) <= 256 * 256 and torch.equal(s.float().double(), s) and torch.equal(q.float().double(), q)
        # the emulation is exact on it, whatever the order of its sums
        x, x16, stats = ref.emulate(a, w, bias, x_old, f16_stream, w_part)
        assert torch.equal(x.double(), want) and torch.equal(stats[..., 0].double(), s) and torch.equal(stats[..., 1].double(), q)
    with pytest.raises(AssertionError):
        ref.exact_case(8, K // 2 - 8, K, seed=0)


def test_rstream_plan_reproduces_the_table_for_256_cus():
    table = [(8179, {(8,)}), (9363, {(9,), (10,)}), (51771, {(10, 9), (10, 10)}), (25619, {(9, 8, 8), (9, 9, 8)})]
    for ((N, K, ln, extra, cut), named), (M, structures) in zip(ref.ROW_RANGE, table):
        assert named == structures
        assert ref.rstream_shape(256, N, ln, extra, cut) == M
        assert ref.rstream_plan(256, M, N, K, N) == structures, (M, N, K)
        assert ref.rstream_plan(256, M, N, K, N + 8, K + 8, K + 16) == structures      # the strided calls take the same kernel
        assert ref.expected_parts(None, 256, M, N, K, True) == ref.expected_parts(16, 256, M, N, K, True) == ref.cdiv(N, 256)


@pytest.mark.parametrize("cus", [64, 228, 256, 304])
def test_rstream_shape_yields_the_named_structures(cus):
    for (N, K, ln, extra, cut), named in ref.ROW_RANGE:
        M = ref.rstream_shape(cus, N, ln, extra, cut)
        assert ref.rstream_plan(cus, M, N, K, N) == named, (cus, M, N, K)
    N, K, ln, extra, cut = ref.ONE_PAIR_SHORT
    M = ref.rstream_shape(cus, N, ln, extra, cut)
    assert ref.cdiv(M, 32) == ref.rstream_groups(cus, N) * 8 - 1
    assert ref.rstream_plan(cus, M, N, K, N) is None, "one pair short of eight per range: not taken"


def test_rstream_plan_refusals():
    M, N, K = 8179, 2048, 448
    assert ref.rstream_plan(256, M, N, K, N) is not None
    assert ref.rstream_plan(256, M, N, 384, N) is None              # six K-steps
    assert ref.rstream_plan(256, M, N, K, N + 4) is None            # ldx % 8
    assert ref.rstream_plan(256, M, 2056, K, 2056) is None          # nine column tiles
    assert ref.rstream_plan(7, M, N, K, N) is None
    for shape in ref.SMALL_SHAPES:                                  # none of the small shapes reaches the row-range kernel
        assert ref.rstream_plan(256, *shape) is None


def test_expected_parts():
    # forced variants: 256-column partials except from the 128 x 128 kernel, which hands over to the 256 x 256 tiles beyond 8 partials
    for M, N, K in ref.SMALL_SHAPES:
        for f16_stream in (True, False):
            for v in (1, 10, 16):
                assert ref.expected_parts(v, 256, M, N, K, f16_stream) == ref.cdiv(N, 256)
            p0 = ref.expected_parts(0, 256, M, N, K, f16_stream)
            assert p0 == (ref.cdiv(N, 128) if ref.cdiv(N, 128) <= 8 else ref.cdiv(N, 256))
    assert ref.expected_parts(0, 256, 300, 1672, 128, True) == 7
    assert ref.expected_parts(0, 256, 300, 264, 128, True) == 3
    # the unforced cost model takes the 128 x 128 kernel for a small problem and the 256-row tiles for a large one
    assert ref.default_variant(256, 300, 264, 128) == 0 and ref.expected_parts(None, 256, 300, 264, 128, False) == 3
    assert ref.default_variant(256, 50432, 768, 768) == 10 and ref.expected_parts(None, 256, 50432, 768, 768, False) == 3
    assert ref.default_variant(256, 321, 264, 64) == 0
