"""tests/lnback_ref.py on the CPU: the emulation of ln_backward_kernel's fp32 arithmetic lies within half of ``ln_backward_bound`` on
every width, dy dtype and row kind (the other half is the device's real rsqrt and the compiler's contraction), every named defect
of the emulation exceeds the bound on a case of the list, and the QuickGELU bound holds its fp32 evaluation over all of fp16.  What
the GPU test (tests/test_gpu_lnback_ops.py) asserts of the kernels is therefore neither unreachable nor slack."""
import pytest
import torch

import lnback_ref as ref


_groups, _case, _scatter = ref.ln_groups, ref.ln_case, ref.ln_scatter


def _run(c, mutant=None):
    """(ratio of g per row, ratio of g16 per row) of the emulation on one case."""
    g, g16 = ref.emulate_ln_backward(c["x"], c["gamma"], c["dy"], c["g0"], row_idx=c["idx"], mutant=mutant)
    per_row = lambda got, tol: [ref.ratio(got[r], c["want"][r], tol[r]) for r in range(got.shape[0])]
    return per_row(g, c["tol"]), per_row(g16, c["tol16"]), g, g16


def _breaks(cases, kinds=None, copy=True, **kw):
    """The worst ratio of g, and of its fp16 copy against its own tolerance unless ``copy`` is off, over the rows of ``kinds`` in
    ``cases``.  The copy's tolerance is mostly its one fp16 rounding, which no factor covers: it is held to 1, g to 0.5."""
    worst = 0.0
    for c in cases:
        rg, r16, _, _ = _run(c, **kw)
        worst = max([worst] + [max(a, b if copy else 0.0) for a, b, k in zip(rg, r16, c["kinds"]) if kinds is None or k in kinds])
    return worst


ALL = [(D, dt, gi) for D in ref.LN_WIDTHS for dt in ref.DY_DTYPES for gi in (0, 1)]


# ------------------------------------------------------------------------------------------------------------ the emulation and the bound
def test_the_case_list_is_what_the_gpu_test_needs():
    for D in ref.LN_WIDTHS:
        groups = _groups(D)
        kinds = [k for g in groups for k in g.kinds]
        assert all(kinds.count(k) >= 2 for k in ref.KINDS), D
        assert all(len(g.kinds) % 4 for g in groups)                           # a partial last workgroup in every launch
        assert (groups[0].gamma == 0).any() and (groups[0].gamma < 0).any() and (groups[1].gamma == 1).all()
        assert all(g.x.shape == g.dy.shape == (len(g.kinds), D) for g in groups)
    assert ref.LN_WIDTHS[0] == 4 and ref.LN_WIDTHS[-1] == 4096


@pytest.mark.parametrize("D", ref.LN_WIDTHS)
def test_emulation_within_half_the_bound(D):
    worst = {k: 0.0 for k in ref.KINDS}
    for dt in ref.DY_DTYPES:
        for gi in (0, 1):
            c = _case(D, dt, gi)
            rg, r16, g, g16 = _run(c)
            assert torch.equal(g16, g.half())
            for k, a, b in zip(c["kinds"], rg, r16):
                worst[k] = max(worst[k], a)
            assert max(r16) <= 1.0
    print(f"lnback-bound: emulation D={D} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 0.5, worst


@pytest.mark.parametrize("D", ref.SCATTER_WIDTHS)
def test_emulation_of_the_scatter_within_half_the_bound(D):
    c = _scatter(D)
    rg, r16, g, g16 = _run(c)
    untouched = torch.ones(g.shape[0], dtype=torch.bool)
    untouched[c["idx"].long()] = False
    assert torch.equal(g[untouched], c["g0"][untouched]) and torch.equal(g16, g.half())
    print(f"lnback-bound: emulation scatter D={D} {max(rg):.3f}")
    assert max(rg) <= 0.5 and max(r16) <= 1.0


def test_zero_stream_drops_the_accumulation_term():
    """g0 = None is the bound of dX alone: the emulation on a zero stream stays within half of it, and it is the smaller bound."""
    for D in (8, 320, 1024):
        grp = _groups(D)[0]
        zero = torch.zeros_like(grp.x)
        g, _ = ref.emulate_ln_backward(grp.x, grp.gamma, grp.dy, zero)
        tol = ref.ln_backward_bound(grp.x, grp.gamma, grp.dy)
        assert ref.ratio(g, ref.ln_backward(grp.x, grp.gamma, grp.dy), tol) <= 0.5
        assert (tol <= ref.ln_backward_bound(grp.x, grp.gamma, grp.dy, zero + 1.0)).all()


# ------------------------------------------------------------------------------------------------- the bound is not slack: mutants break it
@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_exceeds_the_bound(mutant):
    cases = [_case(*a) for a in ALL] + [_scatter(D) for D in ref.SCATTER_WIDTHS]
    worst = _breaks(cases, mutant=mutant)
    print(f"lnback-bound: mutant {mutant} worst ratio {worst:.3g}")
    assert worst > 1.0


def test_the_case_list_holds_each_mutants_catching_case():
    """Which case catches which defect, so that none of them can leave the list unnoticed."""
    at = lambda D, gi: [_case(D, dt, gi) for dt in ref.DY_DTYPES]
    wide = [D for D in ref.LN_WIDTHS if D > ref.TRIP]
    for D in wide:                                                             # any row of any width with a second trip
        assert _breaks(at(D, 0), mutant="drop_second_trip") > 1.0
    assert _breaks([c for D in ref.LN_WIDTHS if D <= ref.TRIP for c in at(D, 0)], copy=False, mutant="drop_second_trip") <= 0.5
    for D in (320, 768, 1024):                                                 # the row with a large common offset
        assert _breaks(at(D, 0), ("bigmean",), mutant="one_pass_variance") > 1.0
        assert _breaks(at(D, 0), ("bigmean",), mutant="m2_uncentred") > 1.0
    for D in ref.LN_WIDTHS:
        for kind in ("constant", "below_eps"):                                 # eps is all of the variance there
            assert _breaks(at(D, 0), (kind,), mutant="no_eps") > 1.0
        assert _breaks(at(D, 1), ("t_constant",), mutant="m1_zero") > 1.0      # dX is near zero only because mean(t) is removed
        assert _breaks(at(D, 0), ("basis",), mutant="m1_zero") > 1.0
        assert _breaks(at(D, 0), ("random",), mutant="inv_d_off_by_one") > 1.0      # 2^-12 at D = 4096, far above (4 n + 11) u
        assert _breaks(at(D, 0), mutant="g16_from_dx") > 1.0                   # g0 is random, never zero
        assert _breaks(at(D, 0), copy=False) <= 0.5 and _breaks(at(D, 1), copy=False) <= 0.5
    for D in ref.SCATTER_WIDTHS:                                               # only a row index tells dy[r] from dy[row(r)]
        assert _breaks([_scatter(D)], mutant="dy_by_target_row") > 1.0
        assert _breaks([_case(D, torch.float32, 0)], copy=False, mutant="dy_by_target_row") <= 0.5


# ----------------------------------------------------------------------------------------------------------------------- QuickGELU
def test_quickgelu_bound_holds_the_fp32_evaluation_over_all_of_fp16():
    h, d_a = ref.gelu_sweep()
    assert set(h[ref.GELU_FILLER:].view(torch.int16).tolist()) == {b - (1 << 16) if b >= 1 << 15 else b for b in range(1 << 16) if b & 0x7C00 != 0x7C00}
    want = ref.quickgelu_backward(h, d_a)
    assert want.abs().max() < 65504 * (1 - ref.U16)                            # no pair overflows fp16
    tol = ref.quickgelu_backward_bound(h, d_a, want)
    got = ref.emulate_quickgelu_backward(h, d_a)
    assert torch.isfinite(got.float()).all()
    ratio = ((got.double() - want).abs() / tol)
    exact = float((got == want.half()).float().mean())
    print(f"lnback-bound: quickgelu fp32 emulation worst ratio {float(ratio.max()):.3f}, correctly rounded {100 * exact:.2f} %")
    assert ratio.max() <= 1.0
    # the fp32 part is a few u32 |d_a| where the derivative vanishes, and never the bulk of the tolerance
    near = (h.double() + 0.751).abs() < 2e-3
    fp32_part = tol - torch.clamp(ref.U16 * want.abs(), min=2.0 ** -25)
    assert near.any() and (fp32_part[near] <= 4 * ref.U32 * d_a.double().abs()[near]).all()
    assert (fp32_part <= 40 * ref.U32 * d_a.double().abs()).all()


def test_quickgelu_bound_catches_a_wrong_constant_and_a_truncating_cast():
    h, d_a = ref.gelu_sweep()
    want = ref.quickgelu_backward(h, d_a)
    tol = ref.quickgelu_backward_bound(h, d_a, want)
    s = torch.sigmoid(1.7 * h.double())                                        # 1.7 where 1.702 belongs
    wrong = (d_a.double() * (s + 1.7 * h.double() * s * (1 - s))).half()
    assert float(((wrong.double() - want).abs() / tol).max()) > 1.0
    bits = want.half().view(torch.int16)
    trunc = torch.where(want.half().double().abs() > want.abs(), bits - 1, bits).view(torch.float16)       # round towards zero
    assert float(((trunc.double() - want).abs() / tol).max()) > 1.0
