"""tests/head_ref.py on the CPU: its float64 values are the existing restatements', its fp32 emulation of the kernels' summation orders
stays inside its derived bound on every listed case and satisfies the constructed-input equalities, and every seeded corruption of the
emulation leaves the bound or breaks such an equality on at least one listed case (the test names them with -s)."""
import numpy as np
import pytest
import torch

import head_ref as ref

RATIOS = {}


def _note(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)


def _hold(got, bound, names, head):
    worst = 0.0
    for n in names:
        r = ref.ratio(got[n], *bound[n])
        _note((head, n), r)
        worst = max(worst, r)
    return worst


def _close(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a.reshape(b.shape) - b).abs().max()) <= 1e-9 * float(b.abs().max()) + 1e-300


@pytest.mark.parametrize("case", ref.SHARED_CASES, ids=str)
def test_bound_values_are_the_restatements(case):
    """The float64 values next to the bounds equal coopfit_ref.head, vptfit_ref.head_image, maplefit_ref.joint_head and
    promptfit_ref.kgcoop_head: the mathematics is not forked."""
    inp = ref.inputs(case)
    want = ref.formulas(inp)
    b, kg = ref.coop_bound(inp), ref.kgcoop_bound(inp, 8.0)
    assert _close(b["loss"][0], want["loss"]) and _close(b["d_text"][0], want["d_text"]) and _close(b["d_feats"][0], want["d_feats"])
    assert _close(b["loss"][0], want["joint"][0]) and _close(b["d_feats"][0], want["joint"][1]) and _close(b["d_text"][0], want["joint"][2])
    assert _close(kg["losses"][0], want["kg_losses"]) and _close(kg["d_text"][0], want["kg_d_text"])


@pytest.mark.parametrize("case", ref.COCOOP_CASES, ids=str)
def test_cocoop_bound_values_are_the_restatement(case):
    inp = ref.inputs(case, True)
    want, b = ref.cocoop_formulas(inp), ref.cocoop_bound(inp)
    assert all(_close(b[n][0], want[n]) for n in ("loss", "d_text", "row_losses"))


@pytest.mark.parametrize("case", ref.SHARED_CASES, ids=str)
def test_emulation_within_bound(case):
    """CoOp / VPT / MaPLe and KgCoOp (w = 8) in the kernels' order, fp32: |emulation - float64| <= tol on every element."""
    inp = ref.inputs(case)
    assert _hold(ref.emulate_coop(inp), ref.coop_bound(inp), ("loss", "d_text", "d_feats"), "coop/vpt/maple") <= 1.0
    assert _hold(ref.emulate_kgcoop(inp, 8.0), ref.kgcoop_bound(inp, 8.0), ("losses", "d_text"), "kgcoop") <= 1.0


@pytest.mark.parametrize("case", ref.COCOOP_CASES, ids=str)
def test_cocoop_emulation_within_bound(case):
    inp = ref.inputs(case, True)
    assert _hold(ref.emulate_cocoop(inp), ref.cocoop_bound(inp), ("loss", "row_losses", "d_text"), "cocoop") <= 1.0


@pytest.mark.parametrize("case", ref.SHARED_CASES, ids=str)
def test_prograd_and_promptsrc_emulation_within_bound(case):
    """ProGrad at T in {1, 2} and PromptSRC at the reference weights and with a zero image weight: the bound's values are
    promptfit_ref.prograd_head's and promptsrcfit_ref.head's (a skipped term reads 0, as the header says), the emulation is within the bound."""
    inp = ref.inputs(case)
    for T in ref.PROGRAD_T:
        b, want = ref.prograd_bound(inp, T), ref.prograd_formulas(inp, T)
        assert all(_close(b[n][0], want[n]) for n in want)
        assert _hold(ref.emulate_prograd(inp, T), b, ("losses", "d_text", "d_text_kl"), "prograd") <= 1.0
    si = ref.src_inputs(inp)
    for ws in ref.SRC_WEIGHT_SETS:
        b, want = ref.promptsrc_bound(si, ws), ref.promptsrc_formulas(si, ws)
        live = [i for i in range(5) if i not in (2, 3, 4) or ws[i - 2] != 0]
        assert _close(b["losses"][0][live], want["losses"][live]) and _close(b["d_feats"][0], want["d_feats"]) and _close(b["d_text"][0], want["d_text"])
        assert _hold(ref.emulate_promptsrc(si, ws), b, ("losses", "d_feats", "d_text"), "promptsrc") <= 1.0


@pytest.mark.parametrize("case", ref.PRODA_CASES, ids=str)
def test_proda_emulation_within_bound(case):
    """ProDA: the bound's values are prodafit_ref.head's, the emulation is within the bound."""
    inp = ref.proda_inputs(case)
    b, want = ref.proda_bound(inp), ref.proda_formulas(inp)
    assert all(_close(b[n][0], want[n]) for n in want)
    assert _hold(ref.emulate_proda(inp), b, ("losses", "d_text"), "proda") <= 1.0


@pytest.mark.parametrize("corrupt", ["drop_class_256", "double_class_256", "label_mod_256", "mean_first_256", "q_single_wave"])
def test_proda_seeded_corruption_is_caught(corrupt):
    """The corruptions that reach ProDA's own loops (its softmax stride, its float64 mean, its projection) leave its bound."""
    with np.errstate(all="ignore"):
        caught = [c for c in ref.PRODA_CASES
                  if any(ref.ratio(ref.emulate_proda(ref.proda_inputs(c), corrupt=corrupt)[n], *ref.proda_bound(ref.proda_inputs(c))[n]) > 1.0 for n in ("losses", "d_text"))]
    print(f"\nproda {corrupt}: caught by {caught}")
    assert caught, f"{corrupt}: no ProDA case sees it"


@pytest.mark.parametrize("shape", ref.EXACT_DZ_CASES, ids=str)
def test_emulation_exact_dz(shape):
    """The uniform rows on two coordinates: d_text and d_feats are dz's serial sums times powers of two, bit for bit."""
    inp, d_text, d_feats, loss = ref.exact_dz_inputs(*shape)
    out = ref.emulate_coop(inp)
    assert torch.equal(out["d_text"], d_text) and torch.equal(out["d_feats"], d_feats) and abs(float(out["loss"][0]) - float(loss)) <= np.spacing(loss)


def test_emulation_bit_identities():
    """What the sources promise, for the emulation: KgCoOp at w = 0 leaves CoOp's d_text and cross-entropy; grad_scale = 2^k is an exact factor."""
    for case in ref.SHARED_CASES[:18]:
        inp = ref.inputs(case)
        a, kg = ref.emulate_coop(inp), ref.emulate_kgcoop(inp, 0.0)
        assert torch.equal(a["d_text"], kg["d_text"]) and torch.equal(a["loss"][0], kg["losses"][1])
        s = ref.emulate_coop(inp, grad_scale=1024.0)
        assert torch.equal(s["d_text"], a["d_text"] * 1024.0) and torch.equal(s["d_feats"], a["d_feats"] * 1024.0)


def _uniform_ok(out, C, labels):
    ulp = np.spacing(np.float32(np.log(np.float32(C))))
    if not abs(float(out["loss"][0]) - float(np.log(np.float32(C)))) <= ulp:
        return False
    others = [c for c in range(C) if c not in set(labels.tolist())]
    return bool((out["d_text"][others] == out["d_text"][others[0]]).all())


@pytest.mark.parametrize("shape", ref.UNIFORM_CASES, ids=str)
def test_emulation_uniform_rows(shape):
    """Equal text rows: S = C exactly, the loss is logf(C) to one unit, and the d_text rows of the classes that are nobody's label have equal bits."""
    inp = ref.uniform_inputs(*shape)
    assert _uniform_ok(ref.emulate_coop(inp), shape[1], inp["labels"])


def _axis_ok(out, want, exact):
    got = float(out["loss"][0])
    return got == float(want) if exact else abs(got - float(want)) <= float(np.spacing(want))


@pytest.mark.parametrize("shape", ref.AXIS_CASES, ids=str)
def test_emulation_axis_rows(shape):
    """Signed powers of two on single coordinates at scale 128: the batch loss is known bit for bit where every row has one maximal class,
    else to one unit."""
    inp, want, exact = ref.axis_inputs(*shape)
    out = ref.emulate_coop(inp)
    assert _axis_ok(out, want, exact)
    assert _hold(out, ref.coop_bound(inp), ("loss", "d_text", "d_feats"), "coop/vpt/maple") <= 1.0


SWEEP_LIMIT = 2_100_000      # the corruption sweep leaves out the shapes with more than this many B C E, for the suite's time: said here, not hidden
# the kinds of check that must see each corruption (a subset of what does)
EXPECTED = {"drop_class_256": {"bound", "uniform", "axis", "exact_dz"}, "double_class_256": {"bound", "uniform", "axis", "exact_dz"},
            "max_first_256": {"axis"}, "label_mod_256": {"bound", "uniform", "exact_dz"}, "skip_last_batch_row": {"bound", "exact_dz"},
            "mean_first_256": {"bound", "axis"}, "k_over_C": {"bound", "exact_dz"}, "norm_role_off_by_one": {"bound", "uniform", "axis"},
            "teacher_norms": {"bound"}, "q_single_wave": {"bound"}, "prograd_T2_dropped": {"bound"}, "src_sign0_plus": {"bound"}}


def _caught_by(corrupt):
    caught = []
    for case in ref.SHARED_CASES:
        B, C, E = case[:3]
        if B * C * E > SWEEP_LIMIT:
            continue
        inp = ref.inputs(case)
        if corrupt == "teacher_norms":
            out, b = ref.emulate_kgcoop(inp, 8.0, corrupt=corrupt), ref.kgcoop_bound(inp, 8.0)
            bad = any(ref.ratio(out[n], *b[n]) > 1.0 for n in ("losses", "d_text"))
        elif corrupt == "prograd_T2_dropped":
            bad = any(ref.ratio(ref.emulate_prograd(inp, T, corrupt=corrupt)["losses"], *ref.prograd_bound(inp, T)["losses"]) > 1.0 for T in ref.PROGRAD_T)
        elif corrupt == "src_sign0_plus":
            si = ref.src_inputs(inp)
            out, b = ref.emulate_promptsrc(si, ref.SRC_WEIGHTS, corrupt=corrupt), ref.promptsrc_bound(si, ref.SRC_WEIGHTS)
            bad = any(ref.ratio(out[n], *b[n]) > 1.0 for n in ("d_feats", "d_text"))
        else:
            out, b = ref.emulate_coop(inp, corrupt=corrupt), ref.coop_bound(inp)
            bad = any(ref.ratio(out[n], *b[n]) > 1.0 for n in ("loss", "d_text", "d_feats"))
        if bad:
            caught.append(("bound", case[:5]))
    if corrupt not in ("teacher_norms", "prograd_T2_dropped", "src_sign0_plus"):
        for shape in ref.EXACT_DZ_CASES:
            inp, d_text, d_feats, _ = ref.exact_dz_inputs(*shape)
            out = ref.emulate_coop(inp, corrupt=corrupt)
            if not (torch.equal(out["d_text"], d_text) and torch.equal(out["d_feats"], d_feats)):
                caught.append(("exact_dz", shape))
        for shape in ref.UNIFORM_CASES:
            inp = ref.uniform_inputs(*shape)
            if not _uniform_ok(ref.emulate_coop(inp, corrupt=corrupt), shape[1], inp["labels"]):
                caught.append(("uniform", shape))
        for shape in ref.AXIS_CASES:
            inp, want, exact = ref.axis_inputs(*shape)
            if not _axis_ok(ref.emulate_coop(inp, corrupt=corrupt), want, exact):
                caught.append(("axis", shape))
    return caught


@pytest.mark.parametrize("corrupt", ref.CORRUPTIONS)
def test_seeded_corruption_is_caught(corrupt):
    """Each defect seeded into the emulation leaves the bound or breaks a constructed-input equality on at least one listed case."""
    with np.errstate(all="ignore"):        # a corrupted sum may be 0 or overflow: that is the point
        caught = _caught_by(corrupt)
    print(f"\n{corrupt}: caught by {len(caught)} cases: {caught}")
    assert caught, f"{corrupt}: no listed case sees it -- the case list or the bound is too weak"
    kinds = {k for k, _ in caught}
    assert EXPECTED[corrupt] <= kinds, f"{corrupt}: not seen by {EXPECTED[corrupt] - kinds}"


def test_zz_report_ratios():
    """The emulation's worst |err| / tol per head and output (printed with -s; the record is profiles/train_heads_parity.txt)."""
    for k in sorted(RATIOS):
        print(f"emulation {k[0]:>16s} {k[1]:>10s} worst ratio {RATIOS[k]:.3f}")
    assert all(v <= 1.0 for v in RATIOS.values())
