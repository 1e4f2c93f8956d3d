"""The training loss heads through their C entry points (clipmi_coop_head, clipmi_prompt_head, clipmi_vpt_head, clipmi_maple_head,
clipmi_promptsrc_head, clipmi_cocoop_head, clipmi_proda_head) beyond 256 classes, rows and columns.

Every input lies inside a NaN-patterned guard (the columns behind a strided feature row are NaN as well), every output is sentinel-prefilled
inside guards, the workspace is a guarded buffer of EXACTLY the bytes the head's sizing function returns, and every launch is made twice.
CoOp, VPT, MaPLe, KgCoOp, ProGrad, PromptSRC, CoCoOp and ProDA are held element by element to the bound tests/head_ref.py derives
(tests/test_head_ref_cpu.py holds an fp32 emulation to the same bound), and so is ProDA.  The header documents no workspace layout, so dz is checked through what reaches the outputs."""
import numpy as np
import pytest
import torch

import head_ref as ref
from clip_calibration_amd import _lib
from test_gpu_glue_ops import Guarded, _assert_bits, _assert_within, _stream

pytestmark = pytest.mark.gpu

L = _lib.lib
RATIOS = {}


def _f32(t):
    return Guarded(t.numel(), torch.float32, t.float().contiguous())


class _Labels:
    """int64 labels in the middle of a buffer of -7 (a label read from outside poisons the row)."""

    def __init__(self, y):
        self.buf = torch.full((y.numel() + 16,), -7, dtype=torch.int64, device="cuda")
        self.buf[8:8 + y.numel()] = y.cuda()
        self.ptr = self.buf[8:].data_ptr()


def _ws_bytes(head, B, E, C, Pb=0, P=0):
    return {"coop": lambda: L.clipmi_coop_head_workspace_bytes(B, E, C), "vpt": lambda: L.clipmi_vpt_head_workspace_bytes(B, E, C),
            "maple": lambda: L.clipmi_maple_head_workspace_bytes(B, E, C), "kgcoop": lambda: L.clipmi_prompt_head_workspace_bytes(B, E, C, 1),
            "prograd": lambda: L.clipmi_prompt_head_workspace_bytes(B, E, C, 2), "promptsrc": lambda: L.clipmi_promptsrc_head_workspace_bytes(B, E, C),
            "cocoop": lambda: L.clipmi_cocoop_head_workspace_bytes(B, C), "proda": lambda: L.clipmi_proda_head_workspace_bytes(B, E, C, Pb, P)}[head]()


def _outputs(head, B, E, C, N):
    f, h = torch.float32, torch.float16
    return {"coop": [("loss", 1, f), ("d_text", C * E, f), ("d_text16", C * E, h)],
            "kgcoop": [("losses", 3, f), ("d_text", C * E, f), ("d_text16", C * E, h)],
            "prograd": [("losses", 3, f), ("d_text", C * E, f), ("d_text16", C * E, h), ("d_text_kl", C * E, f)],
            "vpt": [("loss", 1, f), ("d_feats", B * E, f)],
            "maple": [("loss", 1, f), ("d_feats", B * E, f), ("d_text", C * E, f), ("d_text16", C * E, h)],
            "promptsrc": [("losses", 5, f), ("d_feats", B * E, f), ("d_text", C * E, f), ("d_text16", C * E, h)],
            "cocoop": [("loss", 1, f), ("row_losses", B, f), ("d_text", N * E, f)],
            "proda": [("losses", 3, f), ("d_text", N * E, f)]}[head]


def _launch(head, inp, grad_scale=1.0, w=8.0, T=1.0, weights=ref.SRC_WEIGHTS, alpha=ref.PRODA_ALPHA, null=(), labels=None, short=0, misalign=0, **over):
    """One call.  Returns (rc, {name: Guarded}, workspace Guarded).  ``over``: B, C, E, Pb, P, ld, scale as passed to the call, or teacher=None; ``null``: the outputs passed as NULL."""
    B, C, E = inp["B"], inp["C"], inp["E"]
    Pb, P = inp.get("Pb", 0), inp.get("P", 0)
    N = inp["text"].shape[0]
    feats, text, y = _f32(inp["feats"]), _f32(inp["text"]), _Labels(inp["labels"] if labels is None else labels)
    teacher = _f32(inp["teacher"]) if "teacher" in inp else None
    zs = _f32(inp["zs"]) if "zs" in inp else None
    need = _ws_bytes(head, B, E, C, Pb, P)
    assert need > 0 and need % 4 == 0
    ws = Guarded(need // 4 + (1 if misalign else 0), torch.float32)
    out = {n: Guarded(k, dt) for n, k, dt in _outputs(head, B, E, C, N)}
    a = dict(B=B, C=C, E=E, ld=inp["ld"], scale=inp["scale"], teacher=None if teacher is None else teacher.ptr)
    a.update(over)
    o = {n: None if n in null else g.ptr for n, g in out.items()}
    Pb, P = a.get("Pb", Pb), a.get("P", P)
    wp, wb, s = ws.ptr + misalign, need - short, _stream()
    if head == "coop":
        rc = L.clipmi_coop_head(feats.ptr, a["ld"], y.ptr, text.ptr, a["B"], a["E"], a["C"], a["scale"], grad_scale, o["loss"], o["d_text"], o["d_text16"], wp, wb, s)
    elif head in ("kgcoop", "prograd"):
        rc = L.clipmi_prompt_head(feats.ptr, a["ld"], y.ptr, text.ptr, a["B"], a["E"], a["C"], a["scale"], grad_scale, 1 if head == "kgcoop" else 2, a["teacher"], w, T,
                                  o["losses"], o["d_text"], o["d_text16"], o.get("d_text_kl"), wp, wb, s)
    elif head == "vpt":
        rc = L.clipmi_vpt_head(feats.ptr, a["ld"], y.ptr, text.ptr, a["B"], a["E"], a["C"], a["scale"], grad_scale, o["loss"], o["d_feats"], wp, wb, s)
    elif head == "maple":
        rc = L.clipmi_maple_head(feats.ptr, a["ld"], y.ptr, text.ptr, a["B"], a["E"], a["C"], a["scale"], grad_scale, o["loss"], o["d_feats"], o["d_text"], o["d_text16"], wp, wb, s)
    elif head == "promptsrc":
        rc = L.clipmi_promptsrc_head(feats.ptr, a["ld"], zs.ptr, text.ptr, a["teacher"], y.ptr, a["B"], a["E"], a["C"], a["scale"], grad_scale, *weights, o["losses"],
                                     o["d_feats"], o["d_text"], o["d_text16"], wp, wb, s)
    elif head == "cocoop":
        rc = L.clipmi_cocoop_head(feats.ptr, a["ld"], y.ptr, text.ptr, a["B"], a["E"], a["C"], a["scale"], grad_scale, o["loss"], o["row_losses"], o["d_text"], wp, wb, s)
    else:
        rc = L.clipmi_proda_head(feats.ptr, a["ld"], y.ptr, text.ptr, a["B"], a["E"], a["C"], Pb, P, a["scale"], grad_scale, alpha, o["losses"], o["d_text"], wp, wb, s)
    torch.cuda.synchronize()
    return rc, out, ws


def _run(head, inp, **kw):
    """Two launches on the same input: guards of the outputs and of the exactly-sized workspace intact, same bits; {name: CPU tensor}."""
    got = []
    for _ in range(2):
        rc, out, ws = _launch(head, inp, **kw)
        _lib.check(rc, f"clipmi {head} head")
        ws.result(f"{head}: workspace of exactly the reported bytes")
        got.append({n: g.result(f"{head}: {n}") for n, g in out.items()})
    for n in got[0]:
        assert torch.equal(got[0][n].view(torch.int16 if got[0][n].dtype == torch.float16 else torch.int32),
                           got[1][n].view(torch.int16 if got[1][n].dtype == torch.float16 else torch.int32)), f"{head}: {n}: two launches differ"
    return got[0]


def _within(got, bound, names, head):
    for n in names:
        want, tol = bound[n]
        RATIOS[(head, n)] = max(RATIOS.get((head, n), 0.0), ref.ratio(got[n], want, tol))
    for n in names:
        want, tol = bound[n]
        _assert_within(got[n], want, tol, f"{head}: {n}")


# ------------------------------------------------------------------------------------------------------------ the element-wise bound
@pytest.mark.parametrize("case", ref.SHARED_CASES, ids=str)
def test_shared_heads_within_bound_and_bit_identities(case):
    """CoOp, VPT, MaPLe, KgCoOp (w = 8), ProGrad (T = 1 and 2) and PromptSRC (the reference weights, and with a zero image weight)
    within head_ref's per-element bound, at scale 100 and at scale 1, and at the same sizes the bit identities of the sources:
    MaPLe's sides are CoOp's and VPT's, d_text16 is d_text rounded, KgCoOp at w = 0 and ProGrad's cross-entropy half are CoOp's, PromptSRC
    with three zero weights is MaPLe's, and grad_scale = 2^10 is an exact factor of every gradient."""
    inp = ref.inputs(case)
    bound = ref.coop_bound(inp)
    coop, vpt, maple = _run("coop", inp), _run("vpt", inp), _run("maple", inp)
    _within(coop, bound, ("loss", "d_text"), "coop")
    _within(vpt, bound, ("loss", "d_feats"), "vpt")
    _within(_run("kgcoop", inp, w=8.0), ref.kgcoop_bound(inp, 8.0), ("losses", "d_text"), "kgcoop")
    for n in ("loss", "d_text", "d_text16"):
        _assert_bits(maple[n], coop[n], f"maple vs coop: {n}")
    _assert_bits(maple["d_feats"], vpt["d_feats"], "maple vs vpt: d_feats")
    _assert_bits(vpt["loss"], coop["loss"], "vpt vs coop: loss")
    _assert_bits(coop["d_text16"], coop["d_text"].half(), "coop: d_text16 vs d_text.half()")
    kg0 = _run("kgcoop", inp, w=0.0)
    _assert_bits(kg0["d_text"], coop["d_text"], "kgcoop w = 0 vs coop: d_text")
    _assert_bits(kg0["losses"][1:2], coop["loss"], "kgcoop w = 0 vs coop: cross-entropy")
    for T in ref.PROGRAD_T:
        pg = _run("prograd", inp, T=T)
        _assert_bits(pg["d_text"], coop["d_text"], "prograd vs coop: d_text")
        _assert_bits(pg["losses"][0:1], coop["loss"], "prograd vs coop: xe")
        pg["losses"] = pg["losses"][:2]
        _within(pg, ref.prograd_bound(inp, T), ("losses", "d_text_kl"), "prograd")
    si = ref.src_inputs(inp)
    for ws in ref.SRC_WEIGHT_SETS:
        got = _run("promptsrc", si, weights=ws)
        _within(got, ref.promptsrc_bound(si, ws), ("losses", "d_feats", "d_text"), "promptsrc")
        _assert_bits(got["d_text16"], got["d_text"].half(), "promptsrc: d_text16 vs d_text.half()")
    src = _run("promptsrc", si, weights=(0.0, 0.0, 0.0))
    for n in ("d_feats", "d_text", "d_text16"):
        _assert_bits(src[n], maple[n], f"promptsrc, zero weights, vs maple: {n}")
    _assert_bits(src["losses"][0:1], maple["loss"], "promptsrc, zero weights, vs maple: loss")
    _assert_bits(src["losses"][2:], torch.zeros(3), "promptsrc, zero weights: the skipped terms read 0")
    scaled = _run("maple", inp, grad_scale=1024.0)
    _assert_bits(scaled["d_text"], maple["d_text"] * 1024.0, "maple: grad_scale = 2^10 on d_text")
    _assert_bits(scaled["d_feats"], maple["d_feats"] * 1024.0, "maple: grad_scale = 2^10 on d_feats")


@pytest.mark.parametrize("case", ref.COCOOP_CASES, ids=str)
def test_cocoop_head_within_bound(case):
    inp = ref.inputs(case, True)
    got = _run("cocoop", inp)
    _within(got, ref.cocoop_bound(inp), ("loss", "row_losses", "d_text"), "cocoop")


@pytest.mark.parametrize("case", ref.PRODA_CASES, ids=str)
def test_proda_head_within_bound(case):
    """clipmi_proda_head with (Pb, P) from prodafit_ref.HEAD_CASES at C = 257 .. 1000, E = 1 .. 1024 and B = 257, at scale 100 and at
    prodafit_ref.HEAD_SCALE: losses and every entry of d_text (class rows and no-class rows) within head_ref.proda_bound."""
    inp = ref.proda_inputs(case)
    _within(_run("proda", inp), ref.proda_bound(inp), ("losses", "d_text"), "proda")


# --------------------------------------------------------------------------------------------------------------- constructed inputs
def _one_unit(got, want, what):
    assert abs(float(got) - float(want)) <= float(np.spacing(np.float32(want))), f"{what}: got {float(got)!r}, want {float(want)!r} to one fp32 unit"


@pytest.mark.parametrize("shape", ref.UNIFORM_CASES, ids=str)
def test_uniform_rows(shape):
    """Equal text rows (and equal teacher rows): every logit of a row has the same bits, S = C exactly, the loss is logf(C) to one unit --
    a class skipped or counted twice at the stride seam gives log(C -+ 1) -- and every class that is nobody's label gets the same d_text
    bits.  ProGrad's and PromptSRC's second softmax is uniform too: p = q = fl(1 / C), the logit term adds exactly nothing."""
    B, C, E = shape
    inp = ref.uniform_inputs(*shape)
    want = np.log(np.float32(C))
    coop = _run("coop", inp)
    _one_unit(coop["loss"][0], want, "coop: loss = logf(C)")
    others = [c for c in range(C) if c not in set(inp["labels"].tolist())]
    rows = coop["d_text"].reshape(C, E)
    _assert_bits(rows[others], rows[others[:1]].expand(len(others), E), "coop: d_text rows of the unlabelled classes")
    _within(coop, ref.coop_bound(inp), ("loss", "d_text"), "coop")
    maple = _run("maple", inp)
    src = _run("promptsrc", dict(ref.src_inputs(inp), teacher=inp["teacher"]), weights=(0.0, 0.0, 25.0))     # the teacher's rows stay equal
    for n in ("d_feats", "d_text"):
        _assert_bits(src[n], maple[n], f"promptsrc, uniform p = q, vs maple: {n}")
    assert float(src["losses"][4]) == 0.0 and float(src["losses"][0]) == float(maple["loss"][0])
    pg = _run("prograd", inp, T=2.0)
    assert (pg["d_text_kl"] == 0).all(), "prograd: uniform student and teacher: dz_kl = 0 exactly"
    _one_unit(pg["losses"][0], want, "prograd: xe = logf(C)")
    cc = dict(inp, text=inp["text"].repeat(B, 1))
    got = _run("cocoop", cc)
    _one_unit(got["loss"][0], want, "cocoop: loss = logf(C)")


@pytest.mark.parametrize("shape", ref.AXIS_CASES, ids=str)
def test_axis_rows(shape):
    """Signed powers of two on single coordinates at scale 128: norms, cosines and logits are exact, exp(-128) is 0 in fp32, and the batch loss
    is known bit for bit where every row has one maximal class (a row dropped by the float64 mean at index 256 shifts it by 128 / B),
    else to one unit."""
    inp, want, exact = ref.axis_inputs(*shape)
    for head in ("coop", "vpt"):
        got = _run(head, inp)
        if exact:
            _assert_bits(got["loss"], torch.tensor([float(want)]), f"{head}: batch loss")
        else:
            _one_unit(got["loss"][0], want, f"{head}: batch loss")
    _within(_run("maple", inp), ref.coop_bound(inp), ("loss", "d_text", "d_feats"), "maple")


@pytest.mark.parametrize("shape", ref.EXACT_DZ_CASES, ids=str)
def test_exact_dz_through_the_outputs(shape):
    """Uniform rows on two coordinates (head_ref.exact_dz_inputs): z = 0, p = fl(1 / C), and every product behind dz is by 0, 1 or a power
    of two, so d_text = scale 2 (sum_b dz[b, c]) e_1 and d_feats = scale 2^-b (sum_c dz[b, c]) e_0 in the kernels' serial fp32 order are
    known bit for bit: dz[c] = fl(1 / C) k, (fl(1 / C) - 1) k at the label, read through what reaches the outputs (the header documents no
    workspace offset for dz).  With B = 1 an entry of d_text IS dz times 2^7."""
    inp, d_text, d_feats, loss = ref.exact_dz_inputs(*shape)
    maple, coop, vpt = _run("maple", inp), _run("coop", inp), _run("vpt", inp)
    for got in (maple, coop):
        assert torch.equal(got["d_text"].reshape(d_text.shape), d_text), "d_text is not dz's serial sum bit for bit"
    for got in (maple, vpt):
        assert torch.equal(got["d_feats"].reshape(d_feats.shape), d_feats), "d_feats is not dz's serial sum bit for bit"
        _one_unit(got["loss"][0], loss, "loss = logf(C)")
    src = _run("promptsrc", dict(inp, zs=inp["feats"].clone()), weights=(0.0, 0.0, 25.0))
    assert torch.equal(src["d_text"].reshape(d_text.shape), d_text) and torch.equal(src["d_feats"].reshape(d_feats.shape), d_feats)
    pg = _run("prograd", inp, T=2.0)
    assert torch.equal(pg["d_text"].reshape(d_text.shape), d_text) and (pg["d_text_kl"] == 0).all()


# ---------------------------------------------------------------------------------- the two fits that call the same xent_row
@pytest.mark.parametrize("shape", [(5, 64, 257), (4, 128, 1000)], ids=str)
def test_taskres_step_beyond_256_classes(shape):
    """clipmi_taskres_train_step at C = 257 and 1000 (its own limit is C <= 65535 * its tile: both are admitted) against its float64
    reference under its existing tolerance rule: test_gpu_taskresfit.test_one_step_gradient's body on the new shapes."""
    import test_gpu_taskresfit as tr
    tr.test_one_step_gradient(shape)


@pytest.mark.parametrize("shape", [(5, 64, 16, 257), (4, 128, 32, 1000)], ids=str)
def test_adapter_step_beyond_256_classes(shape, monkeypatch):
    """clipmi_adapter_train_step at C = 257 and 1000 (it asks C >= 2 and sets no upper limit) against its float64 reference under its
    existing tolerance rule: test_gpu_adapterfit.test_one_step_gradient's body on the new shapes, seed 1 (no entry at a ReLU kink)."""
    import adapterfit_ref
    import test_gpu_adapterfit as ad
    monkeypatch.setitem(adapterfit_ref.SHAPES, shape, 1)          # the reference keeps a case's seed next to its shape
    ad.test_one_step_gradient(shape)


@pytest.mark.parametrize("shape", [(3, 257, 64), (4, 1000, 512), (5, 257, 768)], ids=str)
def test_teacher_equal_to_student_adds_nothing(shape):
    """Teacher == student at C = 257, 1000 and E = 768: ProGrad's dz_kl is 0 exactly; PromptSRC's KL rows and L1 rows are 0 and its gradients
    and cross-entropy keep MaPLe's (CoOp's and VPT's) bits."""
    B, C, E = shape
    inp = ref.src_inputs(ref.inputs((B, C, E, True, 100.0, None)), same=True)
    maple = _run("maple", inp)
    pg = _run("prograd", inp, T=2.0)
    assert (pg["d_text_kl"] == 0).all(), "prograd: d_text_kl"
    _assert_bits(pg["d_text"], maple["d_text"], "prograd vs coop: d_text")
    src = _run("promptsrc", inp)
    for n in ("d_feats", "d_text", "d_text16"):
        _assert_bits(src[n], maple[n], f"promptsrc vs maple: {n}")
    _assert_bits(src["losses"][2:], torch.zeros(3), "promptsrc: text L1, image L1, logit KL")
    _assert_bits(src["losses"][0:1], maple["loss"], "promptsrc: total")
    _assert_bits(src["losses"][1:2], maple["loss"], "promptsrc: cross-entropy")


# -------------------------------------------------------------------------------------------------------------------- bad labels
def _bad_case(head):
    B, C, E = 3, 257, 64
    inp = dict(ref.inputs((B, C, E, True, 100.0, (255, 256, 7)), head == "cocoop"))
    if head == "promptsrc":
        inp = ref.src_inputs(inp)
    if head == "proda":
        g = torch.Generator().manual_seed(77)
        inp.update(Pb=2, P=3, text=torch.randn(C * 2 + 3, E, generator=g))
    return inp, torch.tensor([-1, 256, C])


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


@pytest.mark.parametrize("head", ["coop", "kgcoop", "prograd", "vpt", "maple", "promptsrc", "cocoop", "proda"])
def test_bad_labels_poison_exactly_the_documented_set(head):
    """Labels -1 in row 0 and C in row B - 1 at C = 257: exactly what include/clipmi.h documents turns NaN, everything else keeps the bits
    of the same call with good labels, and the guards stay intact."""
    inp, bad = _bad_case(head)
    B, C, E = inp["B"], inp["C"], inp["E"]
    good, got = _run(head, inp), _run(head, inp, labels=bad)
    if head in ("coop", "maple"):
        assert _all_nan(got["loss"]) and _all_nan(got["d_text"]) and _all_nan(got["d_text16"])
    if head in ("vpt", "maple", "promptsrc"):
        d, dg = got["d_feats"].reshape(B, E), good["d_feats"].reshape(B, E)
        assert _all_nan(d[0]) and _all_nan(d[2])
        _assert_bits(d[1], dg[1], f"{head}: d_feats of the row with a good label")
    if head == "vpt":
        assert _all_nan(got["loss"])
    if head == "kgcoop":
        assert _all_nan(got["losses"][:2]) and _all_nan(got["d_text"])
        _assert_bits(got["losses"][2:], good["losses"][2:], "kgcoop: the cosine score")
    if head == "prograd":
        assert _all_nan(got["losses"][:1]) and _all_nan(got["d_text"])
        _assert_bits(got["losses"][1:2], good["losses"][1:2], "prograd: the distillation loss")
        _assert_bits(got["d_text_kl"], good["d_text_kl"], "prograd: d_text_kl")
    if head == "promptsrc":
        assert _all_nan(got["losses"][:2]) and _all_nan(got["d_text"]) and _all_nan(got["d_text16"])
        _assert_bits(got["losses"][2:], good["losses"][2:], "promptsrc: text L1, image L1, logit KL")
    if head == "cocoop":
        d, dg = got["d_text"].reshape(B, C * E), good["d_text"].reshape(B, C * E)
        assert _all_nan(got["loss"]) and _all_nan(got["row_losses"][[0, 2]]) and _all_nan(d[0]) and _all_nan(d[2])
        _assert_bits(d[1], dg[1], "cocoop: d_text rows of the image with a good label")
        _assert_bits(got["row_losses"][1:2], good["row_losses"][1:2], "cocoop: row loss of the image with a good label")
    if head == "proda":
        n = C * inp["Pb"] * E
        assert _all_nan(got["losses"][:2]) and _all_nan(got["d_text"][:n])
        _assert_bits(got["losses"][2:], good["losses"][2:], "proda: the orthogonality term")
        _assert_bits(got["d_text"][n:], good["d_text"][n:], "proda: the no-class rows")


# ---------------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("head", ["coop", "kgcoop", "prograd", "vpt", "maple", "promptsrc", "cocoop", "proda"])
def test_refusals_leave_the_outputs_untouched(head):
    """One refused call per requirement of the launcher: the right code, no output sentinel touched."""
    inp, _ = _bad_case(head)
    E = inp["E"]
    refused = [("workspace one byte short", dict(short=1), _lib.ERR_WORKSPACE), ("C = 1", dict(C=1), _lib.ERR_SHAPE), ("ld < E", dict(ld=E - 1), _lib.ERR_SHAPE),
               ("B = 0", dict(B=0), _lib.ERR_SHAPE), ("scale = inf", dict(scale=float("inf")), _lib.ERR_ARG), ("scale = nan", dict(scale=float("nan")), _lib.ERR_ARG),
               ("grad_scale = inf", dict(grad_scale=float("inf")), _lib.ERR_ARG), ("workspace misaligned by 4", dict(misalign=4), _lib.ERR_ARG)]
    if head in ("kgcoop", "prograd", "promptsrc"):
        refused.append(("null teacher", dict(teacher=None), _lib.ERR_ARG))
    if head == "kgcoop":
        refused.append(("w < 0", dict(w=-1.0), _lib.ERR_ARG))
    grad = "d_feats" if head == "vpt" else "d_text"
    refused.append((f"null {grad}", dict(null=(grad,)), _lib.ERR_ARG))
    if head == "prograd":
        refused.append(("T = 0", dict(T=0.0), _lib.ERR_ARG))
        refused.append(("null d_text_kl", dict(null=("d_text_kl",)), _lib.ERR_ARG))
    if head == "promptsrc":
        refused.append(("w_text < 0", dict(weights=(-1.0, 0.0, 0.0)), _lib.ERR_ARG))
    if head == "proda":
        refused.append(("alpha < 0", dict(alpha=-1.0), _lib.ERR_ARG))
        refused += [("P = 1", dict(P=1, Pb=1), _lib.ERR_SHAPE), ("Pb = 0", dict(Pb=0), _lib.ERR_SHAPE), ("Pb > P", dict(Pb=inp["P"] + 1), _lib.ERR_SHAPE)]
    for what, kw, code in refused:
        rc, out, ws = _launch(head, inp, **kw)
        assert rc == code, f"{head}: {what}: returned {rc}, want {code}"
        assert all(g.untouched() for g in out.values()) and ws.untouched(), f"{head}: {what}: a refused call wrote"


def test_zz_report_ratios():
    """The device's worst |err| / tol per head and output (printed with -s; the record is profiles/train_heads_parity.txt)."""
    for k in sorted(RATIOS):
        print(f"device {k[0]:>10s} {k[1]:>10s} worst ratio {RATIOS[k]:.3f}")
    assert all(v <= 1.0 for v in RATIOS.values())
