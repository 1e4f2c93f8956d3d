"""The calibration tail at operator level: clipmi_l2_normalize_to, clipmi_logits, clipmi_calibrate_rows, clipmi_softmax_rows, clipmi_fused_tail
(tail_unfused 0 and 1), clipmi_ece_accumulate and clipmi_knn_dists, one entry point at a time against tests/tail_ref.py: random inputs within
the per-element tolerances the float64 references return (tests/test_tail_ref_cpu.py holds a CPU emulation to the same tolerances and asserts
that no random row has an ambiguous argmax), and constructed inputs that need none -- one-hot rows (a logit is one text element times the
scale, bit for bit), duplicated classes (ties: identical columns, the lowest index wins), uniform rows (conf = 1 / C), poisoned neighbours
(no bit changes), ECE confidences on every bin edge, lattice kNN sets.  Inputs end right in front of a NaN-patterned guard, outputs sit
between sentinel guards, every launch is made twice (same bits), and after every fused launch the 64 KiB ticket-counter region is zero.
CLIPMI_TAIL_TEST_REPORT=<file> collects the worst |err| / tol per kernel."""
import json
import os

import numpy as np
import pytest
import torch

import tail_ref as ref
from clip_calibration_amd import _lib
from test_gpu_glue_ops import PAD, Guarded, _assert_bits, _assert_within, _stream, _twice, ops  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu

L = _lib.lib
DT = {torch.float16: _lib.F16, torch.float32: _lib.F32}
WORST = {}
COUNTER_BYTES = 64 * 1024
F64_MARK = -1.2345678e300


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("CLIPMI_TAIL_TEST_REPORT")
    if path and WORST:
        with open(path, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


def _note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)


def _id(c):
    return "-".join(str(x).replace("torch.", "") for x in c)


def _inputs_intact(*guards):
    for d in guards:
        b = d.buf.view(d.idt)
        assert bool((b[:PAD] == d.mark).all()) and bool((b[PAD + d.n:] == d.mark).all()), "a launch wrote around one of its inputs"


class GuardedBins:
    """3 (n_bins + 1) doubles between sentinel guards, zero or `init` to begin with."""

    def __init__(self, n_bins, init=None):
        self.n = 3 * (n_bins + 1)
        self.buf = torch.full((2 * PAD + self.n,), F64_MARK, dtype=torch.float64, device="cuda")
        self.view = self.buf[PAD:PAD + self.n]
        self.view.copy_(torch.zeros(self.n, dtype=torch.float64) if init is None else torch.as_tensor(init, dtype=torch.float64).reshape(-1))
        self.ptr = self.view.data_ptr()

    def result(self, what):
        torch.cuda.synchronize()
        b = self.buf.cpu()
        assert (b[:PAD] == F64_MARK).all() and (b[PAD + self.n:] == F64_MARK).all(), f"{what}: wrote outside its bins"
        return b[PAD:PAD + self.n].numpy().reshape(3, -1).copy()


def _same(a, b, what):
    """Two launches on the same input: the same bits in every output but the bins, whose sums depend on the order of the atomics."""
    for k in a:
        if k != "bins" and a[k] is not None:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: two launches on the same input differ in {k}"


def fused_tail(clipmi_option, d_img, dtype, d_txt, scale, dac, normalize, unfused, labels, n_bins, B, C, E):
    """clipmi_fused_tail twice into guarded outputs -> {"logits" [B, C], "img_n" [B, E] or None, "conf", "pred", "bins" [3, n_bins + 1]}."""
    clipmi_option("tail_unfused", int(unfused))
    what = f"clipmi_fused_tail(unfused={int(unfused)}, normalize={int(normalize)}, dac={dac is not None}) {(B, C, E)}"
    need = L.clipmi_fused_tail_workspace_bytes(B, C)
    runs = []
    for _ in range(2):
        ws = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
        ws[need:] = 0xA5
        lg, conf, pred = Guarded(B * C, torch.float32), Guarded(B, torch.float32), Guarded(B, torch.int32)
        img_n = Guarded(B * E, torch.float32) if normalize else None
        bins = GuardedBins(n_bins)
        _lib.check(L.clipmi_fused_tail(d_img.ptr, DT[dtype], int(normalize), d_txt.ptr, float(scale), None if dac is None else dac.data_ptr(), lg.ptr,
                                       img_n.ptr if normalize else None, conf.ptr, pred.ptr, labels.data_ptr(), bins.ptr, n_bins, ws.data_ptr(), need,
                                       B, C, E, _stream()), what)
        out = {"logits": lg.result(what + " logits").reshape(B, C), "conf": conf.result(what + " conf"), "pred": pred.result(what + " pred"),
               "bins": bins.result(what), "img_n": img_n.result(what + " img_n").reshape(B, E) if normalize else None}
        w = ws.cpu()
        assert int(w[:COUNTER_BYTES].view(torch.int32).abs().sum()) == 0, f"{what}: ticket counters left non-zero"
        assert (w[need:] == 0xA5).all(), f"{what}: wrote behind its workspace"
        runs.append(out)
    _inputs_intact(d_img, d_txt)
    _same(runs[0], runs[1], what)
    ref.assert_bins(runs[1]["bins"], runs[0]["bins"], B, what + ": bins of the two launches")
    return runs[0]


def _paths(dtype, normalize, E):
    """(unfused?) settings clipmi_fused_tail takes for these features: the separate launches refuse fp16 features that they do not normalise,
    so fp16 pre-normalised rows run fused only.  Every shape sent through fused_tail() must satisfy clipmi_fused_tail's `fits` (E % 64 == 0 and
    2 RB (2 E + 16) + 16 <= 160 KiB of LDS, RB = 16 up to B = 512 and 32 above): otherwise the library runs the separate launches under
    tail_unfused = 0 as well, and the fused kernel is not tested."""
    assert fused_fits(1, E) and fused_fits(513, E), f"E = {E}: clipmi_fused_tail would fall back to the separate launches"
    return (False, True) if (normalize or dtype == torch.float32) else (False,)


def fused_fits(B, E):
    return E % 64 == 0 and 2 * (16 if B <= 512 else 32) * (2 * E + 16) + 32 <= 160 * 1024


# ---- random, under the derived tolerances -----------------------------------------------------------------------------------------------------------
FUSED_RANDOM = [(s, dt, nz) for s in ref.FUSED_SHAPES for dt in ref.DTYPES for nz in (True, False)]


@pytest.mark.parametrize("case", FUSED_RANDOM, ids=_id)
def test_fused_tail_random(clipmi_option, case):
    """Logits within tol of float64; conf within its tol of the float64 softmax of the returned logits; pred == the float64 argmax; the bins ==
    bin_statistics of the returned (conf, pred): counts and hits exactly, sums to the order of B double additions; fused == unfused bit for bit."""
    (B, C, E, seed), dt, nz = case
    img, txt_n, dac, labels = ref.random_inputs(B, C, E, seed, dt, nz)
    d_img, d_txt, d_dac, d_lab = Guarded(B * E, dt, img), Guarded(C * E, torch.float32, txt_n), dac.cuda(), labels.cuda()
    for scale in ref.SCALES:
        for d in (None, d_dac):
            outs = []
            for unfused in _paths(dt, nz, E):
                o = fused_tail(clipmi_option, d_img, dt, d_txt, scale, d, nz, unfused, d_lab, ref.N_BINS, B, C, E)
                tag = "unfused " if unfused else "fused "
                ref.check_tail(o["img_n"], None, o["logits"], o["conf"], o["pred"], case, scale, None if d is None else dac, labels,
                               lambda k, v: _note(tag + k, v))
                ref.assert_bins(o["bins"], ref.bin_statistics(o["conf"].numpy(), o["pred"].numpy(), labels.numpy(), ref.N_BINS), B, f"{case} bins")
                outs.append(o)
            if len(outs) == 2:
                for k in ("logits", "conf", "pred"):
                    _assert_bits(outs[1][k], outs[0][k], f"{case}: unfused against fused, {k}")


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("shape", ref.LOGITS_SHAPES, ids=_id)
def test_logits_entry_random(shape, normalize):
    """clipmi_l2_normalize_to -> clipmi_logits (E % 32 == 16: split steps, then the exact-f32 tail step), with and without DAC / conf / pred; then
    clipmi_calibrate_rows and clipmi_softmax_rows on the returned logits: bit for bit what clipmi_logits did itself, probs within their tolerance."""
    B, C, E, seed = shape
    case = (shape, torch.float32, normalize)
    img, txt_n, dac, labels = ref.random_inputs(B, C, E, seed, torch.float32, normalize)
    d_img, d_txt, d_dac = Guarded(B * E, torch.float32, img), Guarded(C * E, torch.float32, txt_n), dac.cuda()
    img_n = None
    if normalize:
        img_n = _twice(B * E, torch.float32, "clipmi_l2_normalize_to",
                       lambda p: L.clipmi_l2_normalize_to(d_img.ptr, _lib.F32, p, _lib.F32, B, E, _stream())).reshape(B, E)
        d_in = Guarded(B * E, torch.float32, img_n)
    else:
        d_in = d_img
    for scale in ref.SCALES:
        raw = _twice(B * C, torch.float32, "clipmi_logits",
                     lambda p: L.clipmi_logits(d_in.ptr, d_txt.ptr, scale, None, p, None, None, B, C, E, _stream())).reshape(B, C)
        for d, hd in ((None, None), (d_dac, dac)):
            conf, pred = Guarded(B, torch.float32), Guarded(B, torch.int32)
            lg = _twice(B * C, torch.float32, "clipmi_logits",
                        lambda p: L.clipmi_logits(d_in.ptr, d_txt.ptr, scale, None if d is None else d.data_ptr(), p, conf.ptr, pred.ptr, B, C, E, _stream())).reshape(B, C)
            cf, pr = conf.result("conf"), pred.result("pred")
            ref.check_tail(img_n, raw, lg, cf, pr, case, scale, hd, labels, lambda k, v: _note("logits-entry " + k, v))
            # the row kernels on their own, from the raw logits
            c2, p2 = Guarded(B, torch.float32), Guarded(B, torch.int32)
            sep = _twice(B * C, torch.float32, "clipmi_calibrate_rows",
                         lambda p: L.clipmi_calibrate_rows(p, None if d is None else d.data_ptr(), c2.ptr, p2.ptr, B, C, _stream()), init=raw).reshape(B, C)
            _assert_bits(sep, lg, "clipmi_calibrate_rows against the row pass of clipmi_logits")
            _assert_bits(c2.result("conf"), cf, "calibrate_rows conf")
            _assert_bits(p2.result("pred"), pr, "calibrate_rows pred")
            d_raw, c3, p3 = Guarded(B * C, torch.float32, raw), Guarded(B, torch.float32), Guarded(B, torch.int32)
            probs = _twice(B * C, torch.float32, "clipmi_softmax_rows",
                           lambda p: L.clipmi_softmax_rows(d_raw.ptr, None if d is None else d.data_ptr(), p, c3.ptr, p3.ptr, B, C, _stream())).reshape(B, C)
            _inputs_intact(d_raw)
            _assert_bits(d_raw.view.cpu().reshape(B, C), raw, "clipmi_softmax_rows changed its logits")
            _assert_bits(c3.result("conf"), cf, "softmax_rows conf")
            _assert_bits(p3.result("pred"), pr, "softmax_rows pred")
            _, _, _, p64, ptol = ref.softmax_top1(lg)
            _note("softmax_rows probs", ref.worst_ratio(probs, p64, ptol))
            _assert_within(probs, p64, ptol, "clipmi_softmax_rows probs [b, c]")
            _assert_bits(probs[torch.arange(B), pr.long()], cf, "clipmi_softmax_rows: probs[b, pred] against conf (exp(0) / sum: the same bits)")
    _inputs_intact(d_img, d_txt, d_in)


@pytest.mark.parametrize("case", [(5, 64, torch.float32, torch.float32), (3, 100, torch.float32, torch.float32), (9, 1088, torch.float16, torch.float32),
                                  (7, 72, torch.float32, torch.float16), (4, 512, torch.float16, torch.float16), (1, 16, torch.float32, torch.float32)], ids=_id)
def test_l2_normalize_to(case):
    """Vector path (E % 8 == 0) and element path (E = 100), fp32 and fp16 in and out."""
    rows, E, dti, dto = case
    x = (torch.randn(rows, E, generator=ref._gen(rows, E)) * 3).to(dti)
    d = Guarded(rows * E, dti, x)
    got = _twice(rows * E, dto, "clipmi_l2_normalize_to", lambda p: L.clipmi_l2_normalize_to(d.ptr, DT[dti], p, DT[dto], rows, E, _stream())).reshape(rows, E)
    _inputs_intact(d)
    want, tol = ref.l2_normalize(x, dto)
    _note("l2norm -> " + str(dto).replace("torch.", ""), ref.worst_ratio(got, want, tol))
    _assert_within(got, want, tol, "clipmi_l2_normalize_to [row, e]")


# ---- small components: fp16-subnormal operand halves ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", [False, True], ids=["image-small", "text-small"])
def test_small_components(clipmi_option, mirror):
    """Components in [2^-27, 2^-14) facing 0.7: the hi half is an fp16 subnormal (or zero), the lo half sits on the subnormal grid.  Same tolerance
    formula as the random cases; a flushed operand half would be out by 10x and more (tests/test_tail_ref_cpu.py::test_emulation_small_components)."""
    img_n, txt_n = ref.small_component_rows(mirror)
    B, E = img_n.shape
    C = txt_n.shape[0]
    want, tol, _ = ref.cosine_logits(img_n, txt_n, 100.0, False)
    d_img, d_txt = Guarded(B * E, torch.float32, img_n), Guarded(C * E, torch.float32, txt_n)
    labels = torch.zeros(B, dtype=torch.int64, device="cuda")
    for unfused in (False, True):
        o = fused_tail(clipmi_option, d_img, torch.float32, d_txt, 100.0, None, False, unfused, labels, ref.N_BINS, B, C, E)
        _note(("unfused" if unfused else "fused") + " logits small components", ref.worst_ratio(o["logits"], want, tol))
        _assert_within(o["logits"], want, tol, f"small components (unfused={unfused}) [b, c]")


# ---- exact ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.ONE_HOT, ids=_id)
def test_one_hot_rows(clipmi_option, case):
    """logits[b, c] == fp32(scale) * txt[c, b] bit for bit, j = b walking every column: a dropped or doubled k-step, a swapped fragment, a wrong
    clamp at a ragged edge or a row stored in the wrong place changes bits."""
    E, C, fused = case
    B = E
    labels = torch.zeros(B, dtype=torch.int64, device="cuda")
    for nz in ((True, False) if fused else (False,)):
        img, txt = ref.one_hot_case(E, C, nz)
        for dt in (ref.DTYPES if fused else (torch.float32,)):
            d_img, d_txt = Guarded(B * E, dt, img.to(dt)), Guarded(C * E, torch.float32, txt)
            for scale in ref.SCALES:
                if fused:
                    for unfused in _paths(dt, nz, E):
                        o = fused_tail(clipmi_option, d_img, dt, d_txt, scale, None, nz, unfused, labels, ref.N_BINS, B, C, E)
                        ref.check_one_hot(o["logits"], txt, scale, f"one-hot {case} normalize={nz} {dt} unfused={unfused}")
                        if nz:
                            _assert_bits(o["img_n"], torch.eye(E), "one-hot img_n")
                else:
                    lg = _twice(B * C, torch.float32, "clipmi_logits", lambda p: L.clipmi_logits(d_img.ptr, d_txt.ptr, scale, None, p, None, None, B, C, E, _stream()))
                    ref.check_one_hot(lg.reshape(B, C), txt, scale, f"one-hot {case} clipmi_logits")


@pytest.mark.parametrize("case", ref.TIES, ids=_id)
def test_argmax_ties(clipmi_option, case):
    """Duplicated class prompts: identical logit columns, and wave_argmax, merge_max, the lane-strided DAC pass and the 16-partial chunks all
    give the lowest tied index -- fused and unfused, with and without DAC, and through clipmi_softmax_rows."""
    B, C, cols = case
    E = ref.TIES_E
    img, txt = ref.ties_case(*case)
    dac = torch.linspace(0.5, 1.5, C).cuda()
    d_img, d_txt = Guarded(B * E, torch.float32, img), Guarded(C * E, torch.float32, txt)
    labels = torch.zeros(B, dtype=torch.int64, device="cuda")
    for d in (None, dac):
        for unfused in (False, True):
            o = fused_tail(clipmi_option, d_img, torch.float32, d_txt, 100.0, d, True, unfused, labels, ref.N_BINS, B, C, E)
            ref.check_ties(o["logits"], o["pred"], cols, f"ties {case} dac={d is not None} unfused={unfused}")
        d_lg, pred = Guarded(B * C, torch.float32, o["logits"]), Guarded(B, torch.int32)
        probs = _twice(B * C, torch.float32, "clipmi_softmax_rows",
                       lambda p: L.clipmi_softmax_rows(d_lg.ptr, None if d is None else d.data_ptr(), p, None, pred.ptr, B, C, _stream())).reshape(B, C)
        ref.check_ties(probs, pred.result("pred"), cols, f"ties {case} dac={d is not None} softmax_rows")


@pytest.mark.parametrize("C", ref.UNIFORM_C)
def test_uniform_rows(clipmi_option, C):
    """All classes equal: pred 0, conf = 1 / C to the nearest fp32 value or its neighbour -- every class counted once."""
    img, txt = ref.uniform_case(C)
    B, E = img.shape
    dac = torch.linspace(0.5, 1.5, C).cuda()
    d_img, d_txt = Guarded(B * E, torch.float32, img), Guarded(C * E, torch.float32, txt)
    labels = torch.zeros(B, dtype=torch.int64, device="cuda")
    for d in (None, dac):
        for unfused in (False, True):
            o = fused_tail(clipmi_option, d_img, torch.float32, d_txt, 100.0, d, True, unfused, labels, ref.N_BINS, B, C, E)
            ref.check_uniform(o["logits"], o["conf"], o["pred"], C, f"uniform C={C} dac={d is not None} unfused={unfused}")


@pytest.mark.parametrize("B", [40, 530])
def test_isolation(clipmi_option, B):
    """Image rows of NaN and inf: no bit of the clean rows' logits, conf or pred changes; classes of NaN and inf: no bit of the clean columns;
    rows of NaN / inf logits through clipmi_calibrate_rows: the clean rows as without them.  (B = 530: RB = 32.)"""
    C, E = 130, 64
    g = ref._gen(B, 99)
    img, txt_n, dac, _ = ref.random_inputs(B, C, E, 1, torch.float32, True)
    labels = torch.zeros(B, dtype=torch.int64, device="cuda")
    d_dac = dac.cuda()
    bad_rows = torch.arange(B) % 3 == 1
    bad_cols = torch.arange(C) % 5 == 2
    img_p = torch.where(bad_rows[:, None], ref.poison_rows(img, g), img)
    txt_p = torch.where(bad_cols[:, None], ref.poison_rows(txt_n, g), txt_n)
    keep = (~bad_cols).nonzero().flatten()
    for d in (None, d_dac):
        for unfused in (False, True):
            run = lambda i, t, c, dd: fused_tail(clipmi_option, Guarded(i.numel(), torch.float32, i), torch.float32, Guarded(t.numel(), torch.float32, t), 100.0,   # noqa: E731
                                                 dd, True, unfused, labels, ref.N_BINS, B, c, E)
            clean = run(img, txt_n, C, d)
            rows = run(img_p, txt_n, C, d)
            for k in ("logits", "conf", "pred", "img_n"):
                _assert_bits(rows[k][~bad_rows], clean[k][~bad_rows], f"isolation: clean rows among poisoned rows, {k} (dac={d is not None}, unfused={unfused})")
            if d is None:
                few = run(img, txt_n[keep].contiguous(), keep.numel(), None)
                cols = run(img, txt_p, C, None)
                _assert_bits(cols["logits"][:, keep], few["logits"], f"isolation: clean columns among poisoned classes (unfused={unfused})")
    lg = fused_tail(clipmi_option, Guarded(B * E, torch.float32, img), torch.float32, Guarded(C * E, torch.float32, txt_n), 100.0, None, True, False, labels,
                    ref.N_BINS, B, C, E)["logits"]
    lg_p = torch.where(bad_rows[:, None], ref.poison_rows(lg, g), lg)
    for d in (None, d_dac):
        res = []
        for x in (lg, lg_p):
            conf, pred = Guarded(B, torch.float32), Guarded(B, torch.int32)
            out = _twice(B * C, torch.float32, "clipmi_calibrate_rows",
                         lambda p: L.clipmi_calibrate_rows(p, None if d is None else d.data_ptr(), conf.ptr, pred.ptr, B, C, _stream()), init=x).reshape(B, C)
            res.append((out, conf.result("conf"), pred.result("pred")))
        for a, b, k in zip(res[1], res[0], ("logits", "conf", "pred")):
            _assert_bits(a[~bad_rows], b[~bad_rows], f"isolation: clipmi_calibrate_rows, {k} (dac={d is not None})")


# ---- clipmi_ece_accumulate ---------------------------------------------------------------------------------------------------------------------------------
def _ece(conf, pred, labels, n_bins, init=None):
    d_c, d_p = Guarded(conf.size, torch.float32, torch.from_numpy(conf)), Guarded(pred.size, torch.int32, torch.from_numpy(pred))
    d_l = torch.from_numpy(labels).cuda()
    outs = []
    for _ in range(2):
        bins = GuardedBins(n_bins, init)
        _lib.check(L.clipmi_ece_accumulate(d_c.ptr, d_p.ptr, d_l.data_ptr(), conf.size, bins.ptr, n_bins, _stream()), "clipmi_ece_accumulate")
        outs.append(bins.result("clipmi_ece_accumulate"))
    _inputs_intact(d_c, d_p)
    ref.assert_bins(outs[1], outs[0], conf.size, "two launches")
    return outs[0]


@pytest.mark.parametrize("n_bins", ref.ECE_N_BINS)
def test_ece_bins_at_every_edge(n_bins):
    """The fp32 values just below, at and just above every edge, 0.0, -0.0, the smallest subnormal, nextafter(1, 0) and 1.0: the bins themselves,
    count by count and hit by hit, equal np.digitize's; labels -1 and 2^32 + pred are no hits; a second call adds to the first."""
    conf, pred, labels = ref.ece_case(n_bins)
    want = ref.bin_statistics(conf, pred, labels, n_bins)
    got = _ece(conf, pred, labels, n_bins)
    ref.assert_bins(got, want, conf.size, f"n_bins={n_bins}")
    ref.assert_bins(_ece(conf, pred, labels, n_bins, init=got), 2 * want, 2 * conf.size, f"n_bins={n_bins}, second call into the same bins")


@pytest.mark.parametrize("n", ref.ECE_SIZES)
def test_ece_sizes(n):
    """One thread, one block more or less, and the grid-stride second lap (n > 1024 * 256)."""
    conf, pred, labels = ref.ece_case(15, n)
    ref.assert_bins(_ece(conf, pred, labels, 15), ref.bin_statistics(conf, pred, labels, 15), n, f"n={n}")


def test_ece_nan_confidence():
    """np.digitize puts NaN behind the last edge: bin n_bins, whose sum no metric reads.  No other bin may see it."""
    conf, pred, labels = ref.ece_case(10, 300)
    conf = conf.copy()
    conf[[0, 17, 299]] = np.nan
    ref.assert_bins(_ece(conf, pred, labels, 10), ref.bin_statistics(conf, pred, labels, 10), 300, "NaN confidences")


# ---- clipmi_knn_dists -----------------------------------------------------------------------------------------------------------------------------------------
def _knn(q, refs, K):
    d_q, d_r = Guarded(q.numel(), torch.float32, q), Guarded(refs.numel(), torch.float32, refs)
    Nq, E = q.shape
    out = _twice(Nq * K, torch.float32, "clipmi_knn_dists", lambda p: L.clipmi_knn_dists(d_q.ptr, d_r.ptr, p, Nq, refs.shape[0], E, K, _stream())).reshape(Nq, K)
    _inputs_intact(d_q, d_r)
    return out


@pytest.mark.parametrize("E", ref.KNN_E)
@pytest.mark.parametrize("Nr", ref.KNN_NR + (ref.KNN_DEEP[0],))
def test_knn_lattice(Nr, E):
    """Integer coordinates, neighbours at perfect-square distances, every placement of tests/tail_ref.py::knn_lattice (one lane's list at full
    depth, one per lane, the ragged last tile, indices 63 / 64 / Nr - 1, duplicated rows with their multiplicity), Nq on both sides of 8, K = 1,
    5, 16 and Nr: the nearest fp32 value or its neighbour."""
    cases = [c for c in ref.KNN_GRID if c[0] == Nr and c[3] == E]
    if Nr == ref.KNN_DEEP[0] and E != ref.KNN_DEEP[3]:
        cases = [(Nr, 9, 16, E, "one_lane")]
    assert cases
    for case in cases:
        q, refs, want = ref.knn_lattice(*case)
        ref.check_knn_lattice(_knn(q, refs, case[2]), want, f"kNN {case}")


def test_knn_random():
    q, refs = ref.knn_random()
    want, tol = ref.knn(q, refs, 16)
    got = _knn(q, refs, 16)
    _note("knn", ref.worst_ratio(got, want, tol))
    _assert_within(got, want, tol, "clipmi_knn_dists [query, k]")


def test_knn_nan_reference_row():
    """A reference row of NaN (a zero-norm image after normalisation) is never a neighbour: the output of the same call without the row."""
    q, refs = ref.knn_random()
    for at in (7, 64, refs.shape[0]):
        poisoned = torch.cat([refs[:at], torch.full((1, refs.shape[1]), float("nan")), refs[at:]])
        for K in (1, 5, 16):
            _assert_bits(_knn(q, poisoned, K), _knn(q, refs, K), f"kNN with a NaN row at {at}, K={K} [query, k]")


def test_knn_val_set_with_identical_rows(ops):
    """get_val_image_knn_dists drops ONE zero (the row itself): a set with two identical rows keeps the other, its row starts with 0.0."""
    from clip_calibration_amd import proximity as prox
    _, refs = ref.knn_random(Nr=70, E=64)
    x = refs.numpy().copy()
    x[66] = x[3]
    got = prox.get_val_image_knn_dists(x, 5)
    assert got.shape == (70, 5) and got[3, 0] == 0.0 and got[66, 0] == 0.0 and (np.delete(got[:, 0], [3, 66]) > 0).all()
    want, tol = ref.knn(torch.from_numpy(x), torch.from_numpy(x), 6)
    _assert_within(torch.from_numpy(got), want[:, 1:], tol[:, 1:], "get_val_image_knn_dists [row, k]")
