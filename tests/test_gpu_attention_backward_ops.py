"""clipmi_attention_backward (causal, L <= 80) and clipmi_attention_backward_full (no mask, L <= 224) of csrc/attention.hip through the C ABI,
against the backward half of tests/attention_ref.py: random and peaked inputs within the per-element tolerance the float64 reference returns
(tests/test_attention_ref_cpu.py holds a CPU emulation of the kernels' rounding points to it, and shows that seven wrong variants leave it),
and constructed inputs whose answer is exact -- selection (dq == 0, dk == 0, dv a sum of chosen d_out rows), uniform (q == 0: dk == 0, every
(query, key) pair counted once in dv), copies of a sequence (same bits), isolation among NaN and inf neighbours, a non-finite gradient that
stays visible and stays in its own item and head.  Every length on both sides of every seam the kernels have.  Every qkv and d_out ends right
in front of a NaN-patterned guard, every dqkv starts as NaN inside sentinel guards, every launch is made twice: same bits.
CLIPMI_ATTENTION_BACKWARD_TEST_REPORT=<file> collects the worst |err| / tol per kernel and kind, with the CPU emulation's beside it."""
import os

import pytest
import torch

import attention_ref as ref
from clip_calibration_amd import _lib
from test_gpu_glue_ops import PAD, Guarded, _assert_bits, _assert_within, _stream, _twice, ops  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu

L_ = _lib.lib
ENTRY = {True: L_.clipmi_attention_backward, False: L_.clipmi_attention_backward_full}
NAME = {True: "causal", False: "full"}
REPORT = os.environ.get("CLIPMI_ATTENTION_BACKWARD_TEST_REPORT")
WORST = {}          # (kernel, kind) -> [device worst ratio, emulation worst ratio, cases]
MASKS = pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT and WORST:
        with open(REPORT, "w") as f:
            f.write("attention-backward-parity: tests/test_gpu_attention_backward_ops.py on one MI355X: worst |error| / tolerance per kernel and kind of "
                    "input, the CPU emulation of tests/attention_ref.py at the same cases beside it\n")
            for (kernel, kind), (dev, emu, n) in sorted(WORST.items()):
                f.write(f"attention-backward-parity: {kernel} {kind}: device {dev:.3f} emulation {emu:.3f} ({n} cases)\n")


def _note(causal, kind, dev, emu):
    w = WORST.setdefault((NAME[causal], kind), [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], dev), max(w[1], emu), w[2] + 1


def _dev(t):
    """t on the device, its last row ending right in front of a NaN-patterned guard."""
    return Guarded(t.numel(), torch.float16, t)


def _input_guards_intact(d, what):
    b = d.buf.view(d.idt)
    assert bool((b[:PAD] == d.mark).all()) and bool((b[PAD + d.n:] == d.mark).all()), f"{what}: wrote around its input"


def _run(qkv, d_out, N, L, H, causal, what):
    """-> dqkv [N L, 3 * 64 H] (CPU) after two launches into NaN-filled, guarded buffers; the inputs' guards intact."""
    dq, dd = _dev(qkv), _dev(d_out)
    n = N * L * 3 * 64 * H
    out = _twice(n, torch.float16, what, lambda p: ENTRY[causal](dq.ptr, dd.ptr, p, N, L, H, _stream()),
                 init=torch.full((n,), float("nan"), dtype=torch.float16))
    _input_guards_intact(dq, what + " qkv")
    _input_guards_intact(dd, what + " d_out")
    return out.reshape(N * L, 3 * 64 * H)


# ---- random and peaked inputs, copies of a sequence ------------------------------------------------------------------------------------------
def _within(ops, case, kind):
    N, L, H, causal, S = case[:5]
    qkv, do, order, sq, sd = ref.backward_batch(case)
    want, tol = ref.attention_backward(sq, sd, S, L, H, causal)
    what = f"attention_backward {NAME[causal]} {tuple(case)}"
    got = _run(qkv, do, N, L, H, causal, what).reshape(N, L, -1)
    want, tol = want.reshape(S, L, -1), tol.reshape(S, L, -1)
    first, dev = {}, 0.0
    for i, s in enumerate(order):
        if s in first:
            _assert_bits(got[i], got[first[s]], f"{what}: sequence {i}, a copy of sequence {first[s]} [row, column]")
        else:
            first[s] = i
            dev = max(dev, ref.worst_ratio(got[i], want[s], tol[s]))
    emu = ref.worst_ratio(ref.emulate_backward(sq, sd, S, L, H, causal), want.reshape(S * L, -1), tol.reshape(S * L, -1)) if REPORT else 0.0
    print(f"attention-backward-parity: {NAME[causal]} {kind} {tuple(case)}: device worst |err| / tol = {dev:.3f}")
    _note(causal, kind, dev, emu)
    for s, i in first.items():
        _assert_within(got[i], want[s], tol[s], f"{what} sequence {i} [row, column of dq | dk | dv]")


@pytest.mark.parametrize("case", ref.BACKWARD_RANDOM, ids=str)
def test_attention_backward_random(ops, case):
    """Flat-softmax inputs (the trainers' operator tests' scale): every element within the tolerance, copies of a sequence the same bits."""
    _within(ops, case, "flat")


@pytest.mark.parametrize("case", ref.BACKWARD_PEAKED, ids=str)
def test_attention_backward_peaked(ops, case):
    """qkv at scale 1.5 and 3, rows whose maximum sits in the last key tile, d_out scaled by 2^10 and by 2^-10 (dS in fp16's subnormals)."""
    _within(ops, case, "peaked")


# ---- constructed inputs -----------------------------------------------------------------------------------------------------------------------
def _assert_zero(t, what):
    bad = torch.nonzero(~(t.float() == 0))          # values: -0 passes, NaN does not
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {t.numel()} elements are not zero, first at {bad[0].tolist()}: {t[tuple(bad[0].tolist())].item()}"


def _lengths(causal):
    return [pytest.param(causal, L, id=f"{NAME[causal]}-{L}") for L in ref.BACKWARD_LENGTHS[causal]]


@pytest.mark.parametrize("causal,L", _lengths(True) + _lengths(False))
def test_attention_backward_selection(ops, causal, L):
    """P16 exactly one-hot, dS16 exactly zero: dq == 0 and dk == 0 in every element, dv[j] the sum of the d_out rows that select key j -- bit
    for bit where one row does (perm, diag), value for value where several are summed.  A key counted twice, a mask off by one, two tiles
    swapped or statistics of another query tile change whole rows."""
    N, H = ref.BACKWARD_CONSTRUCTED_SHAPE
    D = 64 * H
    for kind in ref.SELECT_KINDS[causal]:
        qkv, do, dv, _ = ref.selection_backward_batch(N, L, H, kind)
        what = f"{NAME[causal]} selection {kind} L={L}"
        got = _run(qkv, do, N, L, H, causal, what)
        _assert_zero(got[:, :D], what + " dq [row, column]")
        _assert_zero(got[:, D:2 * D], what + " dk [row, column]")
        if kind in ("perm", "diag"):
            _assert_bits(got[:, 2 * D:], dv, what + " dv [row, column]")
        else:
            bad = torch.nonzero(~(got[:, 2 * D:].float() == dv.float()))
            assert bad.numel() == 0, f"{what} dv: {bad.shape[0]} elements differ, first at {bad[0].tolist()}"


@pytest.mark.parametrize("causal,L", _lengths(True) + _lengths(False))
def test_attention_backward_uniform(ops, causal, L):
    """q == 0: dk == 0 exactly, dv within the allowance derived in ``uniform_backward_batch`` (the output rounding, the fp32 sum), dq within
    the general tolerance."""
    N, H = ref.BACKWARD_CONSTRUCTED_SHAPE
    D = 64 * H
    qkv, do, dv, dv_tol = ref.uniform_backward_batch(N, L, H, causal)
    want, tol = ref.attention_backward(qkv, do, N, L, H, causal)
    what = f"{NAME[causal]} uniform L={L}"
    got = _run(qkv, do, N, L, H, causal, what)
    _assert_zero(got[:, D:2 * D], what + " dk [row, column]")
    _note(causal, "uniform dv", ref.worst_ratio(got[:, 2 * D:], dv, dv_tol),
          ref.worst_ratio(ref.emulate_backward(qkv, do, N, L, H, causal)[:, 2 * D:], dv, dv_tol) if REPORT else 0.0)
    _assert_within(got[:, 2 * D:], dv, dv_tol, what + " dv [row, column]")
    _assert_within(got[:, :D], want[:, :D], tol[:, :D], what + " dq [row, column]")


def _isolation():
    return [pytest.param(c, L, id=f"{NAME[c]}-{L}") for c in (True, False) for L in ref.BACKWARD_ISOLATION[c]]


@pytest.mark.parametrize("causal,L", _isolation())
def test_attention_backward_isolation(ops, causal, L):
    """A clean sequence in the middle, at the start and at the end of a batch of three whose other sequences are NaN and +-inf in qkv and in
    d_out: the bits of the same sequence alone."""
    H, N = 2, 3
    g = torch.Generator().manual_seed(L + 1000 * int(causal))
    qkv = (torch.randn(L, 3 * 64 * H, generator=g) * 1.5).half()
    do = (torch.randn(L, 64 * H, generator=g) * 0.5).half()
    alone = _run(qkv, do, 1, L, H, causal, f"{NAME[causal]} L={L} alone")
    assert torch.isfinite(alone.float()).all()
    for pos in (1, 0, 2):
        bq = ref.poison_like(torch.empty(N, L, 3 * 64 * H), g)
        bd = ref.poison_like(torch.empty(N, L, 64 * H), g)
        bq[pos], bd[pos] = qkv, do
        out = _run(bq.reshape(N * L, -1), bd.reshape(N * L, -1), N, L, H, causal, f"{NAME[causal]} L={L} among poisoned neighbours")
        _assert_bits(out.reshape(N, L, -1)[pos], alone, f"{NAME[causal]} L={L}: clean sequence at {pos} of {N} [row, column]")


@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("causal,L", _isolation())
def test_attention_backward_keeps_a_non_finite_gradient_visible(ops, causal, L, value):
    """One non-finite element in d_out at row r, head h of one item: that item's head has a non-finite element in dv, and in dq at row r (the
    loss scale's overflow check reads the gradient, not d_out); every other item and head keeps the bits of the clean run."""
    N, H = 3, 2
    D = 64 * H
    g = torch.Generator().manual_seed(L + 7)
    qkv = (torch.randn(N * L, 3 * D, generator=g) * 0.7).half()
    do = (torch.randn(N * L, D, generator=g) * 0.5).half()
    clean = _run(qkv, do, N, L, H, causal, f"{NAME[causal]} L={L} clean").reshape(N, L, 3, H, 64)
    assert torch.isfinite(clean.float()).all()
    n, h, r = 1, 1, L // 2
    out = _run(qkv, ref.poison_one(do, N, L, H, n, r, h, value), N, L, H, causal, f"{NAME[causal]} L={L} {value} in d_out").reshape(N, L, 3, H, 64)
    assert not torch.isfinite(out[n, :, 2, h].float()).all(), "dv of the item's head is finite"
    assert not torch.isfinite(out[n, r, 0, h].float()).all(), "dq of the row is finite"
    keep = torch.ones(N, H, dtype=torch.bool)
    keep[n, h] = False
    for i, j in torch.nonzero(keep).tolist():
        _assert_bits(out[i, :, :, j], clean[i, :, :, j], f"{NAME[causal]} L={L}: item {i} head {j} beside the non-finite one [row, dq | dk | dv, column]")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_causal_refusals(ops):
    """clipmi_attention_backward, as tests/test_gpu_attention_backward_full.py::test_refusals has it for the kernel without a mask; a refused
    call launches nothing."""
    g = Guarded(4096, torch.float16)
    p, s = g.ptr, _stream()
    f = L_.clipmi_attention_backward
    assert f(p, p, p, 1, 81, 1, s) == _lib.ERR_SHAPE
    assert f(p, p, p, 1, 0, 1, s) == _lib.ERR_SHAPE
    assert f(p, p, p, -1, 8, 1, s) == _lib.ERR_SHAPE
    assert f(p, p, p, 1, 8, 0, s) == _lib.ERR_SHAPE
    assert f(None, p, p, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p, None, p, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p, p, None, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p + 2, p, p, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p, p + 8, p, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p, p, p + 4, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(None, None, None, 0, 8, 1, s) == _lib.OK
    assert g.untouched()
