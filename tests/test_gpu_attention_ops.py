"""clipmi_attention (csrc/attention.hip: every kernel instantiation launch_attention can reach, both sides of every dispatch seam) and
clipmi_attention_cls (csrc/attention_cls.hip), one entry point at a time against tests/attention_ref.py: random inputs within the
per-element tolerance the float64 reference returns (tests/test_attention_ref_cpu.py holds a CPU emulation to the same tolerance), and
constructed inputs that need none -- selection (out of query q comes one chosen V row, bit for bit), uniform (the mean over the allowed keys,
to the nearest fp16 value or its neighbour), repeated sequences (every copy of a sequence: the same bits, every item of the walk under a
reference) and isolation (neighbours full of NaN and inf change no bit).  Every qkv lies inside a NaN-guarded allocation, every output
inside sentinel guards, every launch is made twice: same bits.  CLIPMI_ATTENTION_TEST_REPORT=<file> collects the worst |err| / tol per kernel."""
import json
import os

import pytest
import torch

import attention_ref as ref
from clip_calibration_amd import _lib
from test_gpu_glue_ops import PAD, Guarded, _assert_bits, _assert_within, _stream, _twice, ops  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu

L_ = _lib.lib
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("CLIPMI_ATTENTION_TEST_REPORT")
    if path and WORST:
        with open(path, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


def _note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)


def _dev(qkv):
    """qkv on the device, its last row ending right in front of a NaN-patterned guard."""
    return Guarded(qkv.numel(), torch.float16, qkv)


def _input_guards_intact(d, what):
    b = d.buf.view(d.idt)
    assert bool((b[:PAD] == d.mark).all()) and bool((b[PAD + d.n:] == d.mark).all()), f"{what}: wrote around its input"


def _run(ops, clipmi_option, opts, d, N, L, H, causal, what):
    for k, v in dict(ref.DEFAULTS, **opts).items():
        clipmi_option(k, v)
    out = _twice(N * L * 64 * H, torch.float16, what, lambda p: L_.clipmi_attention(d.ptr, p, N, L, H, int(causal), _stream()))
    _input_guards_intact(d, what)
    return out.reshape(N, L, 64 * H)


def _variants(ops, clipmi_option, qkv, N, L, H, causal, what):
    """Every option setting that changes the kernel at (L, causal) -> [(kernel, out)], with the header's bit-identity claims asserted."""
    d = _dev(qkv)
    outs = []
    for o in ref.option_settings(L, causal):
        k = ref.kernel_for(L, causal, o)
        outs.append((k, _run(ops, clipmi_option, o, d, N, L, H, causal, f"{what} {k}")))
    for k, out in outs[1:]:
        if ref.same_bits(outs[0][0], k):
            _assert_bits(out, outs[0][1], f"{what}: {k} against {outs[0][0]} [sequence, row, column]")
    return outs


# ---- random inputs, repeated sequences ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.RANDOM_CASES, ids=str)
def test_attention_random(ops, clipmi_option, case):
    """Within the per-element tolerance at EVERY sequence of the batch (the reference once per distinct sequence); copies of a sequence: same bits."""
    N, L, H, causal, S = case
    qkv, order, seqs = ref.random_batch(*case)
    want, tol = ref.attention(seqs.reshape(S * L, -1), S, L, H, causal)
    for k, out in _variants(ops, clipmi_option, qkv, N, L, H, causal, f"attention {tuple(case)}"):
        first = {}
        for i, s in enumerate(order):
            if s in first:
                _assert_bits(out[i], out[first[s]], f"{k}: sequence {i}, a copy of sequence {first[s]} [row, column]")
            else:
                first[s] = i
                _note(k, ref.worst_ratio(out[i], want[s], tol[s]))
                _assert_within(out[i], want[s], tol[s], f"{k} {tuple(case)} sequence {i} [row, column]")


@pytest.mark.parametrize("which", ref.PEAKED)
def test_attention_peaked(ops, clipmi_option, which):
    """The two peaked-row inputs of tests/test_gpu_ops.py (the running maximum moves late) under the derived tolerance."""
    qkv, N, L, H = ref.peaked_qkv(which)
    want, tol = ref.attention(qkv, N, L, H, False)
    for k, out in _variants(ops, clipmi_option, qkv, N, L, H, False, f"peaked {which}"):
        _note(k + " peaked", ref.worst_ratio(out, want, tol))
        _assert_within(out, want, tol, f"{k} peaked [sequence, row, column]")


# ---- constructed inputs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("L", ref.LENGTHS)
def test_attention_selection(ops, clipmi_option, L, causal):
    """out[q, :] == V[pi(q), :] bit for bit: a dropped or doubled key, a swapped V row or a mask that is off by one changes whole rows."""
    N, H = ref.constructed_shape(L)
    for kind in ref.SELECT_KINDS[causal]:
        qkv, want, _ = ref.selection_batch(N, L, H, kind)
        for k, out in _variants(ops, clipmi_option, qkv, N, L, H, causal, f"selection {kind} L={L}"):
            _assert_bits(out.reshape(N * L, -1), want, f"{k} selection {kind} L={L} [row, column]")


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("L", ref.LENGTHS)
def test_attention_uniform(ops, clipmi_option, L, causal):
    """q == 0: the mean of V over the allowed keys, the nearest fp16 value or its neighbour -- every key counted once."""
    N, H = ref.constructed_shape(L)
    qkv, exact = ref.uniform_batch(N, L, H, causal)
    for k, out in _variants(ops, clipmi_option, qkv, N, L, H, causal, f"uniform L={L}"):
        steps = ref.fp16_steps_from_nearest(out.reshape(N * L, -1), exact)
        bad = torch.nonzero(steps > ref.UNIFORM_STEPS)
        assert bad.numel() == 0, (f"{k} uniform L={L}: {bad.shape[0]} elements off, first at {bad[0].tolist()}: got "
                                  f"{out.reshape(N * L, -1)[tuple(bad[0].tolist())].item()}, exact {exact[tuple(bad[0].tolist())].item()}")


@pytest.mark.parametrize("kernel", ref.KERNELS)
def test_attention_isolation(ops, clipmi_option, kernel):
    """A clean sequence in the middle, at the start and at the end of a batch whose other sequences are NaN and +-inf: the bits of the same
    sequence alone.  (Rows behind a sequence's last are read as zeros through its own buffer descriptor, never as the neighbour's.)"""
    L, causal, opts = ref.ISOLATION[kernel]
    H, N = 2, 3
    assert ref.kernel_for(L, causal, opts) == kernel
    g = torch.Generator().manual_seed(L)
    clean = (torch.randn(L, 3 * 64 * H, generator=g) * 1.5).half()
    alone = _run(ops, clipmi_option, opts, _dev(clean), 1, L, H, causal, f"{kernel} alone")[0]
    assert torch.isfinite(alone.float()).all()
    for pos in (1, 0, 2):
        batch = ref.poison_like(torch.empty(N, L, 3 * 64 * H), g)
        batch[pos] = clean
        out = _run(ops, clipmi_option, opts, _dev(batch.reshape(N * L, -1)), N, L, H, causal, f"{kernel} among poisoned neighbours")
        _assert_bits(out[pos], alone, f"{kernel}: clean sequence at {pos} of {N} [row, column]")


# ---- clipmi_attention_cls ------------------------------------------------------------------------------------------------------------------
def _cls(d, N, L, H, what):
    """-> out [N, L, D] after two launches into sentinel-filled, guarded buffers: rows 1..L-1 of every sequence keep the sentinel."""
    out = _twice(N * L * 64 * H, torch.float16, what, lambda p: L_.clipmi_attention_cls(d.ptr, p, N, L, H, _stream())).reshape(N, L, 64 * H)
    _input_guards_intact(d, what)
    assert (out[:, 1:].view(torch.int16) == 0x7C01).all(), f"{what}: wrote a row other than row 0 of a sequence"
    return out


@pytest.mark.parametrize("case", ref.CLS_CASES, ids=str)
def test_attention_cls(ops, clipmi_option, case):
    N, L, H = case
    what = f"clipmi_attention_cls {case}"
    # random: its own (smaller) tolerance, and row 0 of clipmi_attention within the sum of the two
    qkv = ref.random_batch(N, L, H, False, N)[0]
    want, tol = ref.attention_cls(qkv, N, L, H)
    d = _dev(qkv)
    got = _cls(d, N, L, H, what)[:, 0]
    _note("cls", ref.worst_ratio(got, want, tol))
    _assert_within(got, want, tol, what + " [sequence, column]")
    full = _run(ops, clipmi_option, {}, d, N, L, H, False, "clipmi_attention")[:, 0]
    tol_full = ref.attention(qkv, N, L, H, False, rows=1)[1][:, 0]
    _assert_within(got, full.double(), tol + tol_full, what + " against row 0 of clipmi_attention [sequence, column]")
    # selection: pi(0) anywhere, and the last key
    for pi0 in (None, L - 1, L // 2):
        qkv, sel, _ = ref.selection_batch(N, L, H, "perm", pi0=pi0)
        _assert_bits(_cls(_dev(qkv), N, L, H, what + " selection")[:, 0], sel.reshape(N, L, -1)[:, 0], what + f" selection pi(0)={pi0} [sequence, column]")
    # uniform
    qkv, exact = ref.uniform_batch(N, L, H, False)
    steps = ref.fp16_steps_from_nearest(_cls(_dev(qkv), N, L, H, what + " uniform")[:, 0], exact.reshape(N, L, -1)[:, 0].contiguous())
    assert (steps <= ref.UNIFORM_STEPS).all(), what + " uniform"


@pytest.mark.parametrize("L,H", [(7, 1), (50, 12), (197, 12), (577, 16)])
def test_attention_cls_isolation(ops, L, H):
    g = torch.Generator().manual_seed(L + H)
    clean = (torch.randn(L, 3 * 64 * H, generator=g) * 1.5).half()
    alone = _cls(_dev(clean), 1, L, H, "cls alone")[0, 0]
    assert torch.isfinite(alone.float()).all()
    for pos in (1, 0, 2):
        batch = ref.poison_like(torch.empty(3, L, 3 * 64 * H), g)
        batch[pos] = clean
        out = _cls(_dev(batch.reshape(3 * L, -1)), 3, L, H, "cls among poisoned neighbours")
        _assert_bits(out[pos, 0], alone, f"cls: clean sequence at {pos} of 3 [column]")
