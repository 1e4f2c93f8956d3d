"""tests/attention_ref.py held to account without a GPU: the float64 reference against torch's own attention, the three conditions on the
per-element tolerance (a CPU emulation of the documented arithmetic stays inside it; it is nowhere looser than the scalar bounds of
tests/test_gpu_ops.py; three wrong emulations leave it), the constructed inputs (score gap, exactness, sensitivity), the case list against
the dispatch of launch_attention, and the argument contract of clipmi_attention and clipmi_attention_cls."""
import ctypes
import functools

import pytest
import torch

import attention_ref as ref
from clip_calibration_amd import _lib


@functools.lru_cache(maxsize=None)
def _random(case):
    qkv, order, seqs = ref.random_batch(*case)
    S, L, H = seqs.shape[0], case.L, case.H
    flat = seqs.reshape(S * L, -1)
    want, tol = ref.attention(flat, S, L, H, case.causal)
    return flat, want, tol


def _peaked(which):
    qkv, n, l, h = ref.peaked_qkv(which)
    return (qkv, n, l, h) + ref.attention(qkv, n, l, h, False)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,H,causal", [(2, 50, 2, False), (2, 77, 3, True), (1, 1, 1, True), (1, 197, 1, False), (3, 9, 2, True)])
def test_reference_matches_torch_sdpa(N, L, H, causal):
    qkv = ref.random_batch(N, L, H, causal, N)[0]
    q, k, v = (t.reshape(N, L, H, 64).transpose(1, 2) for t in qkv.double().reshape(N, L, 3, 64 * H).unbind(2))
    want = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=causal).transpose(1, 2).reshape(N, L, 64 * H)
    got, tol = ref.attention(qkv, N, L, H, causal)
    assert (got - want).abs().max() < 1e-12
    assert (tol > 0).all() and torch.isfinite(tol).all()
    cls, _ = ref.attention_cls(qkv, N, L, H)
    if not causal:
        assert (cls - want[:, 0]).abs().max() < 1e-12


def test_reference_matches_multi_head_attention_forward():
    """The module the reference tower calls (clip/model.py:181-183), with identity projections."""
    N, L, H, D = 2, 33, 2, 128
    qkv = ref.random_batch(N, L, H, True, N)[0]
    x = qkv.double().reshape(N, L, 3, D).transpose(0, 1)          # [L, N, 3, D]
    mask = torch.full((L, L), float("-inf"), dtype=torch.float64).triu_(1)
    eye = torch.eye(D, dtype=torch.float64)
    want, _ = torch.nn.functional.multi_head_attention_forward(
        x[:, :, 0], x[:, :, 1], x[:, :, 2], D, H, None, None, None, None, False, 0.0, eye, torch.zeros(D, dtype=torch.float64), need_weights=False,
        attn_mask=mask, use_separate_proj_weight=True, q_proj_weight=eye, k_proj_weight=eye, v_proj_weight=eye)
    got, _ = ref.attention(qkv, N, L, H, True)
    assert (got - want.transpose(0, 1)).abs().max() < 1e-12


# ---- condition 1: the emulation stays inside the tolerance ----------------------------------------------------------------------
EMULATION_WORST = {}


@pytest.mark.parametrize("case", ref.RANDOM_CASES, ids=str)
def test_emulation_inside_tolerance(case):
    flat, want, tol = _random(case)
    got = ref.emulate(flat, flat.shape[0] // case.L, case.L, case.H, case.causal)
    r = ref.worst_ratio(got, want, tol)
    for o in ref.option_settings(case.L, case.causal):
        k = ref.kernel_for(case.L, case.causal, o)
        EMULATION_WORST[k] = max(EMULATION_WORST.get(k, 0.0), r)
    print(f"{case}: emulation worst |err| / tol = {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("which", ref.PEAKED)
def test_emulation_inside_tolerance_peaked(which):
    qkv, n, l, h, want, tol = _peaked(which)
    r = ref.worst_ratio(ref.emulate(qkv, n, l, h, False), want, tol)
    print(f"peaked {which}: emulation worst |err| / tol = {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("case", ref.CLS_CASES, ids=str)
def test_cls_emulation_inside_its_smaller_tolerance(case):
    N, L, H = case
    qkv = ref.random_batch(N, L, H, False, N)[0]
    want, tol = ref.attention_cls(qkv, N, L, H)
    full, tol_full = ref.attention(qkv, N, L, H, False, rows=1)
    # no P terms: smaller wherever a second key gives them a size; with one key both are the output rounding plus a few fp32 roundings
    assert torch.equal(want, full[:, 0]) and (tol <= 1.001 * tol_full[:, 0]).all() and (L == 1 or (tol < tol_full[:, 0]).all())
    r = ref.worst_ratio(ref.emulate(qkv, N, L, H, False, rows=1, p_fp16=False)[:, 0], want, tol)
    print(f"cls {case}: emulation worst |err| / tol = {r:.3f}")
    assert r <= 1.0


# ---- condition 2: against the scalar of tests/test_gpu_ops.py ----------------------------------------------------------------------
def _legacy_tol(shape):
    n, l, h, causal = shape
    qkv = ref.legacy_qkv(n, l, h)
    if n > 4:      # of a many-sequence batch the sequences the old test compared with its reference: the first three and the last
        qkv = torch.cat([qkv[:3 * l], qkv[(n - 1) * l:]])
        n = 4
    return ref.attention(qkv, n, l, h, causal)[1]


@pytest.mark.parametrize("shape,bound", ref.LEGACY, ids=str)
def test_tolerance_against_the_scalar_bound(shape, bound):
    """Same shape, seed and scale as tests/test_gpu_ops.py.  The derived bound is 9e-4 in the median (1.7e-3 at 2816 tokens) against the scalar 4e-3, and nowhere looser
    than it in 32 of the 44 cases and on both peaked inputs.  It cannot be everywhere: where a row's weight sits on |v| of four standard deviations
    (6 at scale 1.5), the fp16 roundings of P and of the output alone allow 2^-11 (|o| + spread) = 4.0e-3 .. 4.8e-3 -- the scalar was never a
    bound there, only not reached.  That is the case at a few elements in a hundred thousand of (2, 197, 12), (3, 77, 8, causal), (40, 197, 12),
    (2, 300, 3), (1, 576, 2), (70, 257, 16), (40, 577, 16), (300, 577, 1), (1000, 16, 8, causal), (7, 31, 3, causal): max 4.0e-3 .. 4.8e-3.  At 2560
    and 2816 tokens the worst-case fp32 accumulation term, 2 (n + updates) 2^-24 A, adds up to 1.4e-3: max 6.7e-3 and 6.0e-3, 0.03 % of the
    elements above the scalar.  Held here: at most 1 element in 10^4 above the scalar up to 577 tokens (1 in 100 beyond), none above 1.7 x."""
    tol = _legacy_tol(shape)
    over = float((tol > bound).double().mean())
    print(f"{shape}: max tol {tol.max():.3e} (scalar {bound:.0e}), median {tol.median():.3e}, share above the scalar {over:.2e}")
    assert tol.median() <= bound / 2
    assert tol.max() <= (bound if shape not in ref.LEGACY_OVER else 1.7 * bound)
    assert over <= (0.0 if shape not in ref.LEGACY_OVER else 1e-4 if shape[1] <= 577 else 1e-2)


@pytest.mark.parametrize("which", ref.PEAKED)
def test_tolerance_not_looser_than_the_scalar_bound_peaked(which):
    tol = _peaked(which)[5]
    print(f"peaked {which}: max tol {tol.max():.3e} (scalar {ref.PEAKED_BOUND:.0e})")
    assert tol.max() <= ref.PEAKED_BOUND


# ---- condition 3: wrong kernels leave the tolerance -------------------------------------------------------------------------------
def _applies(wrong, case, S):
    if wrong == "drop_last":
        return case.L >= 2
    if wrong == "admit_next":
        return case.causal and case.L >= 2
    return not case.causal and S >= 2          # next_seq: under the causal mask key L is dead for every query


@pytest.mark.parametrize("wrong", ref.WRONG)
@pytest.mark.parametrize("case", ref.RANDOM_CASES, ids=str)
def test_wrong_emulations_leave_the_tolerance(case, wrong):
    flat, want, tol = _random(case)
    S = flat.shape[0] // case.L
    if not _applies(wrong, case, S):
        return
    r = ref.worst_ratio(ref.emulate(flat, S, case.L, case.H, case.causal, wrong=wrong), want, tol)
    print(f"{case} {wrong}: worst |err| / tol = {r:.1f}")
    assert r > 1.0


def test_every_wrong_emulation_applies_somewhere():
    for wrong in ref.WRONG:
        assert sum(_applies(wrong, c, c.distinct) for c in ref.RANDOM_CASES) >= 20


# ---- the constructed inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [1, 2, 33, 200, 577, 2817])
def test_selection_construction(L, causal):
    N, H = (2, 2) if L <= 577 else (1, 1)
    for kind in ref.SELECT_KINDS[causal]:
        qkv, want, pi = ref.selection_batch(N, L, H, kind)
        x = qkv.double().reshape(N, L, 3, H, 64)
        v16 = qkv.reshape(N, L, 3, H, 64)[:, :, 2]
        e = v16.view(torch.int16).to(torch.int32) >> 10 & 31
        assert ((e >= 1) & (e <= 30)).all()                                            # normal, non-zero, finite
        for n in range(N):
            for h in range(H):
                raw = x[n, :, 0, h] @ x[n, :, 1, h].t()
                assert (raw == raw.round()).all() and raw.abs().max() < 2 ** 24          # exact integers in fp32
                s = (raw / 8).masked_fill(~ref._allowed(L, L, causal), float("-inf"))
                tgt = s.gather(1, pi[n, h][:, None])
                rest = s.scatter(1, pi[n, h][:, None], float("-inf")).amax(dim=1, keepdim=True)
                assert (tgt - rest >= 64).all(), (kind, L)
                if causal:
                    assert (pi[n, h] <= torch.arange(L)).all()
                if kind == "decoy" and L > 1:
                    i = torch.arange(L - 1)
                    assert (raw[i, i + 1] > raw[i, pi[n, h][i]]).all()                   # the masked neighbour leads
        got = ref.emulate(qkv, N, L, H, causal)
        assert torch.equal(got.reshape(want.shape).view(torch.int16), want.view(torch.int16)), (kind, L)
        if kind == "decoy" and L > 1:
            off = ref.emulate(qkv, N, L, H, True, wrong="admit_next").reshape(N, L, -1)
            assert (off[:, :L - 1].view(torch.int16) != want.reshape(N, L, -1)[:, :L - 1].view(torch.int16)).any(dim=2).all()
        if kind == "diag" and L > 1:
            off = ref.emulate(qkv, N, L, H, True, wrong="drop_last").reshape(N, L, -1)
            assert (off[:, 1:].view(torch.int16) != want.reshape(N, L, -1)[:, 1:].view(torch.int16)).any(dim=2).all()


def test_selection_class_row_target():
    """pi(0) anywhere: the fp32 class-row emulation returns the V row exactly (other probabilities below 2e-28)."""
    for L, pi0 in [(1, 0), (9, 8), (197, 100), (577, 576)]:
        qkv, want, pi = ref.selection_batch(2, L, 2, "perm", pi0=pi0)
        assert (pi[:, :, 0] == pi0).all() and math_exp_gap() < 2e-28
        got = ref.emulate(qkv, 2, L, 2, False, rows=1, p_fp16=False)[:, 0]
        assert torch.equal(got.view(torch.int16), want.reshape(2, L, -1)[:, 0].view(torch.int16))


def math_exp_gap():
    import math
    return math.exp(-64.0)


@pytest.mark.parametrize("causal", [False, True])
def test_uniform_construction_and_sensitivity(causal):
    """The emulation meets the allowance at every length; at the longest length, dropping or double-counting ANY single key moves some
    output of the rows that see it by more than the allowance."""
    for L in (1, 2, 33, 200, 577):
        N, H = ref.constructed_shape(L)
        qkv, exact = ref.uniform_batch(N, L, H, causal)
        assert (ref.fp16_steps_from_nearest(ref.emulate(qkv, N, L, H, causal), exact) <= ref.UNIFORM_STEPS).all()
    L = max(ref.LENGTHS)
    qkv, exact = ref.uniform_batch(1, L, 1, causal)
    assert (ref.fp16_steps_from_nearest(ref.emulate(qkv, 1, L, 1, causal), exact) <= ref.UNIFORM_STEPS).all()
    v = qkv.double().reshape(L, 3, 64)[:, 2]
    # the last row sees every key under either mask: n = L keys, sum = exact * L
    total, row = v.sum(dim=0), exact[L - 1]
    assert torch.equal(total / L, row)
    for sign, n in ((-1.0, L - 1), (1.0, L + 1)):
        moved = (total[None, :] + sign * v) / n                                                    # [key, d]
        steps = ref.fp16_steps_from_nearest(moved.half(), row[None, :].expand(L, 64).contiguous())
        assert (steps.amax(dim=1) > ref.UNIFORM_STEPS + 1).all()      # beyond the allowance even after its own rounding


# ---- the case list against the dispatch ---------------------------------------------------------------------------------------------
def test_case_list_reaches_every_kernel_and_both_sides_of_every_seam():
    assert tuple(sorted({c.L for c in ref.SWEEP})) == ref.LENGTHS
    reached = {}
    for c in ref.SWEEP:
        assert (c.L, not c.causal) in {(d.L, d.causal) for d in ref.SWEEP}                          # every length under both masks
        for o in ref.option_settings(c.L, c.causal):
            reached.setdefault(ref.kernel_for(c.L, c.causal, o), set()).add(c.causal)
    assert set(reached) == set(ref.KERNELS)
    for k in ref.KERNELS:
        want = {True} if k in ref.CAUSAL_ONLY else {False} if k in ref.NONCAUSAL_ONLY else {True, False}
        assert reached[k] == want, (k, reached[k])
    for s in ref.SEAMS + (ref.RING_MAX,):
        assert s in ref.LENGTHS and s + 1 in ref.LENGTHS
        assert any(ref.kernel_for(s, c) != ref.kernel_for(s + 1, c) for c in (False, True)), s
    # the option settings are exactly those that change the kernel
    for L in ref.LENGTHS:
        for causal in (False, True):
            ks = [ref.kernel_for(L, causal, o) for o in ref.option_settings(L, causal)]
            assert len(set(ks)) == len(ks), (L, causal, ks)
            alls = {ref.kernel_for(L, causal, {"attn_small": a, "attn_loader": b, "attn_ring": c}) for a in (0, 1) for b in (0, 1, 2) for c in (0, 1)}
            assert alls == set(ks), (L, causal)
    assert {c.H for c in ref.RANDOM_CASES} >= set(ref.HEADS)
    assert min(c.N * c.H for c in ref.RANDOM_CASES) == 1 and max(c.N * c.H for c in ref.RANDOM_CASES) > 4 * 256 * 4
    assert set(ref.ISOLATION) == set(ref.KERNELS)
    for k, (L, causal, o) in ref.ISOLATION.items():
        assert ref.kernel_for(L, causal, o) == k
    assert {(N * H) % 4 for N, L, H in ref.CLS_CASES} == {0, 1, 2, 3}
    assert {L for N, L, H in ref.CLS_CASES} == set(ref.CLS_LENGTHS) and {H for N, L, H in ref.CLS_CASES} == {1, 12, 16}


def test_random_batch_repeats_a_few_sequences_in_shuffled_order():
    for c in ref.MANY:
        qkv, order, seqs = ref.random_batch(*c)
        assert set(order) == set(range(c.distinct)) and len(order) == c.N and order != sorted(order)
        b = qkv.reshape(c.N, c.L, -1)
        assert all(torch.equal(b[i], seqs[s]) for i, s in list(enumerate(order))[:: max(1, c.N // 16)])


# ---- the argument contract, no GPU ----------------------------------------------------------------------------------------------------
def _entries():
    L = _lib.lib
    return [("clipmi_attention", lambda q, o, N, Ls, H: L.clipmi_attention(q, o, N, Ls, H, 0, None)),
            ("clipmi_attention causal", lambda q, o, N, Ls, H: L.clipmi_attention(q, o, N, Ls, H, 1, None)),
            ("clipmi_attention_cls", lambda q, o, N, Ls, H: L.clipmi_attention_cls(q, o, N, Ls, H, None))]


@pytest.mark.parametrize("name,call", _entries(), ids=[e[0] for e in _entries()])
def test_attention_entries_validate_arguments_without_a_gpu(name, call):
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    assert call(None, q, 1, 8, 1) == _lib.ERR_ARG and "null" in _lib.last_error()
    assert call(p, None, 1, 8, 1) == _lib.ERR_ARG
    for N, L, H in [(-1, 8, 1), (1, 0, 1), (1, -3, 1), (1, 8, 0), (1, 8, -2), (1 << 30, 8, 2), (1 << 20, 8, 1 << 11)]:
        assert call(p, q, N, L, H) == _lib.ERR_SHAPE, (N, L, H)
    assert call(ctypes.c_void_p(4096 + 8), q, 1, 8, 1) == _lib.ERR_ARG and "unaligned" in _lib.last_error()
    assert call(ctypes.c_void_p(4096 + 2), q, 1, 8, 1) == _lib.ERR_ARG
    assert call(p, ctypes.c_void_p(8192 + 2), 1, 8, 1) == _lib.ERR_ARG
    assert call(p, ctypes.c_void_p(8192 + 4), 1, 8, 1) == _lib.ERR_ARG
    # N == 0 is OK and touches nothing: no launch (there is no device here to launch on), not even a look at the other arguments' values
    assert call(p, q, 0, 8, 1) == _lib.OK
    buf = (ctypes.c_uint16 * 64)(*([0x7C01] * 64))
    assert call(ctypes.addressof(buf), ctypes.addressof(buf), 0, 8, 1) == _lib.OK and all(b == 0x7C01 for b in buf)


def test_class_row_output_needs_16_byte_alignment():
    """include/clipmi.h: clipmi_attention_cls stores 16 bytes per lane (both pointers 16-byte aligned); clipmi_attention's rows need 8."""
    p = ctypes.c_void_p(4096)
    assert _lib.lib.clipmi_attention_cls(p, ctypes.c_void_p(8192 + 8), 1, 8, 1, None) == _lib.ERR_ARG


# ======================================================================================================================= the backward
# clipmi_attention_backward and clipmi_attention_backward_full: the reference against autograd, the emulation inside the tolerance at every
# random and peaked case the GPU test runs, every mutation of WRONG_BACKWARD outside it (or breaking an exact claim), and the exact claims of
# the constructed inputs on the emulation, before anything is asked of the device.
BACKWARD_EMULATION_WORST = {}


@functools.lru_cache(maxsize=None)
def _backward(case):
    _, _, _, sq, sd = ref.backward_batch(case)
    return (sq, sd) + ref.attention_backward(sq, sd, case.distinct, case.L, case.H, case.causal)


def _bkind(case):
    return "flat" if case.scale < 1.0 else "peaked"


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("N,L,H", [(1, 1, 1), (2, 17, 2), (3, 33, 1), (1, 80, 2)])
def test_backward_reference_is_the_gradient_of_the_forward_reference(N, L, H, causal):
    qkv = ref.random_batch(N, L, H, causal, N)[0].double().requires_grad_()
    g = torch.randn(N, L, 64 * H, generator=torch.Generator().manual_seed(L), dtype=torch.float64)
    q, k, v = (t.reshape(N, L, H, 64).transpose(1, 2) for t in qkv.reshape(N, L, 3, 64 * H).unbind(2))
    out = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=causal).transpose(1, 2).reshape(N, L, 64 * H)
    out.backward(g)
    want, tol = ref.attention_backward(qkv.detach(), g, N, L, H, causal)
    assert (want - qkv.grad).abs().max() < 1e-12
    assert (tol > 0).all() and torch.isfinite(tol).all()
    flat = ref.attention_backward(qkv.detach(), g, N, L, H, causal, fp32_terms=False)[1]
    assert (flat <= tol).all()


@pytest.mark.parametrize("case", ref.BACKWARD_RANDOM + ref.BACKWARD_PEAKED, ids=str)
def test_backward_emulation_inside_tolerance(case):
    """The condition that keeps the tolerance honest: worst |err| / tol of the unmutated emulation <= 1, at every case the device is held to."""
    sq, sd, want, tol = _backward(case)
    got = ref.emulate_backward(sq, sd, case.distinct, case.L, case.H, case.causal)
    assert torch.isfinite(got.float()).all()          # nothing overflows fp16: dS, dq at d_out 2^10
    r = ref.worst_ratio(got, want, tol)
    key = ("causal" if case.causal else "full") + " " + _bkind(case)
    BACKWARD_EMULATION_WORST[key] = max(BACKWARD_EMULATION_WORST.get(key, 0.0), r)
    print(f"attention-backward-parity: {tuple(case)}: emulation worst |err| / tol = {r:.3f}")
    assert r <= 1.0


def test_backward_subnormal_and_large_cases_are_what_they_say():
    """d_out 2^-10: most of dS is subnormal in fp16 (or flushed); d_out 2^10: dS reaches past 2^5; late: the rows that see the last key tile peak there."""
    late = {}
    for case in ref.BACKWARD_PEAKED:
        sq, sd, _, _ = _backward(case)
        S, L, H, D = case.distinct, case.L, case.H, 64 * case.H
        x, g = sq.double().reshape(S, L, 3, H, 64), sd.double().reshape(S, L, H, 64)
        s = torch.einsum("nqhd,nkhd->nhqk", x[:, :, 0], x[:, :, 1]) / 8
        s = s.masked_fill(~ref._allowed(L, L, case.causal), float("-inf"))
        p = torch.softmax(s, dim=-1)
        dp = torch.einsum("nqhd,nkhd->nhqk", g, x[:, :, 2])
        ds = p * (dp - (dp * p).sum(-1, keepdim=True))
        if case.dout == "2^-10" and L >= 17:
            assert (ds.abs() < 2.0 ** -14).double().mean() > 0.5
        if case.dout == "2^10" and L >= 17:
            assert ds.abs().max() > 2.0 ** 5
        if case.late and L >= 17:
            rows = torch.arange(L) >= (L - 1) // 16 * 16 if case.causal else torch.ones(L, dtype=torch.bool)
            hit = (s.argmax(-1)[..., rows] >= (L - 1) // 16 * 16).double()
            late[case.causal] = late.get(case.causal, []) + [hit.flatten()]
    for causal in (True, False):
        assert torch.cat(late[causal]).mean() > 0.9


@pytest.mark.parametrize("wrong", ref.WRONG_BACKWARD)
@pytest.mark.parametrize("case", [c for c in ref.BACKWARD_RANDOM + ref.BACKWARD_PEAKED if c.H <= 2], ids=str)
def test_wrong_backward_emulations_leave_the_tolerance(case, wrong):
    if not ref.wrong_backward_applies(wrong, case.distinct, case.L, case.causal):
        return
    sq, sd, want, tol = _backward(case)
    r = ref.worst_ratio(ref.emulate_backward(sq, sd, case.distinct, case.L, case.H, case.causal, wrong=wrong), want, tol)
    print(f"{tuple(case)} {wrong}: worst |err| / tol = {r:.1f}")
    assert r > 1.0


def test_every_wrong_backward_emulation_applies_somewhere():
    cases = [c for c in ref.BACKWARD_RANDOM + ref.BACKWARD_PEAKED if c.H <= 2]
    for wrong in ref.WRONG_BACKWARD:
        for causal in ((True,) if wrong == "admit_next" else (False,) if wrong == "stale_stats" else (True, False)):
            assert sum(ref.wrong_backward_applies(wrong, c.distinct, c.L, c.causal) for c in cases if c.causal == causal) >= 10, (wrong, causal)


def _zero(t):
    return bool((t.float() == 0).all())          # values: -0 passes


# which exact claim of the selection input every mutation breaks (dk_unscaled: none -- dk is zero with or without the 1 / 8; the tolerance
# catches it at every random case with two keys or more)
SELECTION_CATCHES = {"drop_last": ("last", "diag"), "admit_next": ("decoy",), "next_seq": ("perm", "first", "below"),
                     "no_rowsum": ("perm", "last", "diag", "below"), "stale_stats": ("perm", "last"), "swap_pair": ("perm", "diag", "below")}


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_backward_selection_construction_and_sensitivity(causal):
    """On the fp32 emulation, at every length of the GPU test: dq == 0 and dk == 0 in every element, dv the exact answer bit for bit; every
    mutation listed in SELECTION_CATCHES breaks one of the three at the kinds listed, wherever it applies."""
    N, H = ref.BACKWARD_CONSTRUCTED_SHAPE
    D = 64 * H
    caught = set()
    for L in ref.BACKWARD_LENGTHS[causal]:
        for kind in ref.SELECT_KINDS[causal]:
            qkv, do, dv, pi = ref.selection_backward_batch(N, L, H, kind)
            x = qkv.double().reshape(N, L, 3, H, 64)
            dp = torch.einsum("nqhd,nkhd->nhqk", do.double().reshape(N, L, H, 64), x[:, :, 2])
            assert dp.abs().max() < 2.0 ** 25
            if kind != "perm":
                assert (dp == dp.round()).all() and (x[:, :, 2] == x[:, :, 2].round()).all()
            else:
                srt = pi.sort(dim=-1).values
                assert (srt == torch.arange(L)).all()
                e = do.view(torch.int16).to(torch.int32) >> 10 & 31
                assert e.min() == 1 and (e.max() == 30 or L < 8)                       # fp16's whole exponent range
            got = ref.emulate_backward(qkv, do, N, L, H, causal)
            assert _zero(got[:, :D]) and _zero(got[:, D:2 * D]), (kind, L)
            assert torch.equal(got[:, 2 * D:].contiguous().view(torch.int16), dv.view(torch.int16)), (kind, L)
            for wrong, kinds in SELECTION_CATCHES.items():
                if kind in kinds and ref.wrong_backward_applies(wrong, N, L, causal):
                    off = ref.emulate_backward(qkv, do, N, L, H, causal, wrong=wrong)
                    broke = not (_zero(off[:, :D]) and _zero(off[:, D:2 * D]) and torch.equal(off[:, 2 * D:].float(), dv.float()))
                    assert broke, (wrong, kind, L)
                    caught.add(wrong)
    want = set(SELECTION_CATCHES) - ({"stale_stats"} if causal else {"admit_next"})
    assert caught == want


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_backward_uniform_construction_and_sensitivity(causal):
    """The emulation: dk == 0, dv within the uniform allowance, dq within the general tolerance, at every length.  At the longest length,
    dropping or double-counting any single (query, key) pair moves some dv element of that key beyond the allowance."""
    N, H = ref.BACKWARD_CONSTRUCTED_SHAPE
    D = 64 * H
    for L in ref.BACKWARD_LENGTHS[causal]:
        qkv, do, dv, dv_tol = ref.uniform_backward_batch(N, L, H, causal)
        got = ref.emulate_backward(qkv, do, N, L, H, causal)
        want, tol = ref.attention_backward(qkv, do, N, L, H, causal)
        assert _zero(got[:, D:2 * D])
        assert ((got[:, 2 * D:].double() - dv).abs() <= dv_tol).all(), L
        weight = (dv_tol - ref.U16 * dv.abs() - 2.0 ** -25) * 2.0 ** 20                                 # sum_q P16 |d_out|
        assert ((dv - want[:, 2 * D:]).abs() <= ref.U16 * weight + 1e-12).all()                        # the two references: fp16(1 / n) against 1 / n
        assert ((got[:, :D].double() - want[:, :D]).abs() <= tol[:, :D]).all(), L
    # the longest length is the last of the loop: one pair (q, key) more or less moves dv[key, d] by p16[q] |d_out[q, d]|
    ok = ref._allowed(L, L, causal)
    p16 = (1.0 / ok.sum(dim=1).float()).half().double()
    step = p16[:, None] * do.double().reshape(N, L, D)[0].abs()                                       # [q, d]
    moved = (step[:, None, :] / dv_tol.reshape(N, L, D)[0][None, :, :]).amax(dim=-1)                  # [q, key]: the best column
    assert (moved[ok] > 2.5).all()                                                                    # beyond the allowance after its own rounding


def test_backward_case_lists_cover_the_issue():
    T, F = ref.BACKWARD_LENGTHS[True], ref.BACKWARD_LENGTHS[False]
    assert T == (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 77, 79, 80)
    assert F == (1, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 96, 97, 112, 113, 197, 205, 207, 208, 209, 223, 224)
    for causal in (True, False):
        for cases in (ref.BACKWARD_RANDOM, ref.BACKWARD_PEAKED):
            assert {c.L for c in cases if c.causal == causal} == set(ref.BACKWARD_LENGTHS[causal])
        flat = [c for c in ref.BACKWARD_RANDOM if c.causal == causal]
        assert {c.H for c in flat} == {1, 2, 8, 12} and {c.N for c in flat} == {1, 3, 37}
        assert max(c.N * c.H for c in flat) > 256
        assert set(ref.BACKWARD_SEAMS[causal]) <= set(ref.BACKWARD_LENGTHS[causal]) and max(ref.BACKWARD_SEAMS[causal]) == ref.AB_MAX_L[causal]
        assert set(ref.BACKWARD_ISOLATION[causal]) <= set(ref.BACKWARD_LENGTHS[causal])
        peaked = [c for c in ref.BACKWARD_PEAKED if c.causal == causal]
        assert {c.scale for c in peaked} == {1.5, 3.0} and {c.dout for c in peaked} == set(ref.DOUT_SCALES) and any(c.late for c in peaked)
    assert all(c.distinct < c.N for c in ref.BACKWARD_RANDOM if c.N >= 3)             # a copy of a sequence in every batch of three or more


def test_backward_entries_validate_arguments_without_a_gpu():
    p = ctypes.c_void_p(4096)
    for f, most in ((_lib.lib.clipmi_attention_backward, 80), (_lib.lib.clipmi_attention_backward_full, 224)):
        assert f(p, p, p, 1, most + 1, 1, None) == _lib.ERR_SHAPE
        for N, L, H in [(1, 0, 1), (-1, 8, 1), (1, 8, 0), (1 << 30, 8, 2)]:
            assert f(p, p, p, N, L, H, None) == _lib.ERR_SHAPE, (N, L, H)
        for a in ((None, p, p), (p, None, p), (p, p, None), (ctypes.c_void_p(4096 + 2), p, p), (p, ctypes.c_void_p(4096 + 8), p),
                  (p, p, ctypes.c_void_p(4096 + 4))):
            assert f(*a, 1, most, 1, None) == _lib.ERR_ARG
        assert f(None, None, None, 0, 8, 1, None) == _lib.OK
