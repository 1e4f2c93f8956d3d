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
