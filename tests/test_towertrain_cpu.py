"""tests/towertrain_ref.py on the CPU, in the manner of tests/test_text_ref_cpu.py.  The case table covers what it claims to cover; an
fp32 emulation of the training forward, with the device's fp16 rounding points, stays inside every derived stage bound on every case and
on both variants of its tower; the bounds are not slack: every mutant of towertrain_ref.MUTANTS, applied to the one stage it changes,
leaves the bound of that stage on every case it can change (and the number of cases it changes is asserted, so that none passes because
nothing exercises it); and the emulation of the backward is the same function as float64 autograd through the oracle.  No GPU."""
import functools

import pytest
import torch

import coopfit_ref as cref
import towertrain_ref as ref
from oracle import clip_oracle as orc
from test_coopfit_cpu import RESTATEMENT_RTOL

BOTH = [ref.on_tower(c, t) for c in ref.CASES for t in (c.tower, c.tower + "-pass")]


@functools.lru_cache(maxsize=None)
def emulated(c):
    """(stash, features, layout, stages) of a case: computed once, left unchanged."""
    inp = ref.case_input(c)
    stash, feats, lay = ref.emulate_forward(c, inp)
    return stash, feats, lay, ref.forward_stages(c.tower, c.C, lay.L, stash, lay)


# ---------------------------------------------------------------------------------------------------------------------- the case table
def test_case_table_covers_what_the_drivers_branch_on():
    cs = ref.CASES
    L = [ref.live_rows(c) for c in cs]
    assert {c.C for c in cs} == {2, 3, 37}
    assert {1, 4, 16} <= {c.n_ctx for c in cs} and any(c.n_ctx == l - 1 for c, l in zip(cs, L))
    assert {8, 16, 24, 77} <= set(L)
    assert {c.dtype for c in cs} == {ref.F16, ref.F32} and {c.ctx for c in cs} == {"shared", "class", None}
    assert {c.tower for c in cs} == {"tiny", "tiny3"}
    far = [c for c in cs if c.far]
    assert far and all(int(ref.case_input(c)["eot"][-1]) == ref.live_rows(c) - 1 for c in far)
    big = [c for c, l in zip(cs, L) if c.C * l * 4 * ref.geometry(c.tower).transformer_width > ref.STATS_GRID]
    assert big and all(c.tower == "tiny" for c in big)
    for a, b in ref.UNCUT_PAIRS:
        assert a._replace(seq_rows=0) == b and ref.live_rows(a) < ref.live_rows(b) == 77
        ia, ib = ref.case_input(a), ref.case_input(b)
        assert torch.equal(ia["ctx"], ib["ctx"]) and torch.equal(ia["eot"], ib["eot"]) and torch.equal(ia["d_out"], ib["d_out"])
        assert torch.equal(ia["prompts"][:, :ref.live_rows(a)], ib["prompts"][:, :ref.live_rows(a)])
    for c in cs:
        inp = ref.case_input(c)
        assert 0 <= int(inp["eot"].min()) and int(inp["eot"].max()) < ref.live_rows(c)
        if c.dtype == ref.F32:                                  # fp32 prompts and the context are not fp16 numbers: a detour through fp16 shows
            live = inp["prompts"][:, :ref.live_rows(c)]
            assert (live.half().float() != live).float().mean() > 0.9
        if c.ctx:
            assert (inp["ctx"].half().float() != inp["ctx"]).float().mean() > 0.9


def test_pass_through_towers_differ_in_the_two_weights_only():
    for t in ("tiny", "tiny3"):
        a, b = ref.state_dict(t), ref.state_dict(t + "-pass")
        for k in a:
            if k.endswith(ref.PASS_THROUGH) and k.startswith("transformer."):
                assert a[k].any() and not b[k].any(), k
            else:
                assert torch.equal(a[k], b[k]), k


def test_stash_layout_is_the_header_s():
    lay = ref.StashLayout(3, 16, 128, 2)
    M = 48
    assert lay.x_bytes == M * 128 * 4 and lay.qkv_off == 5 * lay.x_bytes and lay.h_off == lay.qkv_off + 2 * M * 128 * 6
    assert lay.idx_off == lay.h_off + 2 * M * 128 * 8 and lay.bytes == lay.idx_off + 256
    odd = ref.StashLayout(1, 1, 64, 3)                          # 256 / 384 / 512 bytes: the second is rounded up
    assert (odd.x_bytes, odd.qkv_bytes, odd.h_bytes) == (256, 512, 512) and odd.bytes == 7 * 256 + 3 * 512 + 3 * 512 + 256
    buf = torch.arange(lay.bytes, dtype=torch.int64).to(torch.uint8)
    assert lay.x(buf, 4).shape == (M, 128) and lay.qkv(buf, 1).shape == (M, 384) and lay.h(buf, 1).shape == (M, 512) and lay.idx(buf).shape == (3,)
    assert lay.idx(buf).data_ptr() - buf.data_ptr() == lay.idx_off and lay.h(buf, 1).data_ptr() - buf.data_ptr() == lay.h_off + lay.h_bytes


# ------------------------------------------------------------------------------------------------------ the emulation inside the bounds
@pytest.mark.parametrize("c", BOTH, ids=ref.case_id)
def test_forward_emulation_stays_inside_every_stage_bound(c):
    _, feats, _, stages = emulated(c)
    worst = {name: ref.worst_ratio(feats if got is None else got, want, tol) for name, got, want, tol in stages}
    print(f"\ntowertrain-cpu: {ref.case_id(c)} worst error / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# --------------------------------------------------------------------------------------------------------------------------- the mutants
def _leaves(got, want, tol):
    return ref.worst_ratio(got, want, tol) > 1.0


def _mutant_outcome(c, mutant):
    """(changed, caught): does the mutant change any bit of what the case's mutated stage writes, and does every layer's (the one)
    mutated stage then leave its bound.  The mutated stage is fed the clean emulation's own stash, as the device's stages are judged."""
    inp = ref.case_input(c)
    stash, feats, lay, stages = emulated(c)
    sd, H = ref.state_dict(c.tower), ref.geometry(c.tower).transformer_heads
    by_name = {name: (got, want, tol) for name, got, want, tol in stages}
    if mutant in ("ctx_prev_class", "ctx_shift", "pos_stride"):
        clean, bad = ref.embed(c, inp), ref.embed(c, inp, mutant)
        assert torch.equal(clean, lay.x(stash, 0))
        changed = not torch.equal(clean.view(torch.int32), bad.view(torch.int32))
        return changed, changed                                # the embedding is compared bit for bit: its bound is zero
    if mutant == "eot_late":
        bad = ref.emu_features(sd, lay.x(stash, 2 * lay.layers), lay.idx(stash), mutant)
        _, want, tol = by_name["features"]
        return not torch.equal(bad, feats), _leaves(bad, want, tol)
    changed, caught = [], []
    for i in range(lay.layers):
        x_in, x_mid = lay.x(stash, 2 * i), lay.x(stash, 2 * i + 1)
        if mutant == "no_b_out":
            name, bad = f"x_mid({i})", ref.emu_x_mid(sd, i, lay.qkv(stash, i), x_in, c.C, lay.L, H, mutant)
        elif mutant == "ln2_from_x_in":
            name, bad = f"h({i})", ref.emu_h(sd, i, x_mid, x_in, mutant)
        else:
            assert mutant == "resid_x_in"
            name, bad = f"x_in({i + 1})", ref.emu_x_out(sd, i, lay.h(stash, i), x_mid, x_in, mutant)
        got, want, tol = by_name[name]
        changed.append(not torch.equal(bad, got))
        caught.append(_leaves(bad, want, tol))
    return any(changed), all(caught)


# cases (of 20: the 10 of the table on both variants of their tower) a mutant can change: a per-class context exists in 3 cases, a context
# in 9, and the flat row index modulo the context length is the token index itself on the three uncut cases; the rest change everywhere
MUTANT_CASES = {"resid_x_in": 20, "no_b_out": 20, "ctx_prev_class": 6, "ctx_shift": 18, "pos_stride": 14, "ln2_from_x_in": 20, "eot_late": 20}


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_mutant_leaves_the_bounds_wherever_it_changes_anything(mutant):
    n = 0
    for c in BOTH:
        changed, caught = _mutant_outcome(c, mutant)
        n += changed
        assert caught or not changed, f"{mutant} stays inside the bounds on {ref.case_id(c)}"
    assert n == MUTANT_CASES[mutant], (mutant, n)


# ------------------------------------------------------------------------------------------------------------------------- the backward
def _oracle_ctx_grad(c, inp):
    """d sum(text * d_out) / d ctx by float64 autograd through the oracle's prompt builder and text encoder."""
    sd = ref.state_dict(c.tower)
    ids = cref.prompt_ids(ref.base(c.tower), c.C, c.n_ctx, 0, c.far)
    sd_c, ids_c = cref.cut(sd, ids)
    ctx = inp["ctx"].double().clone().requires_grad_(True)
    text = orc.text_encoder(sd_c, orc.coop_prompts(sd_c, ids_c, ctx, torch.float64), ids_c, torch.float64)
    (text * inp["d_out"].double()).sum().backward()
    return ctx.grad.detach()


@pytest.mark.parametrize("c", [ref.CASES[0], ref.CASES[3], ref.CASES[8]], ids=ref.case_id)
def test_backward_emulation_is_autograd_s_function(c):
    """With every rounding switched off (hi = lo = float64) the emulation's sequence of steps gives autograd's context gradient within the
    bound tests/test_coopfit_cpu.py holds the restatement to; with the device's formats it stays within fp16's reach of it."""
    assert c.dtype == ref.F16 and c.ctx                          # the prompts are the token embeddings themselves
    inp = ref.case_input(c)
    L = ref.live_rows(c)
    want = _oracle_ctx_grad(c, inp)
    st = ref.Stash64(c.tower, ref.embed(c, inp), ref.eot_rows(c, inp), c.C, L)
    g = ref.emulate_backward(c.tower, st, inp["d_out"], hi=torch.float64, lo=torch.float64)
    assert cref.rel_fro(cref.ctx_gradient(g, c.C, L, c.n_ctx, c.ctx == "class"), want) <= RESTATEMENT_RTOL
    assert cref.rel_fro(g, ref.backward64(c.tower, st, inp["d_out"])) <= 1e-12          # and the restatement's whole stream
    stash, _, lay, _ = emulated(c)
    g32 = ref.emulate_backward(c.tower, ref.StashView(stash, lay), inp["d_out"])
    err = cref.rel_fro(cref.ctx_gradient(g32, c.C, L, c.n_ctx, c.ctx == "class"), want)
    print(f"\ntowertrain-cpu: {ref.case_id(c)} fp32 / fp16 emulation against float64 autograd, context rows: {err:.3e}")
    assert g32.dtype == torch.float32 and err <= 64 * ref.U16     # fp16 operands (u16 each) through 8 GEMMs per block, far from any mutant's 1


def test_operand_counts_and_special_values():
    d = ref.special_d_out(3, 64)
    n, z, s, m = ref.operand_counts(d.half())
    h = d.half()
    assert n == 192 and m == 0x7BFF and z >= 2 and s >= 2
    bits = ref.half_bits(h[0, :6]).tolist()
    assert bits == [0x0000, 0x8000, 0x0001, 0x03FF, 0x0400, 0x7BFF]
    assert ref.operand_counts(h[0, :6]) == (6, 2, 2, 0x7BFF)      # 2^-14 is no subnormal
    assert ref.operand_counts(torch.tensor([1.0, float("nan")]).half())[3] == 0x7FFF
    assert ref.operand_counts(torch.tensor([1.0, float("-inf")]).half())[3] == 0x7C00
