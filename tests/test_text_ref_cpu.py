"""tests/text_ref.py on the CPU.  The case tables reach what they claim to reach (every vocabulary row, the EOT positions 0 / 63 / 64 / L - 1 /
context - 1, every tie form, every clamp, every rows_out / cast instantiation); an fp32 emulation of the kernels' arithmetic -- one fp32
addition, an fp32 two-pass LayerNorm rounded to fp16, an fp32 matrix product -- stays inside the derived bounds on EVERY encoder case; and the
bounds are not slack: each mutant (wrong positional row, last-maximum tie break, clamp off by one, the neighbouring layer's deep prompt,
double rounding of the fp32 -> fp16 output) is applied to every case, and every prompt (every text_blocks case) whose data the mutant changes at
all leaves the bounds.  A mutant cannot change a case that never runs the mutated line (a tie break without a tie); the tests assert how many
cases each mutant does change.  No GPU."""
import numpy as np
import pytest
import torch

import text_ref as ref
from text_ref import F16, F32


def emulate_features(c, rows):
    """fp32 all the way: two-pass LayerNorm of the fp32 rows, rounded to fp16, times the fp16 projection, accumulated in fp32."""
    sd = ref.state_dict(c.tower)
    x = rows.numpy().astype(np.float32)
    D = np.float32(x.shape[1])
    mean = x.sum(axis=1, keepdims=True, dtype=np.float32) / D
    d = x - mean
    var = (d * d).sum(axis=1, keepdims=True, dtype=np.float32) / D
    rstd = (np.float32(1) / np.sqrt(var + np.float32(ref.EPS))).astype(np.float32)
    y = (d * rstd * sd["ln_final.weight"].numpy() + sd["ln_final.bias"].numpy()).astype(np.float16)
    W = sd["text_projection"].half().float().numpy()                 # [D, E]
    return torch.from_numpy(y.astype(np.float32) @ W).double()


def _outside(got, val, tol):
    """per prompt: does any element of its feature leave the bound?"""
    return ((got - val).abs() > tol).any(dim=1)


# ------------------------------------------------------------------------------------------------------------------------- the tables
def test_embeddings_are_not_fp16_numbers_and_every_row_has_its_own_mean():
    for name in ref.TOWERS:
        sd = ref.state_dict(name)
        for k in ("token_embedding.weight", "positional_embedding"):
            t = sd[k]
            assert t.dtype == F32 and (t.half().float() != t).float().mean() > 0.95, (name, k)
            m = t.double().mean(dim=1)
            assert (m.abs() > 0.45).all() and (m[1:] - m[:-1]).abs().min() > 0.01, (name, k)
            assert 0.018 < float((t.double() - m[:, None]).std()) < 0.022
        for i in range(ref.TOWERS[name].layers):
            for k in ref.PASS_THROUGH:
                assert not sd[f"transformer.resblocks.{i}.{k}"].any()


def test_address_cases_cover_every_table_row_and_the_lane_wrap():
    for name, t in ref.TOWERS.items():
        seen, at = set(), set()
        for c in ref.ENC_CASES:
            if c.entry == "ids" and c.tower == name and c.pattern.startswith("addr") and c.seq_rows == 0 and c.C == 37:
                _, plan = ref.enc_rows(c, ref.enc_input(c))
                seen |= {what for _, what, _ in plan}
                at |= {e for e, _, _ in plan}
        assert seen == {f"table[{r}]" for r in range(ref.VOCAB)}, name
        want = {0, t.ctx - 1} | ({63, 64} if t.ctx > 64 else set())
        assert want <= at, (name, at)


def test_tie_rows_are_what_they_say():
    rows = ref._tie_rows(77, 77)
    first = {what: int(np.argmax(r.numpy())) for r, what in rows}
    last = {what: int(76 - np.argmax(r.numpy()[::-1])) for r, what in rows}
    assert first["twice, same lane, strides 0 and 1"] == 5 and last["twice, same lane, strides 0 and 1"] == 69
    assert first["twice, the later lane first"] == 3 and first["three times, across strides"] == 2 and first["three times, stride 1"] == 64
    assert first["constant"] == 0 and last["constant"] == 76
    assert first["ids beyond 2^32: a 32-bit compare sees 3 and 1, a 32-bit table index wraps"] == 4
    assert sum(first[w] != last[w] for w in first) >= 9
    for r, _ in ref._tie_rows(77, 30):
        assert (r[30:] == ref.ID_SENTINEL).all() and int(np.argmax(r.numpy())) < 30


def test_case_tables_reach_every_kernel_form():
    b = ref.BLOCKS_CASES
    bound = lambda c: 0 < c.seq_rows < ref.TOWERS[c.tower].ctx  # noqa: E731
    for dt in (F16, F32):
        for stream in (ref.STREAM_F32, ref.STREAM_F16):
            assert any(bound(c) and c.dtype == dt and c.stream == stream for c in b)          # rows_out_kernel<fp32|fp16, fp16|fp32>
            assert any(not bound(c) and c.dtype == dt and c.stream == stream for c in b)      # cast_kernel / cast16_kernel, both outputs
    assert all(c.fold == 1 for c in b + ref.ENC_CASES if c.stream == ref.STREAM_F16)          # the fp16 stream needs the fold
    for table in (b, ref.ENC_CASES):
        hooks = {c.hook for c in table if c.hook}
        assert {n for n, _ in hooks} == {1, 2, 4} and {d for _, d in hooks} == {0, 1, 2}
        assert all(ref.TOWERS[c.tower].layers == 3 and 1 + c.hook[0] <= ref.live_rows(ref.TOWERS[c.tower].ctx, c.seq_rows) for c in table if c.hook)
        assert {ref.TOWERS[c.tower].width for c in table} == {64, 128, 320, 512} and {c.C for c in table} == {1, 3, 37}
        assert {c.fold for c in table} == {0, 1}
    for c in b + ref.ENC_CASES:
        t = ref.TOWERS[c.tower]
        assert (c.C * ref.live_rows(t.ctx, c.seq_rows) * (t.width // 4)) % 256 or c.C == 1 or t.width == 512 or t.ctx == 9, c
    rows = {c.seq_rows for c in ref.ENC_CASES} & {c.seq_rows for c in b}
    assert {0, 77, 100, -3, 1} <= rows and any(r % 4 for r in rows if 0 < r < 77)
    # an EOT inside the hook's tokens, and a clamp on either side
    assert any(c.hook and c.hook[1] and any("deep" in w for _, w, _ in ref.enc_rows(c, ref.enc_input(c))[1]) for c in ref.ENC_CASES)
    for c in ref.ENC_CASES:
        if c.pattern == "clamp":
            eot = ref.enc_input(c)["eot"]
            L = ref.live_rows(ref.TOWERS[c.tower].ctx, c.seq_rows)
            assert (eot < 0).any() and (eot >= L).any() and (eot == L).any()


def test_round_twice_differs_on_the_planted_ties():
    v = ref.tie_values(64)
    once, twice = v.half(), ref.round_twice(v)
    assert (once != twice).sum() == 32 and ((once.float() - v).abs() <= (twice.float() - v).abs()).all()
    r = torch.randn(4096, generator=torch.Generator().manual_seed(1))
    assert 0.08 < float((r.half() != ref.round_twice(r)).float().mean()) < 0.17      # an eighth of all numbers: within a quarter ulp of a tie, wrong side


# ------------------------------------------------------------------------------------------------------ emulation inside, mutants outside
@pytest.fixture(scope="module")
def enc_refs():
    """case -> (input, rows, value, tol): computed once."""
    out = {}
    for c in ref.ENC_CASES:
        inp = ref.enc_input(c)
        rows, _ = ref.enc_rows(c, inp)
        out[c] = (inp, rows) + ref.enc_features(c, rows)
    return out


def test_fp32_emulation_stays_inside_the_bounds(enc_refs):
    worst = 0.0
    for c, (inp, rows, val, tol) in enc_refs.items():
        got = emulate_features(c, rows)
        assert torch.isfinite(val).all() and torch.isfinite(tol).all() and (tol > 0).all(), ref.enc_case_id(c)
        ratio = float(((got - val).abs() / tol).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{ref.enc_case_id(c)}: error / tolerance = {ratio}"
        assert float((tol / val.abs().max()).max()) < 1e-2, ref.enc_case_id(c)             # the bound stays a small part of the feature
    print(f"\nemulation, worst error / tolerance over {len(enc_refs)} encoder cases: {worst:.3f}")


MUTANTS = {"wrong positional row (next)": dict(pos_shift=1), "wrong positional row (previous)": dict(pos_shift=-1),
           "last-maximum tie break": dict(last_max=True), "clamp off by one": dict(clamp_off=1),
           "deep prompt of the next layer": dict(deep_shift=1), "deep prompt of the previous layer": dict(deep_shift=-1)}
# cases a mutant must change at the least: every case adds a positional row somewhere; ties, clamps and deep prompts live in their own cases
MIN_CHANGED = {"wrong positional row (next)": len(ref.ENC_CASES), "wrong positional row (previous)": len(ref.ENC_CASES),
               "last-maximum tie break": 4, "clamp off by one": 8, "deep prompt of the next layer": 18, "deep prompt of the previous layer": 18}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_encoder_mutants_leave_the_bounds(enc_refs, mutant):
    changed_cases = 0
    for c, (inp, rows, val, tol) in enc_refs.items():
        bad, _ = ref.enc_rows(c, inp, **MUTANTS[mutant])
        changed = (bad != rows).any(dim=1)
        if not changed.any():
            continue
        changed_cases += 1
        out = _outside(emulate_features(c, bad), val, tol)
        assert out[changed].all(), f"{mutant} passes {ref.enc_case_id(c)}: prompts {torch.nonzero(changed & ~out).flatten().tolist()} stay inside the bounds"
        assert not out[~changed].any()
    assert changed_cases >= MIN_CHANGED[mutant], (mutant, changed_cases)


def test_fp16_detour_of_the_embedding_leaves_the_bounds(enc_refs):
    """What the not-fp16-representable embeddings are for: a row that passes through fp16 in the fp32 stream is caught."""
    n = 0
    for c, (inp, rows, val, tol) in enc_refs.items():
        if c.stream == ref.STREAM_F32 and c.dtype != F16:
            emb = torch.tensor(["deep" not in what for _, what, _ in ref.enc_rows(c, inp)[1]])      # (a deep prompt row is no embedding)
            out = _outside(emulate_features(c, rows.half().float()), val, tol)
            assert emb.any() and out[emb].all(), ref.enc_case_id(c)
            n += 1
    assert n >= 20


def test_blocks_references_and_their_mutants():
    """text_blocks is exact: the reference against plain indexing on the spot, and each mutant moves at least one element of every case that runs
    the mutated conversion or overwrite."""
    n_round = n_deep = 0
    for c in ref.BLOCKS_CASES:
        inp = ref.blocks_input(c)
        t = ref.TOWERS[c.tower]
        L = ref.live_rows(t.ctx, c.seq_rows)
        want = ref.blocks_expected(c, inp)
        assert want.dtype == c.dtype and torch.isfinite(want.float()).all() and not want[:, L:].any()
        assert (inp["x"][:, L:].float().abs() > 6e4).all()
        keep = torch.ones(L, dtype=torch.bool)
        if c.hook and c.hook[1]:
            keep[1:1 + c.hook[0]] = False
            src = inp["deep"][c.hook[1] - 1]
            got = want[:, 1:1 + c.hook[0]].float()
            assert torch.equal(got, (src.half().float() if c.dtype == F16 or c.stream == ref.STREAM_F16 else src).expand_as(got))
            for shift in (1, -1):
                bad = ref.blocks_expected(c, inp, deep_shift=shift)
                assert (bad.float() != want.float())[:, 1:1 + c.hook[0]].float().mean() > 0.99, ref.blocks_case_id(c)
            n_deep += 1
        x = inp["x"][:, :L][:, keep].float()
        exact = c.dtype == F16 or (c.dtype == F32 and c.stream == ref.STREAM_F32)
        assert torch.equal(want[:, :L][:, keep].float(), x if exact else x.half().float())
        if not exact:                                                 # an fp32 -> fp16 conversion happens: rounding twice shows
            bad = ref.blocks_expected(c, inp, double_round=True)
            assert (bad.float() != want.float()).any(), ref.blocks_case_id(c)
            n_round += 1
    assert n_round >= 15 and n_deep >= 30


# ---------------------------------------------------------------------------------------------------------------------------- case 6
def test_stale_statistics_partial_misses_the_live_reference_by_ten_tolerances():
    good, bad = ref.live_reference().double().numpy(), ref.live_reference(stale=True).double().numpy()
    assert np.isfinite(good).all() and np.isfinite(bad).all()
    mag = np.abs(bad - good).max() / (ref.LIVE_MAG_TOL * np.abs(good).max())
    cos = np.abs(ref.cos_table(bad, good) - ref.cos_table(good, good)).max() / ref.LIVE_COS_TOL
    print(f"\nstale second partial: magnitude miss {mag:.1f} x tolerance, cosine miss {cos:.1f} x tolerance")
    assert mag >= 10.0 and cos >= 10.0
    inp = ref.live_input()
    assert abs(float(inp["deep"].mean()) - ref.LIVE_OFFSET) < 0.01 and float(inp["prompts"].std()) < 0.03
