"""clipmi_nearest_rows on the GPU (csrc/nearest.hip) through ``ops.nearest_rows`` and ``clip_calibration_amd.interpret``, held to the
float64 restatement of tests/nearest_ref.py.

Exact inputs (integer-valued fp32, entries in -8..8, E <= 512: every squared sum is an integer below 2^24, so fp32 is exact): indices equal
the stable argsort, distances equal np.sqrt(np.float32(sum)) bit for bit, with duplicated reference rows planted on both sides of the
tile / slice boundaries.  Rounded inputs (Gaussian): per-position criteria under the derived bound BOUND(E) = (E/2 + 4) * 2^-24, relative:
one rounding on each difference (2u on its square), one on each of the E accumulations of non-negative terms (E u), halved by the square
root, plus the root's own rounding (u), plus slack for second-order terms (2u).  Split independence, repeatability, NaN, module level."""
import itertools
import random

import numpy as np
import pytest
import torch

import nearest_ref as ref
from clip_calibration_amd import interpret

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def BOUND(E):
    return (E / 2 + 4) * U


@pytest.fixture(scope="module")
def ops():
    from clip_calibration_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _ops


def _run(ops, q, refs, k, splits=0):
    dist, idx = ops.nearest_rows(torch.from_numpy(q).cuda(), torch.from_numpy(refs).cuda(), k, splits)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int32 and dist.shape == idx.shape == (q.shape[0], k)
    return dist.cpu().numpy(), idx.cpu().numpy()


# ---- exact inputs ----------------------------------------------------------------------------------------------------------------------
NQ, NR, ES, KS, SPLITS = (1, 7, 8, 9, 17), ("K", 63, 64, 65, 129, 1000), (64, 128, 512), (1, 10, 16, 32), (0, 1, 2, 3, 7, "over")


def _exact_cases(n=40):
    """A few dozen cases of the cross product (K > Nr dropped), every value of every axis present: a seeded shuffle, first the cases that
    bring a value not seen yet, then the head of the rest."""
    full = [c for c in itertools.product(NQ, NR, ES, KS, SPLITS) if c[1] == "K" or c[3] <= c[1]]
    random.Random(0).shuffle(full)
    seen, picked, rest = set(), [], []
    for c in full:
        new = {(a, v) for a, v in enumerate(c)} - seen
        (picked if new else rest).append(c)
        seen |= new
    picked += rest[:n - len(picked)]
    for axis, values in enumerate((NQ, NR, ES, KS, SPLITS)):
        assert {c[axis] for c in picked} == set(values)
    return picked


def _exact_inputs(nq, nr, e, seed):
    """Integer-valued rows; the rows at both ends of every 64-row tile near the front, and the last row, repeat row 0, and half of the
    queries sit on or next to that row: ties inside a tile, across tiles and across slices, inside the top K."""
    rng = np.random.default_rng(seed)
    refs = rng.integers(-8, 9, (nr, e)).astype(np.float32)
    for r in (1, 62, 63, 64, 65, 127, 128, nr - 1):
        if 0 < r < nr:
            refs[r] = refs[0]
    if nr > 200:
        refs[190:200] = refs[130]                       # a second run of equal rows, not on a boundary
    q = rng.integers(-8, 9, (nq, e)).astype(np.float32)
    for i in range(0, nq, 2):
        q[i] = refs[0]
        if i:
            q[i, rng.integers(0, e, 3)] = rng.integers(-8, 9, 3)
    return q, refs


@pytest.mark.parametrize("nq,nr,e,k,splits", _exact_cases())
def test_exact_inputs(ops, nq, nr, e, k, splits):
    nr = k if nr == "K" else nr
    if splits == "over":
        splits = (nr + 63) // 64 + 3                    # more slices than 64-row tiles: some slices hold no row at all
    q, refs = _exact_inputs(nq, nr, e, seed=nq * 1009 + nr * 7 + e + k)
    want_d, want_i, sq = ref.nearest_rows(q, refs, k)
    assert sq.max() < 2 ** 24 and np.array_equal(sq, np.round(sq))
    if nr > 1:
        assert (np.diff(np.sort(sq, axis=1)[:, :k + 1], axis=1) == 0).any(), "the case holds no tie near the top"
    dist, idx = _run(ops, q, refs, k, splits)
    assert np.array_equal(idx, want_i)
    want32 = np.sqrt(np.take_along_axis(sq, want_i, axis=1).astype(np.float32))
    assert want32.dtype == np.float32 and np.array_equal(dist.view(np.uint32), want32.view(np.uint32))


# ---- rounded inputs --------------------------------------------------------------------------------------------------------------------
ROUNDED = {"small": (8, 1000, 512), "vocab": (16, 49408, 512)}


@pytest.fixture(scope="module")
def rounded():
    """Gaussian inputs and their float64 reference, computed once and left unchanged."""
    out = {}
    for name, (nq, nr, e) in ROUNDED.items():
        rng = np.random.default_rng(nr)
        refs = rng.standard_normal((nr, e), dtype=np.float32)
        refs[nr // 2] = refs[3]                                             # one exact duplicate
        q = rng.standard_normal((nq, e), dtype=np.float32)
        q[1] = refs[nr - 1] + np.float32(0.01) * rng.standard_normal(e, dtype=np.float32)   # a query with one very near row
        sq = ref.sq_dists(q, refs)
        out[name] = (q, refs, np.sqrt(sq), np.sqrt(np.sort(sq, axis=1)))
    return out


@pytest.mark.parametrize("name", sorted(ROUNDED))
def test_rounded_inputs(ops, rounded, name):
    q, refs, d64, sorted64 = rounded[name]
    k, e = 10, q.shape[1]
    dist, idx = _run(ops, q, refs, k)
    own = np.take_along_axis(d64, idx.astype(np.int64), axis=1)
    worst_own = np.abs(dist.astype(np.float64) - own) / own
    worst_pos = np.abs(own - sorted64[:, :k]) / sorted64[:, :k]
    print(f"{name}: max |dist - own| / own = {worst_own.max():.3e}, max |own - j-th smallest| / j-th = {worst_pos.max():.3e}, bound {BOUND(e):.3e}")
    for i in range(q.shape[0]):
        assert len(set(idx[i].tolist())) == k and idx[i].min() >= 0 and idx[i].max() < refs.shape[0]
        assert (np.diff(dist[i]) >= 0).all()
    assert (worst_own <= BOUND(e)).all()
    assert (worst_pos <= BOUND(e)).all()


@pytest.mark.parametrize("name", sorted(ROUNDED))
def test_split_independence_and_repeatability(ops, rounded, name):
    q, refs = rounded[name][:2]
    qd, rd = torch.from_numpy(q).cuda(), torch.from_numpy(refs).cuda()
    base_d, base_i = ops.nearest_rows(qd, rd, 10, 0)
    for splits in (0, 1, 2, 7, 100):
        d, i = ops.nearest_rows(qd, rd, 10, splits)
        assert torch.equal(d.view(torch.int32), base_d.view(torch.int32)) and torch.equal(i, base_i), splits
    # a pair's distance does not depend on the number of queries either: the first rows alone give the same bits
    d, i = ops.nearest_rows(qd[:3].contiguous(), rd, 10, 5)
    assert torch.equal(d.view(torch.int32), base_d[:3].view(torch.int32)) and torch.equal(i, base_i[:3])


# ---- NaN ------------------------------------------------------------------------------------------------------------------------------
def test_nan_rows_come_last(ops):
    """A NaN distance counts as +inf.  (K = Nr cannot be had at Nr = 65 under K <= 32: one case has K = Nr = 32 with one NaN row, which
    comes last; the other has Nr = 65 with more NaN rows than finite ones -- one of them alone in the second tile -- and K = 32, so the
    tail of the result is the NaN rows by index.)"""
    rng = np.random.default_rng(5)
    refs = rng.standard_normal((32, 64), dtype=np.float32)
    refs[11, 40] = np.nan
    q = rng.standard_normal((3, 64), dtype=np.float32)
    q[2, 0] = np.nan
    for splits in (0, 1, 2):
        dist, idx = _run(ops, q, refs, 32, splits)
        want_d, want_i, _ = ref.nearest_rows(q, refs, 32)
        assert np.array_equal(idx, want_i)
        assert (idx[:2, -1] == 11).all() and np.isposinf(dist[:2, -1]).all() and np.isfinite(dist[:2, :-1]).all()
        assert idx[2].tolist() == list(range(32)) and np.isposinf(dist[2]).all()          # a query row with a NaN: every row at +inf, by index
    refs = rng.standard_normal((65, 64), dtype=np.float32)
    bad = sorted(rng.choice(64, 39, replace=False).tolist() + [64])
    refs[bad, 7] = np.nan
    for splits in (0, 1, 2, 5):
        dist, idx = _run(ops, q, refs, 32, splits)
        want_d, want_i, _ = ref.nearest_rows(q, refs, 32)
        assert np.array_equal(idx, want_i)
        assert idx[0, 25:].tolist() == bad[:7] and np.isposinf(dist[:2, 25:]).all() and np.isfinite(dist[:2, :25]).all()
        assert idx[2].tolist() == list(range(32)) and np.isposinf(dist[2]).all()


# ---- module level ---------------------------------------------------------------------------------------------------------------------
class _Tok:
    def symbol(self, i):
        return f"w{int(i)}"


def _vocab(v=300, d=64, seed=3):
    rng = np.random.default_rng(seed)
    emb = rng.integers(-8, 9, (v, d)).astype(np.float32)
    emb[64] = emb[63]
    return emb


def test_nearest_words_generic_and_class_specific(ops):
    emb = _vocab()
    rng = np.random.default_rng(4)
    for shape in ((4, 64), (3, 4, 64)):
        ctx = rng.integers(-8, 9, shape).astype(np.float32)
        ctx.reshape(-1, 64)[1] = emb[63]                                                   # a tie at distance 0: token 63 before token 64
        _, want_i, sq = ref.nearest_rows(ctx.reshape(-1, 64), emb, 5)
        r = interpret.nearest_words(torch.from_numpy(ctx), torch.nn.Embedding.from_pretrained(torch.from_numpy(emb)), topk=5, tokenizer=_Tok())
        assert r.indices.is_cuda and r.indices.shape == r.distances.shape == shape[:-1] + (5,)
        got = r.indices.cpu().numpy()
        assert np.array_equal(got.reshape(-1, 5), want_i) and got.reshape(-1, 5)[1, :2].tolist() == [63, 64]
        assert np.array_equal(r.distances.cpu().numpy().reshape(-1, 5), np.sqrt(np.take_along_axis(sq, want_i, axis=1).astype(np.float32)))
        words = np.array(r.words)
        assert words.shape == got.shape and words.reshape(-1)[7] == f"w{got.reshape(-1)[7]}"
        report = interpret.format_report(r).splitlines()
        assert report[0] == "SHOWING RESULTS FOR CTX Vectors of Layer:  1" and (len(shape) == 3) == ("Class 0:" in report)
    assert interpret.nearest_words(torch.from_numpy(ctx), torch.from_numpy(emb).cuda(), topk=5).words is None
    with pytest.raises(ValueError):
        interpret.nearest_words(torch.zeros(4, 32), torch.from_numpy(emb))


def test_interpret_prompt_learner_on_a_maple_state_dict(ops, tmp_path):
    emb = _vocab()
    rng = np.random.default_rng(6)
    t = lambda *s: torch.from_numpy(rng.integers(-8, 9, s).astype(np.float32))
    sd = {"prompt_learner.compound_prompts_text.1": t(2, 64), "prompt_learner.proj.weight": t(96, 64), "prompt_learner.ctx": t(2, 64),
          "prompt_learner.compound_prompts_text.0": t(2, 64), "prompt_learner.token_prefix": t(3, 1, 64),
          "prompt_learner.compound_prompt_projections.0.weight": t(96, 64)}
    names = ["prompt_learner.ctx", "prompt_learner.compound_prompts_text.0", "prompt_learner.compound_prompts_text.1"]
    from clip_calibration_amd import checkpoint as ck
    path = ck.save_checkpoint(sd, str(tmp_path), "prompt_learner", 5)
    for source in (sd, {"state_dict": sd, "epoch": 5}, path):
        results = interpret.interpret_prompt_learner(source, torch.from_numpy(emb), topk=3, tokenizer=_Tok())
        assert [r.name for r in results] == names
        for r in results:
            _, want_i, _ = ref.nearest_rows(sd[r.name].numpy(), emb, 3)
            assert np.array_equal(r.indices.cpu().numpy(), want_i)
    assert interpret.format_report(results).count("SHOWING RESULTS FOR CTX Vectors of Layer:") == 3


def test_half_inputs(ops):
    """fp16 context and fp16 embedding: nearest_words converts (the reference's .float()), ops.nearest_rows refuses."""
    emb = _vocab()
    ctx = np.random.default_rng(8).integers(-8, 9, (4, 64)).astype(np.float32)
    _, want_i, _ = ref.nearest_rows(ctx, emb, 10)
    r = interpret.nearest_words(torch.from_numpy(ctx).half(), torch.from_numpy(emb).half().cuda(), topk=10)
    assert np.array_equal(r.indices.cpu().numpy(), want_i) and r.distances.dtype == torch.float32
    with pytest.raises(TypeError):
        ops.nearest_rows(torch.from_numpy(ctx).half().cuda(), torch.from_numpy(emb).cuda(), 10)
    with pytest.raises(TypeError):
        ops.nearest_rows(torch.from_numpy(ctx).cuda(), torch.from_numpy(emb).half().cuda(), 10)
    with pytest.raises(ValueError):
        ops.nearest_rows(torch.from_numpy(ctx).cuda(), torch.from_numpy(emb[:, :32].copy()).cuda(), 10)
