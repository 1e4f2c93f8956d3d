"""The class-sharded ProDA fit on one GPU (clip_calibration_amd/prodafit.py ``shard=``, csrc/proda_train.hip): every case runs the ranks of
a ``LocalGather`` -- the kernels and the phase code of the multi-process run, device copies in the all-gather's place.
  1. the new operators against tests/prodashard_ref.py on streams built to cancel     2. one rank is the unsharded path bit for bit, both
  loss scales     3. G = 2, 3 with uneven and one-class shards     4. parity with the float64 oracle     5. the trainer     6. RCCL on one rank
Cases from tests/prodafit_ref.py on the synthetic ``tiny`` / ``tiny3`` towers: n_ctx 4, P 8, Pb 4, batch 2."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import coopfit_ref as ref
import prodafit_ref as dref
import prodashard_ref as sref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import coopfit, ops, prodafit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

FACTOR = 2.0                # profiles/prodafit_parity.txt's criterion: at most twice the fp16 reference's own error
GRAD_SCALE = 256.0          # as tests/test_gpu_prodafit.py: the synthetic weights give gradients far larger than ViT-B/16's
DEFAULT = prodafit.DEFAULT_GRAD_SCALE
OVERFLOWS_AT = {"tiny": 2.0 ** 15, "tiny3": 2.0 ** 13}     # profiles/prodascaler_parity.txt: where the static path of the C = 3 case overflows fp16
RATES = [2e-3, 1e-3, 5e-4, 2e-3]
SGD = dict(momentum=0.9, dampening=0.0, nesterov=False, weight_decay=5e-4)
P, PB, N_CTX, B, SEED = 8, 4, 4, 2, 9
POS = dref.positions(P)
PARITY_LOG = os.environ.get("CLIPMI_PRODASHARD_PARITY")    # a file that receives the parity lines (profiles/prodashard_parity.txt is made so)


def say(line):
    print("prodashard-parity: " + line)
    if PARITY_LOG:
        with open(PARITY_LOG, "a") as f:
            f.write(line + "\n")


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def same(a, b):
    return a.shape == b.shape and a.cpu().contiguous().view(torch.int32).equal(b.cpu().contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def model(geom):
    return build_model(dict(ref.state_dict(geom)), {"trainer": "CoOp"}).cuda()


def case(geom, C):
    return dref.make_case(geom, C, N_CTX, P, PB, B)


# ------------------------------------------------------------------------------------------------------------------ 1. the operators
def cancelling_stream(C, Pb, n_nc, L, D, seed):
    """d_embed [C Pb + n_nc, L, D]: random rows, but for a large and a tiny value per CLASS in three columns, so that a wrong order of
    the classes shows (as tests/test_gpu_shardfit.py builds it); a no-class row carries a value that is lost unless it is added last."""
    rng = np.random.RandomState(seed)
    g = rng.standard_normal((C * Pb + n_nc, L, D)).astype(np.float32)
    cls = np.repeat(np.arange(C), Pb)
    big = np.float32(2.0 ** 24) * np.where(cls % 2 == 0, 1, -1).astype(np.float32)
    g[:C * Pb, :, 0] = big[:, None]
    g[:C * Pb, :, 1] = np.float32(1.0)
    g[:C * Pb, :, 2] = (big + cls.astype(np.float32))[:, None]
    g[C * Pb:, :, 0] = np.float32(1.0)
    return g


@pytest.mark.parametrize("C,Pb,n_ctx,D", [(1, 2, 2, 64), (3, 2, 4, 100), (6, 4, 2, 129)])
def test_proda_ctx_partial(C, Pb, n_ctx, D):
    """A rank's send block: D 64 and 100 take the 16-byte path, 129 the scalar one; more than one workgroup; names of 0, 1, 2 tokens so
    that the three positions read different rows."""
    n_own, L = 3, n_ctx + 5
    name_lens = np.arange(C) % 3
    sel = dref.ordered((1, 6) if Pb == 2 else (1, 6, 2, 5), POS)
    g = cancelling_stream(C, Pb, n_own, L, D, 1)
    want = sref.send_block(g, sel, POS, name_lens, n_own, n_ctx)
    assert want.dtype == np.float32 and np.isfinite(want).all()
    out = ops.proda_ctx_partial(torch.from_numpy(g).cuda().view(-1, D), i32(sel), i32(POS), i32(name_lens), n_own, n_ctx)
    assert out.shape == (Pb + n_own, n_ctx, D) and np.array_equal(out.cpu().numpy(), want)
    if C == 3:                                                           # the order shows: the classes reversed give other bits
        back = g[:C * Pb].reshape(C, Pb, L, D)[::-1].reshape(C * Pb, L, D)
        assert not np.array_equal(want[:Pb], sref.send_block(back, sel, POS, name_lens[::-1], 0, n_ctx)[:Pb])
    # written into the first rows of a padded send block: the padding behind them stays as it was
    block = torch.full((Pb + n_own + 2, n_ctx, D), float("nan")).cuda()
    ops.proda_ctx_partial(torch.from_numpy(g).cuda().view(-1, D), i32(sel), i32(POS), i32(name_lens), n_own, n_ctx, block[:Pb + n_own])
    assert np.array_equal(block[:Pb + n_own].cpu().numpy(), want) and torch.isnan(block[Pb + n_own:]).all()


def gathered_blocks(G, Pb, n_ctx, D, seed):
    """[G, Pb + ceil(P / G), n_ctx, D] fp32: the class sums cancel across the ranks, the padding slots are NaN."""
    rng = np.random.RandomState(seed)
    own = [hi - lo for lo, hi in sref.split(P, G)]
    blocks = rng.standard_normal((G, Pb + -(-P // G), n_ctx, D)).astype(np.float32)
    big = np.float32(2.0 ** 24) * np.where(np.arange(G) % 2 == 0, 1, -1).astype(np.float32)
    blocks[:, :Pb, :, 0] = big[:, None, None]                            # one large value per rank and, in the next, a tiny one beside it
    blocks[:, :Pb, :, 1] = (big + np.arange(G, dtype=np.float32))[:, None, None]
    blocks[:, :Pb, :, 3] = np.array([2.0 ** 24, 1.0, -2.0 ** 24], np.float32)[np.arange(G) % 3][:, None, None]   # 0 in rank order, 1 in the reverse
    blocks[:, Pb:, :, 0] = np.float32(1.0)                               # lost unless the no-class row is added last
    for r in range(G):
        blocks[r, Pb + own[r]:] = np.nan
    return blocks


@pytest.mark.parametrize("G,n_ctx,D", [(1, 4, 64), (3, 4, 100), (8, 2, 129)])
def test_proda_ctx_step_gathered(G, n_ctx, D):
    """P = 8: G = 8 is one no-class prompt per rank; n_ctx D = 258 is no multiple of 4 and takes the scalar path, the others the
    16-byte one.  The padding slots and a padded rank stride are NaN and must never reach the output -- static and scaled alike."""
    sel = dref.ordered((1, 6, 2, 5), POS)
    blocks = gathered_blocks(G, PB, n_ctx, D, 2)
    assert np.isnan(blocks).any() == (P % G != 0)
    inv = np.float32(1 / 256.0)
    want = sref.reduce_blocks(blocks, sel, P, inv)
    assert np.isfinite(want).all()
    d, s = torch.from_numpy(blocks).cuda().view(G, -1), i32(sel)
    assert np.array_equal(ops.proda_ctx_step_gathered(d, s, P, n_ctx, D, 256.0).cpu().numpy(), want)
    if G == 3:
        assert not np.array_equal(want, sref.reduce_blocks(np.concatenate([blocks[::-1, :PB], blocks[:, PB:]], 1), sel, P, inv))   # the order shows
    wide = torch.full((G, d.shape[1] + 5), float("nan")).cuda()          # 5 floats: the rows leave the 16-byte phase
    wide[:, :d.shape[1]] = d
    assert np.array_equal(ops.proda_ctx_step_gathered(wide, s, P, n_ctx, D, 256.0).cpu().numpy(), want)
    # the step: lr = 0.5 makes the product exact, so the fused multiply-add is one rounded fp32 subtraction
    ctx0 = np.random.RandomState(3).standard_normal((P, n_ctx, D)).astype(np.float32)
    lr = torch.tensor([0.5]).cuda()
    ctx = torch.from_numpy(ctx0).cuda()
    ops.proda_ctx_step_gathered(d, s, P, n_ctx, D, 256.0, ctx, None, lr, True, want_grad=False)
    assert np.array_equal(ctx.cpu().numpy(), ctx0 - np.float32(0.5) * want)
    # under the dynamic scale: the same gradient and step at the block's scale, a clean step counted; NaN in the padding trips no flag
    for src in (d, wide):
        state, ctx = ops.new_scaler_state(256.0, "cuda"), torch.from_numpy(ctx0).cuda()
        grad = ops.proda_ctx_reduce_gathered_scaled(src, s, P, n_ctx, D, state, ctx, None, lr, growth_interval=1000)
        assert np.array_equal(grad.cpu().numpy(), want) and np.array_equal(ctx.cpu().numpy(), ctx0 - np.float32(0.5) * want)
        assert ops.scaler_state_dict(state) == {"scale": 256.0, "growth_tracker": 1, "skipped_steps": 0, "applied_steps": 1, "found_inf": 0}
    # an inf in a slot that IS read -- the last rank's own no-class row -- skips the step and backs the scale off
    bad = d.clone().view(blocks.shape)
    bad[G - 1, PB, n_ctx - 1, D - 1] = float("inf")
    state, ctx = ops.new_scaler_state(256.0, "cuda"), torch.from_numpy(ctx0).cuda()
    ops.proda_ctx_reduce_gathered_scaled(bad.view(G, -1), s, P, n_ctx, D, state, ctx, None, lr, backoff_factor=0.25, want_grad=False)
    assert np.array_equal(ctx.cpu().numpy(), ctx0)
    assert ops.scaler_state_dict(state) == {"scale": 64.0, "growth_tracker": 0, "skipped_steps": 1, "applied_steps": 0, "found_inf": 1}


@pytest.mark.parametrize("C,G,E", [(5, 2, 70), (8, 8, 3), (13, 3, 129)])
def test_proda_shard_compact(C, G, E):
    """The gathered text features back in the unsharded order; the padding rows are NaN and must never be read."""
    Pb = 2
    full = np.random.RandomState(0).standard_normal((C * Pb + P, E)).astype(np.float32)
    gathered = sref.gathered_text(full, C, Pb, P, G)
    assert np.isnan(gathered).any() == (C % G != 0 or P % G != 0)
    out = ops.proda_shard_compact(torch.from_numpy(gathered).cuda(), C, Pb, P)
    assert np.array_equal(out.cpu().numpy(), full)
    with pytest.raises(ValueError, match="proda_shard_compact"):
        ops.proda_shard_compact(torch.zeros(G, gathered.shape[1] + 1, E).cuda(), C, Pb, P)


@pytest.mark.parametrize("D", [100, 129])
def test_one_rank_operators_are_proda_ctx_step(D):
    """The anchor at operator level: two steps with momentum, weight decay and Nesterov through both routes and both loss scales give
    the same gradient, context, buffer and scaler block."""
    C, L = 3, N_CTX + 5
    name_lens, sel = np.arange(C) % 3, dref.ordered((0, 3, 7, 5), POS)
    g = torch.from_numpy(cancelling_stream(C, PB, P, L, D, 3)).cuda().view(-1, D)
    s, pos, nl = i32(sel), i32(POS), i32(name_lens)
    ctx0 = torch.from_numpy(np.random.RandomState(4).standard_normal((P, N_CTX, D)).astype(np.float32)).cuda()
    lr, sgd = torch.tensor([0.01]).cuda(), (0.9, 0.0, 5e-4, True)
    ctx = [ctx0.clone() for _ in range(4)]
    buf = [torch.zeros_like(ctx0) for _ in range(4)]
    st = [ops.new_scaler_state(256.0, "cuda") for _ in range(2)]
    for first in (True, False):
        ga = ops.proda_ctx_step(g, s, pos, nl, N_CTX, 256.0, ctx[0], buf[0], lr, first, *sgd)
        part = ops.proda_ctx_partial(g, s, pos, nl, P, N_CTX)
        gb = ops.proda_ctx_step_gathered(part.view(1, -1), s, P, N_CTX, D, 256.0, ctx[1], buf[1], lr, first, *sgd)
        gc = ops.proda_ctx_step_scaled(g, s, pos, nl, N_CTX, st[0], ctx[2], buf[2], lr, 2.0, 0.5, 1000, *sgd)
        gd = ops.proda_ctx_reduce_gathered_scaled(part.view(1, -1), s, P, N_CTX, D, st[1], ctx[3], buf[3], lr, 2.0, 0.5, 1000, *sgd)
        assert same(ga, gb) and same(ga, gc) and same(ga, gd)
        for k in (1, 2, 3):
            assert same(ctx[0], ctx[k]) and same(buf[0], buf[k]), (first, k)
        assert torch.equal(st[0], st[1])
        g = g * 0.5
    assert not same(ctx[0], ctx0) and ops.scaler_state_dict(st[1])["applied_steps"] == 2


# -------------------------------------------------------------------------------------------------------------------------- the fit
@functools.lru_cache(maxsize=None)
def schedule():
    return prodafit.draw_selections(P, PB, 4, torch.Generator().manual_seed(SEED))


def states_of(geom, C, G, **kw):
    """The G shard states of one LocalGather, rank 0 first -- or, with G = None, the one unsharded state."""
    c = case(geom, C)
    kw = dict(dict(prompt_bs=PB, logit_scale=dref.LOGIT_SCALE, **SGD), **kw)
    make = lambda **more: prodafit.ProDAFitState(model(geom), c["ids"], c["ctx"], generator=torch.Generator().manual_seed(SEED), **kw, **more)
    if G is None:
        return [make()]
    local = coopfit.LocalGather(G)
    return [make(shard=coopfit.Shard(G, r, local)) for r in range(G)]


def run(geom, C, G, steps, first=0, own_schedule=False, driver=0, **kw):
    """`steps` steps on the case's one batch at RATES[first:] with the selections schedule()[first:] (``own_schedule``: the driving state
    draws them): (states, losses)."""
    c = case(geom, C)
    states = states_of(geom, C, G, **kw)
    x, y, lr, sels = c["feats"].cuda(), c["labels"].cuda(), torch.tensor(RATES, dtype=torch.float32).cuda(), i32(schedule())
    losses = [states[driver].step(x, y, lr[k:k + 1], sel=None if own_schedule else sels[k], want_loss=True) for k in range(first, first + steps)]
    assert all(s.steps == steps for s in states)
    return states, torch.cat(losses).cpu()


def blocks_agree(states):
    """Every rank holds rank 0's context, buffer and -- under the dynamic scale -- scaler block."""
    for s in states[1:]:
        assert same(s.ctx, states[0].ctx) and same(s.buf, states[0].buf)
        if s.dynamic:
            assert torch.equal(s._scaler.block, states[0]._scaler.block)


# ------------------------------------------------------------------------------------------------- 2. one rank: the unsharded bits
@pytest.mark.parametrize("geom", ["tiny", "tiny3"])
def test_one_rank_is_the_unsharded_fit_bit_for_bit(geom):
    """Static and dynamic routes, given selections and the state's own: three steps leave the unsharded state's context, momentum
    buffer, losses and scaler block."""
    start = case(geom, 3)["ctx"]
    for kw in (dict(grad_scale=GRAD_SCALE), dict(grad_scale="dynamic", scaler={"init_scale": DEFAULT, "growth_interval": 1000})):
        for own in (False, True):
            (plain,), want = run(geom, 3, None, 3, own_schedule=own, **kw)
            (one,), hist = run(geom, 3, 1, 3, own_schedule=own, **kw)
            assert same(one.ctx, plain.ctx) and same(one.buf, plain.buf) and same(hist, want), (kw, own)
            assert torch.isfinite(one.ctx).all() and all(not same(one.ctx[p].cpu(), start[p]) for p in range(P))
            if one.dynamic:                                              # a run that never overflows: the static bits at that scale, too
                assert torch.equal(one._scaler.block, plain._scaler.block)
                assert one.scaler_state() == {"scale": DEFAULT, "growth_tracker": 3, "skipped_steps": 0, "applied_steps": 3, "found_inf": 0}
                (static,), hist_s = run(geom, 3, 1, 3, own_schedule=own, grad_scale=DEFAULT)
                assert same(one.ctx, static.ctx) and same(one.buf, static.buf) and same(hist, hist_s)
    x, y = case(geom, 3)["feats"].cuda(), case(geom, 3)["labels"].cuda()
    with pytest.raises(ValueError, match=r"shard has no one-call step \(one_call=True\)"):
        one.step(x, y, 1e-3, one_call=True)
    with pytest.raises(ValueError, match="shard has no validation"):
        one.validate(x, y, 0)
    assert one.steps == 3


@pytest.mark.parametrize("geom", ["tiny", "tiny3"])
def test_one_rank_gradient_and_fit_context_are_the_unsharded_ones(geom):
    c = case(geom, 3)
    args = (model(geom), c["ids"], c["ctx"], c["feats"].cuda(), c["labels"])
    kw = dict(sel=(1, 6, 2, 5), logit_scale=dref.LOGIT_SCALE, grad_scale=GRAD_SCALE, return_parts=True)
    loss0, grad0, parts0 = prodafit.context_gradient(*args, **kw)
    loss1, grad1, parts1 = prodafit.context_gradient(*args, shard=coopfit.Shard(1, 0, coopfit.LocalGather(1)), **kw)
    assert same(loss1, loss0) and same(grad1, grad0) and torch.isfinite(grad1).all() and sorted(parts1) == sorted(parts0)
    for k in ("upper", "m", "text"):
        assert same(parts1[k], parts0[k]), k
    f = c["feats"].cuda().repeat(2, 1)
    y = c["labels"].repeat(2)
    opt = dict(prompt_bs=PB, logit_scale=dref.LOGIT_SCALE, epochs=2, batch_size=2, lr_per_epoch=RATES[:2], return_history=True, **SGD)
    for kw in (dict(grad_scale=GRAD_SCALE), dict(grad_scale="dynamic", scaler={"init_scale": DEFAULT}, return_scaler_state=True)):
        plain = prodafit.fit_context(f, y, model(geom), c["ids"], c["ctx"], **opt, **kw)
        one = prodafit.fit_context(f, y, model(geom), c["ids"], c["ctx"], shard=coopfit.Shard(1, 0, coopfit.LocalGather(1)), **opt, **kw)
        assert same(one[0], plain[0]) and np.array_equal(one[1], plain[1]) and len(one[1]) == 4 and one[2:] == plain[2:]


@pytest.mark.parametrize("geom,G", [("tiny", 1), ("tiny3", 1), ("tiny", 2)])
def test_overflow_is_skipped_on_every_rank(geom, G):
    """Started at the scale at which the static path overflows fp16 (profiles/prodascaler_parity.txt), with backoff 2^-4: step 1 is
    skipped on every rank -- contexts and buffer unchanged, the schedule moved on -- and steps 2 .. 4 equal, bit for bit, the static
    sharded run at the backed-off scale on steps 2 .. 4 of the same schedule.  With one rank the whole run is the unsharded dynamic run."""
    scale, start = OVERFLOWS_AT[geom], case(geom, 3)["ctx"]
    scaler = {"init_scale": scale, "backoff_factor": 2.0 ** -4, "growth_interval": 1000}
    first, _ = run(geom, 3, G, 1, grad_scale="dynamic", scaler=scaler)
    blocks_agree(first)
    for s in first:
        assert s.scaler_state() == {"scale": scale / 16.0, "growth_tracker": 0, "skipped_steps": 1, "applied_steps": 0, "found_inf": 1}
        assert same(s.ctx.cpu(), start) and not s.buf.any()
    static, hist_s = run(geom, 3, G, 3, first=1, grad_scale=scale / 16.0)
    for own in (False, True):
        dyn, hist = run(geom, 3, G, 4, own_schedule=own, grad_scale="dynamic", scaler=scaler)
        blocks_agree(dyn)
        assert dyn[0].scaler_state() == {"scale": scale / 16.0, "growth_tracker": 3, "skipped_steps": 1, "applied_steps": 3, "found_inf": 0}
        assert same(dyn[0].ctx, static[0].ctx) and same(dyn[0].buf, static[0].buf) and same(hist[1:], hist_s) and torch.isfinite(dyn[0].ctx).all()
        if G == 1:
            (plain,), want = run(geom, 3, None, 4, own_schedule=own, grad_scale="dynamic", scaler=scaler)
            assert same(dyn[0].ctx, plain.ctx) and same(dyn[0].buf, plain.buf) and same(hist, want) and torch.equal(dyn[0]._scaler.block, plain._scaler.block)


# ------------------------------------------------------------------------------------------- 3. uneven shards and shards of one class
@pytest.mark.parametrize("G,C", [(2, 5), (3, 5), (2, 2), (3, 3)], ids=ident)
def test_uneven_and_one_class_shards(G, C):
    c, m = case("tiny", C), model("tiny")
    sel = dref.ordered(schedule()[0], POS)
    for kw in (dict(grad_scale=GRAD_SCALE), dict(grad_scale="dynamic", scaler={"init_scale": GRAD_SCALE, "growth_interval": 1000})):
        first, hist = run("tiny", C, G, 3, **kw)
        assert [s.tower.n_cls for s in first] == [hi - lo for lo, hi in sref.split(C, G)]
        assert [s.nc_hi - s.nc_lo for s in first] == [hi - lo for lo, hi in sref.split(P, G)]
        blocks_agree(first)
        assert torch.isfinite(first[0].ctx).all() and torch.isfinite(hist).all() and not same(first[0].ctx.cpu(), c["ctx"])
        # the gathered blocks of the last step are every rank's, and the text matrix behind the compaction is the shards' own features
        for s in first[1:]:
            assert torch.equal(s._all_part, first[0]._all_part) and torch.equal(s._text, first[0]._text)
        own_cls = torch.cat([s.tower.text[:s.tower.n_cls * PB] for s in first])
        own_nc = torch.cat([s.tower.text[s.tower.n_cls * PB:] for s in first])
        assert torch.equal(first[0]._text, torch.cat([own_cls, own_nc])) and first[0]._text.shape[0] == C * PB + P
        again, hist2 = run("tiny", C, G, 3, driver=G - 1, **kw)          # a second run, driven by the last rank: the same bytes
        blocks_agree(again)
        assert same(again[0].ctx, first[0].ctx) and same(again[0].buf, first[0].buf) and same(hist2, hist)
    # the dynamic run at a scale that never changes is the static run's bits
    assert same(first[0].ctx, run("tiny", C, G, 3, grad_scale=GRAD_SCALE)[0][0].ctx)
    # context_gradient(shard=) is the first step's applied gradient: the restatement's rank-ordered sum of the device's own partials, and
    # what one SGD step without momentum and weight decay at lr = 0.5 moves the contexts by
    local = coopfit.LocalGather(G)
    args = (m, c["ids"], c["ctx"], c["feats"].cuda(), c["labels"])
    loss, grad = prodafit.context_gradient(*args, sel=schedule()[0], logit_scale=dref.LOGIT_SCALE, grad_scale=GRAD_SCALE, shard=coopfit.Shard(G, G - 1, local))
    blocks = local.states[0]._all_part.cpu().numpy().reshape(G, PB + -(-P // G), N_CTX, -1)
    assert np.array_equal(grad.cpu().numpy(), sref.reduce_blocks(blocks, sel, P, np.float32(1 / GRAD_SCALE)))
    stepped = states_of("tiny", C, G, grad_scale=GRAD_SCALE, momentum=0.0, weight_decay=0.0)
    loss1 = stepped[0].step(c["feats"].cuda(), c["labels"].cuda(), 0.5, sel=i32(schedule())[0], want_loss=True)      # lr = 0.5: the product is exact
    assert same(loss1, loss) and np.array_equal(stepped[G - 1].ctx.cpu().numpy(), c["ctx"].numpy() - np.float32(0.5) * grad.cpu().numpy())
    with pytest.raises(ValueError, match="must not be stepped as well"):
        first[1].step(c["feats"].cuda(), c["labels"].cuda(), 1e-3)
    assert first[1].steps == 3


# ------------------------------------------------------------------------------------------------------------------------- 4. parity
def test_sharded_gradient_meets_the_parity_criterion():
    """G = 2, C = 5 on tiny (sel (1, 6, 2, 5)): the relative Frobenius error against float64 autograd through the oracle is at most 2 x
    the fp16 reference's own -- the criterion of every fit here (profiles/prodafit_parity.txt).  The unsharded gradient's ratio stands
    beside it."""
    sel = (1, 6, 2, 5)
    c = case("tiny", 5)
    args = (c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"], sel)
    want, (yard, how) = dref.oracle_parts(*args), dref.yardstick_parts(*args)
    y = ref.rel_fro(yard["grad"], want["grad"])
    dev = (model("tiny"), c["ids"], c["ctx"], c["feats"].cuda(), c["labels"])
    kw = dict(sel=sel, logit_scale=dref.LOGIT_SCALE, grad_scale=GRAD_SCALE)
    loss, grad = prodafit.context_gradient(*dev, shard=coopfit.Shard(2, 0, coopfit.LocalGather(2)), **kw)
    _, plain = prodafit.context_gradient(*dev, **kw)
    e, e0 = ref.rel_fro(grad.cpu(), want["grad"]), ref.rel_fro(plain.cpu(), want["grad"])
    say(f"sharded gradient tiny C=5 G=2 B={B} n_ctx={N_CTX} P={P} Pb={PB}: rel. Frobenius error {e:.3e}, yardstick ({how}) {y:.3e}, ratio {e / y:.2f}; "
        f"unsharded ratio {e0 / y:.2f}; loss {float(loss.cpu()):.6f} vs {want['loss']:.6f}")
    assert torch.isfinite(grad).all() and grad.shape == c["ctx"].shape
    assert e <= FACTOR * y
    assert abs(float(loss.cpu()) - want["loss"]) <= FACTOR * y * max(1.0, abs(want["loss"]))


# ---------------------------------------------------------------------------------------------------------------------- 5. the trainer
def test_trainer_passes_the_shard_on_the_cached_route():
    """``ProDACLIP.fit_context(shard=)`` equals the hand-written loop over the shard states; the loader's "images" are the features
    themselves, passed through by a stand-in for the image tower (tests/test_gpu_prodafit.py)."""
    from clip_calibration_amd import trainers
    m, c = model("tiny"), case("tiny", 5)
    f, y = c["feats"].cuda().repeat(2, 1), c["labels"].repeat(2)
    opt = dict(prompt_bs=PB, grad_scale=GRAD_SCALE, **SGD)

    def fit(shard, **kw):
        clip = trainers.ProDACLIP(m, c["ids"], n_ctx=N_CTX, n_prompt=P)
        with torch.no_grad():
            clip.prompt_learner.ctx.copy_(c["ctx"])
        try:
            m.image_features_f32 = lambda image: image
            out = clip.fit_context([(f, y)], epochs=2, batch_size=2, lr_per_epoch=RATES[:2], return_history=True, generator=torch.Generator().manual_seed(SEED),
                                   **opt, **({} if shard is None else {"shard": shard}), **kw)
        finally:
            del m.image_features_f32
        assert clip.text_features is None and torch.equal(clip.prompt_learner.ctx.detach().float(), out[0].to(clip.prompt_learner.ctx.dtype).float())
        return out, clip
    start = trainers.ProDACLIP(m, c["ids"], n_ctx=N_CTX, n_prompt=P).prompt_learner.ctx.detach().clone()
    start.copy_(c["ctx"])                                                # what the fits start from: the case's contexts in the parameter's dtype
    (plain, hist0), clip = fit(None)
    (one, hist1), _ = fit(coopfit.Shard(1, 0, coopfit.LocalGather(1)))
    assert same(one, plain) and np.array_equal(hist1, hist0)
    local = coopfit.LocalGather(2)
    (two, hist2), _ = fit(coopfit.Shard(2, 1, local))                    # this process is rank 1 of the two it runs
    assert [s.tower.n_cls for s in local.states] == [3, 2] and all(s.steps == 4 for s in local.states)
    blocks_agree(local.states)
    # the hand-written loop: the fit's schedule, drawn once from the same seed, over two fresh shard states
    sels = i32(prodafit.draw_selections(P, PB, 4, torch.Generator().manual_seed(SEED)))
    loop = coopfit.LocalGather(2)
    states = [prodafit.ProDAFitState(m, c["ids"], start, logit_scale=math.log(clip.scale), shard=coopfit.Shard(2, r, loop), **opt) for r in range(2)]
    want = [states[1].step(f[2 * (k % 2):2 * (k % 2) + 2], y[2 * (k % 2):2 * (k % 2) + 2].cuda(), RATES[k // 2], sel=sels[k], want_loss=True) for k in range(4)]
    assert same(two, states[1].ctx) and same(two, states[0].ctx) and np.array_equal(hist2, torch.cat(want).cpu().numpy())
    assert np.isfinite(hist2).all() and not same(two, plain)
    with pytest.raises(ValueError, match="shard has no validation"):
        fit(coopfit.Shard(2, 0, coopfit.LocalGather(2)), val_loader=object())


def test_trainer_transform_route_under_a_local_gather():
    """``transform=``: decoded uint8 batches go transform -> image tower -> ``ProDAFitState.step``, the driving state drawing the
    selections.  One shard gives the unsharded route's bits; with two, the run equals the hand-written loop over the two states."""
    import augment_ref as aref
    from clip_calibration_amd.augment import TrainPreprocess
    from clip_calibration_amd.preprocess import pack_images
    from clip_calibration_amd import trainers
    m, ids = model("tiny"), dref.prompt_ids("tiny", 5, N_CTX)
    start = trainers.ProDACLIP(m, ids, n_ctx=N_CTX, n_prompt=P).prompt_learner.ctx.detach().clone()
    start.copy_(case("tiny", 5)["ctx"])                                  # the case's contexts in the parameter's dtype
    imgs = [aref.synthetic_image(h, w, 70 + i) for i, (h, w) in enumerate([(80, 100), (64, 64), (70, 51), (120, 90)])]
    loader = [(pack_images(imgs).pin_memory(), torch.arange(4) % 5)]
    opt = dict(prompt_bs=PB, grad_scale=GRAD_SCALE, **SGD)

    def run_fit(shard):
        tp = TrainPreprocess.for_model(m, generator=torch.Generator().manual_seed(23))
        clip = trainers.ProDACLIP(m, ids, n_ctx=N_CTX, n_prompt=P)
        with torch.no_grad():
            clip.prompt_learner.ctx.copy_(start)
        return clip.fit_context(loader, transform=tp, epochs=2, lr_per_epoch=RATES[:2], return_history=True, generator=torch.Generator().manual_seed(5), **opt,
                                **({} if shard is None else {"shard": shard})), clip
    (plain, hist0), clip = run_fit(None)
    (one, hist1), _ = run_fit(coopfit.Shard(1, 0, coopfit.LocalGather(1)))
    assert same(one, plain) and np.array_equal(hist1, hist0) and np.isfinite(hist0).all()
    local = coopfit.LocalGather(2)
    (two, hist2), _ = run_fit(coopfit.Shard(2, 0, local))
    assert all(s.steps == 2 for s in local.states)
    blocks_agree(local.states)
    tp = TrainPreprocess.for_model(m, generator=torch.Generator().manual_seed(23))
    loop = coopfit.LocalGather(2)
    states = [prodafit.ProDAFitState(m, ids, start, logit_scale=math.log(clip.scale), generator=torch.Generator().manual_seed(5),
                                     shard=coopfit.Shard(2, r, loop), **opt) for r in range(2)]
    with torch.no_grad():
        want = [states[0].step(m.image_features_f32(tp(images)), lab, RATES[e], want_loss=True) for e in range(2) for images, lab in loader]
    assert same(two, states[0].ctx) and np.array_equal(hist2, torch.cat(want).cpu().numpy()) and not same(two, plain)


# ------------------------------------------------------------------------------------------------- 6. the RCCL gather, on one rank
def test_rccl_gather_with_one_rank_holds_the_local_bits():
    """``parallel.shard_gather`` on a one-rank communicator (this box may have one GPU; tests/test_gpu_prodashard_ranks.py runs two):
    clipmi_allgather moves every block of the step, and the bits are the local gather's, static and dynamic."""
    from clip_calibration_amd import parallel
    c = case("tiny", 3)
    ex = parallel.EmbeddingExchange(torch.device("cuda", torch.cuda.current_device()), backend="rccl")
    try:
        assert ex.rccl_ranks == 1
        x, y, lr, sels = c["feats"].cuda(), c["labels"].cuda(), torch.tensor(RATES, dtype=torch.float32).cuda(), i32(schedule())
        for kw in (dict(grad_scale=GRAD_SCALE), dict(grad_scale="dynamic", scaler={"init_scale": DEFAULT})):
            st = prodafit.ProDAFitState(model("tiny"), c["ids"], c["ctx"], prompt_bs=PB, logit_scale=dref.LOGIT_SCALE,
                                        shard=coopfit.Shard(1, 0, parallel.shard_gather(ex)), **SGD, **kw)
            hist = torch.cat([st.step(x, y, lr[k:k + 1], sel=sels[k], want_loss=True) for k in range(3)]).cpu()
            (local,), want = run("tiny", 3, 1, 3, **kw)
            assert same(hist, want) and same(st.ctx, local.ctx) and same(st.buf, local.buf)
            if st.dynamic:
                assert torch.equal(st._scaler.block, local._scaler.block)
    finally:
        ex.close()
