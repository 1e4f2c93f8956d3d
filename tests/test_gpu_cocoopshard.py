"""The class-sharded CoCoOp fit on one GPU (clip_calibration_amd/cocoopfit.py ``shard=``, csrc/cocoop_train.hip): every case runs the ranks
of a ``LocalGather`` -- the kernels and the phase code of the multi-process run, device copies in the all-gather's place.
  1. the new operators against tests/cocoopshard_ref.py on streams built to cancel     2. one rank is the unsharded path bit for bit: SGD,
  the dynamic scale with a skipped step, Adam     3. G = 2, 3 with uneven and one-class shards     4. parity with the float64 oracle and the
  stash     5. the trainer     6. RCCL on one rank
Cases from tests/cocoopfit_ref.py on the synthetic ``tiny`` / ``tiny3`` towers: n_ctx 4, batch 2 or 3, C up to 5."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import cocoopfit_ref as cref
import cocoopshard_ref as sref
import coopfit_ref as ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import cocoopfit, coopfit, ops  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

FACTOR = 2.0                # the project's standing criterion (tests/test_gpu_cocoopfit.py): at most twice the fp16 reference's own error
GRAD_SCALE = 256.0          # as tests/test_gpu_cocoopfit.py: the synthetic weights give gradients far larger than ViT-B/16's
DEFAULT = cocoopfit.DEFAULT_GRAD_SCALE
OVERFLOW_CASE, OVERFLOWS_AT = ("tiny3", 3, 4, 3), 2.0 ** 15      # profiles/blockscaler_parity.txt: "cocoop: the static path overflows at 2^15"
RATES = [2e-3, 1e-3, 5e-4, 2e-3]
SGD = dict(momentum=0.9, dampening=0.0, nesterov=False, weight_decay=5e-4)
NAMES = cref.NAMES
PARITY_LOG = os.environ.get("CLIPMI_COCOOPSHARD_PARITY")   # a file that receives the parity lines (profiles/cocoopshard_parity.txt is made so)
BIG = np.float32(2.0 ** 24)
TRIPLE = np.array([2.0 ** 24, 1.0, -2.0 ** 24], np.float32)     # added in this order: 0; in the reverse: 1


def say(line):
    print("cocoopshard-parity: " + line)
    if PARITY_LOG:
        with open(PARITY_LOG, "a") as f:
            f.write(line + "\n")


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def same(a, b):
    return a.shape == b.shape and a.cpu().contiguous().view(torch.int32).equal(b.cpu().contiguous().view(torch.int32))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def model(geom):
    return build_model(dict(ref.state_dict(geom)), {"trainer": "CoOp"}).cuda()


# ------------------------------------------------------------------------------------------------------------------ 1. the operators
def cancelling_stream(B, C, L, D, seed):
    """d_embed [B C, L, D]: random rows, but for a large and a tiny value per CLASS in four columns, so that a wrong order of the classes
    shows (as tests/test_gpu_prodashard.py builds it)."""
    g = np.random.RandomState(seed).standard_normal((B * C, L, D)).astype(np.float32)
    cls = np.tile(np.arange(C), B)
    big = BIG * np.where(cls % 2 == 0, 1, -1).astype(np.float32)
    g[:, :, 0] = big[:, None]
    g[:, :, 1] = np.float32(1.0)
    g[:, :, 2] = (big + cls.astype(np.float32))[:, None]
    g[:, :, 3] = TRIPLE[cls % 3][:, None]
    return g


@pytest.mark.parametrize("B,C,n_ctx,D", [(1, 1, 2, 64), (2, 3, 4, 100), (3, 6, 2, 129)])
def test_cocoop_dcs_partial(B, C, n_ctx, D):
    """A rank's partial: D 64 and 100 take the 16-byte path, 129 the scalar one; the last two run more than one workgroup; one class is
    a legal shard."""
    L = n_ctx + 3
    g = cancelling_stream(B, C, L, D, 1)
    want = sref.partial(g, B, n_ctx)
    assert want.dtype == np.float32 and np.isfinite(want).all()
    out = ops.cocoop_dcs_partial(dev(g).view(-1, D), B, C, n_ctx)
    assert out.shape == (B, n_ctx, D) and np.array_equal(out.cpu().numpy(), want)
    if C >= 3:                                                           # the order shows: the classes reversed give other bits
        back = np.ascontiguousarray(g.reshape(B, C, L, D)[:, ::-1]).reshape(B * C, L, D)
        assert not np.array_equal(want, sref.partial(back, B, n_ctx))
    # written into the first rows of a longer block: the bytes behind them stay as they were
    block = torch.full((B + 1, n_ctx, D), float("nan")).cuda()
    ops.cocoop_dcs_partial(dev(g).view(-1, D), B, C, n_ctx, block[:B])
    assert np.array_equal(block[:B].cpu().numpy(), want) and torch.isnan(block[B:]).all()
    with pytest.raises(ValueError, match="cocoop_dcs_partial"):
        ops.cocoop_dcs_partial(dev(g).view(-1, D), B, C + 1, n_ctx)


@pytest.mark.parametrize("C,G,E", [(7, 1, 64), (7, 3, 100), (13, 8, 129)])
def test_cocoop_shard_compact_and_rows(C, G, E):
    """The gathered text features back in the unsharded order, and the rank's rows of d_text out of it.  The padding rows and a padded
    rank stride (4 floats: still on the 16-byte phase; 5: off it) are NaN and must never be read."""
    B = 2
    full = np.random.RandomState(C).standard_normal((B * C, E)).astype(np.float32)
    for extra in (0, 4, 5):
        gathered = sref.gathered_text(full, B, C, G, extra)
        assert np.isnan(gathered).any() == (C % G != 0 or extra > 0)
        room = torch.full((B * C + 1, E), -7.0).cuda()
        out = ops.cocoop_shard_compact(dev(gathered), B, C, E, room[:B * C])
        assert np.array_equal(out.cpu().numpy(), full) and bool((room[B * C:] == -7.0).all())
    assert np.array_equal(ops.cocoop_shard_compact(dev(sref.gathered_text(full, B, C, G)), B, C, E).cpu().numpy(), full)
    with pytest.raises(ValueError, match="cocoop_shard_compact"):
        ops.cocoop_shard_compact(torch.zeros(G, B * sref.pad(C, G) * E - 1).cuda(), B, C, E)
    for r, (lo, hi) in enumerate(sref.split(C, G)):
        assert (lo, hi) == coopfit.shard_classes(C, G, r)
        poisoned = full.copy().reshape(B, C, E)
        poisoned[:, :lo], poisoned[:, hi:] = np.nan, np.nan              # the other ranks' rows must not reach the output
        want = sref.own_rows(full, B, C, lo, hi)
        room = torch.full((B * (hi - lo) + 1, E), -7.0).cuda()
        out = ops.cocoop_shard_rows(dev(poisoned).view(B * C, E), B, lo, hi, room[:B * (hi - lo)])
        assert np.array_equal(out.cpu().numpy(), want) and bool((room[B * (hi - lo):] == -7.0).all())
        # compact is the inverse: the rank's own rows, laid at the head of its block
        assert np.array_equal(sref.gathered_text(full, B, C, G)[r, :want.size], want.reshape(-1))
    with pytest.raises(ValueError, match="cocoop_shard_rows"):
        ops.cocoop_shard_rows(dev(full), B, 3, 3)


def gathered_partials(G, n, extra, seed):
    """[G, n + extra] fp32: a large value per rank and a tiny one beside it, cancelling across the ranks; the padded stride is NaN."""
    blocks = np.concatenate([np.random.RandomState(seed).standard_normal((G, n)), np.zeros((G, extra))], 1).astype(np.float32)
    r = np.arange(G)
    blocks[:, 0:n:4] = (BIG * np.where(r % 2 == 0, 1, -1).astype(np.float32))[:, None]
    blocks[:, 1:n:4] = (BIG * np.where(r % 2 == 0, 1, -1).astype(np.float32) + r.astype(np.float32))[:, None]
    blocks[:, 3:n:4] = TRIPLE[r % 3][:, None]
    blocks[:, n:] = np.nan
    return blocks


@pytest.mark.parametrize("G,B,n_ctx,D", [(1, 2, 4, 64), (3, 2, 4, 100), (8, 3, 3, 129)])
def test_cocoop_reduce_gathered(G, B, n_ctx, D):
    """The same gradient block as clipmi_cocoop_reduce given the rank-ordered sum as its dcs: B n_ctx D = 1161 takes the scalar path, the
    others the 16-byte one, and so does a rank stride padded by 5.  The padding is NaN and never read; the ranks reversed give other bits."""
    E, H, n = 16, 5, B * n_ctx * D
    rng = np.random.RandomState(G)
    x, hid, w2 = (rng.standard_normal(s).astype(np.float32) for s in ((B, E), (B, H), (D, H)))
    hid = np.maximum(hid, 0)
    inv = np.float32(1 / 256.0)
    blocks = gathered_partials(G, n, 0, 2)
    dcs = sref.reduce_partials(blocks, n, inv).reshape(B, n_ctx, D)
    assert np.isfinite(dcs).all()
    # clipmi_cocoop_reduce on a two-class stream: class 0 carries dcs, class 1 zeros, grad_scale 1 -- its own sum is 0 + dcs + 0
    stream = np.zeros((B, 2, 1 + n_ctx, D), np.float32)
    stream[:, 0, 1:] = dcs
    want = ops.cocoop_reduce(dev(stream).view(-1, D), dev(x), dev(hid), dev(w2), 2, n_ctx, 1.0)
    for extra in (0, 4, 5):
        got = ops.cocoop_reduce_gathered(dev(gathered_partials(G, n, extra, 2)), dev(x), dev(hid), dev(w2), n_ctx, 256.0)
        assert same(got, want) and torch.isfinite(got).all(), extra
    dctx = np.zeros((n_ctx, D), np.float32)                              # the block's first tensor, restated: the images ascending from zero
    for b in range(B):
        dctx = dctx + dcs[b]
    assert np.array_equal(want[:n_ctx * D].cpu().numpy().reshape(n_ctx, D), dctx)
    if G >= 3:
        back = ops.cocoop_reduce_gathered(dev(blocks[::-1]), dev(x), dev(hid), dev(w2), n_ctx, 256.0)
        assert not same(back, want) and not np.array_equal(sref.reduce_partials(blocks[::-1], n, inv), dcs.reshape(-1))
    with pytest.raises(ValueError, match="cocoop_reduce_gathered"):
        ops.cocoop_reduce_gathered(torch.zeros(G, n - 1).cuda(), dev(x), dev(hid), dev(w2), n_ctx, 256.0)


@pytest.mark.parametrize("D", [100, 129])
def test_one_rank_operators_are_cocoop_reduce(D):
    """The anchor at operator level: partial, then the gathered reduce over one rank, is clipmi_cocoop_reduce -- 0 + p is p, and the one
    multiplication is the unsharded kernel's."""
    B, C, n_ctx, E, H = 2, 5, 4, 16, 5
    rng = np.random.RandomState(D)
    x, hid, w2 = (dev(rng.standard_normal(s).astype(np.float32)) for s in ((B, E), (B, H), (D, H)))
    g = dev(cancelling_stream(B, C, n_ctx + 3, D, 3)).view(-1, D)
    part = ops.cocoop_dcs_partial(g, B, C, n_ctx)
    for gs in (1.0, 256.0, 3.0):
        assert same(ops.cocoop_reduce_gathered(part.view(1, -1), x, hid, w2, n_ctx, gs), ops.cocoop_reduce(g, x, hid, w2, C, n_ctx, gs)), gs


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_cocoop_embed_classes_is_a_slice_of_cocoop_embed(dtype):
    B, C, Lc, L, D, n_ctx = 2, 5, 16, 12, 8, 4
    g = torch.Generator().manual_seed(5)
    base = torch.randn(C, Lc, D, generator=g).to(dtype).cuda()
    ctx, pi = torch.randn(n_ctx, D, generator=g).cuda(), torch.randn(B, D, generator=g).cuda()
    cls_eot = torch.tensor([6, 7, 9, 8, 11], dtype=torch.int32).cuda()
    full, eot = ops.cocoop_embed(base, ctx, pi, cls_eot, L, torch.zeros(B * C, Lc, D).cuda(), torch.zeros(B * C, dtype=torch.int32).cuda())
    assert bool(full.view(B, C, Lc, D)[:, :, L:].eq(0).all()) and bool(full.view(B, C, Lc, D)[:, :, :L].ne(0).any())
    for lo, hi in ((0, 5), (1, 3), (4, 5), (2, 3)):                       # the whole set, a range, the last class alone, one inner class
        n = B * (hi - lo)
        got, got_eot = ops.cocoop_embed_classes(base, ctx, pi, cls_eot, lo, hi, L, torch.zeros(n, Lc, D).cuda(), torch.zeros(n, dtype=torch.int32).cuda())
        assert same(got.view(B, hi - lo, Lc, D), full.view(B, C, Lc, D)[:, lo:hi]), (lo, hi)
        assert torch.equal(got_eot.view(B, hi - lo), eot.view(B, C)[:, lo:hi])
    with pytest.raises(ValueError, match="cocoop_embed_classes"):
        ops.cocoop_embed_classes(base, ctx, pi, cls_eot, 3, 3)


# -------------------------------------------------------------------------------------------------------------------------- the fit
ROUTES = {"sgd": dict(grad_scale=GRAD_SCALE), "dynamic": dict(grad_scale="dynamic", scaler={"init_scale": GRAD_SCALE, "growth_interval": 1000}),
          "adam": dict(grad_scale=GRAD_SCALE, optimizer="adam"), "adamw-dynamic": dict(grad_scale="dynamic", scaler={"init_scale": GRAD_SCALE}, optimizer="adamw")}


def states_of(key, G, **kw):
    """The G shard states of one LocalGather, rank 0 first -- or, with G = None, the one unsharded state."""
    c = cref.make_case(*key)
    kw = dict(dict(logit_scale=ref.LOGIT_SCALE, **SGD), **kw)
    make = lambda **more: cocoopfit.CoCoOpFitState(model(key[0]), c["ids"], c["params"], **kw, **more)
    if G is None:
        return [make()]
    local = coopfit.LocalGather(G)
    return [make(shard=coopfit.Shard(G, r, local)) for r in range(G)]


def run(key, G, steps, first=0, driver=0, **kw):
    """`steps` steps on the case's one batch at RATES[first:]: (states, losses)."""
    c = cref.make_case(*key)
    states = states_of(key, G, **kw)
    x, y, lr = c["feats"].cuda(), c["labels"].cuda(), torch.tensor(RATES, dtype=torch.float32).cuda()
    losses = [states[driver].step(x, y, lr[k:k + 1], want_loss=True) for k in range(first, first + steps)]
    assert all(s.steps == steps for s in states)
    return states, torch.cat(losses).cpu()


def blocks_of(s):
    """Everything a step may write: the master block, the momentum block, Adam's moments and step count, the scaler block."""
    out = {"block": s.block}
    if s.buf is not None:
        out["buf"] = s.buf
    if s._adam is not None:
        out.update(exp_avg=s._adam.exp_avg, exp_avg_sq=s._adam.exp_avg_sq, adam_steps=torch.tensor([s._adam.steps_taken]))
    if s.dynamic:
        out["scaler"] = s._scaler.block
    return out


def agree(a, b, why=""):
    ba, bb = blocks_of(a), blocks_of(b)
    assert sorted(ba) == sorted(bb)
    for k in ba:
        assert torch.equal(ba[k].cpu().view(-1).view(torch.uint8), bb[k].cpu().view(-1).view(torch.uint8)), (k, why)


def start_block(key):
    c = cref.make_case(*key)
    return torch.cat([c["params"][k].reshape(-1) for k in NAMES])


# ------------------------------------------------------------------------------------------------- 2. one rank: the unsharded bits
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("key", [("tiny", 5, 4, 2), ("tiny3", 3, 4, 3)], ids=ident)
def test_one_rank_is_the_unsharded_fit_bit_for_bit(key, route):
    """Four steps with momentum (or Adam's moments): parameters, momentum, moments, scaler block and losses are the unsharded state's."""
    (plain,), want = run(key, None, 4, **ROUTES[route])
    (one,), hist = run(key, 1, 4, **ROUTES[route])
    agree(one, plain, route)
    assert same(hist, want) and torch.isfinite(one.block).all() and torch.isfinite(hist).all() and not same(one.block.cpu(), start_block(key))
    if one.dynamic:
        assert one.scaler_state()["applied_steps"] == 4 and one.scaler_state()["skipped_steps"] == 0
    c = cref.make_case(*key)
    x, y = c["feats"].cuda(), c["labels"].cuda()
    with pytest.raises(ValueError, match=r"shard has no one-call step \(one_call=True\)"):
        one.step(x, y, 1e-3, one_call=True)
    with pytest.raises(ValueError, match="shard has no validation"):
        one.validate(x, y, 0)
    assert one.steps == 4


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_one_rank_skips_the_overflowed_step_as_the_unsharded_fit_does(optimizer):
    """Started at the scale at which the static path overflows fp16 (profiles/blockscaler_parity.txt), with backoff 2^-4: step 1 is
    skipped -- nothing but the scaler block moves -- and the whole four-step run is the unsharded dynamic run, bit for bit."""
    kw = dict(grad_scale="dynamic", scaler={"init_scale": OVERFLOWS_AT, "backoff_factor": 2.0 ** -4, "growth_interval": 1000}, optimizer=optimizer)
    (first,), _ = run(OVERFLOW_CASE, 1, 1, **kw)
    assert first.scaler_state() == {"scale": OVERFLOWS_AT / 16.0, "growth_tracker": 0, "skipped_steps": 1, "applied_steps": 0, "found_inf": 1}
    assert same(first.block.cpu(), start_block(OVERFLOW_CASE))
    assert not (first.buf.any() if optimizer == "sgd" else first._adam.exp_avg.any() or first._adam.exp_avg_sq.any())
    (plain,), want = run(OVERFLOW_CASE, None, 4, **kw)
    (one,), hist = run(OVERFLOW_CASE, 1, 4, **kw)
    agree(one, plain, optimizer)
    assert same(hist, want) and torch.isfinite(one.block).all()
    assert one.scaler_state() == {"scale": OVERFLOWS_AT / 16.0, "growth_tracker": 3, "skipped_steps": 1, "applied_steps": 3, "found_inf": 0}


@pytest.mark.parametrize("key", [("tiny", 5, 4, 2), ("tiny3", 3, 4, 3)], ids=ident)
def test_one_rank_gradient_and_fit_are_the_unsharded_ones(key):
    c, m = cref.make_case(*key), model(key[0])
    args = (m, c["ids"], c["params"], c["feats"].cuda(), c["labels"])
    kw = dict(logit_scale=ref.LOGIT_SCALE, grad_scale=GRAD_SCALE, return_parts=True)
    loss0, grads0, parts0 = cocoopfit.gradients(*args, **kw)
    loss1, grads1, parts1 = cocoopfit.gradients(*args, shard=coopfit.Shard(1, 0, coopfit.LocalGather(1)), **kw)
    assert same(loss1, loss0) and sorted(parts1) == sorted(parts0)
    for k in NAMES:
        assert same(grads1[k], grads0[k]) and torch.isfinite(grads1[k]).all(), k
    for k in parts0:
        assert same(parts1[k], parts0[k]), k
    B = key[3]
    f, y = c["feats"].cuda().repeat(2, 1), c["labels"].repeat(2)
    opt = dict(logit_scale=ref.LOGIT_SCALE, epochs=2, batch_size=B, lr_per_epoch=RATES[:2], return_history=True, **SGD)
    for route, kw in ROUTES.items():
        plain = cocoopfit.fit_prompt_learner(f, y, m, c["ids"], c["params"], **opt, **kw)
        one = cocoopfit.fit_prompt_learner(f, y, m, c["ids"], c["params"], shard=coopfit.Shard(1, 0, coopfit.LocalGather(1)), **opt, **kw)
        assert all(same(one[0][k], plain[0][k]) for k in NAMES) and np.array_equal(one[1], plain[1]) and len(one[1]) == 4, route


# ------------------------------------------------------------------------------------------- 3. uneven shards and shards of one class
@pytest.mark.parametrize("G,C", [(2, 5), (3, 5), (2, 2), (3, 3)], ids=ident)
def test_uneven_and_one_class_shards(G, C):
    key = ("tiny", C, 4, 2)
    c, m = cref.make_case(*key), model("tiny")
    for route, kw in ROUTES.items():
        first, hist = run(key, G, 3, **kw)
        assert [s.tower(2).n_cls for s in first] == [hi - lo for lo, hi in sref.split(C, G)]
        for s in first[1:]:
            agree(s, first[0], route)                                    # every rank ends every step with identical bits
            assert torch.equal(s.tower(2).all_part, first[0].tower(2).all_part) and torch.equal(s.tower(2).full_text, first[0].tower(2).full_text)
        assert torch.isfinite(first[0].block).all() and torch.isfinite(hist).all() and not same(first[0].block.cpu(), start_block(key))
        if first[0]._adam is not None:
            assert [s._adam.steps_taken for s in first] == [3] * G
        # the text matrix behind the compaction is the shards' own features, class ranges side by side
        own = torch.cat([s.tower(2).text.view(2, s.tower(2).n_cls, -1) for s in first], dim=1)
        assert torch.equal(first[0].tower(2).full_text.view(2, C, -1), own)
        again, hist2 = run(key, G, 3, driver=G - 1, **kw)                # a second run, driven by the last rank: the same bytes
        agree(again[0], first[0], route)
        agree(again[G - 1], first[0], route)
        assert same(hist2, hist)
    # gradients(shard=) is the first step's applied gradient: the restatement's rank-ordered sum of the device's own partials in its ctx
    # part, and what one SGD step without momentum and weight decay at lr = 0.5 moves the block by
    local = coopfit.LocalGather(G)
    loss, grads = cocoopfit.gradients(m, c["ids"], c["params"], c["feats"].cuda(), c["labels"], logit_scale=ref.LOGIT_SCALE, grad_scale=GRAD_SCALE,
                                      shard=coopfit.Shard(G, G - 1, local))
    t = local.states[0].tower(2)
    n = 2 * t.n_ctx * t.D
    dcs = sref.reduce_partials(t.all_part.cpu().numpy(), n, np.float32(1 / GRAD_SCALE)).reshape(2, t.n_ctx, t.D)
    assert np.array_equal(grads["ctx"].cpu().numpy(), (np.zeros_like(dcs[0]) + dcs[0]) + dcs[1])
    stepped = states_of(key, G, grad_scale=GRAD_SCALE, momentum=0.0, weight_decay=0.0)
    loss1 = stepped[0].step(c["feats"].cuda(), c["labels"].cuda(), 0.5, want_loss=True)      # lr = 0.5: the product is exact
    flat = torch.cat([grads[k].reshape(-1) for k in NAMES]).cpu().numpy()
    assert same(loss1, loss) and np.array_equal(stepped[G - 1].block.cpu().numpy(), start_block(key).numpy() - np.float32(0.5) * flat)
    with pytest.raises(ValueError, match="must not be stepped as well"):
        stepped[1].step(c["feats"].cuda(), c["labels"].cuda(), 1e-3)
    assert stepped[1].steps == 1


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("G", [2, 3])
def test_overflow_is_skipped_on_every_rank(G, optimizer):
    """Started above the scale at which fp16 overflows (twice profiles/blockscaler_parity.txt's 2^15, backoff 2^-5): step 1 is skipped on
    every rank -- no block but the scaler's moves -- and steps 2 .. 4 are applied on every rank.  G = 3 gives every rank one class."""
    kw = dict(grad_scale="dynamic", scaler={"init_scale": 2 * OVERFLOWS_AT, "backoff_factor": 2.0 ** -5, "growth_interval": 1000}, optimizer=optimizer)
    first, _ = run(OVERFLOW_CASE, G, 1, **kw)
    for s in first:
        assert s.scaler_state() == {"scale": OVERFLOWS_AT / 16.0, "growth_tracker": 0, "skipped_steps": 1, "applied_steps": 0, "found_inf": 1}
        assert same(s.block.cpu(), start_block(OVERFLOW_CASE))
        assert not (s.buf.any() if optimizer == "sgd" else s._adam.exp_avg.any() or s._adam.exp_avg_sq.any())
    dyn, hist = run(OVERFLOW_CASE, G, 4, **kw)
    for s in dyn:
        agree(s, dyn[0], optimizer)
        assert s.scaler_state() == {"scale": OVERFLOWS_AT / 16.0, "growth_tracker": 3, "skipped_steps": 1, "applied_steps": 3, "found_inf": 0}
    assert torch.isfinite(dyn[0].block).all() and torch.isfinite(hist).all() and not same(dyn[0].block.cpu(), start_block(OVERFLOW_CASE))
    if optimizer == "adam":
        assert [s._adam.steps_taken for s in dyn] == [4] * G             # enqueued steps: the device decides which of them count
    if optimizer == "sgd":                                               # steps 2 .. 4 are the static sharded run at the backed-off scale
        static, hist_s = run(OVERFLOW_CASE, G, 3, first=1, grad_scale=OVERFLOWS_AT / 16.0)
        assert same(dyn[0].block, static[0].block) and same(dyn[0].buf, static[0].buf) and same(hist[1:], hist_s)


# ------------------------------------------------------------------------------------------------------------------------- 4. parity
def test_sharded_gradient_meets_the_parity_criterion():
    """G = 2, C = 5 on tiny, batch 3: each of the five gradients' relative Frobenius error against float64 autograd through the oracle is at
    most 2 x the fp16 reference's own -- the criterion of every fit here.  The unsharded gradient's ratio stands beside it."""
    key = ("tiny", 5, 4, 3)
    c = cref.make_case(*key)
    args = (c["sd"], c["ids"], c["params"], c["feats"], c["labels"])
    want, (yard, how) = cref.oracle_parts(*args), cref.yardstick_parts(*args)
    devargs = (model("tiny"), c["ids"], c["params"], c["feats"].cuda(), c["labels"])
    kw = dict(logit_scale=ref.LOGIT_SCALE, grad_scale=GRAD_SCALE)
    loss, grads = cocoopfit.gradients(*devargs, shard=coopfit.Shard(2, 0, coopfit.LocalGather(2)), **kw)
    _, plain = cocoopfit.gradients(*devargs, **kw)
    ys = {k: ref.rel_fro(yard["grads"][k], want["grads"][k]) for k in NAMES}
    es = {k: ref.rel_fro(grads[k].cpu(), want["grads"][k]) for k in NAMES}
    e0 = {k: ref.rel_fro(plain[k].cpu(), want["grads"][k]) for k in NAMES}
    say(f"sharded gradient tiny C=5 G=2 B=3 n_ctx=4, yardstick ({how}), loss {float(loss.cpu()):.6f} vs {want['loss']:.6f}; rel. Frobenius error / "
        "yardstick = ratio (unsharded ratio): " + ", ".join(f"{k} {es[k]:.3e} / {ys[k]:.3e} = {es[k] / ys[k]:.2f} ({e0[k] / ys[k]:.2f})" for k in NAMES))
    for k in NAMES:
        assert grads[k].shape == c["params"][k].shape and torch.isfinite(grads[k]).all(), k
        assert es[k] <= FACTOR * ys[k], k
    assert abs(float(loss.cpu()) - want["loss"]) <= FACTOR * ys["ctx"] * max(1.0, abs(want["loss"]))


def test_a_ranks_stash_is_sized_by_its_own_classes():
    key = ("tiny", 5, 4, 3)
    c, m = cref.make_case(*key), model("tiny")
    whole = cocoopfit.stash_bytes(m, c["ids"], 3)
    (plain,) = states_of(key, None, grad_scale=GRAD_SCALE)
    assert plain.tower(3).stash_bytes == whole[1] and plain.tower(3).ws.numel() <= max(whole[0], 256)
    for r, s in enumerate(states_of(key, 2, grad_scale=GRAD_SCALE)):
        t, (ws, st) = s.tower(3), cocoopfit.stash_bytes(m, c["ids"], 3, world=2, rank=r)
        assert t.N == 3 * t.n_cls and t.rows == plain.tower(3).rows      # the live-row cut of the whole prompt set
        assert 0 < t.stash_bytes <= st < whole[1] and t.stash.numel() <= max(st, 256) and t.ws.numel() <= max(ws, 256)
    with pytest.raises(ValueError, match="C=5 classes cannot be split over world=8"):
        cocoopfit.stash_bytes(m, c["ids"], 3, world=8)


# ---------------------------------------------------------------------------------------------------------------------- 5. the trainer
def test_trainer_passes_the_shard_on_the_cached_route():
    """``CoCoOpCLIP.fit_prompt_learner(shard=)`` over two epochs equals ``cocoopfit.fit_prompt_learner(shard=)`` from the module's own
    values; the loader's "images" are the features themselves (tests/test_gpu_cocoopfit.py)."""
    from clip_calibration_amd import trainers
    m, c = model("tiny"), cref.make_case("tiny", 5, 4, 2)
    f, y = c["feats"].cuda().repeat(2, 1), c["labels"].repeat(2)
    opt = dict(epochs=2, batch_size=2, lr_per_epoch=RATES[:2], return_history=True, grad_scale=GRAD_SCALE, **SGD)

    def fit(shard, **kw):
        clip = trainers.CoCoOpCLIP(m, c["ids"], n_ctx=4)
        pl = clip.prompt_learner
        with torch.no_grad():
            for k, v in pl.named_parameters():
                if k in NAMES:
                    v.copy_(c["params"][k])
        start = {k: v.detach().clone() for k, v in pl.state_dict().items() if k in NAMES}
        try:
            m.image_features_f32 = lambda image: image
            out = clip.fit_prompt_learner([(f, y)], **opt, **({} if shard is None else {"shard": shard}), **kw)
        finally:
            del m.image_features_f32
        after = {k: v.detach() for k, v in pl.state_dict().items() if k in NAMES}
        assert all(torch.equal(after[k], out[0][k].to(after[k].dtype)) for k in NAMES)
        return out, start, clip
    (plain, hist0), _, _ = fit(None)
    (one, hist1), _, _ = fit(coopfit.Shard(1, 0, coopfit.LocalGather(1)))
    assert all(same(one[k], plain[k]) for k in NAMES) and np.array_equal(hist1, hist0)
    local = coopfit.LocalGather(2)
    (two, hist2), start, clip = fit(coopfit.Shard(2, 1, local))          # this process is rank 1 of the two it runs
    assert [s.tower(2).n_cls for s in local.states] == [3, 2] and all(s.steps == 4 for s in local.states)
    agree(local.states[0], local.states[1])
    want, hist = cocoopfit.fit_prompt_learner(f, y, m, c["ids"], start, logit_scale=math.log(clip.scale), shard=coopfit.Shard(2, 0, coopfit.LocalGather(2)), **opt)
    assert all(same(two[k], want[k]) for k in NAMES) and np.array_equal(hist2, hist) and np.isfinite(hist2).all()
    assert not all(same(two[k], plain[k]) for k in NAMES)
    with pytest.raises(ValueError, match="shard has no validation"):
        fit(coopfit.Shard(2, 0, coopfit.LocalGather(2)), val_loader=object())


def test_trainer_transform_route_under_a_local_gather():
    """``transform=``: decoded uint8 batches go transform -> image tower -> ``CoCoOpFitState.step``.  One shard gives the unsharded
    route's bits; with two, the run equals the hand-written loop over the two states."""
    import augment_ref as aref
    from clip_calibration_amd.augment import TrainPreprocess
    from clip_calibration_amd.preprocess import pack_images
    from clip_calibration_amd import trainers
    m, c = model("tiny"), cref.make_case("tiny", 5, 4, 2)
    imgs = [aref.synthetic_image(h, w, 70 + i) for i, (h, w) in enumerate([(80, 100), (64, 64)])]
    loader = [(pack_images(imgs).pin_memory(), torch.arange(2) % 5)]
    opt = dict(grad_scale=GRAD_SCALE, **SGD)

    def run_fit(shard):
        tp = TrainPreprocess.for_model(m, generator=torch.Generator().manual_seed(23))
        clip = trainers.CoCoOpCLIP(m, c["ids"], n_ctx=4)
        with torch.no_grad():
            for k, v in clip.prompt_learner.named_parameters():
                if k in NAMES:
                    v.copy_(c["params"][k])
        start = {k: v.detach().clone() for k, v in clip.prompt_learner.state_dict().items() if k in NAMES}
        return clip.fit_prompt_learner(loader, transform=tp, epochs=2, lr_per_epoch=RATES[:2], return_history=True, **opt,
                                       **({} if shard is None else {"shard": shard})), start, clip
    (plain, hist0), _, _ = run_fit(None)
    (one, hist1), _, _ = run_fit(coopfit.Shard(1, 0, coopfit.LocalGather(1)))
    assert all(same(one[k], plain[k]) for k in NAMES) and np.array_equal(hist1, hist0) and np.isfinite(hist0).all()
    local = coopfit.LocalGather(2)
    (two, hist2), start, clip = run_fit(coopfit.Shard(2, 0, local))
    assert all(s.steps == 2 for s in local.states)
    agree(local.states[0], local.states[1])
    tp = TrainPreprocess.for_model(m, generator=torch.Generator().manual_seed(23))
    loop = coopfit.LocalGather(2)
    states = [cocoopfit.CoCoOpFitState(m, c["ids"], start, logit_scale=math.log(clip.scale), shard=coopfit.Shard(2, r, loop), **opt) for r in range(2)]
    with torch.no_grad():
        want = [states[0].step(m.image_features_f32(tp(images)), lab, RATES[e], want_loss=True) for e in range(2) for images, lab in loader]
    assert all(same(two[k], states[1].params()[k]) for k in NAMES) and np.array_equal(hist2, torch.cat(want).cpu().numpy())


# ------------------------------------------------------------------------------------------------- 6. the RCCL gather, on one rank
def test_rccl_gather_with_one_rank_holds_the_local_bits():
    """``parallel.shard_gather`` on a one-rank communicator (this box may have one GPU; tests/test_gpu_cocoopshard_ranks.py runs two):
    clipmi_allgather moves every block of the step, and the bits are the local gather's -- SGD, dynamic and Adam."""
    from clip_calibration_amd import parallel
    key = ("tiny", 3, 4, 2)
    c = cref.make_case(*key)
    ex = parallel.EmbeddingExchange(torch.device("cuda", torch.cuda.current_device()), backend="rccl")
    try:
        assert ex.rccl_ranks == 1
        x, y, lr = c["feats"].cuda(), c["labels"].cuda(), torch.tensor(RATES, dtype=torch.float32).cuda()
        for route in ("sgd", "dynamic", "adam"):
            st = cocoopfit.CoCoOpFitState(model("tiny"), c["ids"], c["params"], logit_scale=ref.LOGIT_SCALE,
                                          shard=coopfit.Shard(1, 0, parallel.shard_gather(ex)), **SGD, **ROUTES[route])
            hist = torch.cat([st.step(x, y, lr[k:k + 1], want_loss=True) for k in range(3)]).cpu()
            (local,), want = run(key, 1, 3, **ROUTES[route])
            agree(st, local, route)
            assert same(hist, want)
    finally:
        ex.close()
