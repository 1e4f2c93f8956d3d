"""The class-sharded CoOp, KgCoOp and ProGrad fit on one GPU (clip_calibration_amd/coopfit.py ``shard=``, csrc/shard_train.hip): every case
runs the ranks of a ``LocalGather`` -- the kernels and the phase code of the multi-process run, device copies in the all-gather's place.
  1. G = 1 is the unsharded path bit for bit     2. G = 2, 3 with uneven and one-class shards     3. parity with the float64 oracle
  4. class-specific contexts     5. the new operators against tests/shardfit_ref.py     6. the trainers' pass-through
Batch 4, n_ctx 4, the synthetic ``tiny`` / ``tiny3`` text towers of the CoOp tests."""
import functools
import os

import numpy as np
import pytest
import torch

import coopfit_ref as ref
import promptfit_ref as pref
import shardfit_ref as sref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import coopfit, ops  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

FACTOR = 2.0                # profiles/coopfit_parity.txt's criterion: at most twice the fp16 reference's own error
GRAD_SCALE = 256.0          # as tests/test_gpu_coopfit.py: the synthetic weights give gradients far larger than ViT-B/16's
W = 8.0
RATES = [2e-3, 1e-3, 5e-4]
SGD = dict(momentum=0.9, dampening=0.0, nesterov=False, weight_decay=5e-4)
PARITY_LOG = os.environ.get("CLIPMI_SHARDFIT_PARITY")     # a file that receives the parity lines (profiles/shardfit_parity.txt is made so)


def say(line):
    print("shardfit-parity: " + line)
    if PARITY_LOG:
        with open(PARITY_LOG, "a") as f:
            f.write(line + "\n")


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def model(geom):
    return build_model(dict(ref.state_dict(geom)), {"trainer": "CoOp"}).cuda()


@functools.lru_cache(maxsize=None)
def case(geom, C, csc):
    c = dict(ref.make_case(geom, C, 4, 4, csc))
    c["teacher"] = pref.random_teacher(C, c["feats"].shape[1])
    return c


def method_args(c, method):
    return dict(method=method, teacher=c["teacher"].cuda() if method != "coop" else None, w=W, grad_scale=GRAD_SCALE)


def states_of(c, geom, method, G, **kw):
    """(the G shard states of one LocalGather, rank 0 first) -- or, with G = None, the one unsharded state."""
    m = model(geom)
    kw = dict(method_args(c, method), **SGD, **kw)
    if G is None:
        return [coopfit.CoOpFitState(m, c["ids"], c["ctx"], ref.LOGIT_SCALE, **kw)]
    local = coopfit.LocalGather(G)
    return [coopfit.CoOpFitState(m, c["ids"], c["ctx"], ref.LOGIT_SCALE, shard=coopfit.Shard(G, r, local), **kw) for r in range(G)]


def three_steps(c, geom, method, G, one_call=False):
    """(states, per-step losses [3]) after three steps at RATES."""
    states = states_of(c, geom, method, G)
    f, y, lr = c["feats"].cuda(), c["labels"].cuda(), torch.tensor(RATES, dtype=torch.float32).cuda()
    losses = [states[0].step(f, y, lr[k:k + 1], want_loss=True, one_call=one_call) for k in range(3)]
    assert all(s.steps == 3 for s in states)
    return states, torch.cat(losses).cpu()


def gradient(c, geom, method, shard, **kw):
    loss, grad, parts = coopfit.context_gradient(model(geom), c["ids"], c["ctx"], c["feats"].cuda(), c["labels"], ref.LOGIT_SCALE, return_parts=True,
                                                 shard=shard, **dict(method_args(c, method), **kw))
    return loss.cpu(), grad.cpu(), {k: v.cpu() for k, v in parts.items()}


# ---------------------------------------------------------------------------------------------------- 1. one shard: the unsharded bits
ANCHORS = [("coop", "tiny", False), ("coop", "tiny3", True), ("kgcoop", "tiny", False), ("prograd", "tiny3", False), ("prograd", "tiny", True)]


@pytest.mark.parametrize("method,geom,csc", ANCHORS, ids=ident)
def test_one_shard_is_the_unsharded_path_bit_for_bit(method, geom, csc):
    c = case(geom, 5, csc)
    loss0, grad0, parts0 = gradient(c, geom, method, None)
    loss1, grad1, parts1 = gradient(c, geom, method, coopfit.Shard(1, 0, coopfit.LocalGather(1)))
    assert torch.equal(loss1, loss0) and torch.equal(grad1, grad0) and grad1.shape == c["ctx"].shape and torch.isfinite(grad1).all()
    for k in parts1:
        assert torch.equal(parts1[k], parts0[k]), k
    (sharded,), hist = three_steps(c, geom, method, 1)
    assert not torch.equal(sharded.ctx.cpu(), c["ctx"])
    for one_call in (False, True):                                       # both routes of the unsharded step
        (plain,), want = three_steps(c, geom, method, None, one_call)
        assert torch.equal(hist, want)
        assert torch.equal(sharded.gathered_context(), plain.ctx) and torch.equal(sharded.ctx, plain.ctx) and torch.equal(sharded.buf, plain.buf)
    f = c["feats"].cuda()
    kw = dict(method_args(c, method), **SGD, epochs=3, batch_size=4, lr_per_epoch=RATES, return_history=True)
    ctx_f, hist_f = coopfit.fit_context(f, c["labels"], model(geom), c["ids"], c["ctx"], shard=coopfit.Shard(1, 0, coopfit.LocalGather(1)), **kw)
    assert torch.equal(ctx_f, sharded.ctx) and np.array_equal(hist_f, hist.numpy())
    with pytest.raises(ValueError, match="one_call"):
        sharded.step(f, c["labels"].cuda(), 1e-3, one_call=True)
    with pytest.raises(ValueError, match="no validation"):
        sharded.validate(f, c["labels"].cuda(), 0)


# ------------------------------------------------------------------------------------------- 2. uneven shards and shards of one class
SHARDED = [(m, G, C) for m in ("coop", "prograd") for G in (2, 3) for C in (5, G)]


@pytest.mark.parametrize("method,G,C", SHARDED, ids=ident)
def test_uneven_and_one_class_shards(method, G, C):
    c = case("tiny", C, False)
    local = coopfit.LocalGather(G)
    loss, grad, parts = gradient(c, "tiny", method, coopfit.Shard(G, 0, local))
    states = local.states
    assert [s.tower.C for s in states] == [hi - lo for lo, hi in sref.split(C, G)]
    # the full text-feature matrix behind the compaction: the shards' own features one after the other, on every rank
    own = torch.cat([s.tower.text for s in states])
    assert own.shape[0] == C and torch.isfinite(own).all()
    for s in states:
        assert torch.equal(s._text, own)
    # and each shard's rows are its own classes' features: the unsharded training forward over just those prompts, at the state's live-row
    # cut, is the same call on the same row count -- the same bits.  (That forward takes two prompts or more; a one-class shard runs the
    # slicing the others run.)
    for s, (lo, hi) in zip(states, sref.split(C, G)):
        if hi - lo >= 2:
            assert torch.equal(s.tower.text, coopfit.text_features(model("tiny"), c["ids"][lo:hi], c["ctx"], seq_rows=s.tower.rows))
    # the reduced gradient: the restatement's rank-ordered sum of the device's own partials
    inv = np.float32(1.0 / GRAD_SCALE)
    for s in states:
        assert torch.equal(s._all_part, states[0]._all_part)
    part = states[0]._all_part.cpu().numpy()                             # [G, 1 or 2, n_ctx, D]
    a = sref.rank_sum(part[:, 0]) * inv
    if method == "coop":
        assert np.array_equal(grad.numpy(), a)
    else:
        b = sref.rank_sum(part[:, 1]) * inv
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        assert np.allclose(parts["dots"].numpy(), [(a64 * a64).sum(), (b64 * b64).sum(), (a64 * b64).sum()], rtol=1e-12, atol=0)
        if int(parts["projected"]):
            k = np.float32(float(parts["dots"][2]) / float(parts["dots"][1]))
            a = (a - (k * b).astype(np.float32)).astype(np.float32)
        assert np.array_equal(grad.numpy(), a)
    # three steps: every shard state holds the same context and buffer bits, and a second run gives them again
    first, hist = three_steps(c, "tiny", method, G)
    for s in first[1:]:
        assert torch.equal(s.ctx, first[0].ctx) and torch.equal(s.buf, first[0].buf)
    assert torch.isfinite(first[0].ctx).all() and not torch.equal(first[0].ctx.cpu(), c["ctx"])
    again, hist2 = three_steps(c, "tiny", method, G)
    assert torch.equal(again[0].ctx, first[0].ctx) and torch.equal(again[0].buf, first[0].buf) and torch.equal(hist, hist2)


# ------------------------------------------------------------------------------------------------------------------------- 3. parity
@functools.lru_cache(maxsize=None)
def oracle():
    c = case("tiny", 5, False)
    args = (c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"], c["teacher"], W, 1.0)
    yard, how = pref.yardstick_parts(*args)
    want = pref.oracle_parts(*args)
    _, want["grad_coop"] = ref.oracle_loss_grad(*args[:5])
    yard["grad_coop"], how_c = ref.yardstick_grad(*args[:5])
    return c, want, yard, how if how == how_c else f"{how}/{how_c}"


@pytest.mark.parametrize("method", ["coop", "kgcoop", "prograd"])
def test_sharded_gradient_meets_the_parity_criterion(method):
    """G = 2, C = 5: the relative error against float64 autograd through the oracle is at most 2 x the fp16 reference's own
    (profiles/coopfit_parity.txt, promptfit_parity.txt).  ProGrad's decision is compared where the oracle's |cos(a, b)| >= 0.1."""
    c, want, yard, how = oracle()
    _, grad, parts = gradient(c, "tiny", method, coopfit.Shard(2, 0, coopfit.LocalGather(2)))
    if method != "prograd":
        g64, y = want["grad_" + method], ref.rel_fro(yard["grad_" + method], want["grad_" + method])
    else:
        g64, did = pref.project(want["grad_xe"], want["grad_kl"], 1.0)
        g16, _ = pref.project(yard["grad_xe"], yard["grad_kl"], 1.0)
        y, cos64 = ref.rel_fro(g16, g64), pref.cosine(want["grad_xe"], want["grad_kl"])
    e = ref.rel_fro(grad, g64)
    line = f"sharded gradient {method} tiny C=5 G=2 B=4 n_ctx=4: rel. Frobenius error {e:.3e}, yardstick ({how}) {y:.3e}, ratio {e / y:.2f}"
    if method == "prograd":
        line += f"; float64 cos(a, b) {cos64:+.4f}, projected {int(parts['projected'])} (oracle {int(did)})"
    say(line)
    assert torch.isfinite(grad).all() and e <= FACTOR * y
    if method == "prograd" and abs(cos64) >= pref.MIN_ABS_COS:
        assert int(parts["projected"]) == int(did)


# ------------------------------------------------------------------------------------------------------- 4. class-specific contexts
@functools.lru_cache(maxsize=None)
def csc_oracle():
    c = case("tiny3", 5, True)
    args = (c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"])
    return (ref.oracle_loss_grad(*args)[1],) + ref.yardstick_grad(*args)


@pytest.mark.parametrize("method,G", [("coop", 2), ("coop", 3), ("prograd", 2), ("prograd", 3)], ids=ident)
def test_class_specific_shards_step_their_own_rows(method, G):
    c = case("tiny3", 5, True)
    states, hist = three_steps(c, "tiny3", method, G)
    full = states[0].gathered_context()
    assert full.shape == c["ctx"].shape and torch.isfinite(full).all() and torch.isfinite(hist).all()
    for r, (lo, hi) in enumerate(sref.split(5, G)):
        assert states[r].ctx.shape[0] == hi - lo and torch.equal(full[lo:hi], states[r].ctx)       # the rows of the shards put together
        assert torch.equal(states[r].gathered_context(), full)
        assert not torch.equal(states[r].ctx.cpu(), c["ctx"][lo:hi])                               # every class's rows moved
    if method == "prograd":                                                                        # every rank decided alike
        for s in states[1:]:
            assert torch.equal(s._all_dots, states[0]._all_dots)
    again, hist2 = three_steps(c, "tiny3", method, G)
    assert torch.equal(again[0].gathered_context(), full) and torch.equal(hist, hist2)
    # the gathered gradient has the whole context's shape, every class's rows in their place: CoOp's meets the parity criterion
    _, grad, _ = gradient(c, "tiny3", method, coopfit.Shard(G, 0, coopfit.LocalGather(G)))
    assert grad.shape == c["ctx"].shape and torch.isfinite(grad).all()
    if method == "coop":
        g64, g16, how = csc_oracle()
        e, y = ref.rel_fro(grad, g64), ref.rel_fro(g16, g64)
        say(f"sharded gradient coop class-specific tiny3 C=5 G={G} B=4 n_ctx=4: rel. Frobenius error {e:.3e}, yardstick ({how}) {y:.3e}, ratio {e / y:.2f}")
        assert e <= FACTOR * y


# ------------------------------------------------------------------------------------------------------------------ 5. the operators
@pytest.mark.parametrize("C,G,E", [(13, 8, 70), (8, 8, 1), (5, 2, 300), (1000, 3, 5)])
def test_shard_compact(C, G, E):
    """Rows of 70 floats: every rank's range starts and ends inside a workgroup's span of 256 elements.  The padding rows are NaN and
    must never be read."""
    rng = np.random.RandomState(0)
    full = rng.standard_normal((C, E)).astype(np.float32)
    gathered = sref.padded([full[lo:hi] for lo, hi in sref.split(C, G)])
    assert np.isnan(gathered).any() == (C % G != 0)
    out = ops.shard_compact(torch.from_numpy(gathered).cuda(), C).cpu().numpy()
    assert np.array_equal(out, sref.compact(gathered, C)) and np.array_equal(out, full)
    with pytest.raises(ValueError, match="shard_compact"):
        ops.shard_compact(torch.zeros(G, -(-C // G) + 1, E).cuda(), C)


def cancelling_stream(C, L, D, seed):
    """d_embed [C * L, D]: random rows, but for a large and a tiny value per class in two columns, so that a wrong order shows."""
    rng = np.random.RandomState(seed)
    g = rng.standard_normal((C, L, D)).astype(np.float32)
    big = np.float32(2.0 ** 24) * np.where(np.arange(C) % 2 == 0, 1, -1).astype(np.float32)
    g[:, :, 0] = big[:, None]
    g[:, :, 1] = np.float32(1.0)
    g[:, :, 2] = big[:, None] + np.arange(C, dtype=np.float32)[:, None]
    return g.reshape(C * L, D)


@pytest.mark.parametrize("C,L,n_ctx,D", [(1, 5, 4, 64), (3, 7, 4, 100), (6, 9, 2, 129)])
def test_ctx_partial(C, L, n_ctx, D):
    g = cancelling_stream(C, L, D, 1)
    out = ops.ctx_partial(torch.from_numpy(g).cuda(), C, n_ctx).cpu().numpy()
    assert np.array_equal(out, sref.chain_sum(g.reshape(C, L, D)[:, 1:1 + n_ctx]))


@pytest.mark.parametrize("G,n_ctx,D", [(1, 4, 64), (3, 4, 100), (8, 2, 129)])
def test_ctx_step_gathered(G, n_ctx, D):
    rng = np.random.RandomState(2)
    parts = rng.standard_normal((G, n_ctx, D)).astype(np.float32)
    big = np.float32(2.0 ** 24) * np.where(np.arange(G) % 2 == 0, 1, -1).astype(np.float32)
    parts[:, :, 0] = big[:, None]                                        # one large value per rank and, in the next, a tiny one beside it
    parts[:, :, 1] = (big + np.arange(G, dtype=np.float32))[:, None]
    parts[1:, :, 2] = np.float32(2.0 ** -20)
    parts[0, :, 2] = np.float32(2.0 ** 24)
    parts[:, :, 3] = np.array([2.0 ** 24, 1.0, -2.0 ** 24], np.float32)[np.arange(G) % 3][:, None]   # 0 in rank order, 1 in the reverse
    d = torch.from_numpy(parts).cuda()
    want = (sref.rank_sum(parts) * np.float32(1 / 256.0)).astype(np.float32)
    grad = ops.ctx_step_gathered(d.view(G, -1), n_ctx, D, 256.0).cpu().numpy()
    assert np.array_equal(grad, want)
    if G == 3:
        assert not np.array_equal(want, (sref.rank_sum(parts[::-1]) * np.float32(1 / 256.0)).astype(np.float32))   # the order shows
    # the step: lr = 0.5 makes the product exact, so the fused multiply-add is one rounded fp32 subtraction
    ctx0 = rng.standard_normal((n_ctx, D)).astype(np.float32)
    ctx = torch.from_numpy(ctx0).cuda()
    ops.ctx_step_gathered(d.view(G, -1), n_ctx, D, 256.0, ctx, None, torch.tensor([0.5]).cuda(), True, want_grad=False)
    assert np.array_equal(ctx.cpu().numpy(), ctx0 - np.float32(0.5) * want)
    # a padded rank stride: the elements behind a rank's partial are never read
    wide = torch.full((G, n_ctx * D + 3), float("nan")).cuda()
    wide[:, :n_ctx * D] = d.view(G, -1)
    assert np.array_equal(ops.ctx_step_gathered(wide, n_ctx, D, 256.0).cpu().numpy(), want)


@pytest.mark.parametrize("C,L,n_ctx,D", [(3, 7, 4, 100), (37, 6, 4, 128)])
def test_partial_and_gathered_step_with_one_rank_are_ctx_step(C, L, n_ctx, D):
    """The anchor at operator level: two steps with momentum, weight decay and Nesterov through both routes, the same bits."""
    g = torch.from_numpy(cancelling_stream(C, L, D, 3)).cuda()
    rng = np.random.RandomState(4)
    ctx_a = torch.from_numpy(rng.standard_normal((n_ctx, D)).astype(np.float32)).cuda()
    ctx_b, buf_a, buf_b = ctx_a.clone(), torch.zeros_like(ctx_a), torch.zeros_like(ctx_a)
    lr = torch.tensor([0.01]).cuda()
    for first in (True, False):
        ga = ops.ctx_step(g, C, n_ctx, False, 256.0, ctx_a, buf_a, lr, first, 0.9, 0.0, 5e-4, True)
        part = ops.ctx_partial(g, C, n_ctx)
        gb = ops.ctx_step_gathered(part.view(1, -1), n_ctx, D, 256.0, ctx_b, buf_b, lr, first, 0.9, 0.0, 5e-4, True)
        assert torch.equal(ga, gb) and torch.equal(ctx_a, ctx_b) and torch.equal(buf_a, buf_b)
        g = g * 0.5


@pytest.mark.parametrize("per_class,G", [(False, 1), (False, 3), (True, 1), (True, 3)])
def test_sharded_prograd_operators(per_class, G):
    """ProGrad's two calls: with one rank ``prograd_step``'s bits; with three the dots are the rank-ordered float64 sums and the decision
    and the step follow them.  b = -a + noise: the gradients conflict and the projection is taken."""
    C, L, n_ctx, D, lam = 6, 7, 4, 100, 0.5
    rng = np.random.RandomState(5)
    ga = rng.standard_normal((C * L, D)).astype(np.float32)
    gb = (-ga + 0.5 * rng.standard_normal((C * L, D))).astype(np.float32)
    da, db = torch.from_numpy(ga).cuda(), torch.from_numpy(gb).cuda()
    lr, sgd = torch.tensor([0.01]).cuda(), (0.9, 0.0, 5e-4, False)
    shape = (C, n_ctx, D) if per_class else (n_ctx, D)
    ctx0 = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()
    if G == 1:
        ctx_a, buf_a = ctx0.clone(), torch.zeros_like(ctx0)
        want = ops.prograd_step(da, db, C, n_ctx, per_class, 256.0, lam, ctx_a, buf_a, lr, True, *sgd)
        ws = ops.shard_prograd_workspace(ctx0.numel(), ctx0.device)
        if per_class:
            dots = ops.shard_prograd_dots(da, db, C, n_ctx, True, 256.0, ws)
        else:
            both = torch.stack([ops.ctx_partial(da, C, n_ctx), ops.ctx_partial(db, C, n_ctx)]).unsqueeze(0).contiguous()      # [1, 2, n_ctx, D]
            dots = ops.shard_prograd_dots(both[:, 0], both[:, 1], 1, n_ctx, False, 256.0, ws)
        ctx_b, buf_b = ctx0.clone(), torch.zeros_like(ctx0)
        got = ops.shard_prograd_apply(dots.view(1, 3), lam, ws, shape, ctx_b, buf_b, lr, True, *sgd)
        assert int(want[1]) == 1
        for x, y in zip(got, want):
            assert torch.equal(x, y)
        assert torch.equal(ctx_a, ctx_b) and torch.equal(buf_a, buf_b)
        return
    bounds = sref.split(C, G)
    inv = np.float32(1 / 256.0)
    if per_class:        # every rank's own rows, its own dots; all ranks' dots added in rank order
        wss = [ops.shard_prograd_workspace((hi - lo) * n_ctx * D, ctx0.device) for lo, hi in bounds]
        dots = torch.stack([ops.shard_prograd_dots(da[lo * L:hi * L], db[lo * L:hi * L], hi - lo, n_ctx, True, 256.0, ws) for (lo, hi), ws in zip(bounds, wss)])
        a = ga.reshape(C, L, D)[:, 1:1 + n_ctx] * inv
        b = gb.reshape(C, L, D)[:, 1:1 + n_ctx] * inv
        sums = np.zeros(3)
        for r, (lo, hi) in enumerate(bounds):
            x, y = a[lo:hi].astype(np.float64), b[lo:hi].astype(np.float64)
            assert np.allclose(dots[r].cpu().numpy(), [(x * x).sum(), (y * y).sum(), (x * y).sum()], rtol=1e-12, atol=0)
            sums = sums + dots[r].cpu().numpy()                          # rank order, float64
        outs = [ops.shard_prograd_apply(dots, lam, ws, (hi - lo, n_ctx, D)) for (lo, hi), ws in zip(bounds, wss)]
        grad = torch.cat([o[0] for o in outs]).cpu().numpy()
    else:
        both = torch.stack([torch.stack([ops.ctx_partial(da[lo * L:hi * L], hi - lo, n_ctx), ops.ctx_partial(db[lo * L:hi * L], hi - lo, n_ctx)])
                            for lo, hi in bounds])                       # [G, 2, n_ctx, D]
        ws = ops.shard_prograd_workspace(n_ctx * D, ctx0.device)
        dots = ops.shard_prograd_dots(both[:, 0], both[:, 1], 1, n_ctx, False, 256.0, ws).view(1, 3)
        a = sref.reduced_gradient(ga.reshape(C, L, D)[:, 1:1 + n_ctx], G, 256.0)
        b = sref.reduced_gradient(gb.reshape(C, L, D)[:, 1:1 + n_ctx], G, 256.0)
        x, y = a.astype(np.float64), b.astype(np.float64)
        assert np.allclose(dots[0].cpu().numpy(), [(x * x).sum(), (y * y).sum(), (x * y).sum()], rtol=1e-12, atol=0)
        sums = dots[0].cpu().numpy()
        outs = [ops.shard_prograd_apply(dots, lam, ws, shape)]
        grad = outs[0][0].cpu().numpy()
    for o in outs:
        assert int(o[1]) == 1 and np.array_equal(o[2].cpu().numpy(), sums)
    k = np.float32(lam * (sums[2] / sums[1]))
    assert np.array_equal(grad, (a - (k * b).astype(np.float32)).astype(np.float32).reshape(grad.shape))


# ------------------------------------------------------------------------------------------------------------------ 6. the trainers
def trainer(which, m, ids):
    from clip_calibration_amd import synthetic as syn
    from clip_calibration_amd.trainers import coop, kgcoop, prograd
    if which == "coop":
        return coop.CustomCLIP(m, ids, n_ctx=4)
    return {"kgcoop": kgcoop, "prograd": prograd}[which].CustomCLIP(m, ids, zeroshot_tokenized_prompts=syn.synthetic_token_ids(ids.shape[0], "tiny", seed=7),
                                                                     n_ctx=4)


def fit_trainer(which, shard, **kw):
    """The trainer's ``fit_context`` on the cached route; the loader's "images" are the features themselves, passed through by a stand-in for
    the image tower (tests/test_gpu_promptfit.py).  Returns (fitted context, history, the trainer)."""
    m = model("tiny")
    c = case("tiny", 5, False)
    clip = trainer(which, m, c["ids"])
    try:
        m.image_features_f32 = lambda image: image
        fitted, hist = clip.fit_context([(c["feats"].cuda(), c["labels"])], epochs=3, lr_per_epoch=RATES, batch_size=4, grad_scale=GRAD_SCALE,
                                        return_history=True, **SGD, **({} if shard is None else {"shard": shard}), **kw)
    finally:
        del m.image_features_f32
    return fitted, hist, clip


@pytest.mark.parametrize("which", ["coop", "kgcoop", "prograd"])
def test_trainers_pass_the_shard_on(which):
    plain, hist0, _ = fit_trainer(which, None)
    one, hist1, _ = fit_trainer(which, coopfit.Shard(1, 0, coopfit.LocalGather(1)))
    assert torch.equal(one, plain) and np.array_equal(hist1, hist0)                       # one shard: the trainer's unsharded fit, bit for bit
    local = coopfit.LocalGather(2)
    two, hist2, clip = fit_trainer(which, coopfit.Shard(2, 1, local))                     # this process is rank 1 of the two it runs
    assert [s.tower.C for s in local.states] == [3, 2] and all(s.steps == 3 for s in local.states)
    assert torch.equal(local.states[0].ctx, local.states[1].ctx) and torch.equal(two, local.states[1].ctx)
    assert np.isfinite(hist2).all() and len(hist2) == 3 and not torch.equal(two, plain)
    assert torch.equal(clip.prompt_learner.ctx.detach().float(), two.to(clip.prompt_learner.ctx.dtype).float())
    with pytest.raises(ValueError, match="must not be stepped as well"):                   # the driver is rank 1's state
        local.states[0].step(case("tiny", 5, False)["feats"].cuda(), case("tiny", 5, False)["labels"].cuda(), 1e-3)
    # a validation loader under shard is refused before either tower runs: this loader cannot be iterated
    with pytest.raises(ValueError, match="shard has no validation"):
        fit_trainer(which, coopfit.Shard(2, 0, coopfit.LocalGather(2)), val_loader=object())


def test_trainer_transform_route_under_a_local_gather():
    """``transform=``: decoded uint8 batches go transform -> image tower -> ``CoOpFitState.step``.  One shard gives the unsharded route's
    bits; with two, the one call makes and steps both ranks' states."""
    import augment_ref as aref
    from clip_calibration_amd.augment import TrainPreprocess
    from clip_calibration_amd.preprocess import pack_images
    m = model("tiny")
    ids = case("tiny", 5, False)["ids"]
    imgs = [aref.synthetic_image(h, w, 70 + i) for i, (h, w) in enumerate([(80, 100), (64, 64), (70, 51), (120, 90)])]
    loader = [(pack_images(imgs).pin_memory(), torch.arange(4) % 5)]

    def run(shard):
        tp = TrainPreprocess.for_model(m, generator=torch.Generator().manual_seed(23))
        return trainer("coop", m, ids).fit_context(loader, transform=tp, epochs=2, lr_per_epoch=RATES[:2], grad_scale=GRAD_SCALE, return_history=True, **SGD,
                                                   **({} if shard is None else {"shard": shard}))
    plain, hist0 = run(None)
    one, hist1 = run(coopfit.Shard(1, 0, coopfit.LocalGather(1)))
    assert torch.equal(one, plain) and np.array_equal(hist1, hist0) and np.isfinite(hist0).all()
    local = coopfit.LocalGather(2)
    two, hist2 = run(coopfit.Shard(2, 0, local))
    assert all(s.steps == 2 for s in local.states) and torch.equal(local.states[0].ctx, local.states[1].ctx) and torch.equal(two, local.states[0].ctx)
    assert np.isfinite(hist2).all() and not torch.equal(two, plain)


# ------------------------------------------------------------------------------------------------- 7. the RCCL gather, on one rank
def test_rccl_gather_with_one_rank_holds_the_local_bits():
    """``parallel.shard_gather`` on a one-rank communicator (this box may have one GPU; tests/test_gpu_shardfit_ranks.py runs two):
    clipmi_allgather moves every block of the step, and the bits are the local gather's -- the unsharded path's."""
    from clip_calibration_amd import parallel
    c = case("tiny", 5, False)
    ex = parallel.EmbeddingExchange(torch.device("cuda", torch.cuda.current_device()), backend="rccl")
    try:
        assert ex.rccl_ranks == 1
        f, y, lr = c["feats"].cuda(), c["labels"].cuda(), torch.tensor(RATES, dtype=torch.float32).cuda()
        for method in ("coop", "prograd"):
            kw = dict(method_args(c, method), **SGD)
            st = coopfit.CoOpFitState(model("tiny"), c["ids"], c["ctx"], ref.LOGIT_SCALE, shard=coopfit.Shard(1, 0, parallel.shard_gather(ex)), **kw)
            hist = torch.cat([st.step(f, y, lr[k:k + 1], want_loss=True) for k in range(3)]).cpu()
            (local,), want = three_steps(c, "tiny", method, 1)
            assert torch.equal(hist, want) and torch.equal(st.ctx, local.ctx) and torch.equal(st.buf, local.buf)
    finally:
        ex.close()
