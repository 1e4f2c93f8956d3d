"""The batch-sharded VPT, MaPLe, PromptSRC and IVLP fits on one GPU (``shard=`` on clip_calibration_amd/vptfit.py, maplefit.py,
promptsrcfit.py; csrc/shard_train.hip): every case runs the ranks of a ``coopfit.LocalGather`` -- the kernels and the phase code of the
multi-process run, device copies in the all-gather's place.
  1. G = 1 is the unsharded state bit for bit     2. G = 2, 4: every rank holds the same bits, and so does a second run
  3. parity of the reduced gradient with the float64 oracle of the whole batch     4. the dynamic scale     5. refusals
Batch 4 on the synthetic ``tiny`` / ``tiny3`` towers of the fits' own tests.  The parity lines start with "batchshard-parity:";
profiles/batchshard_parity.txt is one run's lines (CLIPMI_BATCHSHARD_PARITY names a file that receives them)."""
import functools
import math
import os

import pytest
import torch

import maplefit_ref
import promptsrcfit_ref
import vptfit_ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import coopfit, maplefit, promptsrcfit, vptfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

FACTOR = 2.0                # the fits' own criterion: at most twice the fp16 reference's own error against float64
RATES = [2e-3, 1e-3, 5e-4, 2e-3]
SGD = dict(momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=False)
PARITY_LOG = os.environ.get("CLIPMI_BATCHSHARD_PARITY")
FITS = ["vpt", "maple", "promptsrc", "ivlp"]


def say(line):
    print("batchshard-parity: " + line)
    if PARITY_LOG:
        with open(PARITY_LOG, "a") as f:
            f.write(line + "\n")


def same(a, b):
    return a.shape == b.shape and a.contiguous().view(torch.int32).equal(b.contiguous().view(torch.int32))


class Fit:
    """One fit on one small case of batch 4: how to make its state and read its master block."""

    def __init__(self, name):
        self.name = name
        if name == "vpt":
            c = vptfit_ref.make_case("tiny", 2, 2, 4, 5)
            m = build_model(dict(c["sd"]), {"trainer": "VPT", "vision_depth": 2, "vision_ctx": 2, "language_depth": 0, "language_ctx": 0}).cuda()
            self.default = vptfit.DEFAULT_GRAD_SCALE
            self.make = lambda **kw: vptfit.VPTFitState(m, c["text"].cuda(), vptfit_ref.LOGIT_SCALE, c["prompts"], **SGD, **kw)
            self.block = lambda st: st.prompts
        elif name == "maple":
            c = maplefit_ref.make_case("tiny3", 2, 1, 5, 4)
            m = build_model(dict(c["sd"]), maplefit_ref.design(1)).cuda()
            rows = maplefit_ref.live_rows(c["ids"], False)
            self.default = maplefit.DEFAULT_GRAD_SCALE
            self.make = lambda **kw: maplefit.MaPLeFitState(m, c["ids"], c["pl"], maplefit_ref.LOGIT_SCALE, seq_rows=rows, **SGD, **kw)
            self.block = lambda st: st.block
        else:
            c = promptsrcfit_ref.make_case("tiny", 2, 2, 3, 2, 3, 4)
            m = build_model(dict(c["sd"]), promptsrcfit_ref.design(3, 2, 2, 2)).cuda()
            rows = promptsrcfit_ref.live_rows(c["ids"], True)
            self.default = promptsrcfit.DEFAULT_GRAD_SCALE
            self.make = lambda **kw: promptsrcfit.PromptSRCFitState(m, c["ids"], c["p"], c["teacher"].cuda(), promptsrcfit_ref.LOGIT_SCALE, seq_rows=rows,
                                                                    method=name, **SGD, **kw)
            self.block = lambda st: st.block
        self.batch = (c["images"].cuda(), c["labels"].cuda())

    def states(self, G, **kw):
        """The G shard states of one LocalGather, rank 0 first -- or, with G = None, the one unsharded state."""
        if G is None:
            return [self.make(**kw)]
        local = coopfit.LocalGather(G)
        return [self.make(shard=coopfit.Shard(G, r, local), **kw) for r in range(G)]

    def run(self, G, steps, first=0, **kw):
        """``steps`` steps on the batch at RATES[first:], driven through rank 0's state: (states, the steps' returned losses)."""
        states = self.states(G, **kw)
        lr = torch.tensor(RATES, dtype=torch.float32).cuda()
        x, y = self.batch
        losses = [states[0].step(x, y, lr[k:k + 1], want_loss=True) for k in range(first, first + steps)]
        torch.cuda.synchronize()
        assert all(s.steps == steps for s in states)
        return states, torch.cat(losses).cpu()

    def bits(self, st):
        """Everything a step leaves in a state: block, buffer or moments, the last step's losses."""
        out = {"block": self.block(st), "losses": st.last_losses}
        if st.buf is not None:
            out["buf"] = st.buf
        if st._adam is not None:
            out["exp_avg"], out["exp_avg_sq"] = st._adam.exp_avg, st._adam.exp_avg_sq
        return {k: v.detach().cpu().clone() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def fit(name):
    return Fit(name)


def equal_bits(a, b):
    return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)


def scale_args(f, dynamic):
    return dict(grad_scale="dynamic", scaler={"init_scale": f.default, "growth_interval": 1000}) if dynamic else dict(grad_scale=f.default)


# ---------------------------------------------------------------------------------------------------- 1. one rank: the unsharded bits
@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
@pytest.mark.parametrize("optimizer", ["sgd", "adam", "adamw"])
@pytest.mark.parametrize("name", FITS)
def test_one_rank_is_the_unsharded_state_bit_for_bit(name, optimizer, dynamic):
    """Three steps: block, buffer or moments, the losses of every step and scaler_state()."""
    f = fit(name)
    kw = dict(scale_args(f, dynamic), optimizer=optimizer)
    (plain,), want = f.run(None, 3, **kw)
    (one,), got = f.run(1, 3, **kw)
    assert torch.isfinite(f.block(plain)).all() and not same(f.block(plain), f.block(f.make(**kw)))
    assert same(got, want) and equal_bits(f.bits(one), f.bits(plain))
    if dynamic:
        assert one.scaler_state() == plain.scaler_state() == {"scale": f.default, "growth_tracker": 3, "skipped_steps": 0, "applied_steps": 3, "found_inf": 0}


# ------------------------------------------------------------------------------------------------------------- 2. the ranks agree
@pytest.mark.parametrize("how", ["sgd-static", "adam-dynamic"])
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("name", FITS)
def test_every_rank_ends_with_the_same_bits(name, G, how):
    """Batch 4 over two ranks and over four (one image per rank): every rank's block, buffer or moments and losses are the same bits as
    rank 0's and as a second run's; the parameters moved and differ from the unsharded run's (another summation order)."""
    f = fit(name)
    kw = dict(scale_args(f, how == "adam-dynamic"), optimizer=how.split("-")[0])
    states, hist = f.run(G, 3, **kw)
    first = [f.bits(s) for s in states]
    for b in first[1:]:
        assert equal_bits(b, first[0])
    assert torch.isfinite(first[0]["block"]).all() and torch.isfinite(hist).all()
    assert not same(first[0]["block"], f.block(f.make(**kw)).cpu())
    again, hist2 = f.run(G, 3, **kw)
    assert same(hist, hist2) and all(equal_bits(f.bits(s), first[0]) for s in again)
    if how == "adam-dynamic":
        assert all(s.scaler_state() == states[0].scaler_state() for s in states) and states[0].scaler_state()["applied_steps"] == 3
    (plain,), want = f.run(None, 3, **kw)
    assert float((hist - want).abs().max()) <= 1e-2 * float(want.abs().max())      # the same fit up to fp16 operands and summation order


# ------------------------------------------------------------------------------------------------------------------------- 3. parity
def test_vpt_sharded_gradient_meets_the_parity_criterion():
    """G = 2 on tests/test_gpu_vptfit.py's batch-4 case: gradient within 2 x the fp16 reference's own error against float64 autograd
    of the WHOLE batch, the loss within 2 x that reference's loss error plus two fp32 ulps."""
    ref = vptfit_ref
    geom, n_ctx, depth, B, C = ref.GPU_CASES[1]
    assert B == 4
    c = ref.make_case(geom, n_ctx, depth, B, C)
    m = build_model(dict(c["sd"]), {"trainer": "VPT", "vision_depth": depth, "vision_ctx": n_ctx, "language_depth": 0, "language_ctx": 0}).cuda()
    loss64, grad64 = ref.oracle_loss_grad(c["sd"], c["images"], c["prompts"], c["text"], c["labels"])
    loss16, grad16, how = ref.yardstick(c["sd"], c["images"], c["prompts"], c["text"], c["labels"])
    loss, grad = vptfit.prompt_gradient(m, c["prompts"], c["images"].cuda(), c["labels"], c["text"].cuda(), ref.LOGIT_SCALE,
                                        shard=coopfit.Shard(2, 0, coopfit.LocalGather(2)))
    loss, grad = float(loss.cpu()), grad.cpu().double()
    yard, err = ref.rel_fro(grad16, grad64), ref.rel_fro(grad, grad64)
    lyard, lerr = abs(float(loss16 - loss64)), abs(loss - float(loss64))
    say(f"vpt {geom} n_ctx={n_ctx} depth={depth} B={B} C={C} G=2: grad device {err:.3e} yardstick({how}) {yard:.3e} ratio {err / yard:.2f}; "
        f"loss device {lerr:.3e} yardstick {lyard:.3e}")
    assert torch.isfinite(grad).all() and grad.shape == c["prompts"].shape
    assert err <= FACTOR * yard
    assert lerr <= FACTOR * lyard + 2.0 ** -22 * abs(float(loss64))


def test_maple_sharded_gradients_meet_the_parity_criterion():
    """G = 2, batch 4, depth 3 on tiny3 with the live-row cut: every parameter's gradient within 2 x the fp16 reference's own error; the
    loss within tests/test_gpu_maplefit.py's bound, 2 x (2 x the reference's largest fp16 logit error) + 1e-5 |loss|."""
    ref = maplefit_ref
    geom, depth, n_ctx, C, B = "tiny3", 3, 3, 3, 4
    c = ref.make_case(geom, depth, n_ctx, C, B)
    m = build_model(dict(c["sd"]), ref.design(n_ctx)).cuda()
    loss64, grad64, z64 = ref.oracle_loss_grads(c["sd"], c["ids"], c["pl"], c["images"], c["labels"], return_logits=True)
    loss16, grad16, how, z16 = ref.yardstick(c["sd"], c["ids"], c["pl"], c["images"], c["labels"])
    loss, grads = maplefit.gradients(m, c["pl"], c["images"].cuda(), c["labels"], c["ids"], ref.LOGIT_SCALE, seq_rows=ref.live_rows(c["ids"], True),
                                     shard=coopfit.Shard(2, 1, coopfit.LocalGather(2)))
    lerr, zyard = abs(float(loss.cpu()) - float(loss64)), float((z16 - z64).abs().max())
    say(f"maple {geom} depth={depth} n_ctx={n_ctx} C={C} B={B} G=2: loss device {lerr:.3e} bound {2 * FACTOR * zyard + 1e-5 * abs(float(loss64)):.3e} "
        f"(yardstick {how})")
    fails = []
    for name in ref.param_names(depth):
        got, want = grads[name].cpu().double(), grad64[name]
        assert torch.isfinite(got).all() and float(want.norm()) > 0, name
        yard, err = ref.rel_fro(grad16[name], want), ref.rel_fro(got, want)
        say(f"  maple {name}: device {err:.3e} yardstick {yard:.3e} ratio {err / yard:.2f}")
        if err > FACTOR * yard:
            fails.append((name, err, yard))
    assert not fails, fails
    assert lerr <= 2 * FACTOR * zyard + 1e-5 * abs(float(loss64))


@pytest.mark.parametrize("method,wname", [("promptsrc", "text"), ("ivlp", "ivlp")])
def test_promptsrc_sharded_gradients_meet_the_parity_criterion(method, wname):
    """G = 2, batch 4 on tests/test_gpu_promptsrcfit.py's end-to-end construction (its condition on the L1 signs asserted): every
    parameter's gradient within 2 x the fp16 reference's own error.  The total loss is printed, as that test prints it; for IVLP, whose
    loss is the cross-entropy alone, it is held to MaPLe's bound as well."""
    ref = promptsrcfit_ref
    geom, dt, dv, nt, nv, C, B = "tiny", 2, 2, 2, 3, 5, 4
    c = ref.e2e_case(geom, dt, dv, nt, nv, C, B, ref.E2E_WEIGHTS[wname], 0)
    assert c["margin"] >= 4 * c["feature_error"]
    m = build_model(dict(c["sd"]), ref.design(nt, dt, nv, dv)).cuda()
    losses, grads = promptsrcfit.gradients(m, c["p"], c["images"].cuda(), c["labels"], c["ids"], c["teacher"].cuda(), ref.LOGIT_SCALE, *c["weights"],
                                           seq_rows=ref.live_rows(c["ids"], False), method=method, shard=coopfit.Shard(2, 0, coopfit.LocalGather(2)))
    assert losses.shape == (5,)
    lerr, lyard = abs(float(losses[0].cpu()) - float(c["loss64"][0])), abs(float(c["loss16"][0] - c["loss64"][0]))
    zyard = float((c["ex16"]["z"] - c["ex64"]["z"]).abs().max())
    say(f"{method} {geom} depths=({dt},{dv}) n=({nt},{nv}) C={C} B={B} weights={wname} G=2: total loss device {lerr:.3e} own fp16 draw {lyard:.3e} "
        f"(yardstick {c['how']})")
    fails = []
    for name in ref.param_names(dt, dv):
        got, want = grads[name].cpu().double(), c["grad64"][name]
        assert torch.isfinite(got).all() and float(want.norm()) > 0, name
        yard, err = ref.rel_fro(c["grad16"][name], want), ref.rel_fro(got, want)
        say(f"  {method} {name}: device {err:.3e} yardstick {yard:.3e} ratio {err / yard:.2f}")
        if err > FACTOR * yard:
            fails.append((name, err, yard))
    assert not fails, fails
    if method == "ivlp":
        assert lerr <= 2 * FACTOR * zyard + 1e-5 * abs(float(c["loss64"][0]))


# -------------------------------------------------------------------------------------------------------------- 4. the dynamic scale
@functools.lru_cache(maxsize=None)
def overflow_scale(name):
    """tests/test_gpu_blockscaler.py's search: the smallest power of two >= the default at which one unsharded static step leaves a
    non-finite block."""
    f, scale = fit(name), fit(name).default
    for _ in range(40):
        if not torch.isfinite(f.block(f.run(None, 1, grad_scale=scale)[0][0])).all():
            return scale
        scale *= 2.0
    raise AssertionError("no power of two up to 2^40 times the default overflows fp16 on this case")


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("name", FITS)
def test_every_rank_skips_the_same_step(name, optimizer):
    """G = 2 from the scale at which the unsharded fit overflows, backoff 2^-4: step 1 is skipped on every rank (block unchanged, buffer
    or moments zero, the same scaler_state()); steps 2 .. 4 are applied and equal, bit for bit, a G = 2 static run of three steps at the
    backed-off scale on the same rates -- under Adam too, so the skipped step was not one of Adam's steps."""
    f, scale = fit(name), overflow_scale(name)
    kw = dict(grad_scale="dynamic", scaler={"init_scale": scale, "backoff_factor": 2.0 ** -4, "growth_interval": 1000}, optimizer=optimizer)
    start = f.block(f.make(grad_scale=f.default)).cpu().clone()
    states, _ = f.run(2, 1, **kw)
    for s in states:
        assert s.scaler_state() == {"scale": scale / 16.0, "growth_tracker": 0, "skipped_steps": 1, "applied_steps": 0, "found_inf": 1}
        b = f.bits(s)
        assert same(b["block"], start) and all(not v.any() for k, v in b.items() if k in ("buf", "exp_avg", "exp_avg_sq"))
    states, hist = f.run(2, 4, **kw)
    for s in states:
        assert s.scaler_state() == {"scale": scale / 16.0, "growth_tracker": 3, "skipped_steps": 1, "applied_steps": 3, "found_inf": 0}
        assert equal_bits(f.bits(s), f.bits(states[0]))
    static, want = f.run(2, 3, first=1, grad_scale=scale / 16.0, optimizer=optimizer)
    assert torch.isfinite(f.block(static[0])).all()
    assert equal_bits(f.bits(states[0]), f.bits(static[0])) and same(hist[1:], want)


# ------------------------------------------------------------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("name", FITS)
def test_refusals_by_name(name):
    f = fit(name)
    x, y = f.batch
    states = f.states(2, grad_scale=f.default)
    with pytest.raises(ValueError, match="one_call=True"):
        states[0].step(x, y, 1e-3, one_call=True)
    with pytest.raises(ValueError, match=r"B=3 images does not split over G=2"):
        states[0].step(x[:3], y[:3], 1e-3)
    with pytest.raises(ValueError, match="shard has no validation"):
        states[0].validate(x, y, 0)
    assert all(s.steps == 0 for s in states)
    states[1].step(x, y, 1e-3)                                          # the first state that steps drives
    assert all(s.steps == 1 for s in states)
    with pytest.raises(ValueError, match="must not be stepped as well"):
        states[0].step(x, y, 1e-3)
    half = coopfit.LocalGather(2)
    lone = f.make(shard=coopfit.Shard(2, 0, half), grad_scale=f.default)
    with pytest.raises(ValueError, match="holds 1 of its 2 shard states"):
        lone.step(x, y, 1e-3)
    with pytest.raises(ValueError, match="shard must be a coopfit.Shard"):
        f.make(shard=2, grad_scale=f.default)


def test_fit_functions_under_a_local_gather():
    """``fit_prompts`` / ``fit_prompt_learner`` with ``shard=``: one rank gives the unsharded fit's bits, two ranks one result on both;
    PromptSRC's GPA runs on every rank; what ``shard`` refuses is refused by the function's name."""
    import numpy as np
    c = vptfit_ref.make_case("tiny", 2, 2, 4, 5)
    m = build_model(dict(c["sd"]), {"trainer": "VPT", "vision_depth": 2, "vision_ctx": 2, "language_depth": 0, "language_ctx": 0}).cuda()
    kw = dict(epochs=2, lr_per_epoch=RATES[:2], batch_size=4, return_history=True, **SGD)
    call = lambda **s: vptfit.fit_prompts(c["images"].cuda(), c["labels"], m, c["text"].cuda(), c["prompts"], vptfit_ref.LOGIT_SCALE, **kw, **s)
    plain, h0 = call()
    one, h1 = call(shard=coopfit.Shard(1, 0, coopfit.LocalGather(1)))
    assert same(one, plain) and np.array_equal(h0, h1)
    local = coopfit.LocalGather(2)
    two, h2 = call(shard=coopfit.Shard(2, 1, local))
    assert same(two, local.states[1].prompts) and same(local.states[0].prompts, local.states[1].prompts) and np.isfinite(h2).all() and len(h2) == 2
    for bad, match in ((dict(batch_size=3), "B=3 images does not split over G=2"), (dict(val=(c["images"].cuda(), c["labels"])), "shard has no validation"),
                       (dict(final_model="best_val"), "shard has no validation")):
        with pytest.raises(ValueError, match="fit_prompts: .*" + match):
            vptfit.fit_prompts(c["images"].cuda(), c["labels"], m, c["text"].cuda(), c["prompts"], **dict(kw, **bad), shard=coopfit.Shard(2, 0, coopfit.LocalGather(2)))
    with pytest.raises(ValueError, match="return_operand_stats"):
        vptfit.prompt_gradient(m, c["prompts"], c["images"].cuda(), c["labels"], c["text"].cuda(), return_operand_stats=True,
                               shard=coopfit.Shard(2, 0, coopfit.LocalGather(2)))
    # PromptSRC: GPA's running sum and its hand-over on every rank
    p = promptsrcfit_ref.make_case("tiny", 2, 2, 3, 2, 3, 4)
    mp = build_model(dict(p["sd"]), promptsrcfit_ref.design(3, 2, 2, 2)).cuda()
    local = coopfit.LocalGather(2)
    fitted = promptsrcfit.fit_prompts(p["images"].cuda(), p["labels"], mp, p["ids"], p["teacher"].cuda(), p["p"], epochs=2, lr_per_epoch=RATES[:2], batch_size=4,
                                      gpa=(1.0, 1.0), shard=coopfit.Shard(2, 0, local), **SGD)
    a, b = local.states
    assert a.epochs_seen == b.epochs_seen == 2 and same(a.block, b.block) and same(a.gpa, b.gpa) and same(a.block, a.gpa)
    assert same(fitted["ctx"], a.params()["ctx"])
    with pytest.raises(ValueError, match="fit_prompts: shard has no one-call step"):
        promptsrcfit.fit_prompts(p["images"].cuda(), p["labels"], mp, p["ids"], p["teacher"].cuda(), p["p"], epochs=1, one_call=True,
                                 shard=coopfit.Shard(2, 0, coopfit.LocalGather(2)))
