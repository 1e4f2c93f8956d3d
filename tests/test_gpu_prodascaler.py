"""ProDA's dynamic loss scale on the GPU: clipmi_proda_ctx_step_scaled at operator level against the plain restatement
(tests/prodascaler_ref.py, held to torch on the CPU by tests/test_prodascaler_cpu.py) and against the static kernel, and ProDA's fit end
to end on the `tiny` and `tiny3` geometries, both routes: the static path's bits when nothing overflows, a skipped step and the static
path's bits again behind it when fp16 does.  Every comparison is bit for bit: the scales are powers of two, the sums run in the static
kernel's order and the launches are the static path's.  The figures go out on lines that start with "prodascaler-parity:";
profiles/prodascaler_parity.txt is one run's lines."""
import functools
import math

import numpy as np
import pytest
import torch

import coopfit_ref
import prodafit_ref as dref
import prodascaler_ref as pref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import _lib, ops, prodafit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

lib = _lib.lib
CANARY, PAD = 0x5A, 256
RATES = [2e-3, 1e-3, 5e-4, 2e-3]
SGD = dict(momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=False)

# The operator's case: three classes whose names are 0, 3 and 5 tokens long, eight contexts of four vectors (0, 1 front; 2, 3 middle; 4 ..
# 7 end), four of them selected -- one front, one middle, two end.  D = 20: ctx has 8 * 4 * 20 = 640 elements, two and a half workgroups
# of 256; element 0 and elements 255 | 256 (the first seam) belong to the selected contexts 0 and 3, elements 511 | 512 (the second seam)
# to context 6, which is not selected, the last element to the selected context 7.
C, PB, P, L, D, N_CTX = 3, 4, 8, 16, 20, 4
TOTAL = P * N_CTX * D
NAME_LENS = np.array([0, 3, 5])
POS = dref.positions(P)
SEL = dref.ordered((0, 3, 7, 5), POS)
UNSELECTED = sorted(set(range(P)) - set(int(p) for p in SEL))
LR = 2.0 ** -3


def say(line):
    print("prodascaler-parity: " + line)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


class Guarded:
    """A device buffer of `nbytes` bytes between two runs of canary bytes; `t` views the payload with a dtype."""

    def __init__(self, nbytes, dtype=torch.float32, init=None):
        self.raw = torch.full((PAD + nbytes + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        self.nbytes = nbytes
        self.t = self.raw[PAD:PAD + nbytes].view(dtype)
        if init is not None:
            self.t.copy_(torch.as_tensor(init).to(dtype).reshape(self.t.shape))

    def intact(self):
        raw = self.raw.cpu()
        return bool((raw[:PAD] == CANARY).all()) and bool((raw[PAD + self.nbytes:] == CANARY).all())


class ProdaStep:
    """clipmi_proda_ctx_step_scaled on guarded buffers: ctx, buf, grad_out, the state block and a workspace of exactly the reported size."""

    def __init__(self, ctx0, init_scale, growth=2.0, backoff=0.5, interval=2000, momentum=0.5, dampening=0.0, weight_decay=0.0, nesterov=False, sel=SEL):
        n = 4 * TOTAL
        self.ctx, self.buf, self.grad = Guarded(n, init=ctx0), Guarded(n, init=np.zeros(TOTAL, np.float32)), Guarded(n)
        self.state = Guarded(20, torch.int32, init=ops.new_scaler_state(init_scale, "cpu"))
        need = lib.clipmi_proda_ctx_step_scaled_workspace_bytes(P, D, N_CTX)
        assert need == pref.workspace_bytes(P, D, N_CTX)
        self.ws = Guarded(need, torch.uint8)
        assert self.ws.t.data_ptr() % 256 == 0
        self.sel, self.pos, self.nl = i32(sel), i32(POS), i32(NAME_LENS)
        self.scaler = (float(growth), float(backoff), int(interval))
        self.sgd = (float(momentum), float(dampening), float(weight_decay), int(nesterov))

    def __call__(self, d_embed, lr, expect=_lib.OK, **bad):
        d = torch.as_tensor(d_embed).cuda().contiguous()
        lr_d = torch.tensor([lr], dtype=torch.float32).cuda()
        a = dict(d=d.data_ptr(), ctx=self.ctx.t.data_ptr(), sel=self.sel.data_ptr(), pos=self.pos.data_ptr(), nl=self.nl.data_ptr(),
                 state=self.state.t.data_ptr(), rate=lr_d.data_ptr(), ws=self.ws.t.data_ptr(), growth=self.scaler[0], backoff=self.scaler[1],
                 interval=self.scaler[2], ws_bytes=self.ws.nbytes)
        a.update(bad)
        rc = lib.clipmi_proda_ctx_step_scaled(a["d"], a["ctx"], self.buf.t.data_ptr() if self.sgd[0] else None, self.grad.t.data_ptr(), a["sel"], a["pos"],
                                              a["nl"], C, PB, P, L, D, N_CTX, a["state"], a["growth"], a["backoff"], a["interval"], a["rate"], *self.sgd,
                                              a["ws"], a["ws_bytes"], ops._stream())
        assert rc == expect, _lib.last_error()
        torch.cuda.synchronize()
        assert all(b.intact() for b in (self.ctx, self.buf, self.grad, self.state, self.ws)), "a write outside an output"
        return ops.scaler_state_dict(self.state.t)

    def bits(self):
        return tuple(b.t.cpu().numpy().copy() for b in (self.ctx, self.buf, self.grad))


def same_np(a, b):
    return a.shape == b.shape and a.view(np.int32).tobytes() == b.view(np.int32).tobytes()


# ------------------------------------------------------------------------------------------------------------------ 1. operator level
@pytest.mark.parametrize("momentum,wd,nesterov", [(0.9, 5e-4, False), (0.9, 0.0, True), (0.0, 5e-4, False)], ids=["momentum-wd", "nesterov", "wd"])
def test_clean_steps_equal_the_static_kernel(momentum, wd, nesterov):
    """Random fp32 d_embed (nothing exact: every rounding counts), a first step and a later step with a new selection: ctx, buf and grad_out
    equal ops.proda_ctx_step at grad_scale = scale with first_step on the first call only, bit for bit."""
    g = torch.Generator().manual_seed(5)
    ctx0 = 0.02 * torch.randn(P, N_CTX, D, generator=g)
    scale = 2.0 ** 10
    step = ProdaStep(ctx0.numpy(), scale, interval=1000, momentum=momentum, weight_decay=wd, nesterov=nesterov)
    ctx_s, buf_s = ctx0.cuda().clone(), torch.zeros(P, N_CTX, D).cuda()
    lr = torch.tensor([0.05]).cuda()
    for k, sel in enumerate((SEL, dref.ordered((1, 2, 4, 6), POS))):
        step.sel = i32(sel)
        d = (torch.randn((C * PB + P) * L, D, generator=g) * scale).cuda()
        st = step(d, 0.05)
        want = ops.proda_ctx_step(d, i32(sel), i32(POS), i32(NAME_LENS), N_CTX, scale, ctx_s, buf_s if momentum else None, lr, k == 0, momentum, 0.0, wd,
                                  nesterov)
        torch.cuda.synchronize()
        c, b, go = step.bits()
        assert st == {"scale": scale, "growth_tracker": k + 1, "skipped_steps": 0, "applied_steps": k + 1, "found_inf": 0}
        assert same_np(go, want.cpu().numpy().reshape(-1)) and same_np(c, ctx_s.cpu().numpy().reshape(-1)), k
        if momentum:
            assert same_np(b, buf_s.cpu().numpy().reshape(-1)), k
    assert np.isfinite(c).all() and not same_np(c, ctx0.numpy().reshape(-1))
    ours = ops.proda_ctx_step_scaled(d, i32(sel), i32(POS), i32(NAME_LENS), N_CTX, ops.new_scaler_state(scale, "cuda"), ctx0.cuda().clone(), None, lr)
    assert same_np(ours.cpu().numpy().reshape(-1), go)                  # the Python operator reports the same unscaled gradient


def test_clean_steps_equal_the_restatement_and_the_scale_grows():
    """Two clean steps with growth_interval = 2 on exact inputs: ctx, buf and grad_out equal the restatement element for element, the state
    block equals torch's rule, the scale doubles on the second step; from 2^127 the growth is not taken.  Two runs give the same bits."""
    ctx0, ints = pref.exact_inputs(C, PB, P, L, D, N_CTX, 2, seed=3)
    runs = []
    for _ in range(2):
        r = pref.ProdaScalerRef(ctx0, C, POS, NAME_LENS, 2.0 ** 10, 2.0, 0.5, 2, momentum=0.5, weight_decay=2.0 ** -3)
        step = ProdaStep(ctx0, 2.0 ** 10, 2.0, 0.5, 2, weight_decay=2.0 ** -3)
        for k in range(2):
            d = pref.scaled(ints[k], float(r.scale))
            st = step(d, LR)
            assert not r.step(d, LR, SEL)
            assert st == r.state(), (k, st)
            c, b, go = step.bits()
            assert np.array_equal(c, r.ctx.reshape(-1)) and np.array_equal(b, r.buf.reshape(-1)) and np.array_equal(go, r.grad.reshape(-1)), k
        assert st == {"scale": 2048.0, "growth_tracker": 0, "skipped_steps": 0, "applied_steps": 2, "found_inf": 0}
        runs.append(step.bits())
    assert all(same_np(a, b) for a, b in zip(*runs))
    for p in UNSELECTED:                                                # a context outside the selection is its no-class row alone
        want = pref.scaled(ints[1], 1.0).reshape(C * PB + P, L, D)[C * PB + p, 1:1 + N_CTX]
        assert np.array_equal(go.reshape(P, N_CTX, D)[p], want)
    top = ProdaStep(ctx0, 2.0 ** 127, 2.0, 0.5, 1)
    st = top(pref.scaled(ints[0], 2.0 ** 127), LR)
    assert st == {"scale": 2.0 ** 127, "growth_tracker": 0, "skipped_steps": 0, "applied_steps": 1, "found_inf": 0}
    assert np.isfinite(top.bits()[0]).all()


def element(idx):
    return idx // (N_CTX * D), (idx // D) % N_CTX, idx % D


def class_row_source(idx):
    """The element of d_embed [N, L, D] on a class row that feeds element idx of a SELECTED context's gradient."""
    p, j, d = element(idx)
    q, c = [int(v) for v in SEL].index(p), idx % C
    return c * PB + q, dref.ctx_row(int(POS[p]), j, int(NAME_LENS[c]), N_CTX // 2), d


def no_class_source(idx):
    p, j, d = element(idx)
    return C * PB + p, 1 + j, d


# the gradient element whose source is poisoned: in the first workgroup, on a seam between two workgroups (both sides), in the last one
SELECTED_PLACES = (0, 255, 256, TOTAL - 1)                  # contexts 0, 3, 3, 7
UNSELECTED_PLACES = (80, 511, 512, 559)                    # contexts 1, 6, 6, 6


def _skipped_then_applied(source, idx, bad, want_selected):
    p = element(idx)[0]
    assert (p in [int(v) for v in SEL]) == want_selected
    ctx0, ints = pref.exact_inputs(C, PB, P, L, D, N_CTX, 2, seed=11 + idx)
    r = pref.ProdaScalerRef(ctx0, C, POS, NAME_LENS, 2.0 ** 10, 2.0, 2.0 ** -4, 2, momentum=0.5)
    step = ProdaStep(ctx0, 2.0 ** 10, 2.0, 2.0 ** -4, 2)
    before = step.bits()
    d = pref.scaled(ints[0], 2.0 ** 10).reshape(C * PB + P, L, D)
    d[source(idx)] = bad
    d = d.reshape(-1, D)
    st = step(d, LR)
    assert r.step(d, LR, SEL)
    assert st == r.state() == {"scale": 64.0, "growth_tracker": 0, "skipped_steps": 1, "applied_steps": 0, "found_inf": 1}, (idx, bad)
    after = step.bits()
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes(), (idx, bad)
    assert np.array_equal(after[2], r.grad.reshape(-1), equal_nan=True) and not np.isfinite(after[2][idx])       # grad_out is still written
    assert np.isfinite(np.delete(after[2], idx)).all()
    d = pref.scaled(ints[1], 64.0)                                      # the first applied step: buf = its gradient
    st = step(d, LR)
    assert not r.step(d, LR, SEL) and st == r.state() and st["applied_steps"] == 1
    c, b, go = step.bits()
    assert np.array_equal(c, r.ctx.reshape(-1)) and np.array_equal(b, r.buf.reshape(-1)) and np.array_equal(b, go), (idx, bad)


@pytest.mark.parametrize("idx", SELECTED_PLACES)
def test_an_inf_in_a_class_row_of_a_selected_context_skips_the_step(idx):
    for bad in (np.inf, -np.inf):
        _skipped_then_applied(class_row_source, idx, bad, True)


@pytest.mark.parametrize("idx", UNSELECTED_PLACES)
def test_a_nan_in_the_no_class_row_of_an_unselected_context_skips_the_step(idx):
    _skipped_then_applied(no_class_source, idx, np.nan, False)


def test_an_inf_in_a_row_the_gather_does_not_read_does_not_trip_the_flag():
    """EVERY element of d_embed that the gather does not read is an inf -- SOS rows, name tokens, '.', EOT and padding rows of the class
    prompts, and of the no-class prompts everything outside rows 1 .. n_ctx: the step is applied and equals the restatement."""
    ctx0, ints = pref.exact_inputs(C, PB, P, L, D, N_CTX, 1, seed=2)
    mask = pref.read_rows(SEL, POS, NAME_LENS, C, P, L, N_CTX)
    d = pref.scaled(ints[0], 2.0 ** 10).reshape(C * PB + P, L, D)
    d[~mask] = np.inf
    assert (~mask).sum() == (C * PB + P) * L - (C * PB + P) * N_CTX
    d = d.reshape(-1, D)
    r = pref.ProdaScalerRef(ctx0, C, POS, NAME_LENS, 2.0 ** 10, momentum=0.5)
    step = ProdaStep(ctx0, 2.0 ** 10)
    st = step(d, LR)
    assert not r.step(d, LR, SEL)
    assert st == r.state() == {"scale": 1024.0, "growth_tracker": 1, "skipped_steps": 0, "applied_steps": 1, "found_inf": 0}
    c, b, go = step.bits()
    assert np.isfinite(go).all() and np.array_equal(c, r.ctx.reshape(-1)) and np.array_equal(b, r.buf.reshape(-1)) and np.array_equal(go, r.grad.reshape(-1))


def test_a_refused_call_leaves_every_buffer_untouched():
    ctx0, ints = pref.exact_inputs(C, PB, P, L, D, N_CTX, 1, seed=1)
    step = ProdaStep(ctx0, 2.0 ** 10)
    before, state, ws = step.bits(), step.state.t.cpu().clone(), step.ws.t.cpu().clone()
    d = pref.scaled(ints[0], 2.0 ** 10)
    refused = [(dict(growth=0.0), _lib.ERR_ARG), (dict(growth=math.inf), _lib.ERR_ARG), (dict(backoff=math.nan), _lib.ERR_ARG),
               (dict(interval=0), _lib.ERR_ARG), (dict(ws_bytes=step.ws.nbytes - 1), _lib.ERR_WORKSPACE)]
    refused += [({name: None}, _lib.ERR_ARG) for name in ("d", "ctx", "sel", "pos", "nl", "state", "rate", "ws")]
    for bad, rc in refused:
        step(d, 1e-3, expect=rc, **bad)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(step.bits(), before)), bad
        assert torch.equal(step.state.t.cpu(), state) and torch.equal(step.ws.t.cpu(), ws), bad


# ---------------------------------------------------------------------------------------------------------------------- 2. the fit
KEY = {"tiny": ("tiny", 3, 4, 8, 4, 2), "tiny3": ("tiny3", 3, 4, 8, 4, 2)}       # (geometry, C, n_ctx, P, Pb, B)
SEED = 9
DEFAULT = prodafit.DEFAULT_GRAD_SCALE


@functools.lru_cache(maxsize=None)
def model(geom):
    return build_model(dict(coopfit_ref.state_dict(geom)), {"trainer": "CoOp"}).cuda()


@functools.lru_cache(maxsize=None)
def schedule():
    """The selections the state itself draws from a generator seeded with SEED, four steps."""
    return prodafit.draw_selections(P, PB, 4, torch.Generator().manual_seed(SEED))


def run(geom, steps, one_call=False, first=0, own_schedule=False, **kw):
    """`steps` steps on the case's one batch at RATES[first:] with the selections schedule()[first:]: (ctx, buf, losses, state).
    ``own_schedule``: the state draws them itself (an upload per step).  Otherwise they lie on the device, and under the dynamic scale a
    synchronising torch call inside a step raises."""
    c = dref.make_case(*KEY[geom])
    assert len(set(dref.name_lens_of(c["ids"], 4).tolist())) == 3
    st = prodafit.ProDAFitState(model(geom), c["ids"], c["ctx"], prompt_bs=PB, logit_scale=dref.LOGIT_SCALE, generator=torch.Generator().manual_seed(SEED),
                                **SGD, **kw)
    x, y = c["feats"].cuda(), c["labels"].cuda()
    lr = torch.tensor(RATES, dtype=torch.float32).cuda()
    sels = i32(schedule())
    torch.cuda.synchronize()
    losses = []
    if kw.get("grad_scale") == "dynamic" and not own_schedule:
        torch.cuda.set_sync_debug_mode("error")
    try:
        for k in range(first, first + steps):
            losses.append(st.step(x, y, lr[k:k + 1], sel=None if own_schedule else sels[k], want_loss=True, one_call=one_call))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return st.ctx.cpu().clone(), st.buf.cpu().clone(), torch.cat(losses).cpu(), st


def same(a, b):
    return a.view(torch.int32).equal(b.view(torch.int32))


@pytest.mark.parametrize("geom", sorted(KEY))
def test_dynamic_without_overflow_gives_the_static_bits(geom):
    """Three steps at 2^12 with no growth: contexts, momentum buffer and losses are the static path's, bit for bit, on both routes, and a
    second dynamic run gives the first one's bits.  No step reads anything back; scaler_state() is the only synchronising call."""
    assert DEFAULT == 2.0 ** 12
    ctx_s, buf_s, loss_s, st0 = run(geom, 3, grad_scale=DEFAULT)
    start = dref.make_case(*KEY[geom])["ctx"]
    assert torch.isfinite(ctx_s).all() and torch.isfinite(loss_s).all() and not same(ctx_s, start)
    assert all(not same(ctx_s[p], start[p]) for p in range(P))          # every context moves, selected or not
    with pytest.raises(ValueError, match="static grad_scale"):
        st0.scaler_state()
    scaler = {"init_scale": DEFAULT, "growth_interval": 1000}
    for one_call in (False, True):
        ctx_d, buf_d, loss_d, st = run(geom, 3, one_call=one_call, grad_scale="dynamic", scaler=scaler)
        assert st.scaler_state() == {"scale": DEFAULT, "growth_tracker": 3, "skipped_steps": 0, "applied_steps": 3, "found_inf": 0}
        dist = float((ctx_d - ctx_s).abs().max())
        say(f"{geom} {'one call' if one_call else 'separate calls'}: three steps at 2^12, max |dynamic - static| = {dist:g}")
        assert same(ctx_d, ctx_s) and same(buf_d, buf_s) and same(loss_d, loss_s), one_call
        again = run(geom, 3, one_call=one_call, grad_scale="dynamic", scaler=scaler)
        assert same(again[0], ctx_d) and same(again[1], buf_d) and same(again[2], loss_d), one_call


@pytest.mark.parametrize("geom", sorted(KEY))
def test_overflow_is_skipped_and_the_fit_recovers(geom):
    """The smallest power of two >= the default at which one static step leaves a non-finite context is found by doubling; the dynamic
    fit starts there with backoff 2^-4 and draws its own selections: step 1 is skipped (ctx and buffer bytewise unchanged, one skipped
    step, the scale divided by 16) and steps 2 .. 4 equal, bit for bit, a static run at the backed-off scale from the same contexts on
    steps 2 .. 4 of the same schedule of selections and rates -- the schedule moved on over the skipped step."""
    start = dref.make_case(*KEY[geom])["ctx"]
    scale = DEFAULT
    for _ in range(40):
        ctx_o = run(geom, 1, grad_scale=scale)[0]
        if not torch.isfinite(ctx_o).all():
            break
        scale *= 2.0
    assert not torch.isfinite(ctx_o).all(), "no power of two up to 2^40 times the default overflows fp16 on this case"
    say(f"{geom}: the static path overflows at 2^{int(math.log2(scale))} (default 2^{int(math.log2(DEFAULT))})")
    scaler = {"init_scale": scale, "backoff_factor": 2.0 ** -4, "growth_interval": 1000}
    zero = torch.zeros_like(start)
    ctx_s, buf_s, loss_s, _ = run(geom, 3, first=1, grad_scale=scale / 16.0)     # steps 2 .. 4 of the schedule, from the start
    assert torch.isfinite(ctx_s).all()
    assert not np.array_equal(schedule()[0], schedule()[1])
    for one_call in (False, True):
        c1, b1, _, st = run(geom, 1, one_call=one_call, grad_scale="dynamic", scaler=scaler)
        assert st.scaler_state() == {"scale": scale / 16.0, "growth_tracker": 0, "skipped_steps": 1, "applied_steps": 0, "found_inf": 1}
        assert same(c1, start) and same(b1, zero), one_call
        for own in (False, True):
            ctx_d, buf_d, loss_d, st = run(geom, 4, one_call=one_call, own_schedule=own, grad_scale="dynamic", scaler=scaler)
            s = st.scaler_state()
            dist = float((ctx_d - ctx_s).abs().max())
            say(f"{geom} {'one call' if one_call else 'separate calls'}, {'the state draws' if own else 'given'} selections: {s['skipped_steps']} "
                f"skipped, {s['applied_steps']} applied; final scale 2^{int(math.log2(s['scale']))}; max |dynamic - static at the backed-off scale| = "
                f"{dist:g}")
            assert s == {"scale": scale / 16.0, "growth_tracker": 3, "skipped_steps": 1, "applied_steps": 3, "found_inf": 0}
            assert st.steps == 4                                        # a skipped step counts in the schedule
            assert same(ctx_d, ctx_s) and same(buf_d, buf_s) and same(loss_d[1:], loss_s), (one_call, own)


def test_a_synchronising_call_inside_a_step_would_fail():
    """The device of the two tests above: under torch's sync debug mode "error" a read-back raises; a dynamic step, on either route, does not."""
    x = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            x.item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for one_call in (False, True):
        st = run("tiny", 1, one_call=one_call, grad_scale="dynamic", scaler={"init_scale": DEFAULT})[3]
        assert st.scaler_state()["applied_steps"] + st.scaler_state()["skipped_steps"] == 1


def test_trainer_fit_context_under_the_dynamic_scale():
    """trainers.ProDACLIP.fit_context(loader, grad_scale="dynamic"): one short epoch of three steps, the counts in scaler_state(), and the
    static fit's bits when no step was skipped."""
    from clip_calibration_amd import trainers
    m = model("tiny")
    ids = dref.prompt_ids("tiny", 3, 4)
    g = torch.Generator().manual_seed(0)
    centres = torch.randn(3, 128, generator=g)
    labels = torch.arange(3).repeat_interleave(8)
    feats = centres[labels] + 0.1 * torch.randn(24, 128, generator=g)
    opt = dict(epochs=1, lr_per_epoch=[0.002], batch_size=8, prompt_bs=4, momentum=0.9, weight_decay=5e-4, return_history=True)
    out = {}
    try:
        m.image_features_f32 = lambda image: image          # the loader's "images" are the features (tests/test_gpu_prodafit.py)
        for how, kw in (("static", dict(grad_scale=DEFAULT)), ("dynamic", dict(grad_scale="dynamic", scaler={"init_scale": DEFAULT}))):
            clip = trainers.ProDACLIP(m, ids, n_ctx=4, n_prompt=8)
            with pytest.raises(ValueError, match="dynamic"):
                clip.scaler_state()
            out[how] = clip.fit_context([(feats.cuda(), labels)], **opt, **kw)
            assert clip.text_features is None and torch.equal(clip.prompt_learner.ctx.detach().float().cpu(),
                                                              out[how][0].to(clip.prompt_learner.ctx.dtype).float().cpu())
    finally:
        del m.image_features_f32
    s = clip.scaler_state()
    say(f"trainers.ProDACLIP.fit_context dynamic: {s['skipped_steps']} skipped, {s['applied_steps']} applied, scale 2^{int(math.log2(s['scale']))}; "
        f"loss {out['dynamic'][1][0]:.5f} -> {out['dynamic'][1][-1]:.5f}")
    assert len(out["dynamic"]) == 2 and len(out["dynamic"][1]) == 3 and np.isfinite(out["dynamic"][1]).all()
    assert s["skipped_steps"] + s["applied_steps"] == 3 and s["applied_steps"] >= 1 and s["found_inf"] in (0, 1)
    assert s["scale"] == DEFAULT * 0.5 ** s["skipped_steps"] and s["growth_tracker"] <= 3
    if s["skipped_steps"] == 0:
        assert same(out["dynamic"][0].cpu(), out["static"][0].cpu()) and np.array_equal(out["dynamic"][1], out["static"][1])
