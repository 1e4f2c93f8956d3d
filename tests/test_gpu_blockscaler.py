"""The dynamic loss scale of the block fits on the GPU: clipmi_block_step_scaled at operator level against the plain restatement
(tests/blockscaler_ref.py, held to torch on the CPU by tests/test_blockscaler_cpu.py), and CoCoOp's, VPT's, MaPLe's, PromptSRC's and IVLP's
fits end to end on the small cases of their own GPU tests, both routes: the static path's bits when nothing overflows, a skipped step and
the static path's bits again behind it when fp16 does.  The static path is the yardstick; every comparison is bit for bit.  The figures go
out on lines that start with "blockscaler-parity:"; profiles/blockscaler_parity.txt is one run's lines."""
import functools
import math

import numpy as np
import pytest
import torch

import blockscaler_ref as bref
import cocoopfit_ref
import coopfit_ref
import maplefit_ref
import promptsrcfit_ref
import vptfit_ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import _lib, cocoopfit, maplefit, ops, promptsrcfit, vptfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

lib = _lib.lib
CANARY, PAD = 0x5A, 256
RATES = [2e-3, 1e-3, 5e-4, 2e-3]
SGD = dict(momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=False)


def say(line):
    print("blockscaler-parity: " + line)


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


class BlockStep:
    """clipmi_block_step_scaled on guarded buffers: params, buf, grad_out, the state block and a workspace of exactly the reported size."""

    def __init__(self, params0, init_scale, growth=2.0, backoff=0.5, interval=2000, momentum=0.5, dampening=0.0, weight_decay=0.0, nesterov=False):
        self.total = int(np.asarray(params0).size)
        n = 4 * self.total
        self.params, self.buf, self.grad = Guarded(n, init=params0), Guarded(n, init=np.zeros(self.total, np.float32)), Guarded(n)
        self.state = Guarded(20, torch.int32, init=ops.new_scaler_state(init_scale, "cpu"))
        need = lib.clipmi_block_step_scaled_workspace_bytes(self.total)
        assert need == bref.workspace_bytes(self.total)
        self.ws = Guarded(need, torch.uint8)
        assert self.ws.t.data_ptr() % 256 == 0
        self.scaler = (float(growth), float(backoff), int(interval))
        self.sgd = (float(momentum), float(dampening), float(weight_decay), int(nesterov))

    def __call__(self, grad, lr, expect=_lib.OK, **bad):
        g = torch.as_tensor(grad).cuda().contiguous()
        lr_d = torch.tensor([lr], dtype=torch.float32).cuda()
        a = dict(growth=self.scaler[0], backoff=self.scaler[1], interval=self.scaler[2], ws_bytes=self.ws.nbytes, total=self.total)
        a.update(bad)
        rc = lib.clipmi_block_step_scaled(g.data_ptr(), self.params.t.data_ptr(), self.buf.t.data_ptr() if self.sgd[0] else None, self.grad.t.data_ptr(),
                                          a["total"], self.state.t.data_ptr(), a["growth"], a["backoff"], a["interval"], lr_d.data_ptr(), *self.sgd,
                                          self.ws.t.data_ptr(), a["ws_bytes"], ops._stream())
        assert rc == expect, _lib.last_error()
        torch.cuda.synchronize()
        assert all(b.intact() for b in (self.params, self.buf, self.grad, self.state, self.ws)), "a write outside an output"
        return ops.scaler_state_dict(self.state.t)

    def bits(self):
        return tuple(b.t.cpu().numpy().copy() for b in (self.params, self.buf, self.grad))


TOTALS = (1, 255, 256, 257, 65537)


def places(total):
    """Element 0, the last element, element 255, element 256 and the last element of the partial workgroup, where the block has them."""
    last_partial = total - 1 if total % 256 else None
    return sorted({i for i in (0, total - 1, 255, 256, last_partial) if i is not None and 0 <= i < total})


# ------------------------------------------------------------------------------------------------------------------ 1. operator level
@pytest.mark.parametrize("total", TOTALS)
def test_clean_steps_equal_the_restatement_and_the_scale_grows(total):
    """Two clean steps with growth_interval = 2: params, buf and grad_out equal the restatement bit for bit, the state block equals torch's
    rule, the scale grows on the second step; from 2^127 it does not (the product is not finite).  Two runs give the same bits."""
    lr = 2.0 ** -3
    params0, ints = bref.exact_block(total, 2, seed=total)
    runs = []
    for _ in range(2):
        r = bref.BlockRef(params0, 2.0 ** 10, 2.0, 0.5, 2, momentum=0.5)
        step = BlockStep(params0, 2.0 ** 10, 2.0, 0.5, 2)
        for k in range(2):
            g = bref.scaled(ints[k], float(r.scale))
            st = step(g, lr)
            assert not r.step(g, lr)
            assert st == r.state(), (k, st)
            p, b, go = step.bits()
            assert np.array_equal(p, r.params) and np.array_equal(b, r.momentum_buffer) and np.array_equal(go, r.grad.reshape(-1)), k
        assert st == {"scale": 2048.0, "growth_tracker": 0, "skipped_steps": 0, "applied_steps": 2, "found_inf": 0}
        runs.append(step.bits())
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    top = BlockStep(params0, 2.0 ** 127, 2.0, 0.5, 1)
    st = top(bref.scaled(ints[0], 2.0 ** 127), lr)
    assert st == {"scale": 2.0 ** 127, "growth_tracker": 0, "skipped_steps": 0, "applied_steps": 1, "found_inf": 0}
    assert np.isfinite(top.bits()[0]).all()


@pytest.mark.parametrize("total", TOTALS)
def test_one_non_finite_element_skips_the_step(total):
    """One inf, -inf or NaN at every seam of the workgroups: params and buf untouched bytewise, the scale times backoff_factor,
    growth_tracker 0, skipped_steps 1 -- on the very first step, and the momentum buffer then starts at the first applied one."""
    lr = 2.0 ** -3
    params0, ints = bref.exact_block(total, 2, seed=7 + total)
    for at in places(total):
        for bad in bref.POISON:
            r = bref.BlockRef(params0, 2.0 ** 10, 2.0, 2.0 ** -4, 2, momentum=0.5)
            step = BlockStep(params0, 2.0 ** 10, 2.0, 2.0 ** -4, 2)
            before = step.bits()
            g = bref.scaled(ints[0], 2.0 ** 10)
            g[at] = bad
            st = step(g, lr)
            assert r.step(g, lr)
            assert st == r.state() == {"scale": 64.0, "growth_tracker": 0, "skipped_steps": 1, "applied_steps": 0, "found_inf": 1}, (at, bad)
            after = step.bits()
            assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes(), (at, bad)
            g = bref.scaled(ints[1], 64.0)                              # the first applied step: buf = its gradient
            st = step(g, lr)
            assert not r.step(g, lr) and st == r.state() and st["applied_steps"] == 1
            p, b, go = step.bits()
            assert np.array_equal(p, r.params) and np.array_equal(b, r.momentum_buffer) and np.array_equal(b, go), (at, bad)


def test_a_refused_call_leaves_every_buffer_untouched():
    params0, ints = bref.exact_block(257, 1, seed=1)
    step = BlockStep(params0, 2.0 ** 10)
    before, state = step.bits(), step.state.t.cpu().clone()
    ws = step.ws.t.cpu().clone()
    g = bref.scaled(ints[0], 2.0 ** 10)
    for bad, rc in ((dict(growth=0.0), _lib.ERR_ARG), (dict(backoff=math.nan), _lib.ERR_ARG), (dict(interval=0), _lib.ERR_ARG),
                    (dict(ws_bytes=step.ws.nbytes - 1), _lib.ERR_WORKSPACE), (dict(total=0), _lib.ERR_SHAPE)):
        step(g, 1e-3, expect=rc, **bad)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(step.bits(), before)), bad
        assert torch.equal(step.state.t.cpu(), state) and torch.equal(step.ws.t.cpu(), ws), bad


def test_ops_block_step_scaled():
    params0, ints = bref.exact_block(300, 1, seed=2)
    r = bref.BlockRef(params0, 2.0 ** 8, momentum=0.5)
    p, b = torch.from_numpy(params0.copy()).cuda(), torch.zeros(300).cuda()
    state = ops.new_scaler_state(2.0 ** 8, "cuda")
    g = bref.scaled(ints[0], 2.0 ** 8)
    out = ops.block_step_scaled(torch.from_numpy(g).cuda(), state, p, b, torch.tensor([0.125]).cuda(), momentum=0.5)
    r.step(g, 0.125)
    assert np.array_equal(p.cpu().numpy(), r.params) and np.array_equal(out.cpu().numpy(), r.grad.reshape(-1)) and ops.scaler_state_dict(state) == r.state()


# ---------------------------------------------------------------------------------------------------------------------- 2. the fits
class Fit:
    """One fit on one small case: how to make its state, feed it its one batch, and read its master block and momentum buffer."""

    def __init__(self, name):
        self.name = name
        if name == "cocoop":
            c = cocoopfit_ref.make_case("tiny3", 3, 4, 3)
            m = build_model(dict(coopfit_ref.state_dict("tiny3")), {"trainer": "CoOp"}).cuda()
            self.default = cocoopfit.DEFAULT_GRAD_SCALE
            self.make = lambda **kw: cocoopfit.CoCoOpFitState(m, c["ids"], c["params"], logit_scale=cocoopfit_ref.LOGIT_SCALE, **SGD, **kw)
            self.batch = (c["feats"].cuda(), c["labels"].cuda())
            self.block, self.buf = (lambda st: st.block), (lambda st: st.buf)
        elif name == "vpt":
            c = vptfit_ref.make_case("tiny", 2, 2, 3, 5)
            m = build_model(dict(c["sd"]), {"trainer": "VPT", "vision_depth": 2, "vision_ctx": 2, "language_depth": 0, "language_ctx": 0}).cuda()
            self.default = vptfit.DEFAULT_GRAD_SCALE
            self.make = lambda **kw: vptfit.VPTFitState(m, c["text"].cuda(), vptfit_ref.LOGIT_SCALE, c["prompts"], **SGD, **kw)
            self.batch = (c["images"].cuda(), c["labels"].cuda())
            self.block, self.buf = (lambda st: st.prompts), (lambda st: st.buf)
        elif name == "maple":
            c = maplefit_ref.make_case("tiny3", 2, 1, 5, 3)
            m = build_model(dict(c["sd"]), maplefit_ref.design(1)).cuda()
            rows = maplefit_ref.live_rows(c["ids"], False)
            self.default = maplefit.DEFAULT_GRAD_SCALE
            self.make = lambda **kw: maplefit.MaPLeFitState(m, c["ids"], c["pl"], maplefit_ref.LOGIT_SCALE, seq_rows=rows, **SGD, **kw)
            self.batch = (c["images"].cuda(), c["labels"].cuda())
            self.block, self.buf = (lambda st: st.block), (lambda st: st.buf)
        else:
            c = promptsrcfit_ref.make_case("tiny", 2, 2, 3, 2, 3, 3)
            m = build_model(dict(c["sd"]), promptsrcfit_ref.design(3, 2, 2, 2)).cuda()
            rows = promptsrcfit_ref.live_rows(c["ids"], True)
            self.default = promptsrcfit.DEFAULT_GRAD_SCALE
            self.make = lambda **kw: promptsrcfit.PromptSRCFitState(m, c["ids"], c["p"], c["teacher"].cuda(), promptsrcfit_ref.LOGIT_SCALE, seq_rows=rows,
                                                                    method=name, **SGD, **kw)
            self.batch = (c["images"].cuda(), c["labels"].cuda())
            self.block, self.buf = (lambda st: st.block), (lambda st: st.buf)

    def run(self, steps, one_call=False, start=None, first=0, **kw):
        """`steps` steps on the batch at RATES[first:]: (block, buf, losses, state).  `start`: (block, buf) to begin from."""
        st = self.make(**kw)
        if start is not None:
            self.block(st).copy_(start[0].cuda())
            self.buf(st).copy_(start[1].cuda())
        lr = torch.tensor(RATES, dtype=torch.float32).cuda()
        x, y = self.batch
        if self.name == "cocoop":
            st.tower(int(x.shape[0]))                 # the tower of this batch size uploads the token ids when it is made: not a step's work
        torch.cuda.synchronize()
        losses = []
        if kw.get("grad_scale") == "dynamic":         # no read-back inside a step: a synchronising torch call raises here
            torch.cuda.set_sync_debug_mode("error")
        try:
            for k in range(first, first + steps):
                losses.append(st.step(x, y, lr[k:k + 1], want_loss=True, one_call=one_call))
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        return self.block(st).cpu().clone(), self.buf(st).cpu().clone(), torch.cat(losses).cpu(), st


@functools.lru_cache(maxsize=None)
def fit(name):
    return Fit(name)


FITS = ["cocoop", "vpt", "maple", "promptsrc", "ivlp"]


def same(a, b):
    return a.view(torch.int32).equal(b.view(torch.int32))


@pytest.mark.parametrize("name", FITS)
def test_dynamic_without_overflow_gives_the_static_bits(name):
    """Three steps at the fit's static default with no growth: parameters, momentum buffer and losses are the static path's, bit for bit,
    on both routes; scaler_state() is the only synchronising call."""
    f = fit(name)
    block_s, buf_s, loss_s, st0 = f.run(3, grad_scale=f.default)
    assert torch.isfinite(block_s).all() and not same(block_s, f.block(f.make(grad_scale=f.default)).cpu())
    with pytest.raises(ValueError, match="static grad_scale"):
        st0.scaler_state()
    scaler = {"init_scale": f.default, "growth_interval": 1000}
    for one_call in (False, True):
        block_d, buf_d, loss_d, st = f.run(3, one_call=one_call, grad_scale="dynamic", scaler=scaler)
        assert st.scaler_state() == {"scale": f.default, "growth_tracker": 3, "skipped_steps": 0, "applied_steps": 3, "found_inf": 0}
        dist = float((block_d - block_s).abs().max())
        say(f"{name} {'one call' if one_call else 'separate calls'}: three steps at 2^{int(math.log2(f.default))}, max |dynamic - static| = {dist:g}")
        assert same(block_d, block_s) and same(buf_d, buf_s) and same(loss_d, loss_s), one_call


@pytest.mark.parametrize("name", FITS)
def test_overflow_is_skipped_and_the_fit_recovers(name):
    """The smallest power of two >= the default at which one static step leaves a non-finite block is found by doubling; the dynamic fit
    starts there with backoff 2^-4: step 1 is skipped (block and buffer bytewise unchanged, one skipped step, the scale divided by 16) and
    steps 2 .. 4 equal, bit for bit, a static run at the backed-off scale from the same parameters on the same batches and rates.  The
    static path at the overflowing scale ends non-finite."""
    f = fit(name)
    start = f.block(f.make(grad_scale=f.default)).cpu().clone()
    scale = f.default
    for _ in range(40):
        block_o = f.run(1, grad_scale=scale)[0]
        if not torch.isfinite(block_o).all():
            break
        scale *= 2.0
    assert not torch.isfinite(block_o).all(), "no power of two up to 2^40 times the default overflows fp16 on this case"
    say(f"{name}: the static path overflows at 2^{int(math.log2(scale))} (default 2^{int(math.log2(f.default))})")
    scaler = {"init_scale": scale, "backoff_factor": 2.0 ** -4, "growth_interval": 1000}
    zero = torch.zeros_like(start)
    block_s, buf_s, loss_s, _ = f.run(3, first=1, grad_scale=scale / 16.0)       # steps 2 .. 4 of the schedule, from the start
    assert torch.isfinite(block_s).all()
    for one_call in (False, True):
        b1, m1, _, st = f.run(1, one_call=one_call, grad_scale="dynamic", scaler=scaler)
        assert st.scaler_state() == {"scale": scale / 16.0, "growth_tracker": 0, "skipped_steps": 1, "applied_steps": 0, "found_inf": 1}
        assert same(b1, start) and same(m1, zero), one_call
        block_d, buf_d, loss_d, st = f.run(4, one_call=one_call, grad_scale="dynamic", scaler=scaler)
        s = st.scaler_state()
        dist = float((block_d - block_s).abs().max())
        say(f"{name} {'one call' if one_call else 'separate calls'}: {s['skipped_steps']} skipped, {s['applied_steps']} applied; final scale "
            f"2^{int(math.log2(s['scale']))}; max |dynamic - static at the backed-off scale| = {dist:g}")
        assert s == {"scale": scale / 16.0, "growth_tracker": 3, "skipped_steps": 1, "applied_steps": 3, "found_inf": 0}
        assert st.steps == 4                                            # a skipped step counts in the schedule
        assert same(block_d, block_s) and same(buf_d, buf_s) and same(loss_d[1:], loss_s), one_call


def test_promptsrc_end_epoch_aggregates_whatever_the_block_holds():
    f = fit("promptsrc")
    st = f.run(1, grad_scale="dynamic", scaler={"init_scale": 2.0 ** 100, "backoff_factor": 2.0 ** -4})[3]     # 2^100 overflows fp16: skipped
    assert st.scaler_state()["skipped_steps"] == 1
    st.end_epoch(0.5)
    torch.cuda.synchronize()
    assert torch.equal(st.gpa, 0.5 * st.block)
