"""The dynamic loss scale on the GPU (csrc/grad_scaler.hip, clip_calibration_amd/coopfit.py ``grad_scale="dynamic"``): the scaled step
at operator level against clipmi_ctx_step (bit for bit on clean input) and against the plain restatement of the rule
(tests/scalerfit_ref.py, held to torch on the CPU by tests/test_scalerfit_cpu.py), and CoOp's and KgCoOp's fits end to end on the `tiny`
and `tiny3` geometries: the static path's bits when nothing overflows, skipped steps and recovery when fp16 does.

The end-to-end tolerance of the recovery test is measured at run time: twice the largest element-wise distance between two static runs
at 2^10 and 2^14, the existing path's own sensitivity to the scale.  Its figures go out on lines that start with "scalerfit-parity:";
profiles/scalerfit_parity.txt is one run's lines."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import coopfit_ref
import promptfit_ref
import scalerfit_ref as ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import _lib, coopfit, ops  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

lib = _lib.lib
L = 24
CANARY, PAD = 0x5A, 256      # bytes around every output
SGD = dict(momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=False)


def say(line):
    print("scalerfit-parity: " + line)


class Guarded:
    """A device buffer of `nbytes` bytes between two runs of canary bytes; `t` views the payload with a dtype and a shape."""

    def __init__(self, nbytes, dtype=torch.float32, shape=None, init=None):
        self.raw = torch.full((PAD + nbytes + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        self.nbytes = nbytes
        self.t = self.raw[PAD:PAD + nbytes].view(dtype)
        if shape is not None:
            self.t = self.t.view(shape)
        if init is not None:
            self.t.copy_(torch.as_tensor(init).to(dtype).reshape(self.t.shape))

    def intact(self):
        raw = self.raw.cpu()
        return bool((raw[:PAD] == CANARY).all()) and bool((raw[PAD + self.nbytes:] == CANARY).all())


def ctx_shape(C, D, n_ctx, per_class):
    return (C, n_ctx, D) if per_class else (n_ctx, D)


class ScaledStep:
    """clipmi_ctx_step_scaled on guarded buffers: ctx, buf, grad_out, the state block and a workspace of exactly the reported size."""

    def __init__(self, ctx0, C, D, n_ctx, per_class, init_scale, growth=2.0, backoff=0.5, interval=2000, momentum=0.9, dampening=0.0,
                 weight_decay=5e-4, nesterov=False):
        self.C, self.D, self.n_ctx, self.per_class = C, D, n_ctx, per_class
        shape = ctx_shape(C, D, n_ctx, per_class)
        n = int(np.prod(shape)) * 4
        self.ctx, self.buf, self.grad = Guarded(n, shape=shape, init=ctx0), Guarded(n, shape=shape, init=torch.zeros(shape)), Guarded(n, shape=shape)
        self.state = Guarded(20, torch.int32, init=ops.new_scaler_state(init_scale, "cpu"))
        need = lib.clipmi_ctx_step_scaled_workspace_bytes(C, D, n_ctx, int(per_class))
        assert need > 0 and need % 256 == 0
        self.ws = Guarded(need, torch.uint8)
        assert self.ws.t.data_ptr() % 256 == 0
        self.scaler = (float(growth), float(backoff), int(interval))
        self.sgd = (float(momentum), float(dampening), float(weight_decay), int(nesterov))

    def __call__(self, d_embed, lr):
        d = torch.as_tensor(d_embed).cuda().contiguous()
        lr_d = torch.tensor([lr], dtype=torch.float32).cuda()
        rc = lib.clipmi_ctx_step_scaled(d.data_ptr(), self.ctx.t.data_ptr(), self.buf.t.data_ptr() if self.sgd[0] else None, self.grad.t.data_ptr(),
                                        self.C, L, self.D, self.n_ctx, int(self.per_class), self.state.t.data_ptr(), *self.scaler, lr_d.data_ptr(),
                                        *self.sgd, self.ws.t.data_ptr(), self.ws.nbytes, ops._stream())
        assert rc == _lib.OK, _lib.last_error()
        torch.cuda.synchronize()
        assert all(g.intact() for g in (self.ctx, self.buf, self.grad, self.state, self.ws)), "a write outside an output"
        return ops.scaler_state_dict(self.state.t)


def static_step(d_embed, ctx, buf, C, D, n_ctx, per_class, scale, lr, first, momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=False):
    """clipmi_ctx_step in place on ctx and buf; returns grad_out."""
    lr_d = torch.tensor([lr], dtype=torch.float32).cuda()
    return ops.ctx_step(torch.as_tensor(d_embed).cuda(), C, n_ctx, per_class, scale, ctx, buf, lr_d, first, momentum, dampening, weight_decay, nesterov)


def small_ints(C, D, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(-8, 9, size=(C * L, D)).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------- 1. operator, clean input
@pytest.mark.parametrize("per_class", [False, True], ids=["generic", "per_class"])
@pytest.mark.parametrize("D", [64, 128, 516])
@pytest.mark.parametrize("C", [2, 37])
def test_clean_step_is_ctx_step_bit_for_bit(C, D, per_class):
    """Small integers in d_embed (every sum exact): two consecutive calls give ctx, buf and grad_out of clipmi_ctx_step at the same scale,
    the first with first_step = 1; the tracker and applied_steps advance and the scale grows on the second call (growth_interval = 2)."""
    for n_ctx in (1, 4, 16):
        g = torch.Generator().manual_seed(C * 1000 + D + n_ctx)
        ctx0 = 0.02 * torch.randn(*ctx_shape(C, D, n_ctx, per_class), generator=g)
        step = ScaledStep(ctx0, C, D, n_ctx, per_class, 4096.0, interval=2)
        ctx_s, buf_s = ctx0.clone().cuda(), torch.zeros_like(ctx0).cuda()
        scale = 4096.0
        for k, lr in enumerate((2e-3, 1e-3)):
            d = small_ints(C, D, seed=10 * n_ctx + k)
            st = step(d, lr)
            grad_s = static_step(d, ctx_s, buf_s, C, D, n_ctx, per_class, scale, lr, k == 0)
            assert torch.equal(step.grad.t, grad_s) and torch.equal(step.ctx.t, ctx_s) and torch.equal(step.buf.t, buf_s), (n_ctx, k)
            scale = 4096.0 if k == 0 else 8192.0
            assert st == {"scale": scale, "growth_tracker": 1 - k, "skipped_steps": 0, "applied_steps": k + 1, "found_inf": 0}, (n_ctx, k)
        assert not torch.equal(step.ctx.t.cpu(), ctx0)


# ---------------------------------------------------------------------------------------------------- 2. operator, one non-finite element
@pytest.mark.parametrize("per_class", [False, True], ids=["generic", "per_class"])
@pytest.mark.parametrize("C,D,n_ctx", [(2, 64, 1), (37, 516, 4), (37, 128, 16)])
def test_one_non_finite_element_skips_the_step(C, D, n_ctx, per_class):
    g = torch.Generator().manual_seed(7)
    ctx0 = 0.02 * torch.randn(*ctx_shape(C, D, n_ctx, per_class), generator=g)
    d0 = small_ints(C, D, seed=3)
    places = {"first context row of class 0": (0 * L + 1, 0), "last context row of the last class": ((C - 1) * L + n_ctx, 1),
              "last column": (min(1, C - 1) * L + 1, D - 1), "the last workgroup's last element": ((C - 1) * L + n_ctx, D - 1)}
    for what, (row, col) in places.items():
        for bad in ref.POISON:
            step = ScaledStep(ctx0, C, D, n_ctx, per_class, 4096.0, backoff=0.25, interval=2)
            d = d0.clone()
            st = step(d, 1e-3)                                        # a clean step first: the buffer holds something to keep
            assert st["applied_steps"] == 1 and st["growth_tracker"] == 1
            ctx1, buf1 = step.ctx.t.clone(), step.buf.t.clone()
            d[row, col] = bad
            st = step(d, 1e-3)
            assert torch.equal(step.ctx.t, ctx1) and torch.equal(step.buf.t, buf1), (what, bad)
            assert st == {"scale": 1024.0, "growth_tracker": 0, "skipped_steps": 1, "applied_steps": 1, "found_inf": 1}, (what, bad)
    for row in (0, 1 + n_ctx):                                        # rows that are no context rows do not trigger
        for c in (0, C - 1):
            step = ScaledStep(ctx0, C, D, n_ctx, per_class, 4096.0)
            d = d0.clone()
            d[c * L + row, D - 1] = math.nan
            d[c * L + row, 0] = math.inf
            st = step(d, 1e-3)
            ctx_s, buf_s = ctx0.clone().cuda(), torch.zeros_like(ctx0).cuda()
            static_step(d, ctx_s, buf_s, C, D, n_ctx, per_class, 4096.0, 1e-3, True)
            assert st == {"scale": 4096.0, "growth_tracker": 1, "skipped_steps": 0, "applied_steps": 1, "found_inf": 0}
            assert torch.equal(step.ctx.t, ctx_s) and torch.equal(step.buf.t, buf_s) and torch.isfinite(step.ctx.t).all()
    # two finite rows whose sum overflows fp32: the generic context adds them, the class-specific one does not
    d = d0.clone()
    d[0 * L + n_ctx, D - 1] = d[(C - 1) * L + n_ctx, D - 1] = 3.0e38
    assert torch.isfinite(d).all()
    step = ScaledStep(ctx0, C, D, n_ctx, per_class, 4096.0)
    st = step(d, 1e-3)
    if per_class:
        assert st["found_inf"] == 0 and st["applied_steps"] == 1 and torch.isfinite(step.ctx.t).all()
    else:
        assert st == {"scale": 2048.0, "growth_tracker": 0, "skipped_steps": 1, "applied_steps": 0, "found_inf": 1}
        assert torch.equal(step.ctx.t.cpu(), ctx0) and not step.buf.t.any()


# ------------------------------------------------------------------------------------------------------------------------ 3. sequence
@pytest.mark.parametrize("per_class", [False, True], ids=["generic", "per_class"])
@pytest.mark.parametrize("name", sorted(ref.SEQUENCES))
def test_sequence_equals_the_restatement(name, per_class):
    """The CPU test's found-inf patterns (growth_interval = 2): state, ctx and buf equal tests/scalerfit_ref.py exactly after every call --
    a skip on the very first call (the next clean call initialises the momentum buffer), two skips in a row, growth after a skip, the
    growth from 2^127 that is not taken."""
    C, D, n_ctx, lr = 5, 96, 3, 2.0 ** -3
    seq = ref.SEQUENCES[name]
    ctx0, ints = ref.exact_inputs(C, L, D, n_ctx, per_class, len(seq["pattern"]), seed=2)
    r = ref.ScalerRef(ctx0, C, L, n_ctx, per_class, seq["init_scale"], 2.0, 0.5, 2, momentum=0.5)
    step = ScaledStep(ctx0, C, D, n_ctx, per_class, seq["init_scale"], 2.0, 0.5, 2, momentum=0.5, weight_decay=0.0)
    for k, poison in enumerate(seq["pattern"]):
        d = ref.scaled_embed(ints[k], float(r.scale))
        if poison:
            d[(k % C if per_class else C - 1) * L + 1 + k % n_ctx, (5 * k) % D] = ref.POISON[k % 3]
        st = step(d, lr)
        assert r.step(d, lr) == bool(poison)
        assert st == r.state(), (k, st, r.state())
        assert np.array_equal(step.ctx.t.cpu().numpy(), r.ctx), k
        assert np.array_equal(step.buf.t.cpu().numpy(), r.buf if r.buf is not None else np.zeros_like(r.ctx)), k
        if not poison:
            assert np.array_equal(step.grad.t.cpu().numpy(), r.grad), k
    assert r.applied_steps >= 3 and r.skipped_steps >= 1


def test_grad_scale_rows_reads_the_block():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(37, 516, generator=g)
    for scale in (1.0, 4096.0, 2.0 ** -3):
        out = Guarded(x.numel() * 4, shape=tuple(x.shape), init=x)
        ops.grad_scale_rows(out.t, ops.new_scaler_state(scale, "cuda"))
        torch.cuda.synchronize()
        assert out.intact() and torch.equal(out.t.cpu(), x * scale)


# ------------------------------------------------------------------------------------------------------------- 4. end to end, no overflow
@functools.lru_cache(maxsize=None)
def model(geom):
    return build_model(dict(coopfit_ref.state_dict(geom)), {"trainer": "CoOp"}).cuda()


RATES = [2e-3, 1e-3, 5e-4]


def run_steps(c, geom, method, steps, one_call=False, rates=None, **opt):
    """`steps` CoOpFitState steps on the case's one batch: (ctx, buf, losses, the state)."""
    if method != "coop":
        opt = dict(opt, method=method, teacher=c["teacher"].cuda())
    st = coopfit.CoOpFitState(model(geom), c["ids"], c["ctx"], coopfit_ref.LOGIT_SCALE, **SGD, **opt)
    f, y = c["feats"].cuda(), c["labels"].cuda()
    lr = torch.tensor(rates or RATES, dtype=torch.float32).cuda()
    losses = [st.step(f, y, lr[k % lr.numel():k % lr.numel() + 1], want_loss=True, one_call=one_call) for k in range(steps)]
    torch.cuda.synchronize()
    return st.ctx.cpu(), st.buf.cpu(), torch.cat(losses).cpu(), st


@pytest.mark.parametrize("method", ["coop", "kgcoop"])
@pytest.mark.parametrize("geom", ["tiny", "tiny3"])
def test_dynamic_without_overflow_gives_the_static_bits(geom, method):
    c = promptfit_ref.case((geom, 3, 4, 8, False))
    ctx_s, buf_s, loss_s, _ = run_steps(c, geom, method, 3, grad_scale=4096.0)
    assert torch.isfinite(ctx_s).all() and not torch.equal(ctx_s, c["ctx"])
    scaler = {"init_scale": 2.0 ** 12, "growth_interval": 1000}
    for one_call in (False, True):
        ctx_d, buf_d, loss_d, st = run_steps(c, geom, method, 3, one_call=one_call, grad_scale="dynamic", scaler=scaler)
        assert st.scaler_state() == {"scale": 4096.0, "growth_tracker": 3, "skipped_steps": 0, "applied_steps": 3, "found_inf": 0}
        assert torch.equal(ctx_d, ctx_s) and torch.equal(buf_d, buf_s) and torch.equal(loss_d, loss_s), one_call
    kw = {} if method == "coop" else {"method": method, "teacher": c["teacher"].cuda()}
    ctx_f, hist = coopfit.fit_context(c["feats"].cuda(), c["labels"], model(geom), c["ids"], c["ctx"], epochs=3, batch_size=8, lr_per_epoch=RATES,
                                      logit_scale=coopfit_ref.LOGIT_SCALE, return_history=True, grad_scale="dynamic", scaler=scaler, **SGD, **kw)
    assert torch.equal(ctx_f.cpu(), ctx_s) and np.array_equal(hist, loss_s.numpy())


# ------------------------------------------------------------------------------------------------------ 5. end to end, overflow and recovery
@pytest.mark.parametrize("method", ["coop", "kgcoop"])
@pytest.mark.parametrize("geom", ["tiny", "tiny3"])
def test_overflow_is_skipped_and_the_fit_recovers(geom, method):
    """The largest fp16 operand magnitude m of a static 2^12 step is measured; the run starts at the smallest power of two
    >= 2^12 (65504 / m) 2^4, where the static path demonstrably ends non-finite, with a backoff of 2^-8 on the same batch every step.
    After k applied steps ctx lies within 2 x the distance between static runs of k steps at 2^10 and 2^14 of a static 2^12 run.

    On `tiny3` that yardstick does not exist: m = 17504 at 2^12 leaves 2^1.9 of fp16 headroom, so the static run at 2^14 overflows by
    itself and the distance is NaN.  The test then asks for more, not less: the bits of the static 2^12 run (a bound of 0), which is what
    a power-of-two scale gives as long as no operand overflows or falls into the subnormals (measured: 0 on both geometries)."""
    steps, lr = 6, [1e-3]
    c = promptfit_ref.case((geom, 3, 4, 8, False))
    kw = {} if method == "coop" else {"method": method, "teacher": c["teacher"].cuda()}
    stats = coopfit.context_gradient(model(geom), c["ids"], c["ctx"], c["feats"].cuda(), c["labels"], coopfit_ref.LOGIT_SCALE, grad_scale=4096.0,
                                     return_operand_stats=True, **kw)[-1]
    m = stats["max"]
    assert math.isfinite(m) and m > 0.0
    init = 2.0 ** math.ceil(math.log2(4096.0 * (65504.0 / m) * 16.0))
    say(f"{geom} {method}: largest fp16 operand at 2^12 m = {m:g}; init_scale 2^{int(math.log2(init))}")
    ctx_o = run_steps(c, geom, method, 1, rates=lr, grad_scale=init)[0]
    assert not torch.isfinite(ctx_o).all(), "the static path survives the scale chosen to overflow"
    ctx_d, buf_d, loss_d, st = run_steps(c, geom, method, steps, rates=lr, grad_scale="dynamic",
                                         scaler={"init_scale": init, "backoff_factor": 2.0 ** -8, "growth_interval": 1000})
    s = st.scaler_state()
    k = s["applied_steps"]
    say(f"{geom} {method}: {s['skipped_steps']} skipped, {k} applied of {steps}; final scale 2^{math.log2(s['scale']):g}")
    assert s["skipped_steps"] >= 1 and k + s["skipped_steps"] == steps and k >= 1
    assert torch.isfinite(ctx_d).all() and torch.isfinite(buf_d).all() and loss_d.shape == (steps,)
    assert s["scale"] == init * (2.0 ** -8) ** s["skipped_steps"]
    ctx_12 = run_steps(c, geom, method, k, rates=lr, grad_scale=4096.0)[0]
    ctx_10 = run_steps(c, geom, method, k, rates=lr, grad_scale=1024.0)[0]
    ctx_14 = run_steps(c, geom, method, k, rates=lr, grad_scale=16384.0)[0]
    spread = float((ctx_10 - ctx_14).abs().max())
    dist = float((ctx_d - ctx_12).abs().max())
    bound = 2.0 * spread if math.isfinite(spread) else 0.0        # no yardstick (the static 2^14 run overflows): the static 2^12 bits
    say(f"{geom} {method}: after {k} applied steps max |dynamic - static 2^12| = {dist:.3e}; max |static 2^10 - static 2^14| = {spread:.3e}, "
        f"bound {bound:.3e}")
    assert torch.isfinite(ctx_12).all() and dist <= bound
