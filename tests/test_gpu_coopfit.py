"""CoOp's training on the GPU end to end (clip_calibration_amd/coopfit.py, csrc/text_backward.hip, csrc/prompt_train.hip) on the `tiny` and `tiny3` geometries
against float64 autograd through the oracle (tests/coopfit_ref.py).

The parity bound is computed here, at run time: the error measure is the relative Frobenius error of the context's gradient against
float64, the yardstick is the same error of the oracle's autograd at dtype float16 on the CPU (the reference's own precision for CoOp,
PREC fp16), and the device must stay within 2 x the yardstick -- it rounds GEMM operands to fp16 where the fp16 reference does and
accumulates in fp32; the factor covers the rounding points that differ (QuickGELU's derivative from the fp16 pre-activation, fp16 P and dS
in the attention backward).  Every test prints its figures on lines that start with "coopfit-parity:"; profiles/coopfit_parity.txt is
one run's lines."""
import functools

import numpy as np
import pytest
import torch

import coopfit_ref as ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import coopfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
from clip_calibration_amd.trainers.coop import CustomCLIP  # noqa: E402

FACTOR = 2.0
# The synthetic `tiny` / `tiny3` weights give gradients an order of magnitude larger than the ViT-B/16 geometry the default grad_scale
# (2^12) was measured on (|d ctx| up to 158 here): the tests run at 2^8, the larger of the two scales the parity test compares.
GRAD_SCALE = 256.0


def say(line):
    print("coopfit-parity: " + line)


@functools.lru_cache(maxsize=None)
def model(geom):
    return build_model(dict(ref.state_dict(geom)), {"trainer": "CoOp"}).cuda()


@functools.lru_cache(maxsize=None)
def oracle(key, far=False):
    """(case, float64 loss, float64 gradient, yardstick error, how the yardstick was made), computed once per case."""
    c = ref.make_case(*key, far=far)
    loss, grad = ref.oracle_loss_grad(c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"])
    yard, how = ref.yardstick_grad(c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"])
    return c, float(loss), grad, ref.rel_fro(yard, grad), how


def device_gradient(c, geom, **kw):
    kw.setdefault("grad_scale", GRAD_SCALE)
    loss, grad = coopfit.context_gradient(model(geom), c["ids"], c["ctx"], c["feats"].cuda(), c["labels"], ref.LOGIT_SCALE, **kw)[:2]
    return float(loss.cpu()[0]), grad.cpu()


@pytest.mark.parametrize("seq_rows", [None, 0], ids=["cut", "full"])
@pytest.mark.parametrize("key", ref.GRADIENT_CASES, ids=lambda k: "-".join(str(v) for v in k))
def test_context_gradient_against_float64(key, seq_rows):
    c, loss64, grad64, yard, how = oracle(key)
    loss, grad = device_gradient(c, key[0], seq_rows=seq_rows)
    err = ref.rel_fro(grad, grad64)
    say(f"gradient {key} seq_rows={seq_rows} loss {loss:.6f} vs {loss64:.6f}; rel. Frobenius error {err:.3e}, yardstick ({how}) {yard:.3e}, "
        f"ratio {err / yard:.2f}")
    assert grad.shape == c["ctx"].shape and torch.isfinite(grad).all()
    # the loss: logits of scale 100 from features with fp16-operand error; the fp16 reference's own loss error is of the yardstick's order
    assert abs(loss - loss64) <= FACTOR * yard * max(1.0, abs(loss64))
    assert err <= FACTOR * yard


def test_eot_on_the_last_token_of_the_context():
    key = ("tiny", 3, 4, 8, False)
    c, loss64, grad64, yard, how = oracle(key, far=True)
    loss, grad = device_gradient(c, "tiny")
    err = ref.rel_fro(grad, grad64)
    say(f"gradient {key} far EOT: rel. Frobenius error {err:.3e}, yardstick ({how}) {yard:.3e}, ratio {err / yard:.2f}")
    assert err <= FACTOR * yard


@pytest.mark.parametrize("key", [("tiny", 37, 4, 33, False), ("tiny3", 3, 16, 33, False)], ids=lambda k: "-".join(str(v) for v in k))
def test_grad_scale_1_and_256_agree(key):
    c, _, grad64, yard, _ = oracle(key)
    _, g1 = device_gradient(c, key[0], grad_scale=1.0)
    _, g256 = device_gradient(c, key[0], grad_scale=256.0)
    say(f"grad_scale {key}: error at 1 {ref.rel_fro(g1, grad64):.3e}, at 2^8 {ref.rel_fro(g256, grad64):.3e}, between them "
        f"{ref.rel_fro(g1, g256):.3e}, bit-equal {torch.equal(g1, g256)}")
    assert ref.rel_fro(g1, grad64) <= FACTOR * yard and ref.rel_fro(g256, grad64) <= FACTOR * yard
    assert ref.rel_fro(g1, g256) <= FACTOR * yard


def three_steps(c, geom, how, **opt):
    rates = [2e-3, 1e-3, 5e-4]
    m = model(geom)
    f, y = c["feats"].cuda(), c["labels"].cuda()
    if how == "fit":
        ctx, hist = coopfit.fit_context(f, c["labels"], m, c["ids"], c["ctx"], epochs=3, batch_size=f.shape[0], lr_per_epoch=rates,
                                        return_history=True, **opt)
        return ctx.cpu(), hist
    st = coopfit.CoOpFitState(m, c["ids"], c["ctx"], ref.LOGIT_SCALE, **opt)
    lr = torch.tensor(rates, dtype=torch.float32).cuda()
    losses = [st.step(f, y, lr[k:k + 1], want_loss=True, one_call=(how == "one_call")) for k in range(3)]
    return st.ctx.cpu(), torch.cat(losses).cpu().numpy()


@pytest.mark.parametrize("key", [("tiny", 3, 4, 8, False), ("tiny3", 37, 4, 1, True)], ids=lambda k: "-".join(str(v) for v in k))
def test_three_steps_same_bits_every_way(key):
    c = oracle(key)[0]
    opt = dict(momentum=0.9, dampening=0.0, nesterov=False, weight_decay=5e-4, grad_scale=GRAD_SCALE)
    a, la = three_steps(c, key[0], "step", **opt)
    b, lb = three_steps(c, key[0], "fit", **opt)
    d, ld = three_steps(c, key[0], "one_call", **opt)
    e, le = three_steps(c, key[0], "step", **opt)
    assert torch.isfinite(a).all() and not torch.equal(a, c["ctx"])
    assert torch.equal(a, b) and np.array_equal(la, lb)
    assert torch.equal(a, d) and np.array_equal(la, ld)
    assert torch.equal(a, e) and np.array_equal(la, le)          # two runs, the same bits


def two_one_call_steps(c, geom, symbol, want_loss=True):
    """Two steps through one of the library's one-call symbols from a fresh state: (ctx, buf, losses [2], grad_out [2, ...])."""
    import ctypes

    from clip_calibration_amd import _lib, ops
    lib, m = _lib.lib, model(geom)
    st = coopfit.CoOpFitState(m, c["ids"], c["ctx"], ref.LOGIT_SCALE, momentum=0.9, dampening=0.0, nesterov=False, weight_decay=5e-4,
                              grad_scale=GRAD_SCALE)
    t, f, y = st.tower, c["feats"].cuda(), c["labels"].cuda()
    lr = torch.tensor([2e-3, 1e-3], dtype=torch.float32).cuda()
    losses, grads = torch.zeros(2, 3).cuda(), torch.zeros(2, *st.ctx.shape).cuda()
    ws = t.one_call_workspace(f.shape[0])
    for k in range(2):
        head = (m._handle, ctypes.byref(t.dgrad[0]), t.base.data_ptr(), coopfit._DT[t.base.dtype], st.ctx.data_ptr(), st.buf.data_ptr(), t.n_ctx,
                int(t.per_class), t.eot.data_ptr(), t.C, t.rows, f.data_ptr(), f.stride(0), y.data_ptr(), f.shape[0], st.scale, GRAD_SCALE)
        sgd = (lr[k:k + 1].data_ptr(), int(k == 0), 0.9, 0.0, 5e-4, 0)
        tail = (ws.data_ptr(), ws.numel(), t.stash.data_ptr(), t.stash.numel(), ops._stream())
        with m._launch_lock:
            if symbol == "coop":
                rc = lib.clipmi_coop_train_step(*head, *sgd, losses[k].data_ptr() if want_loss else None, grads[k].data_ptr(), *tail)
            else:
                rc = lib.clipmi_prompt_train_step(*head, _lib.PROMPT_COOP, None, 0.0, 0.0, 0.0, *sgd, losses[k].data_ptr(), grads[k].data_ptr(), None,
                                                  None, *tail)
        assert rc == _lib.OK, _lib.last_error()
    return st.ctx.cpu(), st.buf.cpu(), losses[:, 0].cpu(), grads.cpu()


@pytest.mark.parametrize("key", [("tiny", 3, 4, 4, False), ("tiny3", 37, 4, 4, True)], ids=lambda k: "-".join(str(v) for v in k))
def test_coop_train_step_is_mode_0_of_prompt_train_step(key):
    """coopfit steps through clipmi_prompt_train_step alone; CoOp's own symbol is held to it here: the same bits in the context, the momentum
    buffer, the losses and grad_out over two steps with momentum, and a NULL loss (which only the CoOp symbol takes) changes no other bit."""
    c = ref.make_case(*key)
    ctx, buf, losses, grads = two_one_call_steps(c, key[0], "coop")
    ctx_p, buf_p, losses_p, grads_p = two_one_call_steps(c, key[0], "prompt")
    assert torch.isfinite(ctx).all() and not torch.equal(ctx, c["ctx"]) and torch.isfinite(losses).all() and bool((losses > 0).all())
    assert torch.equal(ctx, ctx_p) and torch.equal(buf, buf_p) and torch.equal(losses, losses_p) and torch.equal(grads, grads_p)
    ctx_n, buf_n, losses_n, grads_n = two_one_call_steps(c, key[0], "coop", want_loss=False)
    assert torch.equal(ctx_n, ctx) and torch.equal(buf_n, buf) and torch.equal(grads_n, grads) and not losses_n.any()


def test_three_steps_against_float64_sgd():
    """The optimiser's rule on top of the gradient: three SGD steps with momentum and weight decay follow torch.optim.SGD on the float64
    oracle within the parity bound of the gradient (relative to the distance the context travels)."""
    key = ("tiny", 3, 4, 8, False)
    c, _, _, yard, _ = oracle(key)
    got, _ = three_steps(c, "tiny", "step", momentum=0.9, dampening=0.0, nesterov=False, weight_decay=5e-4, grad_scale=GRAD_SCALE)
    w, buf = c["ctx"].double(), None
    for k, lr in enumerate([2e-3, 1e-3, 5e-4]):
        _, grad = ref.oracle_loss_grad(c["sd"], c["ids"], w, c["feats"], c["labels"])
        w, buf = ref.sgd_step(w, buf, grad, lr, 0.9, 0.0, 5e-4, False, k == 0)
    moved = float((w - c["ctx"].double()).norm())
    err = float((got.double() - w).norm()) / moved
    say(f"three steps {key}: error {err:.3e} of the distance travelled, yardstick {yard:.3e}")
    # each step's gradient carries the gradient's parity error; the later steps also see the earlier steps' error through the curvature:
    # three times the single-gradient bound
    assert err <= 3 * FACTOR * yard


def separable_batch(C, E, per_class, seed=0):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(C, E, generator=g)
    labels = torch.arange(C).repeat_interleave(per_class)
    return centres[labels] + 0.1 * torch.randn(C * per_class, E, generator=g), labels


def test_custom_clip_fit_context_lowers_the_loss():
    m = model("tiny")
    ids = ref.prompt_ids("tiny", 3, 4)
    clip = CustomCLIP(m, ids, n_ctx=4)
    before_ctx = clip.prompt_learner.ctx.detach().clone()
    before_text = clip.text_features().clone()
    feats, labels = separable_batch(3, 128, 8)
    # the loader's "images" are the separable features themselves, passed through by a stand-in for the image tower: the trainer's own
    # plumbing (caching, the fit, the write-back) runs as it does with images
    loader = [(feats.cuda(), labels)]
    orig = m.image_features_f32
    try:
        m.image_features_f32 = lambda image: image
        fitted, hist = clip.fit_context(loader, epochs=20, lr=0.002, lr_per_epoch=[0.002] * 20, batch_size=24, momentum=0.9, weight_decay=5e-4, grad_scale=GRAD_SCALE,
                                        return_history=True)
    finally:
        del m.image_features_f32
    assert m.image_features_f32.__func__ is orig.__func__
    say(f"CustomCLIP.fit_context: loss {hist[0]:.5f} -> {hist[-1]:.5f} over {len(hist)} steps")
    assert len(hist) == 20 and np.isfinite(hist).all() and hist[-1] < hist[0]
    assert torch.equal(clip.prompt_learner.ctx.detach().float().cpu(), fitted.to(clip.prompt_learner.ctx.dtype).float().cpu())
    assert not torch.equal(clip.prompt_learner.ctx.detach(), before_ctx)
    assert not torch.equal(clip.text_features(), before_text)          # the cache retired with the parameter's version
