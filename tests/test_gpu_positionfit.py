"""CoOp, KgCoOp and ProGrad with the class token in the middle or at the front, on the GPU end to end (clip_calibration_amd/coopfit.py and
trainers/coop.py with ``class_token_position=``, csrc/prompt_position.hip) on the `tiny` and `tiny3` geometries, against float64 autograd
over the reference's torch.cat prompts through the oracle (tests/position_ref.py).

The parity bound is tests/test_gpu_coopfit.py's, computed here at run time: the relative Frobenius error of the context's gradient
against float64 within FACTOR = 2 x the same error of the oracle's autograd at float16 over the same prompts (the reference's own
precision; "fp32-rounded" where this torch build lacks an fp16 CPU op).  Every test prints its figures on lines that start with
"positionfit-parity:"; profiles/positionfit_parity.txt is one run's lines."""
import functools

import numpy as np
import pytest
import torch

import coopfit_ref as ref
import position_ref as pos
import promptfit_ref as pfit
from test_gpu_coopfit import separable_batch

pytestmark = pytest.mark.gpu

from clip_calibration_amd import coopfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
from clip_calibration_amd.trainers import CoOpCLIP, KgCoOpCLIP, ProGradFitCLIP  # noqa: E402

FACTOR = 2.0
GRAD_SCALE = 256.0          # as tests/test_gpu_coopfit.py: the synthetic weights give gradients far larger than ViT-B/16's
W = 8.0
COS_TOL = 1e-3              # tests/test_gpu_model.py _feat_close: the bound of the existing CoOp text-feature test
MOVED = ("middle", "front")


def say(line):
    print("positionfit-parity: " + line)


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def model(geom):
    return build_model(dict(ref.state_dict(geom)), {"trainer": "CoOp"}).cuda()


@functools.lru_cache(maxsize=None)
def case(key):
    c = pos.make_case(*key)
    c["teacher"] = pfit.random_teacher(c["ids"].shape[0], c["feats"].shape[1])
    return c


@functools.lru_cache(maxsize=None)
def oracle(key, position, with_teacher=False):
    """(case, float64 parts, float16 parts, how the float16 ones were made), computed once per case and position."""
    c = case(key)
    args = (c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"], position, c["name_lens"], c["teacher"] if with_teacher else None, W)
    yard, how = pos.yardstick_parts(*args)
    assert all(torch.isfinite(g).all() for _, g in yard.values())
    return c, pos.oracle_parts(*args), yard, how


def device(c, geom, position, method="coop", **kw):
    kw.setdefault("grad_scale", GRAD_SCALE)
    if method != "coop":
        kw.update(teacher=c["teacher"].cuda(), w=W)
    out = coopfit.context_gradient(model(geom), c["ids"], c["ctx"], c["feats"].cuda(), c["labels"], ref.LOGIT_SCALE, method=method,
                                   class_token_position=position, **kw)
    return float(out[0].cpu()[0]), out[1].cpu()


# ------------------------------------------------------------------------------------------------------- 1. the context's gradient
@pytest.mark.parametrize("explicit", [False, True], ids=["derived", "explicit"])
@pytest.mark.parametrize("position", MOVED)
@pytest.mark.parametrize("key", pos.GRADIENT_CASES, ids=ident)
def test_context_gradient_against_float64(key, position, explicit):
    c, want, yard, how = oracle(key, position)
    loss64, grad64 = want["coop"]
    y = ref.rel_fro(yard["coop"][1], grad64)
    loss, grad = device(c, key[0], position, name_lens=[int(n) for n in c["name_lens"]] if explicit else None)
    e = ref.rel_fro(grad, grad64)
    say(f"gradient coop {key} {position} name_lens={'explicit' if explicit else 'derived'} loss {loss:.6f} vs {loss64:.6f}; rel. Frobenius error {e:.3e}, "
        f"yardstick ({how}) {y:.3e}, ratio {e / y:.2f}")
    assert grad.shape == c["ctx"].shape and torch.isfinite(grad).all()
    assert abs(loss - loss64) <= FACTOR * y * max(1.0, abs(loss64))
    assert e <= FACTOR * y
    # the position is not a formality: the end route's gradient is far outside the bound
    _, grad_end = device(c, key[0], "end")
    assert ref.rel_fro(grad_end, grad64) > 10 * FACTOR * y


@pytest.mark.parametrize("position", MOVED)
def test_kgcoop_and_prograd_gradients_against_float64(position):
    key = ("tiny", 3, 4, 8, False)
    c, want, yard, how = oracle(key, position, True)
    y = ref.rel_fro(yard["kgcoop"][1], want["kgcoop"][1])
    loss, grad = device(c, key[0], position, "kgcoop")
    e = ref.rel_fro(grad, want["kgcoop"][1])
    say(f"gradient kgcoop {key} {position} loss {loss:.6f} vs {want['kgcoop'][0]:.6f}; rel. Frobenius error {e:.3e}, yardstick ({how}) {y:.3e}, ratio {e / y:.2f}")
    assert abs(loss - want["kgcoop"][0]) <= FACTOR * y * max(1.0, abs(want["kgcoop"][0])) and e <= FACTOR * y
    # ProGrad's applied gradient: the projection of the float64 pair against the one of the float16 pair
    g64, did = pfit.project(want["xe"][1], want["kl"][1], 1.0)
    g16, _ = pfit.project(yard["xe"][1], yard["kl"][1], 1.0)
    y = ref.rel_fro(g16, g64)
    loss, grad, parts = coopfit.context_gradient(model(key[0]), c["ids"], c["ctx"], c["feats"].cuda(), c["labels"], ref.LOGIT_SCALE, grad_scale=GRAD_SCALE,
                                                 method="prograd", teacher=c["teacher"].cuda(), return_parts=True, class_token_position=position)
    e = ref.rel_fro(grad.cpu(), g64)
    say(f"gradient prograd applied {key} {position} xe {float(loss.cpu()):.6f} vs {want['xe'][0]:.6f}, projected {int(parts['projected'].cpu())} vs {int(did)}; "
        f"rel. Frobenius error {e:.3e}, yardstick ({how}) {y:.3e}, ratio {e / y:.2f}")
    assert int(parts["projected"].cpu()) == int(did) and e <= FACTOR * y
    for name in ("xe", "kl"):
        y = ref.rel_fro(yard[name][1], want[name][1])
        assert ref.rel_fro(parts["grad_" + name].cpu(), want[name][1]) <= FACTOR * y


# ------------------------------------------------------------------------------------------------------------- 2. the same bits every way
def three_steps(c, geom, how, method, position, **opt):
    rates = [2e-3, 1e-3, 5e-4]
    m = model(geom)
    f, y = c["feats"].cuda(), c["labels"].cuda()
    if method != "coop":
        opt.update(method=method, teacher=c["teacher"].cuda(), w=W)
    if position is not None:
        opt["class_token_position"] = position
    if how == "fit":
        ctx, hist = coopfit.fit_context(f, c["labels"], m, c["ids"], c["ctx"], epochs=3, batch_size=f.shape[0], lr_per_epoch=rates, return_history=True, **opt)
        return ctx.cpu(), hist
    st = coopfit.CoOpFitState(m, c["ids"], c["ctx"], ref.LOGIT_SCALE, **opt)
    lr = torch.tensor(rates, dtype=torch.float32).cuda()
    losses = [st.step(f, y, lr[k:k + 1], want_loss=True, one_call=(how == "one_call")) for k in range(3)]
    return st.ctx.cpu(), torch.cat(losses).cpu().numpy()


SGD = dict(momentum=0.9, dampening=0.0, nesterov=False, weight_decay=5e-4)


@pytest.mark.parametrize("method", ["coop", "kgcoop", "prograd"])
@pytest.mark.parametrize("key", [("tiny", 3, 4, 8, False), ("tiny3", 37, 5, 33, True)], ids=ident)
def test_three_steps_same_bits_every_way(key, method):
    c = case(key)
    opt = dict(SGD, grad_scale=GRAD_SCALE)
    a, la = three_steps(c, key[0], "step", method, "middle", **opt)
    b, lb = three_steps(c, key[0], "fit", method, "middle", **opt)
    d, ld = three_steps(c, key[0], "one_call", method, "middle", **opt)
    e, le = three_steps(c, key[0], "step", method, "middle", **opt)
    assert torch.isfinite(a).all() and not torch.equal(a, c["ctx"]) and np.isfinite(la).all()
    assert torch.equal(a, b) and np.array_equal(la, lb)
    assert torch.equal(a, d) and np.array_equal(la, ld)
    assert torch.equal(a, e) and np.array_equal(la, le)
    end, _ = three_steps(c, key[0], "step", method, "end", **opt)
    assert not torch.equal(a, end)


@pytest.mark.parametrize("method", ["coop", "kgcoop"])
def test_dynamic_scale_that_never_overflows_gives_the_static_bits(method):
    key = ("tiny", 3, 4, 8, False)
    c = case(key)
    scaler = {"init_scale": GRAD_SCALE, "growth_interval": 1000}
    want, lw = three_steps(c, key[0], "step", method, "front", grad_scale=GRAD_SCALE, **SGD)
    for how in ("step", "one_call", "fit"):
        got, lg = three_steps(c, key[0], how, method, "front", grad_scale="dynamic", scaler=scaler, **SGD)
        assert torch.equal(got, want) and np.array_equal(lg, lw), how


@pytest.mark.parametrize("method", ["coop", "prograd"])
def test_explicit_end_is_the_call_without_the_argument(method):
    key = ("tiny", 3, 4, 8, False)
    c = case(key)
    opt = dict(SGD, grad_scale=GRAD_SCALE)
    for how in ("step", "one_call", "fit"):
        a, la = three_steps(c, key[0], how, method, None, **opt)
        b, lb = three_steps(c, key[0], how, method, "end", **opt)
        assert torch.equal(a, b) and np.array_equal(la, lb), how
    kw = dict(teacher=c["teacher"].cuda()) if method != "coop" else {}
    g0 = coopfit.context_gradient(model(key[0]), c["ids"], c["ctx"], c["feats"].cuda(), c["labels"], grad_scale=GRAD_SCALE, method=method, **kw)[1]
    g1 = coopfit.context_gradient(model(key[0]), c["ids"], c["ctx"], c["feats"].cuda(), c["labels"], grad_scale=GRAD_SCALE, method=method,
                                  class_token_position="end", name_lens=[int(n) for n in c["name_lens"]], **kw)[1]
    assert torch.equal(g0, g1)


# ------------------------------------------------------------------------------------------------------------------------ 3. the trainers
def _cos(a, b):
    a = a / np.linalg.norm(a, axis=-1, keepdims=True)
    b = b / np.linalg.norm(b, axis=-1, keepdims=True)
    return a @ b.T


@pytest.mark.parametrize("cached", [True, False], ids=["cached", "per-batch"])
@pytest.mark.parametrize("csc", [False, True], ids=["generic", "csc"])
@pytest.mark.parametrize("position", MOVED)
def test_custom_clip_text_features_against_the_oracle(position, csc, cached):
    key = ("tiny", 3, 5, 8, csc)
    c = case(key)
    m = model("tiny")
    clip = CoOpCLIP(m, c["ids"], n_ctx=5, csc=csc, class_token_position=position, cache_text_features=cached)
    end = CoOpCLIP(m, c["ids"], n_ctx=5, csc=csc)
    for learner in (clip.prompt_learner, end.prompt_learner):
        with torch.no_grad():
            learner.ctx.copy_(c["ctx"].cuda())
    ctx = clip.prompt_learner.ctx.detach().float().cpu()                      # the learner holds the context in the model's dtype
    want = pos.oracle_text(c["sd"], c["ids"], ctx, position, c["name_lens"], torch.float32).numpy().astype(np.float64)
    got = clip.text_features().cpu().numpy().astype(np.float64)
    got_end = end.text_features().cpu().numpy().astype(np.float64)
    err = float(np.abs(_cos(got, want) - _cos(want, want)).max())
    moved = float(np.abs(_cos(got_end, want) - _cos(want, want)).max())
    say(f"text features CoOpCLIP {position} csc={csc} cached={cached}: cosine error {err:.2e} (bound {COS_TOL:.0e}); the end prompts are {moved:.2e} away")
    assert got.shape == want.shape and np.isfinite(got).all() and err < COS_TOL
    assert np.abs(np.linalg.norm(got, axis=-1) - 1.0).max() < 1e-5
    assert moved > 10 * COS_TOL and not np.array_equal(got, got_end)
    # the prompts themselves: one launch's output is the cat form of what the learner holds
    dtype = m.dtype
    emb = pos.embeddings(c["sd"], c["ids"], dtype).float()
    assert torch.equal(clip.prompt_learner().cpu().float(), pos.cat_prompts(emb, ctx, position, c["name_lens"]))


@pytest.mark.parametrize("cls", [CoOpCLIP, KgCoOpCLIP, ProGradFitCLIP], ids=lambda k: k.__module__.split(".")[-1])
def test_fit_context_at_middle_lowers_the_loss_and_writes_the_context(cls):
    m = model("tiny")
    n_ctx = 4
    ids = pos.proda.prompt_ids("tiny", 3, n_ctx)
    kw = {} if cls is CoOpCLIP else {"zeroshot_tokenized_prompts": ids}
    clip = cls(m, ids, n_ctx=n_ctx, class_token_position="middle", **kw)
    before_ctx = clip.prompt_learner.ctx.detach().clone()
    before_text = clip.text_features().clone()
    feats, labels = separable_batch(3, 128, 8)
    loader = [(feats.cuda(), labels)]      # the "images" are the features themselves, passed through by a stand-in for the image tower
    orig = m.image_features_f32
    seen = {}
    real = coopfit.CoOpFitState.__init__

    def spy(self, *a, **k):
        real(self, *a, **k)
        seen["position"] = self.tower.position
    try:
        m.image_features_f32 = lambda image: image
        coopfit.CoOpFitState.__init__ = spy
        fitted, hist = clip.fit_context(loader, epochs=20, lr=0.002, lr_per_epoch=[0.002] * 20, batch_size=24, momentum=0.9, weight_decay=5e-4,
                                        grad_scale=GRAD_SCALE, return_history=True)
    finally:
        del m.image_features_f32
        coopfit.CoOpFitState.__init__ = real
    assert m.image_features_f32.__func__ is orig.__func__
    say(f"{cls.__module__.split('.')[-1]}.CustomCLIP.fit_context at middle: loss {hist[0]:.5f} -> {hist[-1]:.5f} over {len(hist)} steps")
    assert seen["position"] == 1                                             # the learner's position reached the fit
    assert len(hist) == 20 and np.isfinite(hist).all() and hist[-1] < hist[0]
    after = clip.prompt_learner.ctx.detach()
    assert not torch.equal(after, before_ctx) and torch.equal(after, fitted.to(after.dtype))
    assert not torch.equal(clip.text_features(), before_text)               # the cache retired with the parameter's version
