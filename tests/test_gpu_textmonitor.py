"""Per-epoch validation of the CoCoOp and ProDA fits on the GPU (cocoopfit.fit_prompt_learner / prodafit.fit_context with ``val=``,
CoCoOpFitState / ProDAFitState.validate) on the `tiny` model: 5 classes, 4 context vectors, 70 validation rows (the 64-row partition of
the score is crossed), batches of 2, 3 epochs of 2 steps; ProDA with 8 contexts in slices of 2 -- all three positions are present and a
training step sees a strict subset of the contexts (6 contexts, which the request names, is refused by ProDAFitState as by the reference:
the collection must be a multiple of 4; 8 is the smallest that keeps both properties).

The record is held to the INFERENCE forward: record e equals, byte for byte, ``ops.val_score`` on the logits ``trainers.cocoop.CustomCLIP``
/ ``trainers.proda.CustomCLIP`` give with the parameters after epoch e.  The numbers are held to float64 (tests/textmonitor_ref.py, on the
tower's raw text features) with the bound of tests/test_gpu_fitmonitor_ops.py (``hold_sums``: counts exactly, sums within
max(2 x torch's fp32 distance, 2^-22 relative)) on the forward's logits, and those logits to the float64 restatement within the bounds
derived in tests/textmonitor_ref.py and tests/tail_ref.py."""
import functools

import numpy as np
import pytest
import torch

import cocoopfit_ref as cref
import coopfit_ref
import fitmonitor_ref as ref
import prodafit_ref as dref
import tail_ref
import textmonitor_ref as tref
from test_gpu_fitmonitor_ops import hold_sums

pytestmark = pytest.mark.gpu

from clip_calibration_amd import cocoopfit, ops, prodafit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
from clip_calibration_amd.trainers import cocoop, proda  # noqa: E402

GRAD_SCALE = 256.0     # tests/test_gpu_coopfit.py: the synthetic weights' gradients are large
C, N_CTX, N_TRAIN, N_VAL, BATCH, EPOCHS = 5, 4, 4, 70, 2, 3
P, PB = 8, 2
LS = cref.LOGIT_SCALE
RATES = [2e-3, 1e-3, 5e-4]
SGD = dict(momentum=0.9, weight_decay=5e-4)
SCALES = {"static": dict(grad_scale=GRAD_SCALE), "dynamic": dict(grad_scale="dynamic", scaler=dict(init_scale=GRAD_SCALE))}
NAMES = cocoopfit.NAMES


@functools.lru_cache(maxsize=None)
def model():
    return build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"}).cuda()


@functools.lru_cache(maxsize=None)
def data():
    g = torch.Generator().manual_seed(123)
    E = 128
    centres = torch.randn(C, E, generator=g)
    y = torch.arange(N_TRAIN) % C
    vy = torch.arange(N_VAL) % C
    return {"feats": (centres[y] + 0.3 * torch.randn(N_TRAIN, E, generator=g)).cuda(), "labels": y,
            "val": (centres[vy] + 0.6 * torch.randn(N_VAL, E, generator=g)).cuda(), "val_labels": vy}


class CoCoOp:
    name = "cocoop"

    def __init__(self):
        c = cref.make_case("tiny", C, N_CTX, N_TRAIN)
        self.ids, self.start = c["ids"], {k: v.clone() for k, v in c["params"].items()}

    def state(self, params=None, **kw):
        kw = dict(SGD, **(kw or SCALES["static"]))
        return cocoopfit.CoCoOpFitState(model(), self.ids, self.start if params is None else params, logit_scale=LS, **kw)

    def block(self, st):
        return st.block

    def fit(self, rates, **kw):
        kw.setdefault("grad_scale", GRAD_SCALE)
        d = data()
        out = cocoopfit.fit_prompt_learner(d["feats"], d["labels"], model(), self.ids, self.start, logit_scale=LS, epochs=len(rates), batch_size=BATCH,
                                           lr_per_epoch=list(rates), **SGD, **kw)
        return out if isinstance(out, tuple) else (out,)

    def flat(self, fitted):
        return torch.cat([fitted[k].reshape(-1) for k in NAMES])

    def params_of(self, block, st):
        return {k: v.clone() for k, v in ops.cocoop_block_views(block.clone(), st.n_ctx, st.D, st.E, st.H).items()}

    def trainer(self, st=None, params=None):
        clip = cocoop.CustomCLIP(model(), self.ids, n_ctx=N_CTX, logit_scale=None if st is None else st.scale)
        if params is not None:
            clip.prompt_learner.load_state_dict(params, strict=False)
        return clip

    def inference(self, st, params, feats):
        """(the forward's logits fp32 [N, C], the float64 restatement's, its bound) at ``params``."""
        m, clip = model(), self.trainer(st, params)
        try:
            m.image_features_f32 = lambda image: image
            z = clip(feats)[0]
        finally:
            del m.image_features_f32
        txt = clip.per_image_text_features(ops.l2_normalize(feats))
        z64 = tref.cocoop_logits(feats.cpu().numpy(), txt.cpu().numpy(), st.scale)
        return z, z64, np.full(z64.shape, tref.cocoop_logit_bound(feats.shape[1], st.scale))

    def validate(self, st, e, chunk=None):
        d = data()
        st.validate(d["val"], d["val_labels"], e, chunk)

    chunks = (1, 3, 70)

    def train_fit(self, clip, **kw):
        return clip.fit_prompt_learner([(data()["feats"], data()["labels"])], batch_size=BATCH, logit_scale=LS, **SGD, **kw)

    def module_params(self, clip):
        return torch.cat([dict(clip.prompt_learner.named_parameters())[k].detach().float().reshape(-1) for k in NAMES])


class ProDA:
    name = "proda"

    def __init__(self):
        c = dref.make_case("tiny", C, N_CTX, P, PB, N_TRAIN)
        self.ids, self.start = c["ids"], c["ctx"].clone()

    def state(self, params=None, **kw):
        kw = dict(SGD, **(kw or SCALES["static"]))
        return prodafit.ProDAFitState(model(), self.ids, self.start if params is None else params, prompt_bs=PB, logit_scale=LS,
                                      generator=torch.Generator().manual_seed(5), **kw)

    def block(self, st):
        return st.ctx

    def fit(self, rates, **kw):
        kw.setdefault("grad_scale", GRAD_SCALE)
        d = data()
        out = prodafit.fit_context(d["feats"], d["labels"], model(), self.ids, self.start, prompt_bs=PB, logit_scale=LS, epochs=len(rates),
                                   batch_size=BATCH, lr_per_epoch=list(rates), generator=torch.Generator().manual_seed(5), **SGD, **kw)
        return out if isinstance(out, tuple) else (out,)

    def flat(self, fitted):
        return fitted.reshape(-1)

    def params_of(self, block, st):
        return block.clone()

    def trainer(self, st=None, params=None):
        clip = proda.CustomCLIP(model(), self.ids, n_ctx=N_CTX, n_prompt=P, logit_scale=None if st is None else st.scale)
        if params is not None:
            with torch.no_grad():
                clip.prompt_learner.ctx.copy_(params)
        return clip

    def inference(self, st, params, feats):
        m, clip = model(), self.trainer(st, params)
        try:
            m.image_features_f32 = lambda image: image
            z = clip(feats)[0]
        finally:
            del m.image_features_f32
        prompts, tokenized = clip.prompt_learner(infer=True)
        text = clip.text_encoder(prompts.contiguous(), tokenized).cpu().numpy()
        f = feats.cpu().numpy()
        z64 = tref.proda_logits(f, text, P, st.scale)
        # the fused tail's own bound on the device's means (tests/tail_ref.py) plus the means' distance from float64 through |x_n|
        _, tol, x64 = tail_ref.cosine_logits(feats.cpu(), clip.text_features.cpu(), st.scale, True)
        slack = abs(float(np.float32(st.scale))) * np.abs(x64.numpy()) @ tref.mean_bound(text, P).T
        return z, z64, tol.numpy() + slack

    def validate(self, st, e, chunk=None):
        d = data()
        st.validate(d["val"], d["val_labels"], e, chunk)

    chunks = (1, 2, 5)

    def train_fit(self, clip, **kw):
        return clip.fit_context([(data()["feats"], data()["labels"])], batch_size=BATCH, prompt_bs=PB, logit_scale=LS, **SGD, **kw)

    def module_params(self, clip):
        return clip.prompt_learner.ctx.detach().float().reshape(-1)


@functools.lru_cache(maxsize=None)
def method(name):
    return CoCoOp() if name == "cocoop" else ProDA()


FITS = ["cocoop", "proda"]


def run_epochs(st, rates, one_call=False, validate=None):
    """The state's own loop over the training rows in batches of BATCH; ``validate(st, e)`` behind every epoch.  Returns the block after
    every epoch."""
    d, blocks = data(), []
    labels = d["labels"].cuda()
    for e, lr in enumerate(rates):
        for lo in range(0, N_TRAIN, BATCH):
            st.step(d["feats"][lo:lo + BATCH], labels[lo:lo + BATCH], lr, one_call=one_call)
        if validate is not None:
            validate(st, e)
        blocks.append((st.block if hasattr(st, "block") else st.ctx).clone())
    return blocks


@pytest.mark.parametrize("name", FITS)
def test_the_fit_takes_val_and_returns_a_monitor_of_every_epoch(name):
    """On the parent commit this is a TypeError: neither fit takes ``val``."""
    m, d = method(name), data()
    fitted, mon = m.fit(RATES, val=(d["val"], d["val_labels"]), return_monitor=True)
    assert len(mon["records"]) == EPOCHS and mon["accuracy"].shape == (EPOCHS,) and mon["best_epoch"] is None
    assert all(r["n"] == N_VAL for r in mon["records"]) and np.isfinite(mon["nll"]).all()
    assert torch.isfinite(m.flat(fitted)).all()


@pytest.mark.parametrize("scale", ["static", "dynamic"])
@pytest.mark.parametrize("one_call", [False, True], ids=["separate", "one-call"])
@pytest.mark.parametrize("name", FITS)
def test_validation_leaves_the_fit_unchanged(name, one_call, scale):
    m = method(name)
    plain, watched = m.state(**SCALES[scale]), m.state(**SCALES[scale])
    a = run_epochs(plain, RATES, one_call)
    b = run_epochs(watched, RATES, one_call, validate=m.validate)
    assert torch.isfinite(a[-1]).all() and not torch.equal(a[-1].reshape(-1).cpu(), m.flat(m.start).float().reshape(-1))
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "the fitted block differs"
    assert torch.equal(plain.buf.view(torch.int32), watched.buf.view(torch.int32)), "the momentum block differs"
    if scale == "dynamic":
        assert plain.scaler_state() == watched.scaler_state()
    if name == "proda":     # validation draws nothing: the schedule's generator stands where the plain run's stands
        assert torch.equal(plain.generator.get_state(), watched.generator.get_state()) and np.array_equal(plain._perm, watched._perm)
    assert watched.monitor()["accuracy"].shape == (EPOCHS,)
    # the fit functions: with val the bits of the fit without
    d = data()
    f0 = m.fit(RATES, **SCALES[scale])[0]
    f1, mon = m.fit(RATES, val=(d["val"], d["val_labels"]), return_monitor=True, **SCALES[scale])
    assert torch.equal(m.flat(f0).view(torch.int32), m.flat(f1).view(torch.int32)) and len(mon["records"]) == EPOCHS


@pytest.mark.parametrize("name", FITS)
def test_the_record_is_the_inference_forwards(name):
    m, d = method(name), data()
    st = m.state()
    blocks = run_epochs(st, RATES, validate=m.validate)
    mon = st.monitor()
    got = ops.encode_val_records(mon["records"], 10)
    y = d["val_labels"].numpy()
    for e in range(EPOCHS):
        z, z64, bound = m.inference(st, m.params_of(blocks[e], st), d["val"])
        want = ops.val_score(z, d["val_labels"].cuda(), 10).cpu().numpy()
        assert np.array_equal(want, got[e]), f"record {e} is not val_score's on the inference forward's logits"
        zd = z.cpu().numpy()
        err = np.abs(zd - z64)
        print(f"textmonitor-parity: {name} epoch {e}: max |logit - float64| {err.max():.3e}, worst ratio to its bound {(err / bound).max():.3f}; "
              f"accuracy {mon['accuracy'][e]:.4f} nll {mon['nll'][e]:.6f} ece {mon['ece'][e]:.6f}")
        assert (err <= bound).all(), "the forward's logits leave the float64 restatement's bound"
        wd, r64 = ref.record(zd, y, 10), tref.record(z64, y, 10)
        hold_sums(f"{name} epoch {e}", mon["records"][e], wd, zd, y, 10)
        assert mon["accuracy"][e] == wd["correct"] / N_VAL
        # float64 on the forward's logits against float64 on the restatement's: a row whose top-2 gap exceeds twice the logit bound keeps its
        # prediction, and a row's nll (log-sum-exp minus the label's logit) moves by at most twice the largest logit error
        top = np.sort(z64, axis=1)
        unsafe = int(((top[:, -1] - top[:, -2]) <= 2 * bound.max()).sum())
        assert abs(wd["correct"] - r64["correct"]) <= unsafe
        assert abs(wd["nll_sum"] - r64["nll_sum"]) <= 2 * N_VAL * bound.max() + 1e-9


@pytest.mark.parametrize("name", FITS)
def test_the_record_does_not_depend_on_the_chunking(name):
    m = method(name)
    st = m.state()
    run_epochs(st, RATES[:1])
    for k, chunk in enumerate(m.chunks):
        m.validate(st, k, chunk)
    recs = st.monitor_records()[:len(m.chunks)].cpu().numpy()
    for k in range(1, len(m.chunks)):
        assert np.array_equal(recs[0], recs[k]), f"chunks of {m.chunks[k]} and of {m.chunks[0]} give different records"
    m.validate(st, 0, m.chunks[0])
    assert np.array_equal(st.monitor_records()[0].cpu().numpy(), recs[0]), "two runs differ"


@pytest.mark.parametrize("criterion", ["accuracy", "nll"])
@pytest.mark.parametrize("name", FITS)
def test_selection_keeps_the_better_earlier_epoch(name, criterion):
    m, d = method(name), data()
    rates = [2e-3, 1e3]      # the second epoch wrecks the model
    probe = m.state()
    blocks = run_epochs(probe, rates)
    # labels from the float64 restatement at epoch 0, two of them moved off: epoch 0 is good but not perfect
    _, z0, _ = m.inference(probe, m.params_of(blocks[0], probe), d["val"])
    labels = z0.argmax(axis=1)
    labels[:2] = (labels[:2] + 1) % C
    _, z1, _ = m.inference(probe, m.params_of(blocks[1], probe), d["val"])
    r0, r1 = tref.record(z0, labels, 10), tref.record(z1, labels, 10)
    print(f"textmonitor: {name} float64 correct {r0['correct']} -> {r1['correct']}, nll_sum {r0['nll_sum']:.4f} -> {r1['nll_sum']:.4f}")
    assert tref.worse(r1, r0), "the wrecking rate did not make epoch 1 strictly worse in float64: the selection is not exercised"
    vl = torch.from_numpy(labels)
    st = m.state()
    st.start_monitor(2, 10, True, criterion)
    assert torch.equal(m.flat(st.best_params()), m.block(st).reshape(-1)), "before any epoch the best slot is the starting block"
    run_epochs(st, rates, validate=lambda s, e: s.validate(d["val"], vl, e))
    mon = st.monitor()
    assert mon["best_epoch"] == 0 == ref.best_epoch(mon["records"], criterion)
    assert torch.equal(m.flat(st.best_params()).view(torch.int32), blocks[0].reshape(-1).view(torch.int32))
    # the fit function and the trainer: best_val returns and installs epoch 0's block
    fitted, mon2 = m.fit(rates, val=(d["val"], vl), final_model="best_val", val_criterion=criterion, return_monitor=True)
    assert mon2["best_epoch"] == 0 and torch.equal(m.flat(fitted).view(torch.int32), blocks[0].reshape(-1).view(torch.int32))
    last = m.fit(rates, val=(d["val"], vl), val_criterion=criterion)[0]
    assert torch.equal(m.flat(last).view(torch.int32), blocks[1].reshape(-1).view(torch.int32))
    clip, mod = m.trainer(), model()
    start = m.module_params(clip).clone()
    try:
        mod.image_features_f32 = lambda image: image
        out = m.train_fit(clip, val_loader=[(d["val"][:30], vl[:30]), (d["val"][30:], vl[30:])], final_model="best_val", val_criterion=criterion,
                          return_monitor=True, epochs=2, lr_per_epoch=rates, grad_scale=GRAD_SCALE)
        with pytest.raises(ValueError, match="val_loader and val"):
            m.train_fit(clip, val_loader=[(d["val"], vl)], val=(d["val"], vl), epochs=1)
    finally:
        del mod.image_features_f32
    assert out[-1]["best_epoch"] in (0, -1) and len(out[-1]["records"]) == 2
    installed = m.module_params(clip)
    assert torch.equal(installed, m.flat(out[0]).to(mod.dtype).float()) and torch.isfinite(installed).all()      # stored in the module's type
    assert out[-1]["best_epoch"] == -1 or not torch.equal(installed, start)


@pytest.mark.parametrize("criterion", ["accuracy", "nll"])
@pytest.mark.parametrize("name", FITS)
def test_ties_keep_the_earlier_epoch_and_a_nan_epoch_is_never_taken_under_nll(name, criterion):
    m, d = method(name), data()
    st = m.state()
    st.start_monitor(3, 10, True, criterion)
    run_epochs(st, RATES[:1])
    kept = m.block(st).clone()
    m.validate(st, 0)
    m.validate(st, 1)                      # the same parameters again: a tie
    mon = st.monitor()
    assert mon["records"][0]["correct"] == mon["records"][1]["correct"] and mon["records"][0]["nll_sum"] == mon["records"][1]["nll_sum"]
    assert mon["best_epoch"] == 0
    m.block(st).fill_(float("nan"))        # an all-NaN epoch
    m.validate(st, 2)
    mon = st.monitor()
    assert mon["records"][2]["correct"] == 0 and np.isnan(mon["records"][2]["nll_sum"])
    assert mon["best_epoch"] == 0 and torch.equal(m.flat(st.best_params()).view(torch.int32), kept.reshape(-1).view(torch.int32))
    fresh = m.state()
    fresh.start_monitor(1, 10, True, "nll")
    m.block(fresh).fill_(float("nan"))
    m.validate(fresh, 0)
    assert fresh.monitor()["best_epoch"] == -1, "an all-NaN epoch was taken under nll"
