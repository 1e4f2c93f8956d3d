"""Per-epoch validation and best-val selection of the CoOp-family fits on the GPU (coopfit.fit_context(val=...),
CoOpFitState.validate) on the `tiny` model: a handful of classes, 3-4 epochs, batches of 4.

Fits are bit-reproducible, so the monitor is held to after-the-fact scoring by equality: the record of epoch e is, byte for byte, the
record a fresh state writes for the context of the run truncated behind epoch e.  The monitor's numbers are held to the float64
restatement (tests/fitmonitor_ref.py) on the logits the same kernel produced: counts exactly, sums within max(2 x torch's fp32 distance
from float64, 2^-22 relative)."""
import functools

import numpy as np
import pytest
import torch

import coopfit_ref
import fitmonitor_ref as ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import coopfit, metrics, ops  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
from clip_calibration_amd.trainers.coop import CustomCLIP  # noqa: E402

GRAD_SCALE = 256.0     # tests/test_gpu_coopfit.py: the synthetic weights' gradients are large
C, N_CTX, N_TRAIN, N_VAL, BATCH = 5, 4, 14, 23, 4
WRECK = 1e38           # a rate that takes the context out of fp32's range: every later logit is a NaN


@functools.lru_cache(maxsize=None)
def model():
    return build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"}).cuda()


@functools.lru_cache(maxsize=None)
def case(csc=False):
    c = coopfit_ref.make_case("tiny", C, N_CTX, N_TRAIN, csc=csc)
    g = torch.Generator().manual_seed(77)
    E = c["feats"].shape[1]
    centres = torch.randn(C, E, generator=g)
    c["labels"] = torch.arange(N_TRAIN) % C
    c["feats"] = centres[c["labels"]] + 0.3 * torch.randn(N_TRAIN, E, generator=g)
    c["val_labels"] = torch.arange(N_VAL) % C
    c["val_feats"] = centres[c["val_labels"]] + 0.6 * torch.randn(N_VAL, E, generator=g)
    t = torch.randn(C, E, generator=g)
    c["teacher"] = (t / t.norm(dim=1, keepdim=True)).cuda()
    return c


def fit(c, rates, method="coop", **kw):
    kw.setdefault("grad_scale", GRAD_SCALE)
    if method != "coop":
        kw.setdefault("teacher", c["teacher"])
    return coopfit.fit_context(c["feats"].cuda(), c["labels"], model(), c["ids"], c["ctx"], epochs=len(rates), batch_size=BATCH,
                               lr_per_epoch=list(rates), method=method, **kw)


def val_of(c):
    return c["val_feats"].cuda(), c["val_labels"].cuda()


def fresh_record(c, ctx, method="coop", n_bins=10, logit_scale=coopfit_ref.LOGIT_SCALE, **kw):
    """(record bytes, logits) of ``ctx`` scored by ``validate`` on a fresh state."""
    kw.setdefault("grad_scale", GRAD_SCALE)
    if method != "coop":
        kw.setdefault("teacher", c["teacher"])
    st = coopfit.CoOpFitState(model(), c["ids"], ctx, logit_scale, method=method, **kw)
    st.start_monitor(1, n_bins)
    st.validate(*val_of(c), 0)
    return st.monitor_records()[0].cpu().numpy().copy(), st.val_logits().cpu().numpy().copy()


SCALES = {"static": dict(grad_scale=GRAD_SCALE), "dynamic": dict(grad_scale="dynamic", scaler=dict(init_scale=GRAD_SCALE))}


# ProGrad has no dynamic loss scale (coopfit's module docstring): its two cases are the static ones
UNCHANGED = [(m, p, s) for m in ("coop", "kgcoop", "prograd") for p in ("end", "middle") for s in ("static", "dynamic")
             if not (m == "prograd" and s == "dynamic")]


@pytest.mark.parametrize("method,position,scale", UNCHANGED, ids=["-".join(k) for k in UNCHANGED])
def test_validation_leaves_the_fit_unchanged(method, position, scale):
    c = case()
    rates = [2e-3, 1e-3, 5e-4]
    kw = dict(SCALES[scale], class_token_position=position)
    plain = fit(c, rates, method, **kw)
    watched, mon = fit(c, rates, method, val=val_of(c), final_model="last_step", return_monitor=True, **kw)
    assert torch.isfinite(plain).all() and not torch.equal(plain.cpu(), c["ctx"])
    assert torch.equal(plain, watched)
    assert mon["accuracy"].shape == (3,) and mon["best_epoch"] is None and all(r["n"] == N_VAL for r in mon["records"])


@pytest.mark.parametrize("csc", [False, True], ids=["generic", "class-specific"])
def test_monitor_equals_after_the_fact_scoring(csc):
    c = case(csc)
    rates = coopfit.fitloop.cosine_warmup_schedule(2e-3, 3, warmup_lr=1e-3)
    ctx, mon = fit(c, rates, val=val_of(c), return_monitor=True, val_bins=15)
    whole = fit(c, rates, val=val_of(c), val_bins=15)
    assert torch.equal(ctx, whole)
    for e in range(3):
        ctx_e = fit(c, rates[:e + 1])
        raw, _ = fresh_record(c, ctx_e, n_bins=15)
        (rec,) = ops.decode_val_records(raw, 15)
        got = mon["records"][e]
        assert rec["n"] == got["n"] == N_VAL and rec["correct"] == got["correct"]
        assert np.array([rec["nll_sum"]]).tobytes() == np.array([got["nll_sum"]]).tobytes()
        assert np.array_equal(rec["count"], got["count"]) and np.array_equal(rec["hits"], got["hits"])
        assert rec["conf_sum"].tobytes() == got["conf_sum"].tobytes()
    assert torch.equal(fit(c, rates[:3]), ctx)


def records_of_truncated_runs(c, rates, n_bins=10):
    """Per epoch e: (the context of the run truncated behind e, the float64 restatement's record of its validation logits)."""
    out = []
    for e in range(len(rates)):
        ctx_e = fit(c, rates[:e + 1])
        _, logits = fresh_record(c, ctx_e, n_bins=n_bins)
        out.append((ctx_e, ref.record(logits, c["val_labels"].numpy(), n_bins)))
    return out


@pytest.mark.parametrize("criterion", ["accuracy", "nll"])
def test_best_val_returns_the_best_epochs_context(criterion):
    c = case()
    rates = [2e-3, 2e-3, 1e-3, WRECK]
    runs = records_of_truncated_runs(c, rates)
    want = ref.best_epoch([r for _, r in runs], criterion)
    print("fitmonitor: correct per epoch", [r["correct"] for _, r in runs], "nll_sum", [r["nll_sum"] for _, r in runs], "best", want)
    assert 0 <= want < len(rates) - 1, "the last rate did not wreck the context: the selection is not exercised"
    assert not torch.isfinite(runs[-1][0]).all()
    best, mon = fit(c, rates, val=val_of(c), final_model="best_val", val_criterion=criterion, return_monitor=True)
    assert mon["best_epoch"] == want
    assert torch.equal(best, runs[want][0]) and torch.isfinite(best).all()
    last, mon2 = fit(c, rates, val=val_of(c), final_model="last_step", val_criterion=criterion, return_monitor=True)
    assert last.cpu().numpy().tobytes() == runs[-1][0].cpu().numpy().tobytes()
    assert mon2["best_epoch"] is None and [r["correct"] for r in mon2["records"]] == [r["correct"] for _, r in runs]


@pytest.mark.parametrize("criterion", ["accuracy", "nll"])
def test_equal_epochs_keep_the_earlier_one(criterion):
    """Rates of zero behind the first epoch: the context stops moving, epochs 1 and 2 score what epoch 0 scored, and epoch 0 stays."""
    c = case()
    rates = [2e-3, 0.0, 0.0]
    best, mon = fit(c, rates, val=val_of(c), final_model="best_val", val_criterion=criterion, return_monitor=True, weight_decay=0.0, momentum=0.0)
    recs = mon["records"]
    assert recs[0]["correct"] == recs[1]["correct"] == recs[2]["correct"] and recs[0]["nll_sum"] == recs[1]["nll_sum"] == recs[2]["nll_sum"]
    assert ref.best_epoch(recs, criterion) == 0 and mon["best_epoch"] == 0
    assert torch.equal(best, fit(c, rates[:1], weight_decay=0.0, momentum=0.0))


def test_trainer_installs_the_best_context():
    m = model()
    clip = CustomCLIP(m, case()["ids"], n_ctx=N_CTX)
    c = dict(case(), ctx=clip.prompt_learner.ctx.detach().float().cpu().clone())      # the fit starts from the parameter's values
    rates = [2e-3, 2e-3, 1e-3, WRECK]
    runs = records_of_truncated_runs(c, rates)
    want = ref.best_epoch([r for _, r in runs], "accuracy")
    assert 0 <= want < len(rates) - 1
    train = [(c["feats"].cuda(), c["labels"])]
    val = [(c["val_feats"][:10].cuda(), c["val_labels"][:10]), (c["val_feats"][10:].cuda(), c["val_labels"][10:])]
    try:
        m.image_features_f32 = lambda image: image          # the loaders' "images" are the features: the trainer's plumbing runs as with images
        fitted, mon = clip.fit_context(train, val_loader=val, final_model="best_val", return_monitor=True, epochs=len(rates), lr_per_epoch=rates,
                                       batch_size=BATCH, grad_scale=GRAD_SCALE, logit_scale=coopfit_ref.LOGIT_SCALE)
        with pytest.raises(ValueError, match="val_loader and val"):
            clip.fit_context(train, val_loader=val, val=val_of(c), epochs=1)
    finally:
        del m.image_features_f32
    assert mon["best_epoch"] == want and torch.equal(fitted, runs[want][0])
    assert torch.equal(clip.prompt_learner.ctx.detach().float(), runs[want][0].to(clip.prompt_learner.ctx.dtype).float())


def test_monitor_values_against_metrics_and_numpy():
    c = case()
    rates = [2e-3, 1e-3, 5e-4]
    n_bins = 10
    ls = float(np.log(10.0))     # logits of scale 10: no confidence comes within 2^-20 of 1.0 without reaching it, so the counts can be held exactly
    _, mon = fit(c, rates, val=val_of(c), return_monitor=True, logit_scale=ls)
    y = c["val_labels"].numpy()
    for e in range(3):
        _, logits = fresh_record(c, fit(c, rates[:e + 1], logit_scale=ls), logit_scale=ls)
        hit, nll, conf = ref.score_rows(logits, y)
        assert ref.off_the_edges(conf, n_bins), "a confidence on a bin edge: pick another validation seed"
        pred = np.argmax(logits.astype(np.float64), axis=1)
        got = mon["records"][e]
        want = ref.record(logits, y, n_bins)
        assert got["correct"] == int((pred == y).sum()) and mon["accuracy"][e] == (pred == y).mean()
        assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["hits"], want["hits"])
        zt, yt = torch.from_numpy(logits).cuda(), torch.from_numpy(y).cuda()
        t_nll = torch.nn.functional.cross_entropy(zt, yt, reduction="none").double().sum().item()
        t_conf = torch.softmax(zt, dim=1).max(dim=1).values.double().cpu().numpy()
        b_nll = max(2 * abs(t_nll - nll.sum()), ref.FLOOR * abs(nll.sum()))
        print(f"fitmonitor-parity: fit epoch {e} nll_sum: device {abs(got['nll_sum'] - nll.sum()):.3e}, bound {b_nll:.3e}")
        assert abs(got["nll_sum"] - nll.sum()) <= b_nll
        assert mon["nll"][e] == pytest.approx(nll.mean(), abs=b_nll / N_VAL)
        which = metrics.digitize_bins(conf, n_bins)
        slack = 0.0
        for b in np.unique(which):
            w, t = conf[which == b].sum(), t_conf[which == b].sum()
            bound = max(2 * abs(t - w), ref.FLOOR * abs(w))
            print(f"fitmonitor-parity: fit epoch {e} conf_sum[{b}]: device {abs(got['conf_sum'][b] - w):.3e}, bound {bound:.3e}")
            assert abs(got["conf_sum"][b] - w) <= bound
            slack += bound
        # ECE = sum_b weight_b |mean conf_b - mean acc_b|: a bin's error enters with at most its sum's error over the rows
        assert mon["ece"][e] == pytest.approx(metrics.ECE(conf, pred, y, n_bins), abs=slack / N_VAL + 1e-15)
        assert mon["bins"][e].shape == (3, n_bins + 1) and mon["ece"][e] == metrics.ece_from_bins(mon["bins"][e], n_bins)
