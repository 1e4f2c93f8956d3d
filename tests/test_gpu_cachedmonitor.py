"""Per-epoch validation and best-val selection of the CLIP-Adapter and TaskRes fits on the GPU, on both routes: the one-call monitored run
(fit_adapter / fit_residuals with val=) and State.step + State.validate.  E 128, 5 classes, 40 train rows in batches of 8, 6 epochs, 65
validation rows.

Fits are bit-reproducible, so the monitor is held to after-the-fact scoring by equality: record e is, byte for byte, the record a fresh
state writes for the weights of the run truncated behind epoch e.  The numbers are held to float64: the integer counts exactly, both to the
reference scoring of the device's own logits and to the float64 forward (tests/cachedmonitor_ref.py) of the device's weights, under the
precondition -- asserted -- that no row's top-two margin or distance to a bin edge is below the logits bound; the sums within
max(2 x torch's fp32 distance from float64, 2^-22 relative), tests/test_gpu_fitmonitor.py's bound."""
import functools
import math

import numpy as np
import pytest
import torch

import cachedmonitor_ref as cref
import fitmonitor_ref as ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import adapterfit, metrics, ops, taskresfit  # noqa: E402

E, H, C, N_TRAIN, BATCH, EPOCHS, N_VAL = 128, 32, 5, 40, 8, 6, 65
LS = float(np.log(10.0))    # logits of scale 10: no confidence saturates to 1.0, so the counts can be held exactly
SCALE = float(np.float32(math.exp(LS)))
WRECK = float("inf")     # a rate that takes the weights out of fp32's range: every later logit is a NaN
KINDS = ["adapter", "taskres"]
RATES = {"adapter": [0.05, 0.05, 0.03, 0.02, 0.01, 0.005], "taskres": [0.02, 0.02, 0.01, 0.01, 0.005, 0.002]}


@functools.lru_cache(maxsize=None)
def case():
    g = torch.Generator().manual_seed(123)
    centres = torch.randn(C, E, generator=g)
    y = torch.arange(N_TRAIN) % C
    vy = torch.arange(N_VAL) % C
    T = torch.randn(C, E, generator=g) * 0.5 + centres
    return dict(centres=centres, f=(centres[y] + 1.5 * torch.randn(N_TRAIN, E, generator=g)).cuda(), y=y,
                vf=(centres[vy] + 6.0 * torch.randn(N_VAL, E, generator=g)).cuda(), vy=vy, base=T.cuda(),
                T=(T / T.norm(dim=1, keepdim=True)).cuda(), w1=torch.randn(H, E, generator=g) / math.sqrt(3 * E),
                w2=torch.randn(E, H, generator=g) * (cref.W2_GAIN / math.sqrt(3 * H)))


def fit(kind, rates, **kw):
    """(fitted weights as a tuple, then whatever else the fit returns)."""
    c = case()
    if kind == "adapter":
        out = adapterfit.fit_adapter(c["f"], c["y"], c["T"], c["w1"], c["w2"], ratio=cref.RATIO, logit_scale=LS, epochs=len(rates), batch_size=BATCH,
                                     lr_per_epoch=list(rates), **kw)
        return (out[0], out[1]), out[2:]
    out = taskresfit.fit_residuals(c["f"], c["y"], c["base"], None, alpha=cref.ALPHA, logit_scale=LS, optimizer=kw.pop("optimizer", "sgd"),
                                   epochs=len(rates), batch_size=BATCH, lr_per_epoch=list(rates), **kw)
    return ((out[0],), out[1:]) if isinstance(out, tuple) else ((out,), ())


def new_state(kind, weights=None, **kw):
    c = case()
    if kind == "adapter":
        w1, w2 = weights if weights is not None else (c["w1"], c["w2"])
        return adapterfit.AdapterFitState(c["T"], w1, w2, ratio=cref.RATIO, logit_scale=LS, **kw)
    return taskresfit.TaskResFitState(c["base"], None if weights is None else weights[0], alpha=cref.ALPHA, logit_scale=LS,
                                      optimizer=kw.pop("optimizer", "sgd"), **kw)


def weights_of(kind, st):
    return (st.w1, st.w2) if kind == "adapter" else (st.residuals,)


def best_of(kind, st):
    return st.best_weights() if kind == "adapter" else (st.best_residuals(),)


def same(a, b):
    return len(a) == len(b) and all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))


def val_of():
    return case()["vf"], case()["vy"].cuda()


def fresh_record(kind, weights, n_bins=10, val=None):
    """(record bytes, logits) of ``weights`` scored by ``validate`` on a fresh state."""
    st = new_state(kind, weights)
    st.start_monitor(1, n_bins)
    st.validate(*(val or val_of()), 0)
    return st.monitor_records()[0].cpu().numpy().copy(), st.val_logits().cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def truncated(kind, rates):
    """Per epoch e: the weights of the run truncated behind e."""
    return [fit(kind, rates[:e + 1])[0] for e in range(len(rates))]


def float64_logits(kind, weights, vf=None):
    c = case()
    c = c if vf is None else dict(c, vf=vf)
    if kind == "adapter":
        return cref.adapter_logits_bound(c["vf"].cpu().numpy(), c["T"].cpu().numpy(), weights[0].cpu().numpy(), weights[1].cpu().numpy(), cref.RATIO, SCALE)
    return cref.taskres_logits_bound(c["vf"].cpu().numpy(), c["base"].cpu().numpy(), weights[0].cpu().numpy(), cref.ALPHA, SCALE)


@pytest.mark.parametrize("kind", KINDS)
def test_validation_leaves_the_fit_unchanged(kind):
    rates = tuple(RATES[kind])
    plain, _ = fit(kind, rates)
    watched, (mon,) = fit(kind, rates, val=val_of(), return_monitor=True)
    start = (case()["w1"], case()["w2"]) if kind == "adapter" else (torch.zeros(C, E),)
    assert all(torch.isfinite(w).all() for w in plain) and not same(plain, start)
    assert same(plain, watched)
    assert mon["accuracy"].shape == (EPOCHS,) and mon["best_epoch"] is None and all(r["n"] == N_VAL for r in mon["records"])
    hist, (losses, mon2) = fit(kind, rates, val=val_of(), return_monitor=True, return_history=True)
    assert same(hist, plain) and losses.shape == (EPOCHS * (N_TRAIN // BATCH),) and mon2["records"][0]["correct"] == mon["records"][0]["correct"]


@pytest.mark.parametrize("kind", KINDS)
def test_records_equal_after_the_fact_scoring_and_the_routes_agree(kind):
    rates = tuple(RATES[kind])
    c = case()
    best, (mon,) = fit(kind, rates, val=val_of(), final_model="best_val", return_monitor=True, val_bins=15)
    runs = truncated(kind, rates)
    raws = []
    for e in range(EPOCHS):
        raw, _ = fresh_record(kind, runs[e], n_bins=15)
        raws.append(raw)
        assert ops.encode_val_records([mon["records"][e]], 15)[0].tobytes() == raw.tobytes(), e
    assert same(best, runs[mon["best_epoch"]])
    # the per-step route: State.step over the same batches, validate behind every epoch
    st = new_state(kind)
    st.start_monitor(EPOCHS, 15, select=True)
    lr = torch.tensor(np.repeat(np.asarray(rates, np.float64), N_TRAIN // BATCH).astype(np.float32)).cuda()
    s = 0
    for e in range(EPOCHS):
        for k in range(N_TRAIN // BATCH):
            st.step(c["f"][k * BATCH:(k + 1) * BATCH], c["y"][k * BATCH:(k + 1) * BATCH], lr[s:s + 1])
            s += 1
        st.validate(*val_of(), e)
    assert same(weights_of(kind, st), runs[-1])
    assert st.monitor_records().cpu().numpy().tobytes() == np.stack(raws).tobytes()
    assert st.monitor()["best_epoch"] == mon["best_epoch"] and same(best_of(kind, st), best)


@pytest.mark.parametrize("criterion", ["accuracy", "nll"])
@pytest.mark.parametrize("kind", KINDS)
def test_best_val_returns_the_best_epochs_weights(kind, criterion):
    rates = tuple(RATES[kind][:3]) + (WRECK,)
    runs = truncated(kind, rates)
    recs = [ref.record(fresh_record(kind, w)[1], case()["vy"].numpy(), 10) for w in runs]
    want = ref.best_epoch(recs, criterion)
    print("cachedmonitor: correct per epoch", [r["correct"] for r in recs], "nll_sum", [r["nll_sum"] for r in recs], "best", want)
    assert not all(torch.isfinite(w).all() for w in runs[-1])
    if kind == "taskres":     # non-finite residuals give NaN logits: the last epoch is never the best one
        assert 0 <= want < len(rates) - 1, "the last rate did not wreck the residuals: the selection is not exercised"
    else:                     # the adapter's ReLU is fmaxf, which drops a NaN: wrecked weights leave normalise((1 - ratio) f), finite logits
        assert 0 <= want and np.isfinite(recs[-1]["nll_sum"])
    best, (mon,) = fit(kind, rates, val=val_of(), final_model="best_val", val_criterion=criterion, return_monitor=True)
    assert mon["best_epoch"] == want and same(best, runs[want])
    last, (mon2,) = fit(kind, rates, val=val_of(), val_criterion=criterion, return_monitor=True)
    assert same(last, runs[-1]) and mon2["best_epoch"] is None
    assert [r["correct"] for r in mon2["records"]] == [r["correct"] for r in recs]


@pytest.mark.parametrize("criterion", ["accuracy", "nll"])
@pytest.mark.parametrize("kind", KINDS)
def test_equal_epochs_keep_the_earlier_one(kind, criterion):
    """Rates of zero behind the first epoch, no weight decay, no momentum: the weights stop moving, epochs 1 and 2 score what epoch 0
    scored, and epoch 0 stays."""
    rates = (RATES[kind][0], 0.0, 0.0)
    best, (mon,) = fit(kind, rates, val=val_of(), final_model="best_val", val_criterion=criterion, return_monitor=True, weight_decay=0.0, momentum=0.0)
    recs = mon["records"]
    assert recs[0]["correct"] == recs[1]["correct"] == recs[2]["correct"] and recs[0]["nll_sum"] == recs[1]["nll_sum"] == recs[2]["nll_sum"]
    assert ref.best_epoch(recs, criterion) == 0 and mon["best_epoch"] == 0
    assert same(best, fit(kind, rates[:1], weight_decay=0.0, momentum=0.0)[0])


@pytest.mark.parametrize("kind", KINDS)
def test_a_poisoned_validation_row_is_never_taken_under_nll(kind):
    """One NaN in one validation row makes every epoch's nll_sum a NaN: under "nll" no epoch is taken and the starting weights come back;
    under "accuracy" the row counts as wrong and the selection goes on."""
    rates = tuple(RATES[kind][:3])
    vf, vy = val_of()
    vf = vf.clone()
    vf[7, 3] = float("nan")
    best, (mon,) = fit(kind, rates, val=(vf, vy), final_model="best_val", val_criterion="nll", return_monitor=True)
    assert all(math.isnan(r["nll_sum"]) for r in mon["records"]) and mon["best_epoch"] == -1
    start = (case()["w1"], case()["w2"]) if kind == "adapter" else (torch.zeros(C, E),)
    assert same(best, [w.float() for w in start])
    clean = fit(kind, rates, val=val_of(), return_monitor=True)[1][0]
    _, (mon_a,) = fit(kind, rates, val=(vf, vy), final_model="best_val", val_criterion="accuracy", return_monitor=True)
    assert mon_a["best_epoch"] >= 0
    for a, b in zip(mon_a["records"], clean["records"]):
        assert a["correct"] in (b["correct"], b["correct"] - 1) and a["n"] == N_VAL


@pytest.mark.parametrize("kind", KINDS)
def test_monitor_values_against_float64(kind):
    rates = tuple(RATES[kind])
    n_bins = 10
    runs = truncated(kind, rates)
    # the validation seed: the first of eight whose float64 reference decides every row's arg-max and bin, at every epoch, with room for the
    # logits' bound -- decided on the CPU from the float64 forward alone; every row of the chosen set is compared below, none is left out
    vy = case()["vy"]
    for seed in range(8):
        vf = (case()["centres"][vy] + 6.0 * torch.randn(N_VAL, E, generator=torch.Generator().manual_seed(1000 + seed))).cuda()
        refs = [float64_logits(kind, w, vf) for w in runs]
        if all(cref.clear_of_ties_and_edges(z.numpy(), t.numpy(), n_bins) for z, t in refs):
            break
    else:
        raise AssertionError("no validation seed keeps every row clear of ties and bin edges")
    val = (vf, vy.cuda())
    _, (mon,) = fit(kind, rates, val=val, return_monitor=True)
    y = vy.numpy()
    for e, w in enumerate(runs):
        _, logits = fresh_record(kind, w, val=val)
        z64, tz = refs[e]
        assert float(((torch.from_numpy(logits).double() - z64).abs() / tz).max()) <= 1.0
        assert cref.clear_of_ties_and_edges(z64.numpy(), tz.numpy(), n_bins)      # the precondition, on the CPU
        got, dev, f64 = mon["records"][e], ref.record(logits, y, n_bins), ref.record(z64.numpy(), y, n_bins)
        for want in (dev, f64):              # every row is in both comparisons
            assert got["n"] == want["n"] == N_VAL and got["correct"] == want["correct"]
            assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["hits"], want["hits"])
        hit, nll, conf = ref.score_rows(logits, y)
        zt, yt = torch.from_numpy(logits).cuda(), torch.from_numpy(y).cuda()
        t_nll = torch.nn.functional.cross_entropy(zt, yt, reduction="none").double().sum().item()
        t_conf = torch.softmax(zt, dim=1).max(dim=1).values.double().cpu().numpy()
        b_nll = max(2 * abs(t_nll - nll.sum()), ref.FLOOR * abs(nll.sum()))
        print(f"cachedmonitor-parity: {kind} epoch {e} nll_sum: device {abs(got['nll_sum'] - nll.sum()):.3e}, bound {b_nll:.3e}")
        assert abs(got["nll_sum"] - nll.sum()) <= b_nll
        which = metrics.digitize_bins(conf, n_bins)
        for b in np.unique(which):
            wsum, t = conf[which == b].sum(), t_conf[which == b].sum()
            bound = max(2 * abs(t - wsum), ref.FLOOR * abs(wsum))
            print(f"cachedmonitor-parity: {kind} epoch {e} conf_sum[{b}]: device {abs(got['conf_sum'][b] - wsum):.3e}, bound {bound:.3e}")
            assert abs(got["conf_sum"][b] - wsum) <= bound
        assert mon["accuracy"][e] == got["correct"] / N_VAL and mon["ece"][e] == metrics.ece_from_bins(mon["bins"][e], n_bins)


@pytest.mark.parametrize("kind", KINDS)
def test_trainers_validate_on_both_routes(kind):
    """val_loader= and val= reach the same monitor, best_val installs the best weights into the module, and the transform= route validates
    behind every epoch."""
    from clip_calibration_amd import synthetic as syn
    from clip_calibration_amd.augment import TrainPreprocess
    from clip_calibration_amd.model import build_model
    from clip_calibration_amd.preprocess import pack_images
    from clip_calibration_amd.trainers import CLIPAdapterCLIP, TaskResCLIP
    import augment_ref

    model = build_model(dict(syn.synthetic_state_dict("tiny", seed=0)), {"trainer": "CoOp"}).cuda()
    if kind == "adapter":
        torch.manual_seed(0)
        tr = CLIPAdapterCLIP(model, syn.synthetic_token_ids(5, "tiny", seed=90, n_ctx_placeholders=4), n_ctx=4, ratio=0.2, seed=6)
        params = [tr.adapter.fc[0].weight, tr.adapter.fc[2].weight]
        run = lambda *a, **k: tr.fit_adapter(*a, **k)
        Em = tr.adapter.fc[0].weight.shape[1]
    else:
        tr = TaskResCLIP(model, torch.stack([syn.synthetic_token_ids(5, "tiny", seed=90 + i) for i in range(3)], dim=1), alpha=0.5)
        params = [tr.prompt_learner.text_feature_residuals]
        run = lambda *a, **k: tr.fit_residuals(*a, **k)
        Em = tr.prompt_learner.base_text_features.shape[1]
    before = [p.detach().clone() for p in params]

    def reset():
        with torch.no_grad():
            for p, b in zip(params, before):
                p.copy_(b)

    g = torch.Generator().manual_seed(5)
    feats, labels = torch.randn(16, Em, generator=g).cuda(), torch.arange(16) % 5
    vfeats, vlabels = torch.randn(23, Em, generator=g).cuda(), torch.arange(23) % 5
    train = [(feats[:8], labels[:8]), (feats[8:], labels[8:])]
    val_loader = [(vfeats[:10], vlabels[:10]), (vfeats[10:], vlabels[10:])]
    rates = [0.01, 0.01, WRECK if kind == "taskres" else 0.005]      # wrecked adapter weights still give finite logits (fmaxf)
    common = dict(epochs=3, lr_per_epoch=rates, batch_size=8, return_monitor=True)
    n_w = len(params)
    try:
        model.image_features_f32 = lambda image: image          # the loaders' "images" are the features
        a = run(train, val_loader=val_loader, final_model="best_val", **common)
        installed = [p.detach().clone() for p in params]
        reset()
        b = run(train, val=(vfeats, vlabels), final_model="best_val", **common)
        with pytest.raises(ValueError, match="val_loader and val"):
            run(train, val_loader=val_loader, val=(vfeats, vlabels), epochs=1)
    finally:
        del model.image_features_f32
    assert a[-1]["best_epoch"] == b[-1]["best_epoch"] in ((0, 1) if kind == "taskres" else (0, 1, 2)) and same(a[:n_w], b[:n_w])
    assert [r["correct"] for r in a[-1]["records"]] == [r["correct"] for r in b[-1]["records"]] and len(a[-1]["records"]) == 3
    assert np.array_equal(a[-1]["nll"], b[-1]["nll"], equal_nan=True) and math.isnan(a[-1]["nll"][2]) == (kind == "taskres")
    for p, w in zip(installed, a[:n_w]):
        assert torch.isfinite(p).all() and torch.equal(p, w.to(p.dtype))
    # transform=: decoded images in, one validation behind every epoch, on features computed once
    reset()
    sizes = [(80, 100), (64, 64), (70, 51), (120, 90), (66, 97), (100, 100), (45, 80), (90, 64)]
    imgs = [augment_ref.synthetic_image(h, w, 70 + i) for i, (h, w) in enumerate(sizes)]
    loader = [(pack_images(imgs[i:i + 4]).pin_memory(), (torch.arange(8) % 5)[i:i + 4]) for i in (0, 4)]
    tp = TrainPreprocess.for_model(model, generator=torch.Generator().manual_seed(21))
    out = run(loader, transform=tp, epochs=2, lr_per_epoch=[0.002, 0.001], val=(vfeats, vlabels), final_model="best_val", return_monitor=True,
              return_history=True)
    mon = out[-1]
    assert len(out) == n_w + 2 and out[-2].shape == (4,) and len(mon["records"]) == 2 and all(r["n"] == 23 for r in mon["records"])
    assert mon["best_epoch"] in (0, 1) and np.isfinite(mon["nll"]).all()
    for p, w in zip(params, out[:n_w]):
        assert torch.equal(p.detach(), w.to(p.dtype))
