"""The device sample metrics (csrc/sample_metrics.hip) at operator level and through the evaluator and runner.test(): clipmi_order_stats
against np.sort -- equal values, bit-identical repeats, the NaN count --, clipmi_group_gap_accumulate and clipmi_class_counts against
np.bincount, DeviceCalibrationEvaluator(sample_metrics="device") against its host mode on the reference-generated fixtures, and
runner.test(sample_metrics="device") against the default on the tiny synthetic model.  Outputs sit between sentinel guards."""
import ctypes

import numpy as np
import pytest
import torch

from clip_calibration_amd import _lib, metrics, synthetic as syn
from conftest import load_golden

pytestmark = pytest.mark.gpu

L = _lib.lib
PAD = 64
TOL = 1e-9   # on the percentages: integer counts, and float64 group sums of N fp32 values (N 2^-52 per sum, N <= 2000 here)


@pytest.fixture(scope="module")
def ops():
    from clip_calibration_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """n elements between PAD sentinel elements on either side."""

    def __init__(self, n, dtype, mark, fill=None):
        self.n, self.mark = n, mark
        self.buf = torch.full((2 * PAD + n,), mark, dtype=dtype, device="cuda")
        self.view = self.buf[PAD:PAD + n]
        if fill is not None:
            self.view.fill_(fill)
        self.ptr = self.view.data_ptr()

    def result(self, what):
        torch.cuda.synchronize()
        b = self.buf.cpu()
        assert bool((b[:PAD] == self.mark).all()) and bool((b[PAD + self.n:] == self.mark).all()), f"{what}: wrote outside its output"
        return b[PAD:PAD + self.n].numpy().copy()


# ---- clipmi_order_stats -------------------------------------------------------------------------------------------------------------
def _order_inputs(n, seed):
    rng = np.random.default_rng(seed)
    two = np.where(rng.random(n) < 0.5, np.float32(0.25), np.float32(0.75)).astype(np.float32)
    low8 = (np.uint32(np.float32(0.7).view(np.uint32) & np.uint32(0xffffff00)) + rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    signs = (rng.standard_normal(n) * 4).astype(np.float32)
    signs[rng.permutation(n)[: max(1, n // 4)]] = 0.0
    signs[rng.permutation(n)[: max(1, n // 4)]] = -0.0
    denormal = (rng.integers(1, 1 << 22, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))).view(np.float32)
    with_nan = rng.random(n).astype(np.float32)
    with_nan[n // 2] = np.nan
    return {"uniform": rng.random(n).astype(np.float32), "equal": np.full(n, 0.37, np.float32), "two_values": two, "last_pass_only": low8,
            "signs_and_zeros": signs, "denormals": denormal, "one_nan": with_nan}


def _order_stats(d_x, ranks):
    """clipmi_order_stats into guarded outputs with a workspace of exactly the size asked for -> (values [k], NaN count)."""
    n, k = d_x.numel(), len(ranks)
    out, nans = Guarded(k, torch.float32, -7.0), Guarded(1, torch.int32, -123456789)
    need = L.clipmi_order_stats_workspace_bytes(n, k)
    assert need > 0
    ws = Guarded(need, torch.uint8, 0xAB)
    c_ranks = (ctypes.c_int32 * k)(*[int(r) for r in ranks])
    _lib.check(L.clipmi_order_stats(d_x.data_ptr(), n, c_ranks, k, out.ptr, nans.ptr, ws.ptr, need, _stream()), "clipmi_order_stats")
    ws.result("clipmi_order_stats workspace")
    return out.result("clipmi_order_stats"), int(nans.result("clipmi_order_stats nan_count")[0])


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 255, 256, 257, 4097))
def test_order_stats_equal_numpy_sort(n):
    rng = np.random.default_rng(n)
    rank_sets = {"quantile22": np.sort(metrics.quantile_ranks(n, 10)), "one": np.array([n // 2]), "sixty-four": np.sort(rng.integers(0, n, 64))}
    assert rank_sets["quantile22"].size == 22
    for name, x in _order_inputs(n, 7 * n).items():
        d_x = torch.from_numpy(x).cuda()
        want_sorted = np.sort(x)
        n_nan = int(np.isnan(x).sum())
        for rname, ranks in rank_sets.items():
            what = f"{name} n={n} ranks={rname}"
            got, nans = _order_stats(d_x, ranks)
            again, nans2 = _order_stats(d_x, ranks)
            assert got.tobytes() == again.tobytes() and nans == nans2, f"{what}: two runs differ"
            assert nans == n_nan, what
            want = want_sorted[ranks]
            finite = ~np.isnan(want)
            assert np.array_equal(got[finite], want[finite]), f"{what}: got {got}, want {want}"
            assert np.isnan(got[~finite]).all(), what             # numpy sorts a NaN last; so does the kernel
        assert torch.equal(d_x.cpu().view(torch.int32), torch.from_numpy(x).view(torch.int32)), f"{name}: the input was modified"


def test_order_stats_wrapper_checks_and_returns_device_tensors(ops):
    x = torch.rand(300, device="cuda")
    vals, nans = ops.order_stats(x, [0, 150, 299])
    assert vals.is_cuda and nans.is_cuda
    s = np.sort(x.cpu().numpy())
    assert np.array_equal(vals.cpu().numpy(), s[[0, 150, 299]]) and int(nans.item()) == 0
    for bad in ([], [300], [-1], [5, 4], list(range(65))):
        with pytest.raises(ValueError):
            ops.order_stats(x, bad)
    with pytest.raises(TypeError):
        ops.order_stats(x.double(), [0])


# ---- clipmi_group_gap_accumulate ----------------------------------------------------------------------------------------------------
def _gap_case(n, G, seed):
    """(conf, pred, labels, key or None, key_edges, conf_edges): confidences exactly on every edge (as fp32 roundings of the float64
    edges -- above some, below others -- and as the exactly representable 0.25, 0.5, 0.75) and at 0.0 and 1.0."""
    rng = np.random.default_rng(seed)
    conf_edges = {1: np.zeros(0), 10: np.linspace(0, 1, 11)[1:-1], 110: np.linspace(0, 1, 12)[1:-1]}[G]
    special = np.concatenate([[1.0, 0.0], conf_edges.astype(np.float32), [0.25, 0.5, 0.75]]).astype(np.float32)
    conf = rng.random(n).astype(np.float32)
    m = min(n, special.size)
    conf[:m] = special[:m]
    pred = rng.integers(0, 5, n).astype(np.int32)
    labels = np.where(rng.random(n) < 0.6, pred, rng.integers(0, 5, n)).astype(np.int64)
    key, key_edges = None, np.zeros(0)
    if G == 110:
        key = rng.random(n).astype(np.float32)
        key_edges = np.sort(rng.random(9).astype(np.float32)).astype(np.float64)    # edges a key can hit exactly
        key[rng.permutation(n)[: min(n, 9)]] = key_edges[: min(n, 9)].astype(np.float32)
    return conf, pred, labels, key, key_edges, conf_edges


@pytest.mark.parametrize("n", (1, 65, 4097))
@pytest.mark.parametrize("G", (1, 10, 110))
def test_group_gap_accumulate_against_bincount(ops, n, G):
    conf, pred, labels, key, key_edges, conf_edges = _gap_case(n, G, 13 * n + G)
    assert (key_edges.size + 1) * (conf_edges.size + 1) == G
    kb = np.searchsorted(key_edges, key.astype(np.float64), side="right") if key is not None else np.zeros(n, np.int64)
    group = kb * (conf_edges.size + 1) + np.searchsorted(conf_edges, conf.astype(np.float64), side="right")
    correct = (pred == labels).astype(np.float64)
    want = np.stack([np.bincount(group, minlength=G).astype(np.float64), np.bincount(group, weights=conf.astype(np.float64), minlength=G),
                     np.bincount(group, weights=correct, minlength=G)])
    d = [torch.from_numpy(a).cuda() for a in (conf, pred, labels)]
    d_key = None if key is None else torch.from_numpy(key).cuda()
    out = Guarded(3 * G, torch.float64, -1.2345678e300, fill=0.0)
    got = ops.group_gap_accumulate(*d, key=d_key, key_edges=key_edges, conf_edges=conf_edges, groups=out.view)
    assert got.data_ptr() == out.ptr
    r = out.result("clipmi_group_gap_accumulate").reshape(3, G)
    assert np.array_equal(r[0], want[0]) and np.array_equal(r[2], want[2]), (r, want)
    print(f"n={n} G={G}: max |d sum_conf| = {np.abs(r[1] - want[1]).max():.3e}, bound {n * 2.0 ** -52:.3e}")
    assert np.abs(r[1] - want[1]).max() <= n * 2.0 ** -52
    ops.group_gap_accumulate(*d, key=d_key, key_edges=key_edges, conf_edges=conf_edges, groups=out.view)   # accumulates over calls
    r2 = out.result("clipmi_group_gap_accumulate, second call").reshape(3, G)
    assert np.array_equal(r2[0], 2 * want[0]) and np.array_equal(r2[2], 2 * want[2])
    assert np.abs(r2[1] - 2 * want[1]).max() <= 2 * n * 2.0 ** -52


def test_group_gap_wrapper_checks(ops):
    conf, pred, lab = torch.rand(8, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="need a key"):
        ops.group_gap_accumulate(conf, pred, lab, key_edges=[0.5])
    with pytest.raises(ValueError, match="groups"):
        ops.group_gap_accumulate(conf, pred, lab, key=conf, key_edges=np.linspace(0, 1, 40), conf_edges=np.linspace(0, 1, 40))
    assert ops.group_gap_accumulate(conf, pred, lab).cpu().numpy()[0, 0] == 8


# ---- clipmi_class_counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (1, 2, 1000, 2730, 2731))    # 3 C + 1 = 8191 counters are the last to fit the LDS partials, 8194 do not
@pytest.mark.parametrize("n", (1, 4097))
def test_class_counts_against_bincount(n, C):
    rng = np.random.default_rng(n + C)
    cases = {"random": (rng.integers(0, C, n).astype(np.int32), rng.integers(0, C, n).astype(np.int64)),
             "one_class": (np.full(n, C - 1, np.int32), np.full(n, C - 1, np.int64))}
    p, y = rng.integers(0, C, n).astype(np.int32), rng.integers(0, C, n).astype(np.int64)
    y[n // 2] = C                                                       # one label outside [0, C) ...
    if n > 1:
        p[0], y[n - 1], p[n // 3] = -1, -5, C                           # ... and, where there is room, predictions and a negative label
    cases["outside"] = (p, y)
    for name, (pred, labels) in cases.items():
        ok = (pred >= 0) & (pred < C) & (labels >= 0) & (labels < C)
        pv, yv = pred[ok].astype(np.int64), labels[ok]
        want = np.concatenate([np.bincount(yv[pv == yv], minlength=C), np.bincount(pv, minlength=C), np.bincount(yv, minlength=C),
                               [int((~ok).sum())]]).astype(np.int64)
        d_p, d_y = torch.from_numpy(pred).cuda(), torch.from_numpy(labels).cuda()
        out = Guarded(3 * C + 1, torch.int64, -1234567890123, fill=0)
        _lib.check(L.clipmi_class_counts(d_p.data_ptr(), d_y.data_ptr(), n, C, out.ptr, _stream()), "clipmi_class_counts")
        got = out.result("clipmi_class_counts")
        assert np.array_equal(got, want), f"{name} n={n} C={C}: first difference at {np.nonzero(got != want)[0][:4]}"
        if name == "outside":
            assert got[-1] == (1 if n == 1 else 4)


# ---- the evaluator ------------------------------------------------------------------------------------------------------------------
def _evaluate_both(conf, pred, gt, prox, bins, n_classes):
    from clip_calibration_amd.evaluator import DeviceCalibrationEvaluator
    d_conf, d_pred, d_gt = torch.from_numpy(conf).cuda(), torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    res = []
    for mode in ("host", "device"):
        ev = DeviceCalibrationEvaluator(bins, keep_samples=True, piece_bins=10, sample_metrics=mode, n_classes=n_classes)
        cut = conf.size // 3                                  # two batches: the kept vectors are concatenated
        ev.process(d_conf[:cut], d_pred[:cut], d_gt[:cut])
        ev.process(d_conf[cut:], d_pred[cut:], d_gt[cut:])
        res.append(ev.evaluate(prox if mode == "host" else torch.from_numpy(prox).cuda()))
    return res


def _assert_same_results(host, dev, what):
    assert list(dev) == list(host), what
    for k in host:
        print(f"{what} {k}: host {host[k]!r} device {dev[k]!r}")
        if k in ("accuracy", "error_rate", "total"):
            assert dev[k] == host[k], (what, k)                          # integer counts
        else:   # the two evaluators accumulate their own bins: confidence, ece and mce carry the order of their float64 atomics too
            assert abs(dev[k] - host[k]) <= TOL, (what, k, host[k], dev[k])


def test_evaluator_device_mode_matches_host_mode_on_the_fixtures():
    g = load_golden("ece_cases.npz")
    for n in sorted({k.split(":")[0] for k in g}):
        conf, pred, gt = g[f"{n}:conf"].astype(np.float32), g[f"{n}:pred"].astype(np.int32), g[f"{n}:gt"].astype(np.int64)
        prox, bins = g[f"{n}:prox"].astype(np.float32), int(g[f"{n}:bins"])
        C = int(max(pred.max(), gt.max())) + 1
        host, dev = _evaluate_both(conf, pred, gt, prox, bins, C)
        assert list(host)[:8] == ["accuracy", "error_rate", "macro_f1", "confidence", "ece", "mce", "ace", "piece"]
        _assert_same_results(host, dev, n)
        # a NaN proximity: the quantile bins collapse to one, on the host and on the device alike
        bad = prox.copy()
        bad[bad.size // 2] = np.nan
        host_nan, dev_nan = _evaluate_both(conf, pred, gt, bad, bins, C)
        _assert_same_results(host_nan, dev_nan, f"{n} (NaN proximity)")
        one_bin = 100.0 * metrics.PIECE(conf, np.zeros_like(prox), pred, gt, 10, bins)
        assert abs(dev_nan["piece"] - one_bin) <= TOL


def test_evaluator_device_mode_refuses_labels_outside_the_classes():
    from clip_calibration_amd.evaluator import DeviceCalibrationEvaluator
    ev = DeviceCalibrationEvaluator(10, keep_samples=True, sample_metrics="device", n_classes=3)
    conf = torch.rand(20, device="cuda")
    pred = torch.randint(0, 3, (20,), dtype=torch.int32, device="cuda")
    gt = torch.randint(0, 3, (20,), device="cuda")
    gt[7] = 3
    ev.process(conf, pred, gt)
    with pytest.raises(ValueError, match="outside"):
        ev.evaluate()
    ev.reset()
    with pytest.raises(ValueError, match="no samples"):
        ev.evaluate()


# ---- runner.test() ------------------------------------------------------------------------------------------------------------------
def test_runner_test_device_sample_metrics_match_the_default():
    """The flow of tests/test_gpu_model.py::test_runner_base_to_new_calibration_flow (tiny geometry, 37 test images, DAC on, a val dict
    for the proximity), evaluated both ways."""
    from clip_calibration_amd import runner
    from clip_calibration_amd.calibrator import VLCalibration
    from clip_calibration_amd.model import build_model
    from clip_calibration_amd.trainers import CoOpCLIP, ZeroshotCLIP
    sd = syn.synthetic_state_dict("tiny", seed=0)
    model = build_model(dict(sd), {"trainer": "CoOp", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0}).cuda()
    C, n_ctx, K = 12, 4, 3
    coop_b = CoOpCLIP(model, syn.synthetic_token_ids(C, "tiny", seed=20, n_ctx_placeholders=n_ctx), n_ctx=n_ctx, seed=2)
    coop_n = CoOpCLIP(model, syn.synthetic_token_ids(C, "tiny", seed=21, n_ctx_placeholders=n_ctx), n_ctx=n_ctx, seed=2)
    zs_b = ZeroshotCLIP(model, syn.synthetic_token_ids(C, "tiny", seed=20))
    zs_n = ZeroshotCLIP(model, syn.synthetic_token_ids(C, "tiny", seed=21))
    val_images, test_images = syn.synthetic_images(20, "tiny", seed=30), syn.synthetic_images(37, "tiny", seed=31)
    loader = lambda im, lb, bs: [(im[i:i + bs], lb[i:i + bs]) for i in range(0, len(im), bs)]
    val_labels = torch.arange(20) % C
    tuned = runner.collect_base_val_features(coop_b, loader(val_images, val_labels, 8), image_k=K)
    zsd = runner.collect_base_val_features(zs_b.model_inference, loader(val_images, val_labels, 8), image_k=K)
    cal = VLCalibration(tuned, runner.text_feature_dict(zsd, zs_n.text_features, tuned, coop_n.text_features()), dac_flag=True, k_dac=5)
    cal.fit()
    test_labels = torch.arange(37) % 5           # five of the twelve classes carry labels: macro-F1 averages over the present ones only
    host = runner.test(coop_n, loader(test_images, test_labels, 16), val_dict=tuned, calibrator=cal, image_k=K)
    dev = runner.test(coop_n, loader(test_images, test_labels, 16), val_dict=tuned, calibrator=cal, image_k=K, sample_metrics="device")
    assert host["total"] == 37 and "piece" in host
    _assert_same_results(host, dev, "runner.test")
    with pytest.raises(ValueError, match="sample_metrics"):
        runner.test(coop_n, [], sample_metrics="gpu")
