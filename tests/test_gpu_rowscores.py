"""Row scores on the GPU (csrc/row_scores.hip) through the C ABI and through ``ops``, held to the float64 restatement and the bounds of
tests/rowscores_ref.py: per-row NLL and Brier element-wise, class-wise counts and hits exactly, conf_sum bit for bit (probabilities) or
inside its fixed-point bound (logits), exact-edge probabilities, chunk independence, repeatability, unscorable rows, untouched inputs, no
read-back before the finish, agreement with the fit monitor's NLL, and runner.test(proper_scores=True) end to end on the tiny model."""
import numpy as np
import pytest
import torch

import rowscores_ref as ref
from clip_calibration_amd import _lib, metrics, synthetic as syn

pytestmark = pytest.mark.gpu

L = _lib.lib


@pytest.fixture(scope="module")
def ops():
    from clip_calibration_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _abi(rows, labels, from_probs, n_bins):
    """The C entry points on raw pointers: (row_out [N, 2], acc [3, C, n_bins + 1], out float64 [4]) as device tensors."""
    N, C = rows.shape
    assert L.clipmi_row_scores_acc_bytes(C, n_bins) == 24 * C * (n_bins + 1)
    acc = torch.zeros(3, C, n_bins + 1, dtype=torch.int64, device="cuda")
    row_out = torch.full((N, 2), -7.0, dtype=torch.float32, device="cuda")
    out = torch.zeros(4, dtype=torch.float64, device="cuda")
    ws = torch.empty(max(L.clipmi_row_scores_finish_workspace_bytes(N, C), 256), dtype=torch.uint8, device="cuda")
    _lib.check(L.clipmi_row_scores(rows.data_ptr(), rows.stride(0), labels.data_ptr(), N, C, int(from_probs), n_bins, row_out.data_ptr(),
                                   acc.data_ptr(), _stream()), "clipmi_row_scores")
    _lib.check(L.clipmi_row_scores_finish(row_out.data_ptr(), N, acc.data_ptr(), C, n_bins, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
               "clipmi_row_scores_finish")
    return row_out, acc, out


def _no_sync(fn):
    """Run ``fn`` with torch raising on every synchronising call: nothing may be read back before the finish."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        return fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _check_finish(fin, row_out, acc, N):
    r = row_out.astype(np.float64)
    assert fin["n"] == N
    assert abs(fin["nll"] - r[:, 0].mean()) <= 1e-12 * (1 + abs(r[:, 0].mean()))
    assert abs(fin["brier"] - r[:, 1].mean()) <= 1e-12 * (1 + abs(r[:, 1].mean()))
    assert abs(fin["cw_ece"] - metrics.classwise_from_bins(acc, N)) <= 1e-12


WORST = {}


@pytest.mark.parametrize("N", ref.NS)
@pytest.mark.parametrize("C", ref.CS)
def test_scores_and_bins_against_the_restatement(ops, N, C):
    for from_probs in (False, True):
        rows_h, labels_h = ref.case_inputs(N, C, from_probs)
        wide = torch.full((N, C + 5), 3.0e38, dtype=torch.float32, device="cuda")      # ld > C: the columns behind C must not be read
        wide[:, :C] = torch.from_numpy(rows_h).cuda()
        rows, labels = wide[:, :C], torch.from_numpy(labels_h).cuda()
        before = wide.clone()
        for n_bins in ref.BINS:
            row_out, acc = _no_sync(lambda: ops.row_scores(rows, labels, from_probs=from_probs, n_bins=n_bins))
            fin = ops.row_scores_finish(row_out, acc)
            got = ref.compare_case(rows_h, labels_h, n_bins, from_probs, row_out.cpu().numpy(), acc.cpu().numpy())
            _check_finish(fin, row_out.cpu().numpy(), acc.cpu().numpy(), N)
            key = "probs" if from_probs else "logits"
            for k in ("nll_ratio", "brier_ratio", "conf_ratio"):
                WORST[(key, k)] = max(WORST.get((key, k), 0.0), got[k])
            assert got["excluded"] == 0      # the seeds keep the reference clear of the edges (tests/test_rowscores_cpu.py)
            # the C ABI on the contiguous copy: the same bytes
            r2, a2, o2 = _abi(torch.from_numpy(rows_h).cuda(), labels, from_probs, n_bins)
            assert torch.equal(r2, row_out) and torch.equal(a2, acc)
            assert o2.cpu().numpy().tolist() == [fin["nll"], fin["brier"], fin["cw_ece"], float(N)]
        assert torch.equal(wide, before), "the inputs are not written"
    print("worst error / bound so far:", {f"{a}:{b}": round(v, 3) for (a, b), v in sorted(WORST.items())})


@pytest.mark.parametrize("n_bins", [1, 2, 4, 10, 15])
def test_exactly_representable_probabilities_land_where_digitize_puts_them(ops, n_bins):
    def bins_of(rows, labels, from_probs):
        row_out, acc = ops.row_scores(rows.cuda(), labels.cuda(), from_probs=from_probs, n_bins=n_bins)
        return row_out.cpu().numpy(), acc.cpu().numpy()

    for C, p in ((2, 0.5), (4, 0.25)):       # equal logits: exp(0) = 1, S = C, p = 1 / C exactly
        N = 3
        labels = torch.arange(N) % C
        row_out, acc = bins_of(torch.full((N, C), 1.75), labels, False)
        b = int(metrics.digitize_bins(np.array([p]), n_bins)[0])
        want = np.zeros((3, C, n_bins + 1), np.int64)
        want[0, :, b] = N
        want[1, :, b] = N * int(p * 2 ** 32)
        for i in range(N):
            want[2, int(labels[i]), b] += 1
        assert np.array_equal(acc, want), (C, n_bins)
        assert np.allclose(row_out[:, 0], np.log(C), rtol=0, atol=float(ref.nll_bound(np.log(C), C, 1.75)))
        assert np.array_equal(row_out[:, 1], np.full(N, np.float32((1 - p) ** 2 + (C - 1) * p * p)))
    # one-hot probabilities: p = 1 in bin n_bins (digitize's), p = 0 in bin 0; a right row scores 0, a wrong one -log(FLT_MIN) and 2
    labels = torch.tensor([0, 1, 2, 0])
    onehot = torch.eye(3)[torch.tensor([0, 1, 2, 1])]
    row_out, acc = bins_of(onehot, labels, True)
    assert int(metrics.digitize_bins(np.array([1.0]), n_bins)[0]) == n_bins and int(metrics.digitize_bins(np.array([0.0]), n_bins)[0]) == 0
    assert np.array_equal(acc, metrics.classwise_fixed_point(onehot.numpy().astype(np.float64), labels.numpy(), n_bins))
    assert acc[0, :, n_bins].tolist() == [1, 2, 1] and acc[0, :, 0].tolist() == [3, 2, 3] and acc[2, :, n_bins].tolist() == [1, 1, 1]
    assert acc[1, :, n_bins].tolist() == [2 ** 32, 2 * 2 ** 32, 2 ** 32] and acc[1, :, 0].tolist() == [0, 0, 0]
    assert row_out[:3].tolist() == [[0.0, 0.0]] * 3
    assert row_out[3, 1] == 2.0 and abs(row_out[3, 0] + np.log(np.finfo(np.float32).tiny)) <= ref.F * 88
    assert metrics.classwise_from_bins(acc, 4) == metrics.ClasswiseECE(onehot.numpy(), labels.numpy(), n_bins)


@pytest.mark.parametrize("C,from_probs", [(65, False), (1000, False), (1000, True)])
def test_chunks_and_repeats_give_the_same_bytes(ops, C, from_probs):
    N, n_bins = 257, 10
    rows_h, labels_h = ref.case_inputs(N, C, from_probs)
    rows, labels = torch.from_numpy(rows_h).cuda(), torch.from_numpy(labels_h).cuda()

    def run(cuts):
        def body():
            acc = ops.new_row_scores_acc(C, n_bins, "cuda")
            row_out = torch.zeros(N, 2, dtype=torch.float32, device="cuda")
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                ops.row_scores(rows[lo:hi], labels[lo:hi], from_probs=from_probs, n_bins=n_bins, acc=acc, row_out=row_out, row0=lo)
            return row_out, acc, ops.row_scores_finish_device(row_out, acc)
        return _no_sync(body)

    whole = run([0, N])
    for cuts in ([0, N], [0, 64, 128, 192, N], list(range(N + 1))):       # again; 64 + 64 + 64 + 65; 257 calls of one row
        other = run(cuts)
        for a, b in zip(whole, other):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), len(cuts)
    ref.compare_case(rows_h, labels_h, n_bins, from_probs, whole[0].cpu().numpy(), whole[1].cpu().numpy())


@pytest.mark.parametrize("from_probs", [False, True])
def test_unscorable_rows_and_labels(ops, from_probs):
    """clipmi_val_score's rule: a label outside [0, C) or a row without a softmax gives NaN scores and no hit; such a row counts in the
    last bin only and adds nothing to conf_sum; the other rows are scored as ever."""
    N, C, n_bins = 70, 65, 10
    rows_h, labels_h = ref.case_inputs(N, C, from_probs)
    rows_h, labels_h = rows_h.copy(), labels_h.copy()
    labels_h[3], labels_h[66] = C, -1
    rows_h[5, 64] = np.nan
    rows_h[40, 0] = np.inf
    rows_h[69, :] = -np.inf
    rows_h[7, (labels_h[7] + 1) % C] = 0.0 if from_probs else -np.inf      # a -inf logit is a probability of 0: the row stays scorable
    row_out, acc = ops.row_scores(torch.from_numpy(rows_h).cuda(), torch.from_numpy(labels_h).cuda(), from_probs=from_probs, n_bins=n_bins)
    row_out, acc = row_out.cpu().numpy(), acc.cpu().numpy()
    bad = [3, 66, 5, 40, 69]
    good = np.setdiff1d(np.arange(N), bad)
    assert np.isnan(row_out[bad]).all() and np.isfinite(row_out[good]).all()
    r = ref.reference(rows_h, labels_h, n_bins, from_probs)
    assert np.array_equal(acc[0], r["acc"][0]) and np.array_equal(acc[2], r["acc"][2])
    assert acc[2].sum() == N - len(bad) and np.array_equal(acc[0].sum(axis=1), np.full(C, N))
    if from_probs:
        assert np.array_equal(acc[1], r["acc"][1])
    zmax = r["zmax"]
    assert (np.abs(row_out[good, 0] - r["nll"][good]) <= ref.nll_bound(r["nll"][good], C, zmax, from_probs)).all()
    fin = ops.row_scores_finish(torch.from_numpy(row_out).cuda(), torch.from_numpy(acc).cuda())
    assert np.isnan(fin["nll"]) and np.isnan(fin["brier"]) and np.isfinite(fin["cw_ece"]) and fin["n"] == N


def test_mean_nll_agrees_with_the_fit_monitor(ops):
    """The same logits and labels through clipmi_val_score: its record's nll_sum / n and the finish's mean nll each lie within the mean
    of the per-row bound of the float64 value, so they lie within twice that of one another (the reductions differ)."""
    N, C = 257, 1000
    rows_h, labels_h = ref.case_inputs(N, C)
    rows, labels = torch.from_numpy(rows_h).cuda(), torch.from_numpy(labels_h).cuda()
    row_out, acc = ops.row_scores(rows, labels, n_bins=10)
    fin = ops.row_scores_finish(row_out, acc)
    rec = ops.decode_val_records(ops.val_score(rows, labels, 10), 10)[0]
    r = ref.reference(rows_h, labels_h, 10)
    bound = float(ref.nll_bound(r["nll"], C, r["zmax"]).mean()) + 1e-12
    print(f"mean nll: row scores {fin['nll']!r}, monitor {rec['nll_sum'] / rec['n']!r}, float64 {r['nll'].mean()!r}, bound {bound:.3e}")
    assert rec["n"] == N and abs(fin["nll"] - rec["nll_sum"] / rec["n"]) <= 2 * bound
    assert abs(fin["nll"] - r["nll"].mean()) <= bound


def test_ops_refusals(ops):
    rows, labels = torch.zeros(4, 3, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="GPU"):
        ops.row_scores(rows.cpu(), labels)
    with pytest.raises(TypeError):
        ops.row_scores(rows.double(), labels)
    with pytest.raises(ValueError, match="n_bins"):
        ops.row_scores(rows, labels, n_bins=0)
    with pytest.raises(ValueError, match="labels"):
        ops.row_scores(rows, labels[:3])
    with pytest.raises(TypeError, match="acc"):
        ops.row_scores(rows, labels, acc=torch.zeros(3, 3, 10, dtype=torch.int64, device="cuda"))
    row_out, acc = ops.row_scores(rows[:0], labels[:0])       # an empty batch: nothing launched, nothing added
    assert row_out.shape == (0, 2) and int(acc.abs().sum()) == 0


# ---- runner.test(proper_scores=True) ------------------------------------------------------------------------------------------------
def _host_scores(rows, labels, from_probs, n_bins=10):
    """The host restatement on rows read back from the device, with the tolerances the fp32 format allows on the three numbers."""
    rows, labels = rows.cpu().numpy(), labels.cpu().numpy()
    N, C = rows.shape
    r = ref.reference(rows, labels, n_bins, from_probs)
    rel = ref.eps_prob(C, r["zmax"], from_probs)
    moved = int(ref.near_edge(r["p"], n_bins, rel).sum()) if rel else 0
    tol = {"nll": float(ref.nll_bound(r["nll"], C, r["zmax"], from_probs).mean()) + 1e-12,
           "brier": float(ref.brier_bound(r["p"], labels, C, r["zmax"], from_probs).mean()) + 1e-12,
           "cw_ece": 100.0 * (float((rel * r["p"] + 2.0 ** -32).sum()) + 2.0 * moved) / (N * C) + 1e-12}
    want = {"nll": float(r["nll"].mean()), "brier": float(r["brier"].mean()),
            "cw_ece": 100.0 * metrics.ClasswiseECE(r["p"], labels, n_bins)}
    return want, tol


@pytest.mark.parametrize("mode", ["plain", "procal", "bin_mean_shift"])
def test_runner_test_with_proper_scores(mode):
    from clip_calibration_amd import runner
    from clip_calibration_amd.calibrator import VLCalibration
    from clip_calibration_amd.model import build_model
    from clip_calibration_amd.proximity import knn_dists_device
    from clip_calibration_amd.trainers import CoOpCLIP, ZeroshotCLIP
    sd = syn.synthetic_state_dict("tiny", seed=0)
    model = build_model(dict(sd), {"trainer": "CoOp", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0}).cuda()
    C, n_ctx, K = 12, 4, 3
    coop_b = CoOpCLIP(model, syn.synthetic_token_ids(C, "tiny", seed=20, n_ctx_placeholders=n_ctx), n_ctx=n_ctx, seed=2)
    coop_n = CoOpCLIP(model, syn.synthetic_token_ids(C, "tiny", seed=21, n_ctx_placeholders=n_ctx), n_ctx=n_ctx, seed=2)
    zs_b = ZeroshotCLIP(model, syn.synthetic_token_ids(C, "tiny", seed=20))
    zs_n = ZeroshotCLIP(model, syn.synthetic_token_ids(C, "tiny", seed=21))
    val_images, test_images = syn.synthetic_images(40, "tiny", seed=30), syn.synthetic_images(37, "tiny", seed=31)
    loader = lambda im, lb, bs: [(im[i:i + bs], lb[i:i + bs]) for i in range(0, len(im), bs)]
    val_labels = torch.arange(40) % C
    tuned = runner.collect_base_val_features(coop_b, loader(val_images, val_labels, 8), image_k=K)
    zsd = runner.collect_base_val_features(zs_b.model_inference, loader(val_images, val_labels, 8), image_k=K)
    tfd = runner.text_feature_dict(zsd, zs_n.text_features, tuned, coop_n.text_features())
    kw = {"plain": {}, "procal": dict(base_calibration_mode="scaling_based", procal_flag=True),
          "bin_mean_shift": dict(base_calibration_mode="bin_based", base_bin_calibrator_name="multi_isotonic_regression", procal_flag=True)}[mode]
    cal = VLCalibration(tuned, tfd, dac_flag=True, k_dac=5, **kw)
    cal.fit()
    test_labels = torch.arange(37) % 5
    args = dict(val_dict=tuned, calibrator=cal, image_k=K)
    base = runner.test(coop_n, loader(test_images, test_labels, 16), **args)
    res = runner.test(coop_n, loader(test_images, test_labels, 16), proper_scores=True, **args)
    assert list(res) == list(base) + ["nll", "brier", "cw_ece"]
    for k in base:       # the existing keys: the same bits
        assert res[k] == base[k], (k, res[k], base[k])
    # what was deployed, read back: the DAC-scaled logits, or the calibrated matrix of the whole split
    dac = cal.class_confidence_device("cuda")
    outs = [coop_n(im.cuda(), dac_conf=dac, want_conf_pred=True) for im, _ in loader(test_images, test_labels, 16)]
    logits = torch.cat([o[0] for o in outs]).float()
    labels = test_labels.cuda()
    if mode == "plain":
        want, tol = _host_scores(logits, labels, False)
    else:
        refs = torch.as_tensor(np.asarray(tuned["val_image_features"]), dtype=torch.float32, device="cuda")
        prox = torch.exp(-knn_dists_device(torch.cat([o[1] for o in outs]).float(), refs, min(K, refs.shape[0])).mean(dim=1))
        probs, _, _ = cal.row_calibrator_device()[0].predict_device(logits, prox, want_probs=True)
        want, tol = _host_scores(probs, labels, True)
    for k in ("nll", "brier", "cw_ece"):
        print(f"runner.test {mode} {k}: device {res[k]!r} host {want[k]!r} tolerance {tol[k]:.3e}")
        assert abs(res[k] - want[k]) <= tol[k], (mode, k, res[k], want[k], tol[k])
