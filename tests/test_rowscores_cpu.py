"""Row scores without a GPU: the numpy restatement (clip_calibration_amd/metrics.py NLL / Brier / ClasswiseECE) against direct float64
formulas, closed forms of the class-wise ECE, the fixed-point restatement, the seeded GPU cases' distance from the bin edges, the fp32
emulation inside the derived bounds, the C entry points' refusals, the default keys of the evaluator and runner.test, and the two-rank sum."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from scipy.special import log_softmax, softmax

import rowscores_ref as ref
from clip_calibration_amd import _lib, metrics, parallel


def _case(N, C, seed):
    rng = np.random.default_rng(seed)
    return 3.0 * rng.standard_normal((N, C)), rng.integers(0, C, N)


@pytest.mark.parametrize("N,C", [(1, 1), (5, 2), (33, 7), (40, 130)])
def test_restatement_against_direct_float64_formulas(N, C):
    z, y = _case(N, C, 11 * N + C)
    p = softmax(z, axis=1)
    nll, brier = metrics.row_scores(z, y)
    assert np.abs(nll - (-log_softmax(z, axis=1)[np.arange(N), y])).max() < 1e-12
    want_b = np.array([sum((p[i, c] - (1.0 if c == y[i] else 0.0)) ** 2 for c in range(C)) for i in range(N)])
    assert np.abs(brier - want_b).max() < 1e-12
    assert abs(metrics.NLL(z, y) - (-log_softmax(z, axis=1)[np.arange(N), y]).mean()) < 1e-12
    assert abs(metrics.Brier(z, y) - want_b.mean()) < 1e-12
    # probabilities as given, not summing to 1
    q = p * 0.8
    nll_p, brier_p = metrics.row_scores(q, y, from_probs=True)
    assert np.abs(nll_p + np.log(q[np.arange(N), y])).max() < 1e-12
    assert np.abs(brier_p - np.array([sum((q[i, c] - (c == y[i])) ** 2 for c in range(C)) for i in range(N)])).max() < 1e-12
    for n_bins in (1, 10, 15):
        edges = np.linspace(0, 1, n_bins + 1)
        total = 0.0
        for c in range(C):       # explicit loops over classes and closed-right last interval
            for b in range(n_bins):
                lo, hi = edges[b], edges[b + 1]
                sel = (q[:, c] >= lo) & ((q[:, c] < hi) | (b == n_bins - 1))
                if sel.any():
                    total += sel.sum() / N * abs((y[sel] == c).mean() - q[sel, c].mean())
        assert abs(metrics.ClasswiseECE(q, y, n_bins) - total / C) < 1e-12
        fixed = metrics.classwise_fixed_point(q, y, n_bins)
        assert fixed.dtype == np.int64 and np.array_equal(fixed[0].sum(axis=1), np.full(C, N)) and fixed[2].sum() == N
        assert abs(metrics.classwise_from_bins(fixed, N) - total / C) <= N * C * 2.0 ** -33 / N / C + 1e-15   # half a unit per element


def test_classwise_ece_closed_forms():
    # one class: every row holds p = 1 and is labelled 0 -- hits = conf = N in the last interval
    assert metrics.ClasswiseECE(np.ones((9, 1)), np.zeros(9, np.int64), 10) == 0.0
    # one class with a constant p: the gap is |1 - p|
    assert abs(metrics.ClasswiseECE(np.full((9, 1), 0.25), np.zeros(9, np.int64), 10) - 0.75) < 1e-15
    # one-hot rows: right rows give 0; rows that are one-hot on the wrong class leave gap 1 in two classes each
    y = np.arange(12) % 4
    onehot = np.eye(4)[y]
    assert metrics.ClasswiseECE(onehot, y, 15) == 0.0
    wrong = np.eye(4)[(y + 1) % 4]
    assert abs(metrics.ClasswiseECE(wrong, y, 15) - 2.0 / 4) < 1e-15
    assert metrics.NLL(onehot, y, from_probs=True) == 0.0 and metrics.Brier(onehot, y, from_probs=True) == 0.0
    assert metrics.Brier(wrong, y, from_probs=True) == 2.0
    assert abs(metrics.NLL(wrong, y, from_probs=True) + np.log(np.finfo(np.float32).tiny)) < 1e-12


def test_unscorable_rows_and_labels_follow_the_monitors_rule():
    z = np.array([[0.0, 1.0, 2.0], [np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0], [-np.inf, -np.inf, -np.inf], [-np.inf, 0.0, 1.0], [0.0, 0.0, 0.0]])
    y = np.array([2, 0, 0, 0, 1, 3])
    nll, brier = metrics.row_scores(z, y)
    assert np.isfinite(nll[[0, 4]]).all() and np.isnan(nll[[1, 2, 3, 5]]).all() and np.isnan(brier[[1, 2, 3, 5]]).all()
    assert list(metrics.unscorable_rows(z)) == [False, True, True, True, False, False]
    acc = ref.reference(z.astype(np.float32), y, 10)["acc"]
    assert np.array_equal(acc[0].sum(axis=1), [6, 6, 6]) and acc[0][:, 10].tolist() == [3, 3, 3]   # three rows sit in the last bin only
    assert acc[2].sum() == 2                                                                     # rows 0 and 4 alone can hit


@pytest.mark.parametrize("N", ref.NS)
@pytest.mark.parametrize("C", ref.CS)
def test_seeded_cases_stay_clear_of_the_bin_edges_and_inside_the_bounds(N, C):
    """The inputs of tests/test_gpu_rowscores.py: no float64 probability lies within the derived fp32 error of a bin edge, so the GPU
    comparison of counts and hits excludes nothing; and numpy's fp32 arithmetic at the kernel's rounding points meets the bounds."""
    for from_probs in (False, True):
        rows, labels = ref.case_inputs(N, C, from_probs)
        r = ref.reference(rows, labels, 10, from_probs)
        rel = ref.eps_prob(C, r["zmax"], False)      # the logits' bound also for the probabilities: the stricter statement
        for n_bins in ref.BINS:
            assert rel == 0.0 or not ref.near_edge(r["p"], n_bins, rel).any(), (N, C, n_bins, from_probs)
        if N * C <= 65 * 257:
            nll, brier, p = ref.emulate_fp32(rows, labels, from_probs)
            rn = np.abs(nll - r["nll"]) / ref.nll_bound(r["nll"], C, r["zmax"], from_probs)
            rb = np.abs(brier - r["brier"]) / ref.brier_bound(r["p"], labels, C, r["zmax"], from_probs)
            print(f"fp32 emulation N={N} C={C} probs={int(from_probs)}: nll err/bound {rn.max():.3f}, brier err/bound {rb.max():.3f}")
            assert rn.max() <= 1.0 and rb.max() <= 1.0
            if not from_probs:
                assert (np.abs(p - r["p"]) <= rel * r["p"]).all()


def test_argument_refusals_need_no_gpu():
    L = _lib.lib
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)
    rs = lambda rows=p, ld=8, labels=p, N=3, C=8, fp=0, nb=10, out=p, acc=p: L.clipmi_row_scores(rows, ld, labels, N, C, fp, nb, out, acc, None)
    for kw in (dict(rows=None), dict(labels=None), dict(out=None), dict(acc=None)):
        assert rs(**kw) == _lib.ERR_ARG, kw
    for kw in (dict(labels=odd), dict(out=odd), dict(acc=odd), dict(rows=ctypes.c_void_p(4096 + 2)), dict(nb=0), dict(nb=1025), dict(fp=2)):
        assert rs(**kw) == _lib.ERR_ARG, kw
    for kw in (dict(C=0, ld=0), dict(ld=7), dict(N=-1)):
        assert rs(**kw) == _lib.ERR_SHAPE, kw
    assert "row_scores" in _lib.last_error()
    assert rs(N=0) == _lib.OK and rs(N=0, rows=None, labels=None, out=None, acc=None) == _lib.OK      # nothing to do, no launch
    assert rs(N=0, C=0, ld=0) == _lib.ERR_SHAPE and rs(N=0, nb=0) == _lib.ERR_ARG                      # but the shape is still checked
    assert L.clipmi_row_scores_acc_bytes(1000, 10) == 3 * 8 * 1000 * 11
    assert L.clipmi_row_scores_acc_bytes(0, 10) == 0 and L.clipmi_row_scores_acc_bytes(4, 0) == 0 and L.clipmi_row_scores_acc_bytes(4, 1025) == 0
    ws = L.clipmi_row_scores_finish_workspace_bytes(50000, 1000)
    assert ws >= 8 * (2 * 13 + 4) and ws % 256 == 0 and L.clipmi_row_scores_finish_workspace_bytes(0, 4) == 0
    w = ctypes.c_void_p(8192)
    fin = lambda ro=p, N=3, acc=p, C=8, nb=10, out=p, work=w, wb=1 << 20: L.clipmi_row_scores_finish(ro, N, acc, C, nb, out, work, wb, None)
    for kw in (dict(ro=None), dict(acc=None), dict(out=None), dict(work=None), dict(ro=odd), dict(out=odd), dict(work=ctypes.c_void_p(8192 + 128)),
               dict(nb=0), dict(nb=1025)):
        assert fin(**kw) == _lib.ERR_ARG, kw
    assert fin(N=0) == _lib.ERR_SHAPE and fin(C=0) == _lib.ERR_SHAPE
    assert fin(wb=8) == _lib.ERR_WORKSPACE
    assert _lib.ABI_VERSION == 16 and L.clipmi_abi_version() == 16


def test_default_keys_are_todays():
    """Without ``proper_scores`` -- and with it, as long as no rows were processed -- the evaluator answers today's keys."""
    from clip_calibration_amd.evaluator import DeviceCalibrationEvaluator
    import inspect
    from clip_calibration_amd import runner
    assert inspect.signature(runner.test).parameters["proper_scores"].default is False
    assert inspect.signature(DeviceCalibrationEvaluator.__init__).parameters["proper_scores"].default is False
    rng = np.random.default_rng(3)
    conf = rng.uniform(0.2, 1.0, 50).astype(np.float32)
    pred, gt = rng.integers(0, 4, 50), rng.integers(0, 4, 50)
    want = None
    for proper in (False, True):
        ev = DeviceCalibrationEvaluator(10, device="cpu", keep_samples=True, proper_scores=proper)
        ev.bins += torch.from_numpy(metrics.bin_statistics(conf, pred, gt, 10)).reshape(-1)    # what process() adds on the device
        ev._conf, ev._pred, ev._gt = [torch.from_numpy(conf)], [torch.from_numpy(pred)], [torch.from_numpy(gt)]
        res = ev.evaluate()
        assert list(res) == ["accuracy", "error_rate", "macro_f1", "confidence", "ece", "mce", "ace", "total"]
        want = want or res
        assert res == want
    with pytest.raises(RuntimeError, match="proper_scores"):
        DeviceCalibrationEvaluator(10, device="cpu").process_rows(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class _HostEvaluator:
    """CPU stand-in with the fields gather_samples touches; its row scores are the restatement's, rounded as the device stores them."""
    keep_samples = True
    proper_scores = True

    def __init__(self, probs, gt, n_bins=10):
        n = len(gt)
        conf, pred = probs.max(axis=1).astype(np.float32), probs.argmax(axis=1)
        self.bins = torch.from_numpy(metrics.bin_statistics(conf, pred, gt, n_bins)).reshape(-1)
        self._conf, self._pred, self._gt = [torch.from_numpy(conf)], [torch.from_numpy(pred)], [torch.from_numpy(gt)]
        self._row_out, self._class_acc = [], None
        if n:
            nll, brier = metrics.row_scores(probs, gt, from_probs=True)
            self._row_out = [torch.from_numpy(np.stack([nll, brier], axis=1).astype(np.float32))]
            self._class_acc = torch.from_numpy(metrics.classwise_fixed_point(probs, gt, n_bins))


def _finish(ev):
    from clip_calibration_amd.evaluator import DeviceCalibrationEvaluator
    res = {}
    DeviceCalibrationEvaluator._append_proper_scores(ev, res)
    return res


def _worker(rank, world, port, split, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=__import__("datetime").timedelta(seconds=60))
    try:
        rows, gt = ref.case_inputs(65, 7, from_probs=True)
        rows = rows.astype(np.float64)
        one = _finish(_HostEvaluator(rows, gt))
        lo, hi = (0, split) if rank == 0 else (split, 65)
        ev = _HostEvaluator(rows[lo:hi], gt[lo:hi])
        parallel.gather_samples(ev)
        assert np.array_equal(ev._class_acc.numpy(), metrics.classwise_fixed_point(rows, gt, 10))       # integer sums: exact
        both = _finish(ev)
        assert list(both) == ["nll", "brier", "cw_ece"] and both == one, (both, one)
        assert abs(both["cw_ece"] - 100.0 * metrics.ClasswiseECE(rows, gt, 10)) < 1e-7
        assert abs(both["nll"] - metrics.NLL(rows, gt, True)) < 1e-6 and abs(both["brier"] - metrics.Brier(rows, gt, True)) < 1e-6
        np.save(os.path.join(out_dir, f"r{rank}.npy"), np.array(list(both.values())))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("split", [33, 65])      # 65: rank 1 holds an empty shard and learns the block's shape from rank 0
def test_two_rank_sum_equals_one_rank(tmp_path, split):
    mp.spawn(_worker, args=(2, _free_port(), split, str(tmp_path)), nprocs=2, join=True)
    assert np.array_equal(np.load(tmp_path / "r0.npy"), np.load(tmp_path / "r1.npy"))
