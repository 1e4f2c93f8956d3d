"""Time of the evaluator's sample-level tail -- macro-F1, AdaptiveECE and PIECE from the kept (conf, pred, gt) vectors and the proximity --
at N = 25 000 and N = 50 000 samples of C = 1 000 classes: the host tail (the D2H copy of the four vectors plus the three numpy metrics of
clip_calibration_amd/metrics.py) against the device tail (csrc/sample_metrics.hip plus the host arithmetic on its small outputs), and every
kernel entry point alone.  Measurement only; bench.py does not run it.

Tails: wall time around work that ends with its results on the host (the device tail's copies synchronise), median / min / max of --iters
after --warmup, the two alternating.  Entry points: device events around one call, the same statistics, in microseconds.
Usage: python tools/sample_metrics_bench.py [--out profiles/sample_metrics_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clip_calibration_amd import metrics, ops  # noqa: E402
from clip_calibration_amd.evaluator import DeviceCalibrationEvaluator  # noqa: E402

BINS = 10


def split(n, C, seed):
    """Confidences like a softmax top-1's, predictions right about 70 % of the time, a proximity like exp(-mean kNN distance)."""
    rng = np.random.default_rng(seed)
    conf = rng.beta(5, 2, n).astype(np.float32)
    gt = rng.integers(0, C, n).astype(np.int64)
    pred = np.where(rng.random(n) < 0.7, gt, rng.integers(0, C, n)).astype(np.int32)
    prox = np.exp(-(0.5 + rng.normal(0.25, 0.05, n))).astype(np.float32)
    return conf, pred, gt, prox


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def timed_us(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return stats(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_metrics_bench.json"))
    a = ap.parse_args()
    torch.set_num_threads(16)
    props = torch.cuda.get_device_properties(0)
    res = {"device": f"{torch.cuda.get_device_name(0)} ({props.gcnArchName}, {props.multi_processor_count} CUs)", "classes": a.classes,
           "iters": a.iters, "warmup": a.warmup, "host_threads": torch.get_num_threads(), "runs": []}
    for n in (25000, 50000):
        conf, pred, gt, prox = split(n, a.classes, n)
        d_conf, d_pred, d_gt, d_prox = (torch.from_numpy(v).cuda() for v in (conf, pred, gt, prox))

        def host_tail():
            c, p, y, x = d_conf.cpu().numpy(), d_pred.cpu().numpy().astype(np.int64), d_gt.cpu().numpy(), d_prox.cpu().numpy()
            return metrics.macro_f1(p, y), metrics.AdaptiveECE(c, p, y, BINS), metrics.PIECE(c, x, p, y, BINS, BINS)

        ev = DeviceCalibrationEvaluator(BINS, keep_samples=True, piece_bins=BINS, sample_metrics="device", n_classes=a.classes)
        ev.note_processed(d_conf, d_pred, d_gt)

        def device_tail():
            r = ev._device_sample_metrics(d_prox)
            return r["macro_f1"], r["ace"], r["piece"]

        for _ in range(a.warmup):
            h, d = host_tail(), device_tail()
        torch.cuda.synchronize()
        host_s, dev_s = [], []
        for _ in range(a.iters):
            for fn, sink in ((host_tail, host_s), (device_tail, dev_s)):
                t0 = time.perf_counter()
                fn()
                sink.append((time.perf_counter() - t0) * 1e6)
        ranks = np.unique(metrics.quantile_ranks(n, BINS))
        key_edges = np.quantile(prox.astype(np.float64), np.linspace(0, 1, BINS + 1)[1:-1])
        conf_edges = np.linspace(0, 1, BINS + 1)[1:-1]
        d_ke, d_ce = torch.from_numpy(key_edges).cuda(), torch.from_numpy(conf_edges).cuda()
        groups = torch.zeros(3, BINS * BINS, dtype=torch.float64, device="cuda")
        run = {"n": n, "max_abs_difference": max(abs(x - y) for x, y in zip(h, d)),
               "host_tail_us": stats(host_s), "device_tail_us": stats(dev_s),
               "host_over_device": statistics.median(host_s) / statistics.median(dev_s),
               "order_stats_us": timed_us(lambda: ops.order_stats(d_conf, ranks), a.warmup, a.iters), "order_stats_ranks": int(ranks.size),
               "group_gap_accumulate_us": timed_us(lambda: ops.group_gap_accumulate(d_conf, d_pred, d_gt, key=d_prox, key_edges=d_ke,
                                                                                    conf_edges=d_ce, groups=groups), a.warmup, a.iters),
               "class_counts_us": timed_us(lambda: ops.class_counts(d_pred, d_gt, a.classes), a.warmup, a.iters)}
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
