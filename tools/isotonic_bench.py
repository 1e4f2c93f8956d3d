"""Time of multi-class isotonic calibration (clip_calibration_amd/isotonic.py, csrc/isotonic.hip) at an ImageNet base-to-new shape --
N_test = 25 000 rows of C = 500 classes against N_val = 2 000 and 8 000 val rows, plain and Bin-Mean-Shift (5 bins) -- next to a same-run
timing of the numpy restatement of tests/isotonic_ref.py on the host (sort-based float64 fit; float64 np.interp per element), which is
the arithmetic of the reference's numpy + sklearn + scipy path.  Measurement only; bench.py does not run it.

Device predict: median of --iters launches between two events, after --warmup.  Device fit: wall time of the whole fit_device (two
launches, the host's sort of the keys, the copies and the float64 pooling), median of --fit-iters.  Host: one run each.
Usage: python tools/isotonic_bench.py [--out profiles/isotonic_bench.json]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import isotonic_ref as ref  # noqa: E402
from clip_calibration_amd import isotonic as iso  # noqa: E402

BINS = 5


def split(n, C, seed):
    """Cosine-like logits x 100 around a class prototype, and a proximity."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, n)
    noise = rng.uniform(0.6, 1.6, n)
    cos = rng.normal(0.2, 0.035, (n, C)) * noise[:, None]
    cos[np.arange(n), labels] += rng.normal(0.07, 0.05, n)
    prox = np.exp(-(0.5 + 0.25 * noise + rng.normal(0, 0.05, n))).astype(np.float32)
    return (cos * 100.0).astype(np.float32), labels.astype(np.int64), prox


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-test", type=int, default=25000)
    ap.add_argument("--classes", type=int, default=500)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--fit-iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isotonic_bench.json"))
    a = ap.parse_args()
    torch.set_num_threads(16)
    lg, _, prox = split(a.n_test, a.classes, 1)
    d_lg, d_prox = torch.from_numpy(lg).cuda(), torch.from_numpy(prox).cuda()
    props = torch.cuda.get_device_properties(0)
    res = {"device": f"{torch.cuda.get_device_name(0)} ({props.gcnArchName}, {props.multi_processor_count} CUs)", "n_test": a.n_test,
           "classes": a.classes, "host_threads": torch.get_num_threads(), "runs": []}
    for n_val in (2000, 8000):
        vl, vy, vp = split(n_val, a.classes, 2)
        d_vl = torch.from_numpy(vl).cuda()
        for bms in (False, True):
            cal = iso.BinMeanShift(BINS) if bms else iso.MultiIsotonicRegression()
            fit = (lambda: cal.fit_device(d_vl, vy, vp)) if bms else (lambda: cal.fit_device(d_vl, vy))
            fit()
            torch.cuda.synchronize()
            fits = []
            for _ in range(a.fit_iters):
                t0 = time.perf_counter()
                fit()
                fits.append(time.perf_counter() - t0)
            run = {"n_val": n_val, "bin_mean_shift": bms, "thresholds": [int(X.size) for X, _ in cal._tables],
                   "fit_device_s_median": statistics.median(fits), "fit_device_s_min": min(fits)}
            for want_probs in (False, True):
                for _ in range(a.warmup):
                    cal.predict_device(d_lg, d_prox, want_probs=want_probs)
                torch.cuda.synchronize()
                times = []
                for _ in range(a.iters):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    cal.predict_device(d_lg, d_prox, want_probs=want_probs)
                    e1.record()
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1) * 1e3)
                key = "predict_rows_us" if want_probs else "predict_top1_us"
                run[key + "_median"], run[key + "_min"] = statistics.median(times), min(times)
            # the host path: softmax and second softmax in float32, sort-based float64 fit, np.interp per element, argmax
            t0 = time.perf_counter()
            xv = ref.second_softmax(ref.softmax32(vl))
            if bms:
                edges, tables = ref.fit_bins(xv, vy, vp, BINS)
            else:
                X, Y = ref.fit_plain(xv, vy)
            t1 = time.perf_counter()
            xt = ref.second_softmax(ref.softmax32(lg))
            out = ref.calibrate_bins(edges, tables, xt, prox) if bms else ref.calibrate(X, Y, xt)
            ref.conf_pred(out)
            t2 = time.perf_counter()
            run["fit_host_s"], run["predict_host_s"] = t1 - t0, t2 - t1
            run["fit_speedup"] = run["fit_host_s"] / run["fit_device_s_median"]
            run["predict_speedup"] = run["predict_host_s"] / (run["predict_rows_us_median"] * 1e-6)
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
