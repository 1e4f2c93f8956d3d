"""Time of ProCal's evaluation (DensityRatioCalibration.predict_device: one clipmi_procal_rows launch, csrc/procal.hip) at an ImageNet
base-to-new shape -- N_test = 25 000 rows of C = 500 classes against N_val = 2 000 and 8 000 fitted val points -- against the float64
numpy oracle of tests/procal_ref.py on the host (the reference's statsmodels loop does the same arithmetic one test row at a time).
Measurement only; bench.py does not run it.

Device: median of --iters launches between two events, after --warmup.  Host: one run of the oracle's c* and rescale on --host-rows
rows, scaled to N_test (it is linear in the rows).  Usage: python tools/procal_bench.py [--out profiles/procal_bench.json]"""
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
import procal_ref as ref  # noqa: E402
from clip_calibration_amd.procal import DensityRatioCalibration  # noqa: E402


def fitted(n_val, seed=0):
    rng = np.random.default_rng(seed)
    C = 500
    lg = rng.normal(0, 3, (n_val, C)).astype(np.float32)
    probs = ref.softmax(lg)
    preds = probs.argmax(1)
    true = np.where(rng.random(n_val) < 0.7, preds, rng.integers(0, C, n_val))
    prox = rng.normal(0.5, 0.05, n_val)
    cal = DensityRatioCalibration()
    cal.fit(probs, preds, true, prox)
    return cal, ref.ProCalRef(probs, preds, true, prox)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-test", type=int, default=25000)
    ap.add_argument("--classes", type=int, default=500)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "procal_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    lg = rng.normal(0, 3, (a.n_test, a.classes)).astype(np.float32)
    prox = rng.normal(0.5, 0.05, a.n_test).astype(np.float32)
    d_lg, d_prox = torch.from_numpy(lg).cuda(), torch.from_numpy(prox).cuda()
    props = torch.cuda.get_device_properties(0)
    res = {"device": f"{torch.cuda.get_device_name(0)} ({props.gcnArchName}, {props.multi_processor_count} CUs)", "n_test": a.n_test, "classes": a.classes, "runs": []}
    for n_val in (2000, 8000):
        cal, orc = fitted(n_val)
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
            run = {"n_val": n_val, "n_true": int(cal.data_true.shape[0]), "n_false": int(cal.data_false.shape[0]),
                   "want_probs": want_probs, "device_us_median": statistics.median(times), "device_us_min": min(times)}
            if not want_probs:
                t0 = time.perf_counter()
                orc.predict_logits(lg[:a.host_rows], prox[:a.host_rows])
                host = (time.perf_counter() - t0) * a.n_test / a.host_rows
                run["host_oracle_s_scaled"] = host
                run["host_rows_timed"] = a.host_rows
                run["speedup"] = host / (run["device_us_median"] * 1e-6)
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
