"""Cost of per-epoch validation inside the one-call CLIP-Adapter and TaskRes fits (``adapterfit.fit_adapter`` / ``taskresfit.fit_residuals``
with ``val=``), of the two validation-logits kernels alone, and of the same scoring done with torch on the same GPU with the read-back a
Python loop over epochs needs.  Measurement only; bench.py does not run it.

The shapes of the two fits' own bench tools: E 512, H 128; 1 600 train rows x 100 classes and 16 000 x 1 000 (16 shots), the fits'
default batches (32 and 256, the last short batch dropped), --epochs epochs; N_val = 5 000 and 50 000.  The yardstick of the cost is the
unmonitored run OF THE SAME PROCESS: the monitored and the unmonitored run take turns, one host-timed whole fit (its one wait included)
each per round, --iters rounds after --warmup; the figure is the median with the run's own min-to-max spread, and ``monitor_cost_ms`` is
reported beside the larger of the two spreads (a difference inside it is not resolved).  The kernels alone are timed between two device
events around --kernel-window calls; the torch scoring ends in ``.item()``, so its sample is host time around one call.

Usage: python tools/cachedmonitor_bench.py [--iters 5] [--warmup 2] [--epochs 20] [--out profiles/cachedmonitor_bench.json]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clip_calibration_amd import adapterfit, ops, taskresfit  # noqa: E402

E, H, SHOTS, BINS, RATIO, ALPHA, LOGIT_SCALE = 512, 128, 16, 10, 0.2, 0.5, 4.6052


def window_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def host_ms(fn, n=1):
    """Host time of a call that ends in a wait or a read-back."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def summary(samples):
    med = statistics.median(samples)
    return {"median_ms": med, "min_ms": min(samples), "max_ms": max(samples), "spread_ms": max(samples) - min(samples)}


def alternate(calls, iters, warmup):
    """{name: summary}: ``calls`` maps a name to (fn, window, timer); every round takes one sample of each."""
    samples = {name: [] for name in calls}
    for k in range(warmup + iters):
        for name, (fn, window, timer) in calls.items():
            ms = timer(fn, window)
            if k >= warmup:
                samples[name].append(ms)
    return {name: summary(s) for name, s in samples.items()}


def torch_scoring(z_of, labels):
    """What a Python loop does behind an epoch: the logits' matmul, cross-entropy, arg-max, a histogram of the confidences, the read-back."""
    z = z_of()
    nll = torch.nn.functional.cross_entropy(z, labels, reduction="sum")
    conf, pred = torch.softmax(z, dim=1).max(dim=1)
    hit = (pred == labels)
    which = torch.bucketize(conf.double(), torch.linspace(0, 1, BINS + 1, dtype=torch.float64, device=z.device), right=True) - 1
    count = torch.bincount(which, minlength=BINS + 1)
    hits = torch.bincount(which, weights=hit.double(), minlength=BINS + 1)
    sums = torch.bincount(which, weights=conf.double(), minlength=BINS + 1)
    return hit.sum().item(), nll.item(), count.cpu(), hits.cpu(), sums.cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--kernel-window", type=int, default=20)
    ap.add_argument("--classes", type=int, nargs="*", default=[100, 1000])
    ap.add_argument("--rows", type=int, nargs="*", default=[5000, 50000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(1)
    scale = math.exp(LOGIT_SCALE)
    out = {"E": E, "H": H, "val_bins": BINS, "epochs": a.epochs, "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "kernel_window": a.kernel_window, "cases": []}
    for C in a.classes:
        n, batch = SHOTS * C, (32, 256)
        feats = torch.randn(n, E, generator=g).cuda()
        labels = (torch.arange(n) % C).cuda()
        text = torch.randn(C, E, generator=g)
        text_n = (text / text.norm(dim=1, keepdim=True)).cuda()
        text = text.cuda()
        w1, w2 = torch.randn(H, E, generator=g) / math.sqrt(3 * E), torch.randn(E, H, generator=g) / math.sqrt(3 * H)
        res = torch.zeros(C, E, device="cuda")
        for N in a.rows:
            vf = torch.randn(N, E, generator=g).cuda()
            vl = torch.randint(0, C, (N,), generator=g).cuda()
            w1d, w2d = w1.cuda(), w2.cuda()
            logits = torch.empty(N, C, device="cuda")
            fit_a = lambda **kw: adapterfit.fit_adapter(feats, labels, text_n, w1, w2, RATIO, LOGIT_SCALE, epochs=a.epochs, batch_size=batch[0], **kw)
            fit_t = lambda **kw: taskresfit.fit_residuals(feats, labels, text, None, ALPHA, LOGIT_SCALE, epochs=a.epochs, batch_size=batch[1], **kw)

            def torch_adapter():
                x = RATIO * torch.relu(torch.relu(vf @ w1d.t()) @ w2d.t()) + (1 - RATIO) * vf
                return scale * (x / x.norm(dim=1, keepdim=True)) @ text_n.t()

            def torch_taskres():
                t = text + ALPHA * res
                return scale * (vf / vf.norm(dim=1, keepdim=True)) @ (t / t.norm(dim=1, keepdim=True)).t()

            calls = {
                "adapter_fit": (lambda: fit_a(), 1, host_ms),
                "adapter_fit_monitored": (lambda: fit_a(val=(vf, vl), final_model="best_val"), 1, host_ms),
                "taskres_fit": (lambda: fit_t(), 1, host_ms),
                "taskres_fit_monitored": (lambda: fit_t(val=(vf, vl), final_model="best_val"), 1, host_ms),
                "adapter_val_logits": (lambda: ops.adapter_val_logits(vf, text_n, w1d, w2d, RATIO, scale, out=logits), a.kernel_window, window_ms),
                "taskres_val_logits": (lambda: ops.taskres_val_logits(vf, text, res, ALPHA, scale, out=logits), a.kernel_window, window_ms),
                "torch_adapter_scoring_with_readback": (lambda: torch_scoring(torch_adapter, vl), 1, host_ms),
                "torch_taskres_scoring_with_readback": (lambda: torch_scoring(torch_taskres, vl), 1, host_ms),
            }
            t = alternate(calls, a.iters, a.warmup)
            r = {"classes": C, "train_rows": n, "val_rows": N, "times": t, "logits_bytes": 4 * N * C}
            for kind in ("adapter", "taskres"):
                plain, watched = t[f"{kind}_fit"], t[f"{kind}_fit_monitored"]
                r[f"{kind}_monitor_cost_ms"] = watched["median_ms"] - plain["median_ms"]
                r[f"{kind}_monitor_cost_per_epoch_ms"] = r[f"{kind}_monitor_cost_ms"] / a.epochs
                r[f"{kind}_spread_ms"] = max(plain["spread_ms"], watched["spread_ms"])
                r[f"{kind}_monitor_cost_share"] = r[f"{kind}_monitor_cost_ms"] / plain["median_ms"]
            out["cases"].append(r)
            print(json.dumps(r))
            del vf, vl, logits, calls
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
