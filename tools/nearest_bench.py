"""Time of ops.nearest_rows (csrc/nearest.hip: the K nearest reference rows with their indices) at the shapes of the prompt-interpretation
use: 16, 144 and 16 000 context rows against the 49 408 x 512 token embedding, and 16 rows against a 49 408 x 768 one, all at K = 10.
Comparators, in the same process on the same GPU, taken in turn inside every repetition:
  cdist_topk   torch.cdist + torch.topk(largest=False) on fp32 -- what a user would otherwise write (it forms the [Nq, Nr] matrix);
  knn_dists    clipmi_knn_dists at the same shape -- distances only, one workgroup per 8 queries walks the whole reference set;
  splits_1     ops.nearest_rows with one slice per query block.
Measurement only; bench.py does not run it.  Device events around `calls` back-to-back calls (allocation of the outputs included), the time
per call; median / min / max of --iters repetitions after --warmup.  The rates are the algorithm's 3 Nq Nr E flop and one read of refs
over the median time.  Usage: python tools/nearest_bench.py [--out profiles/nearest_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clip_calibration_amd import _lib, ops  # noqa: E402
from clip_calibration_amd.proximity import knn_dists_device  # noqa: E402

SHAPES = [(16, 49408, 512), (144, 49408, 512), (16000, 49408, 512), (16, 49408, 768)]
K = 10


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def once_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nearest_bench needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "k": K, "iters": a.iters, "warmup": a.warmup, "unit": "microseconds per call", "runs": []}
    for nq, nr, e in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(nq + e)
        refs = torch.randn(nr, e, generator=g, device="cuda")
        q = torch.randn(nq, e, generator=g, device="cuda")
        fns = {"nearest_rows": lambda: ops.nearest_rows(q, refs, K),
               "splits_1": lambda: ops.nearest_rows(q, refs, K, 1),
               "knn_dists": lambda: knn_dists_device(q, refs, K),
               "cdist_topk": lambda: torch.topk(torch.cdist(q, refs), K, dim=1, largest=False)}
        calls = 1 if nq >= 1000 else 20
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in fns}
        for _ in range(a.iters):
            for name, fn in fns.items():
                times[name].append(once_us(fn, calls))
        dist, idx = fns["nearest_rows"]()
        d1, i1 = fns["splits_1"]()
        td, ti = fns["cdist_topk"]()
        med = statistics.median(times["nearest_rows"])
        run = {"nq": nq, "nr": nr, "e": e, "calls_per_sample": calls, "splits": _lib.lib.clipmi_nearest_rows_splits(nq, nr),
               "workgroups": _lib.lib.clipmi_nearest_rows_splits(nq, nr) * ((nq + 15) // 16),
               **{name + "_us": stats(ts) for name, ts in times.items()},
               "tflops_fp32": 3.0 * nq * nr * e / med / 1e6, "refs_read_gb_per_s": 4.0 * nr * e / med / 1e3,
               "same_bits_as_splits_1": bool(torch.equal(dist.view(torch.int32), d1.view(torch.int32)) and torch.equal(idx, i1)),
               "max_abs_difference_to_knn_dists": float((dist - fns["knn_dists"]()).abs().max()),
               "index_agreement_with_cdist_topk": float((idx.long() == ti).float().mean())}
        for name in ("splits_1", "knn_dists", "cdist_topk"):
            run[name + "_over_nearest_rows"] = statistics.median(times[name]) / med
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
        del refs, q, dist, idx, d1, i1, td, ti
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
