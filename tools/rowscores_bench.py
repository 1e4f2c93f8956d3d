"""Times ops.row_scores + ops.row_scores_finish (csrc/row_scores.hip) at test-split sizes against (a) the same scoring written in torch on
the same GPU, read-back included, and (b) the time a copy kernel needs for the bytes the scoring must read, at the copy bandwidth measured in
the same run:  python tools/rowscores_bench.py [out.json]  (a GPU is required).  profiles/rowscores_bench.json is this tool's output.
Every timing is a host clock around work that ends in the read-back of the result, median of 5 after 2 warm-up runs, with the spread."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clip_calibration_amd import ops  # noqa: E402

N_BINS, C, REPEATS, WARMUP = 10, 1000, 5, 2


def timed(fn):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                   # ends in a read-back: synchronises
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}


def hip_scores(rows, labels, from_probs):
    row_out, acc = ops.row_scores(rows, labels, from_probs=from_probs, n_bins=N_BINS)
    return ops.row_scores_finish(row_out, acc)


def torch_scores(rows, labels, from_probs):
    """The same three numbers with torch ops: float64 bin sums by bincount, one read-back."""
    N, Cn = rows.shape
    if from_probs:
        p = rows
        nll = -torch.log(p.gather(1, labels[:, None]).clamp_min(torch.finfo(torch.float32).tiny)).squeeze(1)
    else:
        lp = torch.log_softmax(rows, dim=1)
        p = lp.exp()
        nll = -lp.gather(1, labels[:, None]).squeeze(1)
    onehot = torch.zeros_like(p).scatter_(1, labels[:, None], 1.0)
    brier = ((p - onehot) ** 2).sum(dim=1)
    edges = torch.linspace(0, 1, N_BINS + 1, dtype=torch.float64, device=rows.device)
    b = (torch.bucketize(p.double(), edges, right=True) - 1).clamp_(0, N_BINS - 1)       # p == 1.0 into the last interval
    cell = (torch.arange(Cn, device=rows.device)[None, :] * N_BINS + b).reshape(-1)
    conf = torch.bincount(cell, weights=p.double().reshape(-1), minlength=Cn * N_BINS)
    hits = torch.bincount(cell.reshape(N, Cn).gather(1, labels[:, None]).squeeze(1), minlength=Cn * N_BINS).double()
    out = torch.stack([nll.double().mean(), brier.double().mean(), (hits - conf).abs().sum() / N / Cn])
    o = out.cpu().numpy()
    return {"nll": float(o[0]), "brier": float(o[1]), "cw_ece": float(o[2]), "n": N}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rowscores_bench.json")
    assert torch.cuda.is_available(), "rowscores_bench needs a GPU"
    torch.manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "n_bins": N_BINS, "classes": C, "repeats": REPEATS, "warmup": WARMUP, "cases": []}
    for N in (25000, 50000):
        logits = (2.5 * torch.randn(N, C, device="cuda")).contiguous()
        labels = torch.randint(0, C, (N,), device="cuda")
        probs = torch.softmax(logits, dim=1)
        dst = torch.empty_like(logits)
        copy = timed(lambda: (dst.copy_(logits), torch.cuda.synchronize()))
        nbytes = logits.numel() * 4
        copy_gbs = 2 * nbytes / (copy["median_ms"] * 1e-3) / 1e9       # a copy reads and writes every byte
        for kind, rows, fp in (("logits", logits, False), ("probs", probs, True)):
            hip = timed(lambda: hip_scores(rows, labels, fp))
            ref = timed(lambda: torch_scores(rows, labels, fp))
            a, b = hip_scores(rows, labels, fp), torch_scores(rows, labels, fp)
            floor_ms = nbytes / (copy_gbs * 1e9) * 1e3                 # the rows read once at the measured copy bandwidth
            case = {"rows": N, "kind": kind, "input_bytes": nbytes, "hip": hip, "torch": ref, "copy": copy, "copy_gb_per_s": copy_gbs,
                    "read_once_floor_ms": floor_ms, "hip_over_floor": hip["median_ms"] / floor_ms,
                    "torch_over_hip": ref["median_ms"] / hip["median_ms"],
                    "hip_result": a, "torch_result": b}
            print(json.dumps(case))
            result["cases"].append(case)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
