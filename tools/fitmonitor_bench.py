"""Time of one validation of a CoOp fit on the device (``CoOpFitState.validate``: training forward, cosine logits, ``clipmi_val_score``,
``clipmi_best_select``), of the two new entry points alone, of a CoOp step of the same state, and of the same scoring done with torch on
the same GPU with the read-back a Python loop over epochs needs.  Measurement only; bench.py does not run it.

ViT-B/16 text geometry with synthetic weights, n_ctx 16, the live-row cut on, batch 32; N_val = 5 000 and 50 000 cached validation
features against C = 100 and 1 000 classes.  A sample is the time between two device events around --window consecutive calls, divided
by the window (the torch scoring ends in ``.item()``, so its sample is host time around one call); everything of one (N_val, C) takes
turns sample by sample in the same process, --iters samples each after --warmup; the figure is the median, the run's own spread is
beside it.  ``share_of_epoch``: one validation over the steps of an epoch of the reference's length, 16 shots x C / batch 32.

Usage: python tools/fitmonitor_bench.py [--iters 5] [--warmup 2] [--out profiles/fitmonitor_bench.json]"""
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
from clip_calibration_amd import coopfit, ops, synthetic as syn  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

GEOM, N_CTX, BATCH, SHOTS, BINS = "ViT-B/16", 16, 32, 16, 10


def prompt_ids(C, seed=0):
    """[SOT, X * 16, 1 .. 7 name tokens, '.', EOT, 0 ..]: the last EOT sits at token 25 of 77, as for "X .. X <name>." prompts."""
    g = syn.GEOMETRIES[GEOM]
    rng = np.random.RandomState(seed)
    ids = np.zeros((C, g.context_length), np.int64)
    for c in range(C):
        k = 1 + c % 7
        ids[c, 0] = g.vocab_size - 2
        ids[c, 1:1 + N_CTX] = 1
        ids[c, 1 + N_CTX:1 + N_CTX + k] = rng.randint(3, g.vocab_size - 2, size=k)
        ids[c, 1 + N_CTX + k] = 2
        ids[c, 2 + N_CTX + k] = g.vocab_size - 1
    return torch.from_numpy(ids)


def window_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def host_ms(fn, n):
    """Host time of a call that ends in a read-back."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def summary(samples):
    med = statistics.median(samples)
    return {"median_ms": med, "min_ms": min(samples), "max_ms": max(samples), "spread": (max(samples) - min(samples)) / med}


def alternate(calls, iters, warmup):
    """{name: summary}: ``calls`` maps a name to (fn, window, timer); every round takes one sample of each."""
    samples = {name: [] for name in calls}
    for k in range(warmup + iters):
        for name, (fn, window, timer) in calls.items():
            ms = timer(fn, window)
            if k >= warmup:
                samples[name].append(ms)
    return {name: summary(s) for name, s in samples.items()}


def torch_scoring(img_n, txt, scale, labels):
    """What a Python loop does behind an epoch: matmul, cross-entropy, arg-max, a histogram of the confidences, and the read-back."""
    txt_n = txt / txt.norm(dim=1, keepdim=True)
    z = scale * img_n @ txt_n.t()
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
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--kernel-window", type=int, default=50)
    ap.add_argument("--classes", type=int, nargs="*", default=[100, 1000])
    ap.add_argument("--rows", type=int, nargs="*", default=[5000, 50000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    model = build_model(dict(syn.synthetic_state_dict(GEOM, seed=0)), {"trainer": "CoOp"}).cuda()
    g = torch.Generator().manual_seed(1)
    geom = syn.GEOMETRIES[GEOM]
    ctx = 0.02 * torch.randn(N_CTX, geom.transformer_width, generator=g)
    feats = torch.randn(BATCH, geom.embed_dim, generator=g).cuda()
    lr = torch.full((1,), 0.002, device="cuda")
    out = {"geometry": GEOM, "batch": BATCH, "n_ctx": N_CTX, "val_bins": BINS, "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "window": a.window, "kernel_window": a.kernel_window, "cases": []}
    for C in a.classes:
        ids = prompt_ids(C)
        labels = torch.randint(0, C, (BATCH,), generator=g).cuda()
        for N in a.rows:
            st = coopfit.CoOpFitState(model, ids, ctx)
            st.start_monitor(4, BINS, select=True)
            vf = torch.randn(N, geom.embed_dim, generator=g).cuda()
            vl = torch.randint(0, C, (N,), generator=g).cuda()
            st.validate(vf, vl, 0)
            st.step(feats, labels, lr)
            torch.cuda.synchronize()
            mon = st._mon
            rec, img_n = mon.records[1], mon.val[1]
            text = st.tower.text
            calls = {
                "validate": (lambda: st.validate(vf, vl, 1), a.window, window_ms),
                "step": (lambda: st.step(feats, labels, lr), a.window, window_ms),
                "val_score": (lambda: ops.val_score(mon.logits, vl, BINS, rec, mon.score_ws), a.kernel_window, window_ms),
                "best_select": (lambda: ops.best_select(rec, mon.block, "accuracy", 1, st.ctx, mon.best, mon.select_ws), a.kernel_window, window_ms),
                "torch_scoring_with_readback": (lambda: torch_scoring(img_n, text, st.scale, vl), 1, host_ms),
            }
            res = alternate(calls, a.iters, a.warmup)
            steps_per_epoch = -(-SHOTS * C // BATCH)
            r = {"classes": C, "val_rows": N, "times": res, "logits_bytes": 4 * N * C, "steps_per_reference_epoch": steps_per_epoch,
                 "validate_share_of_epoch": res["validate"]["median_ms"] / (steps_per_epoch * res["step"]["median_ms"]),
                 "validate_over_step": res["validate"]["median_ms"] / res["step"]["median_ms"],
                 "torch_scoring_over_val_score": res["torch_scoring_with_readback"]["median_ms"] / res["val_score"]["median_ms"]}
            out["cases"].append(r)
            print(json.dumps(r))
            del st, vf, vl, mon, rec, img_n, text, calls
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
