"""Cost of per-epoch validation in the image-tower fits (``VPTFitState`` / ``MaPLeFitState`` / ``PromptSRCFitState.validate``), and of
the row-chunked score (``clipmi_val_score_rows`` + ``clipmi_val_score_finish``) against ``clipmi_val_score`` on the same logits.
Measurement only; bench.py does not run it.

Each fit runs at the first shape of its own bench tool (ViT-B/16 with synthetic weights, 100 classes, batch 4; VPT n_ctx 8 depth 12,
MaPLe n_ctx 2 depth 9, PromptSRC n_ctx 4 depth 9).  A sample is the time between two device events around --steps training steps
(unmonitored) or around the same steps followed by one validation of N_val images in chunks of --val-batch (monitored); the two take
turns sample by sample in one process, --iters samples each after --warmup, and the figure is the median.  The cost per validated epoch
is the difference of the medians; the run's own min-to-max spread of either side is printed beside it -- a difference inside that spread
is not a difference.  N_val = 400 and 1 600 (4 and 16 shots x 100 classes).  No threshold is set here.

Usage: python tools/blockmonitor_bench.py [--iters 5] [--warmup 2] [--steps 8] [--out profiles/blockmonitor_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clip_calibration_amd import maplefit, ops, promptsrcfit, synthetic as syn, vptfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

GEOM, CLASSES, BATCH, BINS = "ViT-B/16", 100, 4, 10


def window_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summary(samples):
    med = statistics.median(samples)
    return {"median_ms": med, "min_ms": min(samples), "max_ms": max(samples), "spread_ms": max(samples) - min(samples)}


def alternate(calls, iters, warmup):
    samples = {name: [] for name in calls}
    for k in range(warmup + iters):
        for name, fn in calls.items():
            ms = window_ms(fn)
            if k >= warmup:
                samples[name].append(ms)
    return {name: summary(s) for name, s in samples.items()}


def states(sd, gen):
    g = syn.GEOMETRIES[GEOM]
    ids = syn.synthetic_token_ids(CLASSES, GEOM, seed=0)
    out = {}
    m = build_model(dict(sd), {"trainer": "VPT", "vision_depth": 12, "vision_ctx": 8, "language_depth": 0, "language_ctx": 0}).cuda()
    out["vpt"] = vptfit.VPTFitState(m, torch.randn(CLASSES, g.embed_dim, generator=gen).cuda())
    m = build_model(dict(sd), {"trainer": "MaPLe", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0, "maple_length": 2}).cuda()
    out["maple"] = maplefit.MaPLeFitState(m, ids, maplefit.init_learner_params(m, 2, 9))
    m = build_model(dict(sd), {"trainer": "IVLP", "vision_depth": 9, "language_depth": 9, "vision_ctx": 4, "language_ctx": 4}).cuda()
    out["promptsrc"] = promptsrcfit.PromptSRCFitState(m, ids, promptsrcfit.init_params(m), torch.randn(CLASSES, g.embed_dim, generator=gen).cuda())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--val-batch", type=int, default=32)
    ap.add_argument("--rows", type=int, nargs="*", default=[400, 1600])
    ap.add_argument("--fits", nargs="*", default=["vpt", "maple", "promptsrc"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    gen = torch.Generator().manual_seed(1)
    R = syn.GEOMETRIES[GEOM].image_resolution
    images = torch.randn(BATCH, 3, R, R, generator=gen).half().cuda()
    labels = torch.randint(0, CLASSES, (BATCH,), generator=gen).cuda()
    lr = torch.full((1,), 0.002, device="cuda")
    out = {"geometry": GEOM, "classes": CLASSES, "batch": BATCH, "steps_per_sample": a.steps, "val_batch_size": a.val_batch, "val_bins": BINS,
           "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "fits": [], "score": []}
    sts = states(syn.synthetic_state_dict(GEOM, seed=0), gen)
    for N in a.rows:
        vi = torch.randn(N, 3, R, R, generator=gen).half().cuda()
        vl = torch.randint(0, CLASSES, (N,), generator=gen).cuda()
        for name in a.fits:
            st = sts[name]
            st.start_monitor(1, BINS, "accuracy", select=True)

            def plain():
                for _ in range(a.steps):
                    st.step(images, labels, lr)

            def monitored():
                plain()
                st.validate(vi, vl, 0, a.val_batch)

            res = alternate({"unmonitored": plain, "monitored": monitored}, a.iters, a.warmup)
            row = {"fit": name, "n_val": N, **{k: v for k, v in res.items()},
                   "validation_ms": res["monitored"]["median_ms"] - res["unmonitored"]["median_ms"],
                   "step_ms": res["unmonitored"]["median_ms"] / a.steps}
            row["validation_in_steps"] = row["validation_ms"] / row["step_ms"]
            out["fits"].append(row)
            print(f"{name} N_val={N}: {a.steps} steps {res['unmonitored']['median_ms']:.2f} ms (spread {res['unmonitored']['spread_ms']:.2f}), with one "
                  f"validation {res['monitored']['median_ms']:.2f} ms (spread {res['monitored']['spread_ms']:.2f}): validation "
                  f"{row['validation_ms']:.2f} ms = {row['validation_in_steps']:.1f} steps")
        # the score alone, on the same logits
        z = 100.0 * torch.randn(N, CLASSES, generator=gen).cuda()
        rec, rows = ops.new_val_records(1, BINS, "cuda")[0], ops.new_val_row_results(N, "cuda")
        ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        chunks = [(lo, min(lo + a.val_batch, N)) for lo in range(0, N, a.val_batch)]

        def whole():
            for _ in range(20):
                ops.val_score(z, vl, BINS, rec, ws)

        def chunked():
            for _ in range(20):
                for lo, hi in chunks:
                    ops.val_score_rows(z[lo:hi], vl[lo:hi], BINS, rows, lo)
                ops.val_score_finish(rows, BINS, rec, ws)

        def one_chunk():
            for _ in range(20):
                ops.val_score_rows(z, vl, BINS, rows, 0)
                ops.val_score_finish(rows, BINS, rec, ws)

        res = alternate({"val_score": whole, "rows_and_finish_chunked": chunked, "rows_and_finish_one_chunk": one_chunk}, a.iters, a.warmup)
        res = {k: {kk: vv / 20 for kk, vv in v.items()} for k, v in res.items()}
        out["score"].append({"n_val": N, "classes": CLASSES, "chunks": len(chunks), **res})
        print(f"score N_val={N}: val_score {res['val_score']['median_ms'] * 1e3:.1f} us, rows + finish in {len(chunks)} chunks "
              f"{res['rows_and_finish_chunked']['median_ms'] * 1e3:.1f} us, in one chunk {res['rows_and_finish_one_chunk']['median_ms'] * 1e3:.1f} us "
              f"(spreads {res['val_score']['spread_ms'] * 1e3:.1f} / {res['rows_and_finish_chunked']['spread_ms'] * 1e3:.1f} / "
              f"{res['rows_and_finish_one_chunk']['spread_ms'] * 1e3:.1f} us)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"blockmonitor_bench": "done", "rows": a.rows}))


if __name__ == "__main__":
    main()
