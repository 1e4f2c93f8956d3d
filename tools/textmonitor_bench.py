"""Cost of per-epoch validation in the CoCoOp and ProDA fits (``CoCoOpFitState`` / ``ProDAFitState.validate``), and of the two fused
validation kernels alone.  Measurement only; bench.py does not run it.

ViT-B/16 text geometry with synthetic weights, 100 classes, each fit at the first shape of its own bench tool (CoCoOp: n_ctx 4, batch 1;
ProDA: n_ctx 16, 32 contexts in slices of 4, batch 32).  A sample is the time between two device events around --steps training steps
(unmonitored) or around the same steps followed by one validation of N_val cached image features (monitored); the two take turns sample
by sample in one process, --iters samples each after --warmup, and the figure is the median.  The cost of a validation is the difference of
the medians; the run's own min-to-max spread of either side is printed beside it -- a difference inside that spread is not a difference.
N_val = 50 and 500 for CoCoOp (a validation runs N_val x C prompts through the text tower by construction), 500 and 5 000 for ProDA
(C x n_prompt prompts whatever N_val).  The kernels alone: ``ops.cocoop_val_rows`` on one chunk of --val-batch images and
``ops.proda_val_mean`` on all C x n_prompt rows, 20 launches per sample.  No threshold is set here.

Usage: python tools/textmonitor_bench.py [--iters 5] [--warmup 2] [--steps 4] [--out profiles/textmonitor_bench.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clip_calibration_amd import cocoopfit, ops, prodafit, synthetic as syn  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
from blockmonitor_bench import alternate  # noqa: E402
from cocoopfit_bench import N_CTX as COCOOP_N_CTX, params_for  # noqa: E402
from prodafit_bench import BATCH as PRODA_BATCH, GEOM, N_CTX as PRODA_N_CTX, N_PROMPT, PROMPT_BS, prompt_ids  # noqa: E402

CLASSES, BINS = 100, 10


def fit_rows(name, st, feats, labels, rows, steps, iters, warmup, gen, E, validate):
    lr = torch.full((1,), 0.002, device="cuda")
    out = []
    for N in rows:
        vf = torch.randn(N, E, generator=gen).cuda()
        vl = torch.randint(0, CLASSES, (N,), generator=gen).cuda()
        st.start_monitor(1, BINS, True, "accuracy")

        def plain():
            for _ in range(steps):
                st.step(feats, labels, lr)

        def monitored():
            plain()
            validate(st, vf, vl)

        res = alternate({"unmonitored": plain, "monitored": monitored}, iters, warmup)
        row = {"fit": name, "n_val": N, **res, "validation_ms": res["monitored"]["median_ms"] - res["unmonitored"]["median_ms"],
               "step_ms": res["unmonitored"]["median_ms"] / steps}
        row["validation_in_steps"] = row["validation_ms"] / row["step_ms"]
        out.append(row)
        print(f"{name} N_val={N}: {steps} steps {res['unmonitored']['median_ms']:.2f} ms (spread {res['unmonitored']['spread_ms']:.2f}), with one "
              f"validation {res['monitored']['median_ms']:.2f} ms (spread {res['monitored']['spread_ms']:.2f}): validation "
              f"{row['validation_ms']:.2f} ms = {row['validation_in_steps']:.1f} steps")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--val-batch", type=int, default=10, help="CoCoOp: images per validation chunk (x 100 classes = prompts per tower call)")
    ap.add_argument("--cocoop-rows", type=int, nargs="*", default=[50, 500])
    ap.add_argument("--proda-rows", type=int, nargs="*", default=[500, 5000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    gen = torch.Generator().manual_seed(1)
    g = syn.GEOMETRIES[GEOM]
    E = g.embed_dim
    model = build_model(dict(syn.synthetic_state_dict(GEOM, seed=0)), {"trainer": "CoOp"}).cuda()
    out = {"geometry": GEOM, "classes": CLASSES, "steps_per_sample": a.steps, "val_bins": BINS, "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "warmup": a.warmup, "cocoop": {"n_ctx": COCOOP_N_CTX, "batch": 1, "val_batch_size": a.val_batch},
           "proda": {"n_ctx": PRODA_N_CTX, "n_prompt": N_PROMPT, "prompt_bs": PROMPT_BS, "batch": PRODA_BATCH, "val_class_chunk": max(1, 4096 // N_PROMPT)},
           "fits": [], "kernels": []}

    feats = torch.randn(1, E, generator=gen).cuda()
    labels = torch.randint(0, CLASSES, (1,), generator=gen).cuda()
    st = cocoopfit.CoCoOpFitState(model, prompt_ids(CLASSES, COCOOP_N_CTX), params_for(model, feats))
    out["fits"] += fit_rows("cocoop", st, feats, labels, a.cocoop_rows, a.steps, a.iters, a.warmup, gen, E,
                            lambda s, vf, vl: s.validate(vf, vl, 0, a.val_batch))
    del st
    feats = torch.randn(PRODA_BATCH, E, generator=gen).cuda()
    labels = torch.randint(0, CLASSES, (PRODA_BATCH,), generator=gen).cuda()
    st = prodafit.ProDAFitState(model, prompt_ids(CLASSES, PRODA_N_CTX), prodafit.init_context(model, PRODA_N_CTX, N_PROMPT), prompt_bs=PROMPT_BS)
    out["fits"] += fit_rows("proda", st, feats, labels, a.proda_rows, a.steps, a.iters, a.warmup, gen, E, lambda s, vf, vl: s.validate(vf, vl, 0))
    del st

    # the two fused kernels alone
    img = torch.nn.functional.normalize(torch.randn(a.val_batch, E, generator=gen), dim=1).cuda()
    txt = torch.randn(a.val_batch, CLASSES, E, generator=gen).cuda()
    vl = torch.randint(0, CLASSES, (a.val_batch,), generator=gen).cuda()
    rows = ops.new_val_row_results(a.val_batch, "cuda")
    text = torch.randn(CLASSES * N_PROMPT, E, generator=gen).cuda()

    def fused_rows():
        for _ in range(20):
            ops.cocoop_val_rows(img, txt, 100.0, vl, BINS, rows, 0)

    def two_calls():
        for _ in range(20):
            ops.val_score_rows(ops.logits_per_image(img, txt, 100.0, want_conf_pred=False, want_last_text=False)[0], vl, BINS, rows, 0)

    def fused_mean():
        for _ in range(20):
            ops.proda_val_mean(text, N_PROMPT)

    def two_means():
        for _ in range(20):
            ops.group_mean(ops.l2_normalize(text), N_PROMPT)

    res = alternate({"cocoop_val_rows": fused_rows, "logits_per_image_then_val_score_rows": two_calls, "proda_val_mean": fused_mean,
                     "l2_normalize_then_group_mean": two_means}, a.iters, a.warmup)
    res = {k: {kk: vv / 20 for kk, vv in v.items()} for k, v in res.items()}
    out["kernels"] = {"cocoop_rows": {"images": a.val_batch, "classes": CLASSES}, "proda_mean": {"classes": CLASSES, "n_prompt": N_PROMPT}, **res}
    for k, v in res.items():
        print(f"{k}: {v['median_ms'] * 1e3:.1f} us per call (spread {v['spread_ms'] * 1e3:.1f} us; host-enqueued, 20 calls per sample)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"textmonitor_bench": "done", "cocoop_rows": a.cocoop_rows, "proda_rows": a.proda_rows}))


if __name__ == "__main__":
    main()
