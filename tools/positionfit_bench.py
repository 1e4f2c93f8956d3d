"""Time of one CoOp training step on the device with the class token at the end, in the middle and at the front
(clip_calibration_amd.coopfit with ``class_token_position=``, csrc/prompt_position.hip), and of the two copy kernels alone.  Measurement
only; bench.py does not run it.

ViT-B/16 text geometry with synthetic weights, batch 32 of cached image features, n_ctx 16, the live-row cut on, C = 100 and C = 1000
classes.  A sample is the time between two device events around --window consecutive ``CoOpFitState.step`` calls, divided by the window;
the three positions take turns sample by sample (end, middle, front, end, ..) in the same process, --iters samples each after --warmup;
the figure is the median, and the run's own spread (min and max) is reported beside it.  ``ops.prompt_place`` and ``ops.prompt_unplace``
alone at the step's shapes: the same with a window of --kernel-window launches.  ``end`` is the route of tools/coopfit_bench.py: the
output repeats that file's figure for the same shape when --compare names it.

Usage: python tools/positionfit_bench.py [--iters 5] [--warmup 2] [--window 10] [--compare profiles/coopfit_bench.json]
                                         [--out profiles/positionfit_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clip_calibration_amd import coopfit, ops, synthetic as syn  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

GEOM, N_CTX, BATCH = "ViT-B/16", 16, 32
POSITIONS = ("end", "middle", "front")


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
    """Per-call time of n consecutive calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def summary(samples):
    med = statistics.median(samples)
    return {"median_ms": med, "min_ms": min(samples), "max_ms": max(samples), "spread": (max(samples) - min(samples)) / med}


def alternate(calls, iters, warmup, window):
    """{name: summary} of the calls timed in turn: every round takes one sample of each, the first --warmup rounds are dropped."""
    samples = {name: [] for name in calls}
    for k in range(warmup + iters):
        for name, fn in calls.items():
            ms = window_ms(fn, window)
            if k >= warmup:
                samples[name].append(ms)
    return {name: summary(s) for name, s in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--kernel-window", type=int, default=200)
    ap.add_argument("--classes", type=int, nargs="*", default=[100, 1000])
    ap.add_argument("--compare", default=None, help="a coopfit_bench.json whose end-route figures are repeated beside this run's")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    model = build_model(dict(syn.synthetic_state_dict(GEOM, seed=0)), {"trainer": "CoOp"}).cuda()
    g = torch.Generator().manual_seed(1)
    geom = syn.GEOMETRIES[GEOM]
    ctx = 0.02 * torch.randn(N_CTX, geom.transformer_width, generator=g)
    feats = torch.randn(BATCH, geom.embed_dim, generator=g).cuda()
    lr = torch.full((1,), 0.002, device="cuda")
    earlier = {}
    if a.compare:
        with open(a.compare) as f:
            earlier = {r["classes"]: r["step_ms"] for r in json.load(f)["steps"] if r.get("live_row_cut") is True}
    out = {"geometry": GEOM, "batch": BATCH, "n_ctx": N_CTX, "device": torch.cuda.get_device_name(0), "iters": a.iters, "window": a.window,
           "kernel_window": a.kernel_window, "classes": []}
    for C in a.classes:
        ids = prompt_ids(C)
        labels = torch.randint(0, C, (BATCH,), generator=g).cuda()
        states = {p: coopfit.CoOpFitState(model, ids, ctx, class_token_position=p) for p in POSITIONS}
        steps = alternate({p: (lambda st=st: st.step(feats, labels, lr)) for p, st in states.items()}, a.iters, a.warmup, a.window)
        t = states["middle"].tower
        d_embed = torch.randn(t.C * t.L, t.D, device="cuda")
        kernels = alternate({"place": lambda: ops.prompt_place(t.base, states["middle"].ctx, "middle", t.name_lens, t.rows, t.prompts),
                             "unplace": lambda: ops.prompt_unplace(d_embed, "middle", t.name_lens, t.n_ctx, t.compact)}, a.iters, a.warmup, a.kernel_window)
        end = steps["end"]["median_ms"]
        copies = kernels["place"]["median_ms"] + kernels["unplace"]["median_ms"]
        r = {"classes": C, "token_rows_per_prompt": t.L, "step": steps, "kernels": kernels,
             "place_bytes": t.C * t.L * t.D * (4 + t.base.element_size()), "unplace_bytes": 2 * t.C * (1 + t.n_ctx) * t.D * 4,
             "copies_share_of_end_step": copies / end, "middle_over_end": steps["middle"]["median_ms"] / end,
             "front_over_end": steps["front"]["median_ms"] / end}
        if C in earlier:
            r["end_step_ms_in_compare_file"] = earlier[C]
            r["end_over_compare_file"] = end / earlier[C]
        out["classes"].append(r)
        print(json.dumps(r))
        del states
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
