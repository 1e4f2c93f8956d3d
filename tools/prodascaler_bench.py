"""Time of one ProDA training step under the dynamic loss scale (``grad_scale="dynamic"``, clipmi_proda_ctx_step_scaled) against the static
step of the same run.  Measurement only; bench.py does not run it.

The first shape of tools/prodafit_bench.py: ViT-B/16 text geometry with synthetic weights, batch 32 of cached image features, n_ctx 16, 32
contexts in slices of 4, C = 100 classes, the live-row cut on (N = 432 prompts per step), one fixed selection.  For each route (separate
calls, one call) a static and a dynamic state are stepped ALTERNATELY -- static, dynamic, static, ... -- so that clocks and caches treat
both alike; every step lies between two device events; the figures are the median, minimum and maximum of --iters steps of each after
--warmup untimed pairs.  The static step of the same run is the yardstick.  The dynamic state starts at the static scale with a growth
interval no run reaches, so both do the same arithmetic; the dynamic one adds the launch that multiplies d_text by the scale, the decision
launch, and a step launch that reads the gradient back from the workspace.  The scaler's block is read once, after the last step.

Usage: python tools/prodascaler_bench.py [--iters 5] [--warmup 2] [--out profiles/prodascaler_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clip_calibration_amd import prodafit, synthetic as syn  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
import coopfit_bench as cb  # noqa: E402
import prodafit_bench as pb  # noqa: E402

CLASSES = 100


def summary(ms):
    return {"step_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def alternate(states, step, iters, warmup):
    """{name: [ms]}: the states stepped in turn, `warmup` untimed rounds and then `iters` timed ones."""
    ms = {name: [] for name in states}
    for k in range(warmup + iters):
        for name, st in states.items():
            a, b = cb.events(2)
            a.record()
            step(st)
            b.record()
            torch.cuda.synchronize()
            if k >= warmup:
                ms[name].append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    model = build_model(dict(syn.synthetic_state_dict(pb.GEOM, seed=0)), {"trainer": "CoOp"}).cuda()
    g = torch.Generator().manual_seed(1)
    E, D = syn.GEOMETRIES[pb.GEOM].embed_dim, syn.GEOMETRIES[pb.GEOM].transformer_width
    feats = torch.randn(pb.BATCH, E, generator=g).cuda()
    labels = torch.randint(0, CLASSES, (pb.BATCH,), generator=g).cuda()
    ids = pb.prompt_ids(CLASSES, pb.N_CTX)
    ctx = 0.02 * torch.randn(pb.N_PROMPT, pb.N_CTX, D, generator=g)
    lr = torch.full((1,), 0.002, device="cuda")
    sel = torch.from_numpy(prodafit.reference_order(pb.SEL, prodafit.positions(pb.N_PROMPT))).cuda()
    out = {"geometry": pb.GEOM, "batch": pb.BATCH, "n_ctx": pb.N_CTX, "n_prompt": pb.N_PROMPT, "prompt_bs": pb.PROMPT_BS, "classes": CLASSES,
           "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "steps": []}
    for one_call in (False, True):
        states = {"static": prodafit.ProDAFitState(model, ids, ctx, prompt_bs=pb.PROMPT_BS, alpha=pb.ALPHA, grad_scale=prodafit.DEFAULT_GRAD_SCALE),
                  "dynamic": prodafit.ProDAFitState(model, ids, ctx, prompt_bs=pb.PROMPT_BS, alpha=pb.ALPHA, grad_scale="dynamic",
                                                    scaler={"init_scale": prodafit.DEFAULT_GRAD_SCALE, "growth_interval": 1 << 20})}
        ms = alternate(states, lambda st: st.step(feats, labels, lr, sel=sel, one_call=one_call), a.iters, a.warmup)
        r = {name: summary(v) for name, v in ms.items()}
        spread = max(r[n]["max_ms"] - r[n]["min_ms"] for n in r)
        diff = r["dynamic"]["step_ms"] - r["static"]["step_ms"]
        rec = dict(one_call=one_call, prompts=states["static"].tower.N, token_rows_per_prompt=states["static"].tower.L, static=r["static"],
                   dynamic=r["dynamic"], dynamic_minus_static_ms=diff, largest_min_to_max_spread_ms=spread, difference_inside_the_spread=abs(diff) <= spread,
                   scaler_state=states["dynamic"].scaler_state(),
                   same_bits=bool(states["dynamic"].ctx.view(torch.int32).equal(states["static"].ctx.view(torch.int32))))
        out["steps"].append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
