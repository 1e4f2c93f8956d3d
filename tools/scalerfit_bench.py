"""What the dynamic loss scale costs per training step on the device (clip_calibration_amd.coopfit ``grad_scale="dynamic"``,
csrc/grad_scaler.hip) against the static scale's step.  Measurement only; bench.py does not run it.

ViT-B/16 text geometry with synthetic weights, batch 32 of cached image features, n_ctx 16, C = 100 and C = 1000 classes, the live-row
cut on.  Four states on the same model and the same batch -- static and dynamic, each through the separate calls and through the one-call
entry -- take one step each in turn (alternating, so that a drift of the machine reaches all four alike), every step between two device
events with a synchronisation behind it; the median of --iters rounds after --warmup untimed ones.  The dynamic state starts at 2^12,
the static default, with a growth interval beyond the run: both paths do the same arithmetic and no step is skipped.  The tail of a step
-- clipmi_ctx_step against clipmi_grad_scale_rows + clipmi_ctx_step_scaled, the launches the option adds or replaces -- is timed
between events of its own.

Usage: python tools/scalerfit_bench.py [--iters 5] [--warmup 2] [--classes 100 1000] [--out profiles/scalerfit_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clip_calibration_amd import coopfit, ops, synthetic as syn  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
import coopfit_bench as cb  # noqa: E402

GEOM, N_CTX, BATCH = cb.GEOM, cb.N_CTX, cb.BATCH
SCALER = {"init_scale": coopfit.DEFAULT_GRAD_SCALE, "growth_interval": 1 << 20}
WAYS = [("static", False), ("dynamic", False), ("static", True), ("dynamic", True)]


def time_steps(model, ids, ctx, feats, labels, iters, warmup):
    states = {}
    for kind, one_call in WAYS:
        kw = {"grad_scale": "dynamic", "scaler": SCALER} if kind == "dynamic" else {}
        states[kind, one_call] = coopfit.CoOpFitState(model, ids, ctx, **kw)
    lr = torch.full((1,), 0.002, device="cuda")
    ms = {w: [] for w in states}
    for k in range(warmup + iters):
        for w, st in states.items():
            a, b = cb.events(2)
            a.record()
            st.step(feats, labels, lr, one_call=w[1])
            b.record()
            torch.cuda.synchronize()
            if k >= warmup:
                ms[w].append(a.elapsed_time(b))
    same = torch.equal(states["static", False].ctx, states["dynamic", False].ctx) and torch.equal(states["static", True].ctx, states["dynamic", True].ctx)
    # the launches the option adds or replaces, on the gradients the last step left
    st_s, st_d = states["static", False], states["dynamic", False]
    t = st_d.tower
    d_text = torch.randn(t.C, t.E, device="cuda")
    tails = {"static": [], "dynamic": []}
    sgd = (st_d.momentum, st_d.dampening, st_d.weight_decay, st_d.nesterov)
    for k in range(warmup + iters):
        e = cb.events(4)
        e[0].record()
        ops.ctx_step(st_s.tower.d_embed, t.C, t.n_ctx, t.per_class, st_s.grad_scale, st_s.ctx, st_s.buf, lr, False, *sgd, want_grad=False)
        e[1].record()
        torch.cuda.synchronize()
        e[2].record()
        ops.grad_scale_rows(d_text, st_d._scaler.block)
        ops.ctx_step_scaled(t.d_embed, t.C, t.n_ctx, t.per_class, st_d._scaler.block, st_d.ctx, st_d.buf, lr, 2.0, 0.5, SCALER["growth_interval"], *sgd,
                            want_grad=False, workspace=st_d._scaler.ws)
        e[3].record()
        torch.cuda.synchronize()
        if k >= warmup:
            tails["static"].append(e[0].elapsed_time(e[1]))
            tails["dynamic"].append(e[2].elapsed_time(e[3]))
    state = st_d.scaler_state()
    out = {"token_rows_per_prompt": t.L, "same_bits_as_static": bool(same), "skipped_steps": state["skipped_steps"]}
    for (kind, one_call), v in ms.items():
        out[f"{kind}_{'one_call' if one_call else 'separate'}_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    for one_call in (False, True):
        s, d = statistics.median(ms["static", one_call]), statistics.median(ms["dynamic", one_call])
        out[f"dynamic_over_static_{'one_call' if one_call else 'separate'}"] = d / s
    out["tail_static_ms"] = statistics.median(tails["static"])
    out["tail_dynamic_ms"] = statistics.median(tails["dynamic"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--classes", type=int, nargs="*", default=[100, 1000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    model = build_model(dict(syn.synthetic_state_dict(GEOM, seed=0)), {"trainer": "CoOp"}).cuda()
    g = torch.Generator().manual_seed(1)
    E, D = syn.GEOMETRIES[GEOM].embed_dim, syn.GEOMETRIES[GEOM].transformer_width
    feats = torch.randn(BATCH, E, generator=g).cuda()
    out = {"geometry": GEOM, "batch": BATCH, "n_ctx": N_CTX, "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup,
           "scaler": SCALER, "steps": []}
    for C in a.classes:
        labels = torch.randint(0, C, (BATCH,), generator=g).cuda()
        ctx = 0.02 * torch.randn(N_CTX, D, generator=g)
        r = dict(classes=C, **time_steps(model, cb.prompt_ids(C), ctx, feats, labels, a.iters, a.warmup))
        out["steps"].append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
