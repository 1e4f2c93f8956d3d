"""What an Adam step costs per training step of a prompt fit (``optimizer="adam"``, csrc/optim_step.hip clipmi_block_step_adam) against
the fit's SGD step, and the step kernel alone against torch.optim.Adam on a block of the same size.  Measurement only; bench.py does not
run it.

CoOp runs at 100 classes on tools/coopfit_bench.py's shape, MaPLe on the first shape of tools/maplefit_bench.py (ViT-B/16 with synthetic
weights).  An SGD state and an Adam state on the same model and the same batch take one step each in turn (alternating, so that a drift
of the machine reaches both alike), every step between two device events with a synchronisation behind it; a window is --steps such
rounds, and the report is the median of --iters windows' mean step times with their minimum and maximum, after --warmup untimed rounds.
``block_step_adam`` alone, and ``torch.optim.Adam(foreach=False)`` and ``torch.optim.Adam(fused=True)`` on a same-sized fp32 block on
the same GPU, are timed the same way at the two block sizes.

Usage: python tools/optimstep_bench.py [--iters 5] [--steps 10] [--warmup 3] [--out profiles/optimstep_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clip_calibration_amd import coopfit, fitloop, maplefit, ops, synthetic as syn  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
import coopfit_bench as cb  # noqa: E402
import maplefit_bench as mb  # noqa: E402

COOP_CLASSES = 100


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def coop():
    model = build_model(dict(syn.synthetic_state_dict(cb.GEOM, seed=0)), {"trainer": "CoOp"}).cuda()
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(cb.BATCH, syn.GEOMETRIES[cb.GEOM].embed_dim, generator=g).cuda()
    labels = torch.randint(0, COOP_CLASSES, (cb.BATCH,), generator=g).cuda()
    ids, ctx = cb.prompt_ids(COOP_CLASSES), coopfit.init_context(model, cb.N_CTX)
    shape = dict(fit="coop", geometry=cb.GEOM, batch=cb.BATCH, classes=COOP_CLASSES, n_ctx=cb.N_CTX)
    return shape, 0.002, (feats, labels), lambda **kw: coopfit.CoOpFitState(model, ids, ctx, **kw), lambda st: st.ctx


def maple():
    Cn = mb.CLASSES[0]
    design = {"trainer": "MaPLe", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0, "maple_length": mb.N_CTX}
    model = build_model(dict(syn.synthetic_state_dict(mb.GEOM, seed=0)), design).cuda()
    pl = maplefit.init_learner_params(model, mb.N_CTX, mb.DEPTH, seed=0)
    g = torch.Generator().manual_seed(1)
    images = torch.randn(mb.BATCH, 3, 224, 224, generator=g).half().cuda()
    ids = syn.synthetic_token_ids(Cn, mb.GEOM, seed=0)
    labels = torch.randint(0, Cn, (mb.BATCH,), generator=g).cuda()
    shape = dict(fit="maple", geometry=mb.GEOM, batch=mb.BATCH, classes=Cn, n_ctx=mb.N_CTX, depth=mb.DEPTH)
    return shape, mb.LR, (images, labels), lambda **kw: maplefit.MaPLeFitState(model, ids, pl, **kw), lambda st: st.block


FITS = {"coop": coop, "maple": maple}


def windows(ms, steps):
    """(median, min, max) of the windows' mean step times."""
    w = [statistics.fmean(ms[i:i + steps]) for i in range(0, len(ms), steps)]
    return {"median": statistics.median(w), "min": min(w), "max": max(w)}


def time_fit(name, iters, steps, warmup):
    shape, rate, batch, make, block = FITS[name]()
    states = {"sgd": make(), "adam": make(optimizer="adam")}
    lr = torch.full((1,), rate, device="cuda")
    ms = {k: [] for k in states}
    for k in range(warmup + iters * steps):
        for w, st in states.items():
            a, b = events(2)
            a.record()
            st.step(*batch, lr)
            b.record()
            torch.cuda.synchronize()
            if k >= warmup:
                ms[w].append(a.elapsed_time(b))
    out = dict(shape, block_floats=block(states["sgd"]).numel(), finite=bool(torch.isfinite(block(states["adam"])).all()))
    for w in states:
        out[f"{w}_step_ms"] = windows(ms[w], steps)
    diff = out["adam_step_ms"]["median"] - out["sgd_step_ms"]["median"]
    spread = max(out[f"{w}_step_ms"]["max"] - out[f"{w}_step_ms"]["min"] for w in states)
    out.update(adam_minus_sgd_ms=diff, adam_over_sgd=out["adam_step_ms"]["median"] / out["sgd_step_ms"]["median"], widest_spread_ms=spread,
               difference_inside_spread=bool(abs(diff) <= spread))
    return out


def time_block(total, iters, steps, warmup):
    """clipmi_block_step_adam alone, and torch's two Adams, on a block of ``total`` floats."""
    g = torch.Generator().manual_seed(total)
    grad = torch.randn(total, generator=g).cuda()
    lr = torch.full((1,), 0.002, device="cuda")
    table = torch.from_numpy(fitloop.adam_bias_table((0.9, 0.999), warmup + iters * steps + 1)).cuda()
    p, m, v = torch.randn(total, generator=g).cuda(), torch.zeros(total).cuda(), torch.zeros(total).cuda()
    runs = {"block_step_adam": lambda k: ops.block_step_adam(grad, p, m, v, lr, k + 1, table, 1.0, weight_decay=5e-4, want_grad=False)}
    for label, kw in (("torch_adam_single_tensor", dict(foreach=False)), ("torch_adam_fused", dict(fused=True))):
        q = torch.nn.Parameter(torch.randn(total, generator=g).cuda())
        q.grad = grad.clone()
        opt = torch.optim.Adam([q], lr=0.002, weight_decay=5e-4, **kw)
        runs[label] = lambda k, opt=opt: opt.step()
    out = dict(block_floats=total)
    for label, run in runs.items():
        ms = []
        for k in range(warmup + iters * steps):
            a, b = events(2)
            a.record()
            run(k)
            b.record()
            torch.cuda.synchronize()
            if k >= warmup:
                ms.append(a.elapsed_time(b))
        out[f"{label}_ms"] = windows(ms, steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fits", nargs="*", default=list(FITS), choices=list(FITS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "steps": a.steps, "warmup": a.warmup, "fits": [], "blocks": []}
    for name in a.fits:
        r = time_fit(name, a.iters, a.steps, a.warmup)
        out["fits"].append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    for total in sorted({r["block_floats"] for r in out["fits"]}):
        r = time_block(total, a.iters, a.steps, a.warmup)
        out["blocks"].append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
