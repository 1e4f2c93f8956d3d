"""What the dynamic loss scale costs per training step for the fits that step one master block -- CoCoOp, VPT, MaPLe, PromptSRC
(``grad_scale="dynamic"``, csrc/grad_scaler.hip clipmi_block_step_scaled) -- against the static scale's step.  Measurement only; bench.py
does not run it.

Each fit runs on the first shape of its own bench tool (tools/{cocoopfit,vptfit,maplefit,promptsrcfit}_bench.py: ViT-B/16 with synthetic
weights).  Four states on the same model and the same batch -- static and dynamic, each through the separate calls and through the
one-call entry -- take one step each in turn (alternating, so that a drift of the machine reaches all four alike), every step between two
device events with a synchronisation behind it; the median of --iters rounds after --warmup untimed ones.  The dynamic state starts at
the fit's static default with a growth interval beyond the run: both paths do the same arithmetic and no step is skipped.

Usage: python tools/blockscaler_bench.py [--iters 5] [--warmup 2] [--fits cocoop vpt maple promptsrc] [--out profiles/blockscaler_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clip_calibration_amd import cocoopfit, maplefit, promptsrcfit, synthetic as syn, vptfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
import cocoopfit_bench as ccb  # noqa: E402
import maplefit_bench as mb  # noqa: E402
import promptsrcfit_bench as pb  # noqa: E402
import vptfit_bench as vb  # noqa: E402

WAYS = [("static", False), ("dynamic", False), ("static", True), ("dynamic", True)]
FAR = 1 << 20        # a growth interval beyond the run


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def cocoop():
    B, Cn = ccb.SHAPES[0]
    model = build_model(dict(syn.synthetic_state_dict(ccb.GEOM, seed=0)), {"trainer": "CoOp"}).cuda()
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(B, syn.GEOMETRIES[ccb.GEOM].embed_dim, generator=g).cuda()
    labels = torch.randint(0, Cn, (B,), generator=g).cuda()
    ids, params = ccb.prompt_ids(Cn, ccb.N_CTX), ccb.params_for(model, feats)
    shape = dict(geometry=ccb.GEOM, batch=B, classes=Cn, n_ctx=ccb.N_CTX)
    return shape, cocoopfit.DEFAULT_GRAD_SCALE, 0.002, (feats, labels), lambda **kw: cocoopfit.CoCoOpFitState(model, ids, params, **kw), lambda st: st.block


def vpt():
    B = vb.BATCHES[0]
    design = {"trainer": "VPT", "vision_depth": vb.DEPTH, "vision_ctx": vb.N_CTX, "language_depth": 0, "language_ctx": 0}
    model = build_model(dict(syn.synthetic_state_dict(vb.GEOM, seed=0)), design).cuda()
    g = torch.Generator().manual_seed(1)
    text = torch.randn(vb.CLASSES, syn.GEOMETRIES[vb.GEOM].embed_dim, generator=g).cuda()
    images = torch.randn(B, 3, 224, 224, generator=g).half().cuda()
    labels = torch.randint(0, vb.CLASSES, (B,), generator=g).cuda()
    shape = dict(geometry=vb.GEOM, batch=B, classes=vb.CLASSES, n_ctx=vb.N_CTX, depth=vb.DEPTH)
    return shape, vptfit.DEFAULT_GRAD_SCALE, 0.0025, (images, labels), lambda **kw: vptfit.VPTFitState(model, text, **kw), lambda st: st.prompts


def maple():
    Cn = mb.CLASSES[0]
    design = {"trainer": "MaPLe", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0, "maple_length": mb.N_CTX}
    model = build_model(dict(syn.synthetic_state_dict(mb.GEOM, seed=0)), design).cuda()
    pl = maplefit.init_learner_params(model, mb.N_CTX, mb.DEPTH, seed=0)
    g = torch.Generator().manual_seed(1)
    images = torch.randn(mb.BATCH, 3, 224, 224, generator=g).half().cuda()
    ids = syn.synthetic_token_ids(Cn, mb.GEOM, seed=0)
    labels = torch.randint(0, Cn, (mb.BATCH,), generator=g).cuda()
    shape = dict(geometry=mb.GEOM, batch=mb.BATCH, classes=Cn, n_ctx=mb.N_CTX, depth=mb.DEPTH)
    return shape, maplefit.DEFAULT_GRAD_SCALE, mb.LR, (images, labels), lambda **kw: maplefit.MaPLeFitState(model, ids, pl, **kw), lambda st: st.block


def promptsrc():
    Cn = pb.CLASSES[0]
    sd = syn.synthetic_state_dict(pb.GEOM, seed=0)
    design = {"trainer": "IVLP", "vision_depth": pb.DEPTH, "language_depth": pb.DEPTH, "vision_ctx": pb.N_CTX, "language_ctx": pb.N_CTX}
    model = build_model(dict(sd), design).cuda()
    plain = build_model(dict(sd), {"trainer": "CoOp", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0}).cuda()
    pl = promptsrcfit.init_params(model, seed=0)
    g = torch.Generator().manual_seed(1)
    images = torch.randn(pb.BATCH, 3, 224, 224, generator=g).half().cuda()
    ids = syn.synthetic_token_ids(Cn, pb.GEOM, seed=0)
    labels = torch.randint(0, Cn, (pb.BATCH,), generator=g).cuda()
    teacher = plain.text_features_f32(ids.cuda())
    shape = dict(geometry=pb.GEOM, batch=pb.BATCH, classes=Cn, n_ctx=pb.N_CTX, depth=pb.DEPTH)
    return (shape, promptsrcfit.DEFAULT_GRAD_SCALE, pb.LR, (images, labels), lambda **kw: promptsrcfit.PromptSRCFitState(model, ids, pl, teacher, **kw),
            lambda st: st.block)


FITS = {"cocoop": cocoop, "vpt": vpt, "maple": maple, "promptsrc": promptsrc}


def time_fit(name, iters, warmup):
    shape, default, rate, batch, make, block = FITS[name]()
    scaler = {"init_scale": default, "growth_interval": FAR}
    states = {(kind, one_call): make(**({"grad_scale": "dynamic", "scaler": scaler} if kind == "dynamic" else {})) for kind, one_call in WAYS}
    lr = torch.full((1,), rate, device="cuda")
    ms = {w: [] for w in states}
    for k in range(warmup + iters):
        for w, st in states.items():
            a, b = events(2)
            a.record()
            st.step(*batch, lr, one_call=w[1])
            b.record()
            torch.cuda.synchronize()
            if k >= warmup:
                ms[w].append(a.elapsed_time(b))
    same = all(torch.equal(block(states["static", oc]), block(states["dynamic", oc])) for oc in (False, True))
    out = dict(fit=name, **shape, init_scale=default, same_bits_as_static=bool(same),
               skipped_steps=[states["dynamic", oc].scaler_state()["skipped_steps"] for oc in (False, True)])
    for (kind, one_call), v in ms.items():
        out[f"{kind}_{'one_call' if one_call else 'separate'}_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    for one_call in (False, True):
        out[f"dynamic_over_static_{'one_call' if one_call else 'separate'}"] = (statistics.median(ms["dynamic", one_call]) /
                                                                               statistics.median(ms["static", one_call]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fits", nargs="*", default=list(FITS), choices=list(FITS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "steps": []}
    for name in a.fits:
        r = time_fit(name, a.iters, a.warmup)
        out["steps"].append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
