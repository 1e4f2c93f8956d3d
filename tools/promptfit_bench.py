"""Time of one KgCoOp and one ProGrad training step on the device (clip_calibration_amd.coopfit with ``method=``,
csrc/prompt_train.hip) against our CoOp step and against a torch fp16 autograd + SGD step over the torch mirror of the same method.
Measurement only; bench.py does not run it.

ViT-B/16 text geometry with synthetic weights, batch 32 of cached image features, C = 100 and C = 1000 classes, the live-row cut on;
n_ctx 16 for every method and n_ctx 4 for KgCoOp as well (its shipped configuration).  ``CoOpFitState.step`` between two device events
per step, the median of --iters steps after --warmup untimed ones; the teacher is a random normalised matrix.  Baseline: the
repository's torch mirror -- ``oracle.clip_oracle``'s ``coop_prompts`` + ``text_encoder`` with the state dict on the GPU at dtype
float16, the method's loss, ``backward`` (two for ProGrad, the first with ``retain_graph``, and the projection in torch) and
``torch.optim.SGD.step`` on an fp16 context -- on the same GPU, the same features, the whole context (the mirror has no cut).

Two properties are expected and recorded, not promised: KgCoOp's step costs a CoOp step (the head gains one term); ProGrad's costs a
CoOp step plus one more backward.

Usage: python tools/promptfit_bench.py [--iters 5] [--warmup 2] [--classes 100 1000] [--no-torch] [--out profiles/promptfit_bench.json]"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clip_calibration_amd import coopfit, synthetic as syn  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
import coopfit_bench as cb  # noqa: E402

GEOM, BATCH = cb.GEOM, cb.BATCH


def prompt_ids(C, n_ctx, seed=0):
    """[SOT, X * n_ctx, 1 .. 7 name tokens, EOT, 0 ..], as tools/coopfit_bench.py builds them for n_ctx = 16."""
    g = syn.GEOMETRIES[GEOM]
    rng = np.random.RandomState(seed)
    ids = np.zeros((C, g.context_length), np.int64)
    for c in range(C):
        k = 1 + c % 7
        ids[c, 0] = g.vocab_size - 2
        ids[c, 1:1 + n_ctx] = 1
        ids[c, 1 + n_ctx:1 + n_ctx + k] = rng.randint(2, g.vocab_size - 2, size=k)
        ids[c, 1 + n_ctx + k] = g.vocab_size - 1
    return torch.from_numpy(ids)


def time_device(model, ids, ctx, feats, labels, teacher, method, iters, warmup):
    st = coopfit.CoOpFitState(model, ids, ctx, method=method, teacher=teacher)
    lr = torch.full((1,), 0.002, device="cuda")
    ms = []
    for k in range(warmup + iters):
        a, b = cb.events(2)
        a.record()
        st.step(feats, labels, lr)
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(a.elapsed_time(b))
    return {"step_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "token_rows_per_prompt": st.tower.L}


def time_torch(sd16, ids, ctx, feats, labels, teacher, method, iters, warmup, w=8.0, T=1.0, lam=1.0):
    from oracle import clip_oracle as orc
    p = torch.nn.Parameter(ctx.half().cuda())
    opt = torch.optim.SGD([p], lr=0.002, momentum=0.9, weight_decay=5e-4)
    ids_d, f = ids.cuda(), feats.half()
    fn = f / f.norm(dim=-1, keepdim=True)
    o = teacher.half()
    z_tea = (math.exp(4.6052) * fn @ o.t()).float()
    ms = []
    with torch.device("cuda"):                 # the mirror builds its causal mask and row indices on the default device
        for k in range(warmup + iters):
            a, b = cb.events(2)
            a.record()
            tf = orc.text_encoder(sd16, orc.coop_prompts(sd16, ids_d, p, torch.float16), ids_d, torch.float16)
            u = tf / tf.norm(dim=-1, keepdim=True)
            logits = (math.exp(4.6052) * fn @ u.t()).float()
            xe = torch.nn.functional.cross_entropy(logits, labels)
            opt.zero_grad(set_to_none=True)
            if method == "kgcoop":
                (xe + w * (1.0 - (u * o).sum(-1).float().mean())).backward()
            else:
                kl = (-torch.softmax(z_tea / T, -1) * torch.log_softmax(logits / T, -1) * T * T).sum(1).mean()
                kl.backward(retain_graph=True)
                gb = p.grad.clone()
                opt.zero_grad(set_to_none=True)
                xe.backward()
                ga = p.grad
                bn = gb / torch.linalg.norm(gb)
                if torch.dot((ga / torch.linalg.norm(ga)).flatten(), bn.flatten()) < 0:      # the reference reads this on the host too
                    p.grad = ga - lam * torch.dot(ga.flatten(), bn.flatten()) * bn
            opt.step()
            b.record()
            torch.cuda.synchronize()
            if k >= warmup:
                ms.append(a.elapsed_time(b))
    return {"step_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--classes", type=int, nargs="*", default=[100, 1000])
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    sd = syn.synthetic_state_dict(GEOM, seed=0)
    model = build_model(dict(sd), {"trainer": "CoOp"}).cuda()
    sd16 = {k: (v.cuda().half() if v.is_floating_point() else v.cuda()) for k, v in sd.items() if not k.startswith("visual.")}
    g = torch.Generator().manual_seed(1)
    E, D = syn.GEOMETRIES[GEOM].embed_dim, syn.GEOMETRIES[GEOM].transformer_width
    feats = torch.randn(BATCH, E, generator=g).cuda()
    out = {"geometry": GEOM, "batch": BATCH, "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "steps": []}
    for C in a.classes:
        labels = torch.randint(0, C, (BATCH,), generator=g).cuda()
        teacher = torch.nn.functional.normalize(torch.randn(C, E, generator=g), dim=-1).cuda()
        for method, n_ctx in (("coop", 16), ("kgcoop", 16), ("kgcoop", 4), ("prograd", 16)):
            ids = prompt_ids(C, n_ctx)
            ctx = 0.02 * torch.randn(n_ctx, D, generator=g)
            r = dict(classes=C, method=method, n_ctx=n_ctx, **time_device(model, ids, ctx, feats, labels, teacher, method, a.iters, a.warmup))
            out["steps"].append(r)
            print(json.dumps(r), flush=True)
            if not a.no_torch and method != "coop":
                r = dict(classes=C, method=method, n_ctx=n_ctx, baseline="torch fp16 autograd + SGD, whole context",
                         **time_torch(sd16, ids, ctx, feats, labels, teacher, method, a.iters, a.warmup))
                out["steps"].append(r)
                print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
