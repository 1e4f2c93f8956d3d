"""Time of one CoCoOp training step on the device (clip_calibration_amd.cocoopfit, csrc/cocoop_train.hip) against a torch fp16 autograd +
SGD step over a torch mirror of the same loss, and against our CoOp step at the same number of prompts.  Measurement only; bench.py does
not run it.

ViT-B/16 text geometry with synthetic weights, n_ctx 4, the live-row cut on, cached image features: B = 1 at C = 100 and C = 1000 classes
(the reference's configuration: batch 1) and B = 4 at C = 100, N = B C prompts per step.  ``CoCoOpFitState.step`` between two device events
per step, the median of --iters steps after --warmup untimed ones.  (a) The CoOp step at N prompts in the same run isolates what meta,
embed, head, reduce and step add to the tower.  (b) Baseline: the repository's torch mirror -- ``oracle.clip_oracle.text_encoder`` with the
state dict on the GPU at dtype float16, the meta-net in half, the B C prompts built in one batch (the reference loops over the images),
``backward`` and ``torch.optim.SGD.step`` over the five fp16 tensors -- on the same GPU, the same features, the whole context (the
mirror has no cut).  The stash the backward reads is recorded in bytes.

--grad-scale-stats: the operand statistics ``clipmi_text_encoder_backward`` collects, at B = 1, C = 100 of the same geometry, for grad_scale
2^0 .. 2^16 -- the measurement behind the default (profiles/cocoopfit_parity.txt).

Usage: python tools/cocoopfit_bench.py [--iters 5] [--warmup 2] [--no-torch] [--grad-scale-stats] [--out profiles/cocoopfit_bench.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clip_calibration_amd import cocoopfit, coopfit, synthetic as syn  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
import coopfit_bench as cb  # noqa: E402
from prodafit_bench import prompt_ids, timed  # noqa: E402

GEOM = cb.GEOM
N_CTX = 4
SHAPES = [(1, 100), (1, 1000), (4, 100)]          # (B, C)


def params_for(model, feats, seed=0):
    """init_params with the meta-net's second layer scaled so that the shift is of the context's own size."""
    p = cocoopfit.init_params(model, n_ctx=N_CTX, seed=seed)
    p[cocoopfit.NAMES[3]] = p[cocoopfit.NAMES[3]] * 0.1
    p[cocoopfit.NAMES[4]] = p[cocoopfit.NAMES[4]] * 0.1
    return p


def time_device(model, ids, params, feats, labels, iters, warmup, one_call):
    st = cocoopfit.CoCoOpFitState(model, ids, params)
    lr = torch.full((1,), 0.002, device="cuda")
    r = timed(lambda: st.step(feats, labels, lr, one_call=one_call), iters, warmup)
    t = st.tower(feats.shape[0])
    return dict(r, token_rows_per_prompt=t.L, prompts=t.N, stash_bytes=t.stash_bytes)


def time_coop(model, n_prompts, feats, labels, iters, warmup):
    ids = prompt_ids(n_prompts, N_CTX, dot=False)
    ctx = 0.02 * torch.randn(N_CTX, syn.GEOMETRIES[GEOM].transformer_width, generator=torch.Generator().manual_seed(2))
    st = coopfit.CoOpFitState(model, ids, ctx)
    lr = torch.full((1,), 0.002, device="cuda")
    r = timed(lambda: st.step(feats, labels, lr), iters, warmup)
    return dict(r, token_rows_per_prompt=st.tower.L, prompts=n_prompts, stash_bytes=st.tower.stash_bytes)


def time_torch(sd16, ids, params, feats, labels, iters, warmup):
    from oracle import clip_oracle as orc
    Cn = ids.shape[0]
    B = feats.shape[0]
    ps = [torch.nn.Parameter(params[k].half().cuda()) for k in cocoopfit.NAMES]
    ctx, w1, b1, w2, b2 = ps
    opt = torch.optim.SGD(ps, lr=0.002, momentum=0.9, weight_decay=5e-4)
    ids_d = ids.cuda()
    emb = sd16["token_embedding.weight"][ids_d]
    tok = ids_d.repeat(B, 1)
    f = feats.half()
    x = f / f.norm(dim=-1, keepdim=True)
    s = math.exp(4.6052)

    def step():
        pi = torch.relu(x @ w1.t() + b1) @ w2.t() + b2
        shifted = ctx[None] + pi[:, None]                                        # [B, n_ctx, D]
        prompts = torch.cat([emb[None, :, :1].expand(B, -1, -1, -1), shifted[:, None].expand(-1, Cn, -1, -1),
                             emb[None, :, 1 + N_CTX:].expand(B, -1, -1, -1)], dim=2).reshape(B * Cn, emb.shape[1], -1)
        tf = orc.text_encoder(sd16, prompts, tok, torch.float16)
        u = torch.nn.functional.normalize(tf, dim=-1).view(B, Cn, -1)
        z = s * (x[:, None] * u).sum(-1)
        loss = torch.nn.functional.cross_entropy(z.float(), labels)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    with torch.device("cuda"):                 # the mirror builds its causal mask and row indices on the default device
        return timed(step, iters, warmup)


def grad_scale_stats(model, feats, labels, ids, params):
    rows = []
    for e in (0, 4, 8, 9, 10, 11, 12, 16):
        _, grads, st = cocoopfit.gradients(model, ids, params, feats, labels, grad_scale=2.0 ** e, return_operand_stats=True)
        finite = all(bool(torch.isfinite(g).all()) for g in grads.values())
        r = {"grad_scale": f"2^{e}", "elements": st["elements"], "zero_fraction": st["zeros"] / st["elements"],
             "subnormal_fraction": st["subnormals"] / st["elements"], "max_log2": math.log2(st["max"]) if st["max"] > 0 and math.isfinite(st["max"]) else None,
             "headroom_log2": math.log2(65504.0 / st["max"]) if st["max"] > 0 and math.isfinite(st["max"]) else None, "gradients_finite": finite}
        rows.append(r)
        print("cocoopfit-grad-scale: " + json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--grad-scale-stats", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    sd = syn.synthetic_state_dict(GEOM, seed=0)
    model = build_model(dict(sd), {"trainer": "CoOp"}).cuda()
    sd16 = {k: (v.cuda().half() if v.is_floating_point() else v.cuda()) for k, v in sd.items() if not k.startswith("visual.")}
    g = torch.Generator().manual_seed(1)
    E = syn.GEOMETRIES[GEOM].embed_dim
    out = {"geometry": GEOM, "n_ctx": N_CTX, "hidden": E // 16, "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "steps": []}

    def record(r):
        out["steps"].append(r)
        print(json.dumps(r), flush=True)

    if a.grad_scale_stats:
        feats = torch.randn(1, E, generator=g).cuda()
        labels = torch.randint(0, 100, (1,), generator=g).cuda()
        out["grad_scale_stats"] = {"batch": 1, "classes": 100, "rows": grad_scale_stats(model, feats, labels, prompt_ids(100, N_CTX), params_for(model, feats))}
    for B, Cn in SHAPES:
        feats = torch.randn(B, E, generator=g).cuda()
        labels = torch.randint(0, Cn, (B,), generator=g).cuda()
        ids = prompt_ids(Cn, N_CTX)
        params = params_for(model, feats)
        for one_call in (False, True):
            record(dict(batch=B, classes=Cn, method="cocoop", one_call=one_call, **time_device(model, ids, params, feats, labels, a.iters, a.warmup, one_call)))
        coop_labels = torch.randint(0, B * Cn, (B,), generator=g).cuda()
        record(dict(batch=B, classes=Cn, method="coop", note="our CoOp step at the same number of prompts",
                    **time_coop(model, B * Cn, feats, coop_labels, a.iters, a.warmup)))
        if not a.no_torch:
            try:
                r = time_torch(sd16, ids, params, feats, labels, a.iters, a.warmup)
            except torch.OutOfMemoryError as e:
                r = {"error": "out of memory: " + str(e).splitlines()[0]}
                torch.cuda.empty_cache()
            record(dict(batch=B, classes=Cn, method="cocoop", baseline="torch fp16 autograd + SGD, whole context", **r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
