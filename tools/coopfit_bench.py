"""Time of one CoOp training step on the device (clip_calibration_amd.coopfit, csrc/text_backward.hip, csrc/prompt_train.hip) against a torch fp16 autograd +
SGD step over the same model, and the measurement behind ``grad_scale``'s default.  Measurement only; bench.py does not run it.

1. step: ViT-B/16 text geometry with synthetic weights, batch 32 of cached image features, n_ctx 16, C = 100 and C = 1000 classes, the
   live-row cut on (token rows behind the last EOT are not computed) and off.  ``CoOpFitState.step`` between two device events, median of
   --iters steps after --warmup; the four phases of a step (training forward, loss head, backward, context step) between events of their
   own; the stash and workspace sizes.  Baseline: the repository's torch mirror of the same computation -- ``oracle.clip_oracle``'s
   ``coop_prompts`` + ``text_encoder`` with the state dict on the GPU at dtype float16, ``F.cross_entropy``, ``backward`` and
   ``torch.optim.SGD.step`` on an fp16 context -- on the same GPU, the same features, the whole context (the mirror has no cut).
2. --scale-table: at C = 100 with the cut on, the share of fp16 dgrad-GEMM operand elements that are zero or subnormal and the largest
   magnitude, at grad_scale 2^0, 2^4, 2^8, 2^12 and 2^16 (``context_gradient(..., return_operand_stats=True)``).

Usage: python tools/coopfit_bench.py [--iters 5] [--warmup 2] [--scale-table] [--out profiles/coopfit_bench.json]"""
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
from clip_calibration_amd import coopfit, ops, synthetic as syn  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

GEOM, N_CTX, BATCH = "ViT-B/16", 16, 32


def prompt_ids(C, seed=0):
    """[SOT, X * 16, 1 .. 7 name tokens, EOT, 0 ..]: the last EOT sits at token 24 of 77, as for "X .. X a <name>." prompts."""
    g = syn.GEOMETRIES[GEOM]
    rng = np.random.RandomState(seed)
    ids = np.zeros((C, g.context_length), np.int64)
    for c in range(C):
        k = 1 + c % 7
        ids[c, 0] = g.vocab_size - 2
        ids[c, 1:1 + N_CTX] = 1
        ids[c, 1 + N_CTX:1 + N_CTX + k] = rng.randint(2, g.vocab_size - 2, size=k)
        ids[c, 1 + N_CTX + k] = g.vocab_size - 1
    return torch.from_numpy(ids)


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def time_device(model, ids, ctx, feats, labels, cut, iters, warmup):
    st = coopfit.CoOpFitState(model, ids, ctx, seq_rows=None if cut else 0)
    lr = torch.full((1,), 0.002, device="cuda")
    ms, phases = [], []
    t = st.tower
    for k in range(warmup + iters):
        a, b = events(2)
        a.record()
        st.step(feats, labels, lr)
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(a.elapsed_time(b))
    for k in range(iters):                     # the same four calls with an event behind each
        e = events(5)
        e[0].record()
        text = t.forward(st.ctx)
        e[1].record()
        _, d_text = ops.coop_head(feats, labels, text, st.scale, st.grad_scale)
        e[2].record()
        d_embed = t.backward(d_text)
        e[3].record()
        ops.ctx_step(d_embed, t.C, t.n_ctx, t.per_class, st.grad_scale, st.ctx, st.buf, lr, False, st.momentum, st.dampening, st.weight_decay,
                     st.nesterov, want_grad=False)
        e[4].record()
        torch.cuda.synchronize()
        phases.append([e[i].elapsed_time(e[i + 1]) for i in range(4)])
    med = [statistics.median(p[i] for p in phases) for i in range(4)]
    return {"step_ms": statistics.median(ms), "step_ms_min": min(ms), "step_ms_max": max(ms), "forward_ms": med[0], "head_ms": med[1], "backward_ms": med[2], "ctx_step_ms": med[3],
            "token_rows_per_prompt": t.L, "stash_bytes": t.stash_bytes, "workspace_bytes": t.ws.numel()}


def time_torch(sd16, ids, ctx, feats, labels, iters, warmup):
    from oracle import clip_oracle as orc
    p = torch.nn.Parameter(ctx.half().cuda())
    opt = torch.optim.SGD([p], lr=0.002, momentum=0.9, weight_decay=5e-4)
    ids_d, f = ids.cuda(), feats.half()
    fn = f / f.norm(dim=-1, keepdim=True)
    ms = []
    with torch.device("cuda"):                 # the mirror builds its causal mask and row indices on the default device
        for k in range(warmup + iters):
            a, b = events(2)
            a.record()
            tf = orc.text_encoder(sd16, orc.coop_prompts(sd16, ids_d, p, torch.float16), ids_d, torch.float16)
            logits = math.exp(4.6052) * fn @ (tf / tf.norm(dim=-1, keepdim=True)).t()
            loss = torch.nn.functional.cross_entropy(logits.float(), labels)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            b.record()
            torch.cuda.synchronize()
            if k >= warmup:
                ms.append(a.elapsed_time(b))
    return {"step_ms": statistics.median(ms), "loss": float(loss.detach())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--classes", type=int, nargs="*", default=[100, 1000])
    ap.add_argument("--scale-table", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    sd = syn.synthetic_state_dict(GEOM, seed=0)
    model = build_model(dict(sd), {"trainer": "CoOp"}).cuda()
    sd16 = {k: (v.cuda().half() if v.is_floating_point() else v.cuda()) for k, v in sd.items() if not k.startswith("visual.")}
    g = torch.Generator().manual_seed(1)
    E, D = syn.GEOMETRIES[GEOM].embed_dim, syn.GEOMETRIES[GEOM].transformer_width
    ctx = 0.02 * torch.randn(N_CTX, D, generator=g)
    feats = torch.randn(BATCH, E, generator=g).cuda()
    out = {"geometry": GEOM, "batch": BATCH, "n_ctx": N_CTX, "device": torch.cuda.get_device_name(0), "steps": []}
    if a.scale_table:
        ids = prompt_ids(100)
        labels = torch.randint(0, 100, (BATCH,), generator=g)
        table = []
        for e in (0, 4, 8, 12, 16):
            loss, grad, s = coopfit.context_gradient(model, ids, ctx, feats, labels, grad_scale=2.0 ** e, return_operand_stats=True)
            row = {"grad_scale": f"2^{e}", "elements": s["elements"], "zero_share": s["zeros"] / s["elements"],
                   "subnormal_share": s["subnormals"] / s["elements"], "max": s["max"], "headroom_log2": math.log2(65504.0 / s["max"]) if s["max"] > 0 else None,
                   "grad_finite": bool(torch.isfinite(grad).all()), "grad_norm": float(grad.norm())}
            table.append(row)
            print("coopfit-parity: grad_scale " + json.dumps(row))
        out["grad_scale_table"] = table
    for C in a.classes:
        ids = prompt_ids(C)
        labels = torch.randint(0, C, (BATCH,), generator=g).cuda()
        for cut in (True, False):
            r = dict(classes=C, live_row_cut=cut, **time_device(model, ids, ctx, feats, labels, cut, a.iters, a.warmup))
            out["steps"].append(r)
            print(json.dumps(r))
        if not a.no_torch:
            r = dict(classes=C, baseline="torch fp16 autograd + SGD, whole context", **time_torch(sd16, ids, ctx, feats, labels, a.iters, a.warmup))
            out["steps"].append(r)
            print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
