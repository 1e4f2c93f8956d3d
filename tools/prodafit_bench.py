"""Time of one ProDA training step on the device (clip_calibration_amd.prodafit, csrc/proda_train.hip) against a torch fp16 autograd + SGD
step over a torch mirror of the same loss, and against our CoOp step at the same number of prompts.  Measurement only; bench.py does not
run it.

ViT-B/16 text geometry with synthetic weights, batch 32 of cached image features, n_ctx 16, 32 contexts in slices of 4, C = 100 and
C = 1000 classes, the live-row cut on: N = 4 C + 32 prompts per step.  ``ProDAFitState.step`` between two device events per step with one
fixed selection (one front, one middle, two end contexts), the median of --iters steps after --warmup untimed ones.  Baseline: the
repository's torch mirror -- ``oracle.clip_oracle.text_encoder`` with the state dict on the GPU at dtype float16 on prompts gathered by an
index table made once outside the timed region (the reference loops over the classes instead), the loss as proda.py:272-302 writes it,
``backward`` and ``torch.optim.SGD.step`` on an fp16 context -- on the same GPU, the same features, the whole context (the mirror has no
cut).  The CoOp step at N prompts shows what the head, the assembly and the step cost beyond the tower.  The stash the backward reads is
recorded in bytes.

Usage: python tools/prodafit_bench.py [--iters 5] [--warmup 2] [--classes 100 1000] [--no-torch] [--out profiles/prodafit_bench.json]"""
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
from clip_calibration_amd import coopfit, prodafit, synthetic as syn  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
import coopfit_bench as cb  # noqa: E402

GEOM, BATCH = cb.GEOM, cb.BATCH
N_CTX, N_PROMPT, PROMPT_BS, ALPHA = 16, 32, 4, 0.1
SEL = (0, 8, 16, 24)          # front, middle, end, end


def prompt_ids(C, n_ctx, dot=True, seed=0):
    """[SOT, X * n_ctx, 1 .. 7 name tokens, '.', EOT, 0 ..]; without ``dot`` the layout of tools/promptfit_bench.py."""
    g = syn.GEOMETRIES[GEOM]
    rng = np.random.RandomState(seed)
    ids = np.zeros((C, g.context_length), np.int64)
    for c in range(C):
        k = 1 + c % 7
        ids[c, 0] = g.vocab_size - 2
        ids[c, 1:1 + n_ctx] = 1
        ids[c, 1 + n_ctx:1 + n_ctx + k] = rng.randint(3, g.vocab_size - 2, size=k)
        if dot:
            ids[c, 1 + n_ctx + k] = 2
        ids[c, 1 + n_ctx + k + int(dot)] = g.vocab_size - 1
    return torch.from_numpy(ids)


def timed(step, iters, warmup):
    ms = []
    for k in range(warmup + iters):
        a, b = cb.events(2)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(a.elapsed_time(b))
    return {"step_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def time_device(model, ids, ctx, feats, labels, iters, warmup, one_call):
    st = prodafit.ProDAFitState(model, ids, ctx, prompt_bs=PROMPT_BS, alpha=ALPHA)
    lr = torch.full((1,), 0.002, device="cuda")
    sel = torch.from_numpy(prodafit.reference_order(SEL, prodafit.positions(N_PROMPT))).cuda()
    r = timed(lambda: st.step(feats, labels, lr, sel=sel, one_call=one_call), iters, warmup)
    return dict(r, token_rows_per_prompt=st.tower.L, prompts=st.tower.N, stash_bytes=st.tower.stash_bytes)


def time_coop(model, n_prompts, feats, labels, iters, warmup):
    ids = prompt_ids(n_prompts, N_CTX, dot=False)
    ctx = 0.02 * torch.randn(N_CTX, syn.GEOMETRIES[GEOM].transformer_width, generator=torch.Generator().manual_seed(2))
    st = coopfit.CoOpFitState(model, ids, ctx)
    lr = torch.full((1,), 0.002, device="cuda")
    r = timed(lambda: st.step(feats, labels, lr), iters, warmup)
    return dict(r, token_rows_per_prompt=st.tower.L, prompts=n_prompts, stash_bytes=st.tower.stash_bytes)


def gather_table(ids, sel, pos, n_ctx):
    """src [C Pb, Lc]: the row of cat([class embeddings [C Lc], selected contexts [Pb n_ctx]]) every prompt row comes from."""
    Cn, Lc = ids.shape
    nl = (ids.argmax(dim=-1) - n_ctx - 2).numpy()
    h = n_ctx // 2
    src = np.empty((Cn, len(sel), Lc), np.int64)
    for c in range(Cn):
        for q, p in enumerate(sel):
            row = np.arange(Lc) + c * Lc
            ctx_rows = [1 + nl[c] + j if pos[p] == 0 else (1 + j if (pos[p] == 2 or j < h) else 1 + nl[c] + j) for j in range(n_ctx)]
            free = [r for r in range(1, 1 + n_ctx + nl[c]) if r not in ctx_rows]
            row[ctx_rows] = Cn * Lc + q * n_ctx + np.arange(n_ctx)
            row[free] = c * Lc + 1 + n_ctx + np.arange(nl[c])
            src[c, q] = row
    return torch.from_numpy(src.reshape(Cn * len(sel), Lc))


def time_torch(sd16, ids, ctx, feats, labels, iters, warmup):
    from oracle import clip_oracle as orc
    Cn, Lc = ids.shape
    pos = prodafit.positions(N_PROMPT)
    sel = prodafit.reference_order(SEL, pos)
    p = torch.nn.Parameter(ctx.half().cuda())
    opt = torch.optim.SGD([p], lr=0.002, momentum=0.9, weight_decay=5e-4)
    ids_d = ids.cuda()
    src = gather_table(ids, sel, pos, N_CTX).cuda()
    sel_d = torch.from_numpy(sel.astype(np.int64)).cuda()
    emb = sd16["token_embedding.weight"][ids_d]
    D = emb.shape[-1]
    nc_ids = torch.cat([ids_d[:1, :1 + N_CTX], ids_d[:1, 1 + N_CTX + 1:], ids_d.new_zeros(1, 1)], dim=1)     # class 0's name is one token long
    nc_emb = sd16["token_embedding.weight"][nc_ids]
    tok = ids_d.unsqueeze(1).repeat(1, len(sel), 1).view(Cn * len(sel), -1)
    nc_tok = nc_ids.repeat(N_PROMPT, 1)
    f = feats.half()
    x = f / f.norm(dim=-1, keepdim=True)
    s = math.exp(4.6052)
    off = ~torch.eye(N_PROMPT, dtype=torch.bool, device="cuda")
    Pb, rows, classes = len(sel), torch.arange(feats.shape[0], device="cuda"), torch.arange(Cn, device="cuda")

    def step():
        table = torch.cat([emb.reshape(Cn * Lc, D), p[sel_d].reshape(-1, D)])
        prompts = table[src]
        nc_prompts = torch.cat([nc_emb[:, :1].expand(N_PROMPT, -1, -1), p, nc_emb[:, 1 + N_CTX:].expand(N_PROMPT, -1, -1)], dim=1)
        tf = orc.text_encoder(sd16, torch.cat([prompts, nc_prompts]), torch.cat([tok, nc_tok]), torch.float16)
        u = torch.nn.functional.normalize(tf, dim=-1)
        cls, n = u[:Cn * Pb].view(Cn, Pb, -1), u[Cn * Pb:]
        centre = cls.mean(dim=1)
        v = (cls - centre[:, None]).permute(2, 0, 1)                                   # [E, C, Pb]
        R = torch.einsum("be,eik->bik", x * x, (v @ v.transpose(1, 2)) / (Pb + 1))    # through the [E, C, C] covariance, as the reference
        sigma = R[rows, labels, labels][:, None] + R[:, classes, classes] - 2.0 * R[rows, labels]
        z = s * (x @ centre.t()) + 0.5 * s * s * sigma
        loss = torch.nn.functional.cross_entropy(z.float(), labels) + ALPHA * (n @ n.t())[off].float().abs().mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    with torch.device("cuda"):                 # the mirror builds its causal mask and row indices on the default device
        return timed(step, iters, warmup)


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
    out = {"geometry": GEOM, "batch": BATCH, "n_ctx": N_CTX, "n_prompt": N_PROMPT, "prompt_bs": PROMPT_BS, "device": torch.cuda.get_device_name(0),
           "iters": a.iters, "warmup": a.warmup, "steps": []}

    def record(r):
        out["steps"].append(r)
        print(json.dumps(r), flush=True)

    for C in a.classes:
        labels = torch.randint(0, C, (BATCH,), generator=g).cuda()
        ids = prompt_ids(C, N_CTX)
        ctx = 0.02 * torch.randn(N_PROMPT, N_CTX, D, generator=g)
        for one_call in (False, True):
            record(dict(classes=C, method="proda", one_call=one_call, **time_device(model, ids, ctx, feats, labels, a.iters, a.warmup, one_call)))
        record(dict(classes=C, method="coop", note="our CoOp step at the same number of prompts",
                    **time_coop(model, C * PROMPT_BS + N_PROMPT, feats, labels, a.iters, a.warmup)))
        if not a.no_torch:
            try:
                r = time_torch(sd16, ids, ctx, feats, labels, a.iters, a.warmup)
            except torch.OutOfMemoryError as e:
                r = {"error": "out of memory: " + str(e).splitlines()[0]}
                torch.cuda.empty_cache()
            record(dict(classes=C, method="proda", baseline="torch fp16 autograd + SGD, whole context", **r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
