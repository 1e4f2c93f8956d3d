"""Time of one VPT training step on the device (clip_calibration_amd.vptfit, csrc/vision_backward.hip, csrc/attention.hip, csrc/prompt_train.hip)
against a torch fp16 autograd + SGD step over the same model, each kernel's share of the step, and the measurement behind ``grad_scale``'s
default.  Measurement only; bench.py does not run it.

1. step: ViT-B/16 with synthetic weights, n_ctx 8, depth 12, 100 classes, batches 4 and 32 of preprocessed fp16 images.
   ``VPTFitState.step`` between two device events, through the separate calls and through the one-call step, median of --iters steps after
   --warmup; the four phases (training forward, loss head, backward, SGD step) between events of their own; the stash and workspace sizes.
2. kernels: one step under ``torch.profiler``; the device time of every kernel name, its launches and its share of the step's kernel
   time.  The attention backward's share is reported as it is measured.
3. baseline: the repository's torch mirror of the same computation -- ``oracle.clip_oracle.encode_image`` with the state dict on the
   GPU at dtype float16 and the prompts as its ``shared_ctx`` / ``deep_prompts``, ``F.cross_entropy``, ``backward`` and
   ``torch.optim.SGD.step`` on an fp16 prompt block -- on the same GPU and the same batch.
4. --scale-table: at batch 4, the share of fp16 dgrad-GEMM operand elements that are zero or subnormal and the largest magnitude at
   grad_scale 2^0 .. 2^16 (``prompt_gradient(..., return_operand_stats=True)``).

Usage: python tools/vptfit_bench.py [--iters 5] [--warmup 2] [--scale-table] [--no-torch] [--no-kernels] [--out profiles/vptfit_bench.json]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clip_calibration_amd import synthetic as syn, vptfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

GEOM, N_CTX, DEPTH, CLASSES, BATCHES = "ViT-B/16", 8, 12, 100, (4, 32)


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def time_device(model, text, images, labels, iters, warmup):
    out = {}
    lr = torch.full((1,), 0.0025, device="cuda")
    for name, one_call in (("separate_calls", False), ("one_call", True)):
        st = vptfit.VPTFitState(model, text)
        ms = []
        for k in range(warmup + iters):
            a, b = events(2)
            a.record()
            st.step(images, labels, lr, one_call=one_call)
            b.record()
            torch.cuda.synchronize()
            if k >= warmup:
                ms.append(a.elapsed_time(b))
        out[f"step_ms_{name}"] = statistics.median(ms)
    t, phases = st.tower, []
    for k in range(iters):                     # the same four calls with an event behind each
        e = events(5)
        e[0].record()
        feats = t.forward(images, st.prompts)
        e[1].record()
        _, d_feats = vptfit.vpt_head(feats, labels, st.text, st.scale, st.grad_scale)
        e[2].record()
        d_prompts = t.backward(d_feats)
        e[3].record()
        vptfit.vpt_step(d_prompts, st.grad_scale, st.prompts, st.buf, lr, False, st.momentum, st.dampening, st.weight_decay, st.nesterov, want_grad=False)
        e[4].record()
        torch.cuda.synchronize()
        phases.append([e[i].elapsed_time(e[i + 1]) for i in range(4)])
    med = [statistics.median(p[i] for p in phases) for i in range(4)]
    out.update(forward_ms=med[0], head_ms=med[1], backward_ms=med[2], sgd_step_ms=med[3], stash_bytes=t.stash.numel(), workspace_bytes=t.ws.numel(),
               token_rows_per_image=197 + N_CTX)
    return out, st


def kernel_shares(st, images, labels):
    """Device time per kernel name over one step (separate calls), from torch.profiler's device events."""
    from torch.profiler import ProfilerActivity, profile
    lr = torch.full((1,), 0.0025, device="cuda")
    st.step(images, labels, lr)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        st.step(images, labels, lr)
        torch.cuda.synchronize()
    rows = {}
    for ev in prof.events():
        if str(getattr(ev, "device_type", "")).endswith("CUDA") and ev.device_time > 0:
            r = rows.setdefault(ev.name, [0, 0.0])
            r[0] += 1
            r[1] += ev.device_time
    total = sum(v[1] for v in rows.values())
    if not rows or total <= 0:
        raise RuntimeError("the profiler recorded no device kernel: no shares to report")
    table = [{"kernel": k, "launches": v[0], "device_us": v[1], "share": v[1] / total} for k, v in sorted(rows.items(), key=lambda kv: -kv[1][1])]
    return {"kernel_time_us": total, "kernels": table}


def time_torch(sd16, prompts, text, images, labels, iters, warmup):
    from oracle import clip_oracle as orc
    p = torch.nn.Parameter(prompts.half().cuda())
    opt = torch.optim.SGD([p], lr=0.0025, momentum=0.9, weight_decay=5e-4)
    t = text.half()
    tn = t / t.norm(dim=-1, keepdim=True)
    ms = []
    with torch.device("cuda"):
        for k in range(warmup + iters):
            a, b = events(2)
            a.record()
            f = orc.encode_image(sd16, images, torch.float16, p[0], [p[i] for i in range(1, p.shape[0])])
            logits = math.exp(4.6052) * (f / f.norm(dim=-1, keepdim=True)) @ tn.t()
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
    ap.add_argument("--scale-table", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    sd = syn.synthetic_state_dict(GEOM, seed=0)
    model = build_model(dict(sd), {"trainer": "VPT", "vision_depth": DEPTH, "vision_ctx": N_CTX, "language_depth": 0, "language_ctx": 0}).cuda()
    sd16 = {k: (v.cuda().half() if v.is_floating_point() else v.cuda()) for k, v in sd.items() if k.startswith("visual.")}
    g = torch.Generator().manual_seed(1)
    E = syn.GEOMETRIES[GEOM].embed_dim
    text = torch.randn(CLASSES, E, generator=g).cuda()
    prompts = vptfit.model_prompts(model)
    out = {"geometry": GEOM, "n_ctx": N_CTX, "depth": DEPTH, "classes": CLASSES, "device": torch.cuda.get_device_name(0), "steps": []}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")

    if a.scale_table:
        images = torch.randn(4, 3, 224, 224, generator=g).cuda()
        labels = torch.randint(0, CLASSES, (4,), generator=g)
        table = []
        for e in (0, 4, 8, 12, 16):
            loss, grad, s = vptfit.prompt_gradient(model, prompts, images, labels, text, grad_scale=2.0 ** e, return_operand_stats=True)
            row = {"grad_scale": f"2^{e}", "elements": s["elements"], "zero_share": s["zeros"] / s["elements"],
                   "subnormal_share": s["subnormals"] / s["elements"], "max": s["max"], "headroom_log2": math.log2(65504.0 / s["max"]) if s["max"] > 0 else None,
                   "grad_finite": bool(torch.isfinite(grad).all()), "grad_norm": float(grad.norm())}
            table.append(row)
            print("vptfit-parity: grad_scale " + json.dumps(row), flush=True)
        out["grad_scale_table"] = table
    for B in BATCHES:
        images = torch.randn(B, 3, 224, 224, generator=g).half().cuda()
        labels = torch.randint(0, CLASSES, (B,), generator=g).cuda()
        r, st = time_device(model, text, images, labels, a.iters, a.warmup)
        r = dict(batch=B, **r)
        out["steps"].append(r)
        print(json.dumps(r), flush=True)
        save()
        if not a.no_torch:
            t = dict(batch=B, baseline="torch fp16 autograd + SGD over the torch mirror", **time_torch(sd16, prompts, text, images, labels, a.iters, a.warmup))
            out["steps"].append(t)
            print(json.dumps(t), flush=True)
            save()
        if not a.no_kernels:
            k = kernel_shares(st, images, labels)
            r["kernel_time_us"] = k["kernel_time_us"]
            r["kernels"] = k["kernels"]
            att = sum(x["share"] for x in k["kernels"] if "attention_backward_full" in x["kernel"])
            r["attention_backward_share"] = att
            print(json.dumps({"batch": B, "attention_backward_share": att, "top": k["kernels"][:8]}), flush=True)
            save()
        del st
    save()


if __name__ == "__main__":
    main()
