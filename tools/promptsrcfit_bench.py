"""Time of one PromptSRC training step on the device (clip_calibration_amd.promptsrcfit, csrc/promptsrc_train.hip, csrc/prompt_train.hip,
csrc/text_backward.hip, csrc/vision_backward.hip) beside a CoOp step at the same prompts, a VPT step at the same batch and the frozen
image forward from the same run, against a torch fp16 autograd + SGD step over the torch mirror, each kernel's share of the step, and the
measurement behind ``grad_scale``'s default.  Measurement only; bench.py does not run it.

ViT-B/16 with synthetic weights, nt = nv = 4, depths 9 / 9, batch 4 of preprocessed fp16 images, at 100 and 1 000 classes, the loss
weights 25 / 10 / 1; the median of --iters steps after --warmup, between two device events.
1. ``PromptSRCFitState.step`` through the separate calls and through the one-call step; the stash bytes of both towers.
2. ``CoOpFitState.step`` on the same prompt set (n_ctx 4, cached image features), ``VPTFitState.step`` on the same batch (n_ctx 4, depth 9)
   and the frozen plain image forward as the step issues it: the yardstick is their sum.
3. kernels: one step under ``torch.profiler``: the device time of every kernel name, its launches and its share; ``new_kernels`` lists
   this method's own launches.
4. baseline: the repository's torch mirror -- ``oracle.clip_oracle`` with the state dict on the GPU at float16 --, the reference's loss
   expression, ``backward`` and ``torch.optim.SGD.step`` over the parameter list, on the same GPU and batch.
5. --scale-table: per tower, the share of fp16 dgrad-GEMM operand elements that are zero or subnormal and the largest magnitude at
   grad_scale 2^0 .. 2^16 (``promptsrcfit.gradients(..., return_operand_stats=True)``), at 100 classes.

Usage: python tools/promptsrcfit_bench.py [--iters 5] [--warmup 2] [--scale-table] [--no-torch] [--no-kernels] [--out profiles/promptsrcfit_bench.json]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clip_calibration_amd import coopfit, promptsrcfit, synthetic as syn, vptfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

GEOM, N_CTX, DEPTH, BATCH, CLASSES = "ViT-B/16", 4, 9, 4, (100, 1000)
LR = 0.0025
NEW_KERNELS = ("promptsrc_softmax_kernel", "promptsrc_l1_kernel", "promptsrc_loss_kernel", "promptsrc_step_kernel", "gpa_accumulate_kernel")


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def median_ms(step, iters, warmup):
    ms = []
    for k in range(warmup + iters):
        a, b = events(2)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def kernel_shares(step):
    from torch.profiler import ProfilerActivity, profile
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
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


def time_torch(sd16, ids, pl, images, labels, teacher, iters, warmup):
    from oracle import clip_oracle as orc
    F = torch.nn.functional
    p = {n: torch.nn.Parameter(v.half().cuda()) for n, v in pl.items()}
    opt = torch.optim.SGD(list(p.values()), lr=LR, momentum=0.9, weight_decay=5e-4)
    ids = ids.cuda()
    deep_t = [p[f"transformer.resblocks.{i}.VPT_shallow"] for i in range(1, DEPTH)]
    deep_v = [p[f"visual.transformer.resblocks.{i}.VPT_shallow"] for i in range(1, DEPTH)]
    o = (teacher / teacher.norm(dim=-1, keepdim=True)).half()
    state = {}

    def step():
        with torch.device("cuda"):
            tf = orc.text_encoder(sd16, orc.coop_prompts(sd16, ids, p["ctx"], torch.float16), ids, torch.float16, deep_t, N_CTX)
            f = orc.encode_image(sd16, images, torch.float16, p["visual.VPT"], deep_v)
            with torch.no_grad():
                zs = orc.encode_image(sd16, images, torch.float16)
            x, u, y = f / f.norm(dim=-1, keepdim=True), tf / tf.norm(dim=-1, keepdim=True), zs / zs.norm(dim=-1, keepdim=True)
            s = math.exp(4.6052)
            z, zz = (s * x @ u.t()).float(), (s * y @ o.t()).float()
            loss = (F.cross_entropy(z, labels) + 25.0 * F.l1_loss(u.float(), o.float()) + 10.0 * F.l1_loss(x.float(), y.float())
                    + F.kl_div(F.log_softmax(z, dim=1), F.log_softmax(zz, dim=1), reduction="sum", log_target=True) / z.numel())
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            state["loss"] = loss.detach()
    return {"step_ms": median_ms(step, iters, warmup), "loss": float(state["loss"])}


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
    design = {"trainer": "IVLP", "vision_depth": DEPTH, "language_depth": DEPTH, "vision_ctx": N_CTX, "language_ctx": N_CTX}
    model = build_model(dict(sd), design).cuda()
    plain = build_model(dict(sd), {"trainer": "CoOp", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0}).cuda()
    vpt_model = build_model(dict(sd), {"trainer": "VPT", "vision_depth": DEPTH, "vision_ctx": N_CTX, "language_depth": 0, "language_ctx": 0}).cuda()
    sd16 = {k: (v.cuda().half() if v.is_floating_point() else v.cuda()) for k, v in sd.items()}
    pl = promptsrcfit.init_params(model, seed=0)
    g = torch.Generator().manual_seed(1)
    images = torch.randn(BATCH, 3, 224, 224, generator=g).half().cuda()
    lr = torch.full((1,), LR, device="cuda")
    out = {"geometry": GEOM, "n_ctx": N_CTX, "depth": DEPTH, "weights": [25.0, 10.0, 1.0], "batch": BATCH, "device": torch.cuda.get_device_name(0), "steps": []}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")

    if a.scale_table:
        ids = syn.synthetic_token_ids(CLASSES[0], GEOM, seed=0)
        labels = torch.randint(0, CLASSES[0], (BATCH,), generator=g)
        table = []
        for e in (0, 4, 8, 10, 12, 14, 16):
            teacher = plain.text_features_f32(ids.cuda())
            loss, grads, stats = promptsrcfit.gradients(model, pl, images, labels, ids, teacher, grad_scale=2.0 ** e, return_operand_stats=True)
            shown = ("ctx", "transformer.resblocks.1.VPT_shallow", f"transformer.resblocks.{DEPTH - 1}.VPT_shallow", "visual.VPT",
                     f"visual.transformer.resblocks.{DEPTH - 1}.VPT_shallow")
            row = {"grad_scale": f"2^{e}", "loss": [float(v) for v in loss], "grad_finite": all(bool(torch.isfinite(t).all()) for t in grads.values()),
                   "grad_norm": {k: float(grads[k].norm()) for k in shown}}
            for tower, s in stats.items():
                row[tower] = {"elements": s["elements"], "zero_share": s["zeros"] / s["elements"], "subnormal_share": s["subnormals"] / s["elements"],
                              "max": s["max"], "headroom_log2": math.log2(65504.0 / s["max"]) if 0 < s["max"] < float("inf") else None}
            table.append(row)
            print("promptsrcfit-parity: grad_scale " + json.dumps(row), flush=True)
        out["grad_scale_table"] = table
        save()
    for Cn in CLASSES:
        ids = syn.synthetic_token_ids(Cn, GEOM, seed=0)
        labels = torch.randint(0, Cn, (BATCH,), generator=g).cuda()
        r = {"classes": Cn}
        teacher = plain.text_features_f32(ids.cuda())
        for name, one_call in (("separate_calls", False), ("one_call", True)):
            st = promptsrcfit.PromptSRCFitState(model, ids, pl, teacher)
            r[f"promptsrc_step_ms_{name}"] = median_ms(lambda: st.step(images, labels, lr, one_call=one_call), a.iters, a.warmup)
        r["losses"] = [float(v) for v in st.last_losses]
        r["frozen_forward_ms"] = median_ms(lambda: st.towers.frozen(images), a.iters, a.warmup)
        r["text_stash_bytes"], r["vision_stash_bytes"] = st.towers.text.stash.numel(), st.towers.vision.stash.numel()
        with torch.no_grad():
            feats = plain.image_features_f32(images)
        coop = coopfit.CoOpFitState(plain, ids, pl["ctx"])
        r["coop_step_ms"] = median_ms(lambda: coop.step(feats, labels, lr), a.iters, a.warmup)
        text = torch.randn(Cn, syn.GEOMETRIES[GEOM].embed_dim, generator=g).cuda()
        vpt = vptfit.VPTFitState(vpt_model, text)
        r["vpt_step_ms"] = median_ms(lambda: vpt.step(images, labels, lr), a.iters, a.warmup)
        r["promptsrc_over_coop_plus_vpt_plus_frozen"] = r["promptsrc_step_ms_separate_calls"] / (r["coop_step_ms"] + r["vpt_step_ms"] + r["frozen_forward_ms"])
        del coop, vpt
        print(json.dumps(r), flush=True)
        out["steps"].append(r)
        save()
        if not a.no_torch:
            t = dict(classes=Cn, baseline="torch fp16 autograd + SGD over the torch mirror", **time_torch(sd16, ids, pl, images, labels, teacher, a.iters, a.warmup))
            out["steps"].append(t)
            print(json.dumps(t), flush=True)
            save()
        if not a.no_kernels:
            st = promptsrcfit.PromptSRCFitState(model, ids, pl, teacher)
            k = kernel_shares(lambda: st.step(images, labels, lr))
            r["kernel_time_us"], r["kernels"] = k["kernel_time_us"], k["kernels"]
            r["new_kernels"] = [row for row in k["kernels"] if any(n in row["kernel"] for n in NEW_KERNELS)]
            print(json.dumps({"classes": Cn, "new_kernels": r["new_kernels"]}), flush=True)
            print(json.dumps({"classes": Cn, "top": k["kernels"][:8]}), flush=True)
            save()
        del st
    save()


if __name__ == "__main__":
    main()
