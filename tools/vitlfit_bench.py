"""Time of one MaPLe and one PromptSRC training step at ViT-L/14 on the device with the library option ``vision_train_long`` on (the image
tower's training path beyond 224 token rows per image: csrc/vision_backward.hip with clipmi_attention_backward_long), against a torch fp16
autograd + SGD step over the torch mirror on the same GPU in the same process, and of clipmi_attention_backward_long alone.  Measurement
only; bench.py does not run it.

ViT-L/14's towers with synthetic weights (``synthetic.GEOMETRIES["ViT-L/14"]``: width 1024, 24 layers, 257 tokens), 100 classes, batch 4 of
preprocessed fp16 images.  The training forward's patch embedding serves patches of 8, 16 and 32 pixels and refuses 14, so the tower that is
timed reaches the same 257 tokens as 16 x 16 patches of 16 pixels at 256 px: everything behind conv1 is ViT-L/14's.
1. MaPLe's configuration (n_ctx 2, depth 9; 259 rows per image) and PromptSRC's (nt = nv = 4, depths 9 / 9; 261 rows): the median, the
   minimum and the maximum of --iters steps after --warmup, each between two device events, through the separate calls; the stash and
   workspace bytes of the image tower and ``clipmi_vision_train_bytes`` per image.
2. baseline: ``oracle.clip_oracle`` with the state dict on the GPU at float16, ``backward`` and ``torch.optim.SGD.step``.
3. the operator alone at N H = 64 items (N = 4, H = 16): L = 259 and 581, and L = 205 beside clipmi_attention_backward_full on the same
   inputs (what streaming costs where both run); median, minimum and maximum of --op-iters launches.

Usage: python tools/vitlfit_bench.py [--iters 5] [--warmup 2] [--op-iters 20] [--no-torch] [--out profiles/vitlfit_bench.json]"""
import argparse
import dataclasses
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clip_calibration_amd import _lib, maplefit, ops, promptsrcfit, synthetic as syn, vptfit  # noqa: E402
from clip_calibration_amd._lib import lib  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

GEOM, BATCH, CLASSES = "ViT-L/14", 4, 100
PATCH, RESOLUTION = 16, 256      # 257 tokens through a patch size the training forward serves
MAPLE = dict(n_ctx=2, depth=9, lr=0.0035)
SRC = dict(n_ctx=4, depth=9, lr=0.0025)


def timed_ms(step, iters, warmup):
    ms = []
    for k in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "steps": iters}


def torch_maple(sd16, ids, pl, images, labels, iters, warmup):
    from oracle import clip_oracle as orc
    p = {n: torch.nn.Parameter(pl[n].half().cuda()) for n in maplefit.param_names(MAPLE["depth"])}
    opt = torch.optim.SGD(list(p.values()), lr=MAPLE["lr"], momentum=0.9, weight_decay=5e-4)
    ids = ids.cuda()

    def step():
        with torch.device("cuda"):
            prompts, shared, deep_t, deep_v = orc.maple_prompt_learner(sd16, ids, p, torch.float16)
            tf = orc.text_encoder(sd16, prompts, ids, torch.float16, deep_t, MAPLE["n_ctx"])
            f = orc.encode_image(sd16, images, torch.float16, shared, deep_v)
            logits = math.exp(4.6052) * (f / f.norm(dim=-1, keepdim=True)) @ (tf / tf.norm(dim=-1, keepdim=True)).t()
            loss = torch.nn.functional.cross_entropy(logits.float(), labels)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
    return timed_ms(step, iters, warmup)


def torch_promptsrc(sd16, ids, pl, images, labels, teacher, iters, warmup):
    from oracle import clip_oracle as orc
    F = torch.nn.functional
    n, depth = SRC["n_ctx"], SRC["depth"]
    p = {k: torch.nn.Parameter(v.half().cuda()) for k, v in pl.items()}
    opt = torch.optim.SGD(list(p.values()), lr=SRC["lr"], momentum=0.9, weight_decay=5e-4)
    ids = ids.cuda()
    deep_t = [p[f"transformer.resblocks.{i}.VPT_shallow"] for i in range(1, depth)]
    deep_v = [p[f"visual.transformer.resblocks.{i}.VPT_shallow"] for i in range(1, depth)]
    o = (teacher / teacher.norm(dim=-1, keepdim=True)).half()

    def step():
        with torch.device("cuda"):
            tf = orc.text_encoder(sd16, orc.coop_prompts(sd16, ids, p["ctx"], torch.float16), ids, torch.float16, deep_t, n)
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
    return timed_ms(step, iters, warmup)


def operator_times(iters, warmup):
    N, H = 4, 16
    D = 64 * H
    rows = []
    g = torch.Generator().manual_seed(3)
    for L in (205, 259, 581):
        qkv = (torch.randn(N * L, 3 * D, generator=g) * 0.7).half().cuda()
        do = (torch.randn(N * L, D, generator=g) * 0.5).half().cuda()
        out = torch.empty_like(qkv)
        ws = torch.empty(lib.clipmi_attention_backward_long_bytes(N, L, H), dtype=torch.uint8, device="cuda")
        r = {"items": N * H, "L": L, "attention_backward_long": timed_ms(lambda: ops.attention_backward_long(qkv, do, N, H, out, ws), iters, warmup)}
        if L <= 224:
            def full():
                _lib.check(lib.clipmi_attention_backward_full(qkv.data_ptr(), do.data_ptr(), out.data_ptr(), N, L, H, ops._stream()),
                           "clipmi_attention_backward_full")
            r["attention_backward_full"] = timed_ms(full, iters, warmup)
            r["long_over_full"] = r["attention_backward_long"]["median_ms"] / r["attention_backward_full"]["median_ms"]
        print(json.dumps(r), flush=True)
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--op-iters", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    _lib.set_option("vision_train_long", 1)
    geom = dataclasses.replace(syn.GEOMETRIES[GEOM], vision_patch_size=PATCH, image_resolution=RESOLUTION)
    name = f"{GEOM} towers, patch {PATCH} at {RESOLUTION} px"
    out = {"geometry": name, "classes": CLASSES, "batch": BATCH, "device": torch.cuda.get_device_name(0), "option": {"vision_train_long": 1},
           "tokens": geom.grid ** 2 + 1, "operator": [], "steps": []}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")

    out["operator"] = operator_times(a.op_iters, 3)
    save()
    sd = syn.synthetic_state_dict(geom, seed=0)
    sd16 = {k: (v.cuda().half() if v.is_floating_point() else v.cuda()) for k, v in sd.items()}
    g = torch.Generator().manual_seed(1)
    images = torch.randn(BATCH, 3, geom.image_resolution, geom.image_resolution, generator=g).half().cuda()
    ids = syn.synthetic_token_ids(CLASSES, geom, seed=0)
    labels = torch.randint(0, CLASSES, (BATCH,), generator=g).cuda()

    # MaPLe
    model = build_model(dict(sd), {"trainer": "MaPLe", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0,
                                   "maple_length": MAPLE["n_ctx"]}).cuda()
    pl = maplefit.init_learner_params(model, MAPLE["n_ctx"], MAPLE["depth"], seed=0)
    lr = torch.full((1,), MAPLE["lr"], device="cuda")
    st = maplefit.MaPLeFitState(model, ids, pl)
    r = {"fit": "MaPLe", **MAPLE, "rows_per_image": out["tokens"] + MAPLE["n_ctx"], "device_step": timed_ms(lambda: st.step(images, labels, lr), a.iters, a.warmup)}
    r["vision_stash_bytes"], r["vision_workspace_bytes"] = st.towers.vision.stash.numel(), st.towers.vision.ws.numel()
    ws1, st1 = vptfit.stash_bytes(model, 1, MAPLE["n_ctx"])
    r["vision_train_bytes_per_image"] = {"workspace": ws1, "stash": st1}
    del st
    if not a.no_torch:
        r["torch_step"] = torch_maple(sd16, ids, pl, images, labels, a.iters, a.warmup)
        r["torch_over_device"] = r["torch_step"]["median_ms"] / r["device_step"]["median_ms"]
    print(json.dumps(r), flush=True)
    out["steps"].append(r)
    save()
    del model
    torch.cuda.empty_cache()

    # PromptSRC
    n, depth = SRC["n_ctx"], SRC["depth"]
    model = build_model(dict(sd), {"trainer": "IVLP", "vision_depth": depth, "language_depth": depth, "vision_ctx": n, "language_ctx": n}).cuda()
    plain = build_model(dict(sd), {"trainer": "CoOp", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0}).cuda()
    pl = promptsrcfit.init_params(model, seed=0)
    teacher = plain.text_features_f32(ids.cuda())
    lr = torch.full((1,), SRC["lr"], device="cuda")
    st = promptsrcfit.PromptSRCFitState(model, ids, pl, teacher)
    r = {"fit": "PromptSRC", **SRC, "weights": [25.0, 10.0, 1.0], "rows_per_image": out["tokens"] + n,
         "device_step": timed_ms(lambda: st.step(images, labels, lr), a.iters, a.warmup)}
    r["vision_stash_bytes"], r["vision_workspace_bytes"] = st.towers.vision.stash.numel(), st.towers.vision.ws.numel()
    ws1, st1 = vptfit.stash_bytes(model, 1, n)
    r["vision_train_bytes_per_image"] = {"workspace": ws1, "stash": st1}
    del st
    if not a.no_torch:
        r["torch_step"] = torch_promptsrc(sd16, ids, pl, images, labels, teacher, a.iters, a.warmup)
        r["torch_over_device"] = r["torch_step"]["median_ms"] / r["device_step"]["median_ms"]
    print(json.dumps(r), flush=True)
    out["steps"].append(r)
    save()


if __name__ == "__main__":
    main()
