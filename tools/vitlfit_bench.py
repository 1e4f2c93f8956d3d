"""Time of one MaPLe and one PromptSRC training step on ViT-L/14 and ViT-L/14@336px on the device with the library option
``vision_train_long`` on (the image tower's training path beyond 224 token rows per image: csrc/vision_backward.hip with
clipmi_attention_backward_long), against the stand-in tower this tool timed before the training forward took patches of 14 pixels, and
against a torch fp16 autograd + SGD step over the torch mirror on the same GPU, all in the same run and process.  Measurement only;
bench.py does not run it and no time here is a pass criterion.

The towers carry synthetic weights (``synthetic.GEOMETRIES``: width 1024, 24 layers), 100 classes, batch 4 of preprocessed fp16 images.
Per resolution -- ViT-L/14 at 224 px (257 tokens) and ViT-L/14@336px (577 tokens) --:
1. the real geometry, patches of 14 pixels: the training forward's patchify route (csrc/vision_backward.hip: patchify, the dense GEMM with
   the positional epilogue, ln_pre);
2. the stand-in: the same tower with conv1 replaced by patches of 16 pixels at 256 / 384 px, which reaches the same 257 / 577 tokens
   through the im2col-free loader; it differs only in front of ln_pre;
3. baseline: ``oracle.clip_oracle`` on the real geometry with the state dict on the GPU at float16, ``backward`` and
   ``torch.optim.SGD.step``.
For each, MaPLe's configuration (n_ctx 2, depth 9) and PromptSRC's (nt = nv = 4, depths 9 / 9): the median, the minimum and the maximum of
--iters steps after --warmup, each between two device events, through the separate calls; the stash and workspace bytes of the image
tower and ``vptfit.stash_bytes`` per image.
4. the front end alone at batch 4, n_ctx 2, median of --op-iters: patch 14 as clipmi_patchify, the patch GEMM and clipmi_embed_ln without
   the positional add; patch 16 as clipmi_patch_embed and clipmi_embed_ln with it (an fp16 batch needs no cast launch).  The C ABI does not
   export the dense GEMM's positional epilogue on its own, so the patch-14 GEMM is timed as clipmi_gemm_f16 on the same operands, shape
   and fp32 output without the positional add and the row scatter: the same tile kernel and bytes but for the positional rows.
5. with --operator, clipmi_attention_backward_long alone at N H = 64 items (N = 4, H = 16): L = 259 and 581, and L = 205 beside
   clipmi_attention_backward_full on the same inputs.

--out names a JSON file: the new results go under its key ``vit_l14`` (and ``operator`` with --operator); every other key already in
the file stays as it is.

Usage: python tools/vitlfit_bench.py [--iters 5] [--warmup 2] [--op-iters 20] [--no-torch] [--operator] [--only 224|336]
       [--out profiles/vitlfit_bench.json]"""
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

BATCH, CLASSES = 4, 100
# (geometry, the stand-in's patch size and resolution: the same token count through the im2col-free loader)
RUNS = {224: ("ViT-L/14", 16, 256), 336: ("ViT-L/14@336px", 16, 384)}
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


def front_end_times(geom, standin, iters, warmup, n_ctx=2):
    """The launches in front of the first block, alone, on random operands at the towers' shapes (docstring, 4)."""
    D, s = geom.vision_width, ops._stream()
    g = torch.Generator().manual_seed(5)
    dev = lambda t: t.cuda().contiguous()
    out = {"batch": BATCH, "n_ctx": n_ctx, "image_dtype": "fp16"}
    for key, gm in (("patch14", geom), ("patch16_standin", standin)):
        R, P, G = gm.image_resolution, gm.vision_patch_size, gm.grid
        L0 = G * G + 1
        L, K = L0 + n_ctx, 3 * P * P
        kpad = (K + 63) // 64 * 64
        img = dev(torch.randn(BATCH, 3, R, R, generator=g).half())
        w = dev((torch.randn(D, kpad, generator=g) * K ** -0.5).half())
        cls, pos, shallow = dev(torch.randn(D, generator=g)), dev(torch.randn(L0, D, generator=g) * 0.1), dev(torch.randn(n_ctx, D, generator=g))
        gam, bet = dev(torch.ones(D)), dev(torch.zeros(D))
        x0 = torch.zeros(BATCH * L, D, dtype=torch.float32, device="cuda")
        y = torch.empty_like(x0)
        loader = P in (8, 16, 32)

        def ln():
            _lib.check(lib.clipmi_embed_ln(x0.data_ptr(), _lib.F32, int(loader), cls.data_ptr(), pos.data_ptr(), shallow.data_ptr(), gam.data_ptr(),
                                           bet.data_ptr(), y.data_ptr(), None, None, BATCH, L, L0, D, 1e-5, s), "clipmi_embed_ln")
        if loader:
            def embed():
                _lib.check(lib.clipmi_patch_embed(img.data_ptr(), _lib.F16, None, w.data_ptr(), kpad, None, x0.data_ptr(), _lib.F32, BATCH, R, P, D, L, s),
                           "clipmi_patch_embed")
            stages = {"patch_embed": embed, "embed_ln": ln}
        else:
            col = torch.empty(BATCH * G * G, kpad, dtype=torch.float16, device="cuda")
            rows = torch.empty(BATCH * G * G, D, dtype=torch.float32, device="cuda")

            def patchify():
                _lib.check(lib.clipmi_patchify(img.data_ptr(), _lib.F16, col.data_ptr(), BATCH, R, P, kpad, s), "clipmi_patchify")

            def gemm():
                _lib.check(lib.clipmi_gemm_f16(col.data_ptr(), kpad, w.data_ptr(), kpad, None, None, rows.data_ptr(), D, _lib.F32, BATCH * G * G, D, kpad,
                                               _lib.EPI_NONE, s), "clipmi_gemm_f16")
            stages = {"patchify": patchify, "patch_gemm_without_pos": gemm, "embed_ln": ln}
        r = {"patch": P, "resolution": R, "tokens": L0, "kpad": kpad, "launches": len(stages)}
        for name, fn in stages.items():
            r[name] = timed_ms(fn, iters, warmup)

        def together():
            for fn in stages.values():
                fn()
        r["together"] = timed_ms(together, iters, warmup)
        out[key] = r
    return out


def device_fit(sd, ids, images, labels, fit, tokens, iters, warmup):
    """One fit's device step on the tower of ``sd`` -> (record, what the torch baseline needs)."""
    if fit == "MaPLe":
        model = build_model(dict(sd), {"trainer": "MaPLe", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0,
                                       "maple_length": MAPLE["n_ctx"]}).cuda()
        pl = maplefit.init_learner_params(model, MAPLE["n_ctx"], MAPLE["depth"], seed=0)
        lr = torch.full((1,), MAPLE["lr"], device="cuda")
        st = maplefit.MaPLeFitState(model, ids, pl)
        r = {"fit": "MaPLe", **MAPLE}
        n, teacher = MAPLE["n_ctx"], None
    else:
        n, depth = SRC["n_ctx"], SRC["depth"]
        model = build_model(dict(sd), {"trainer": "IVLP", "vision_depth": depth, "language_depth": depth, "vision_ctx": n, "language_ctx": n}).cuda()
        plain = build_model(dict(sd), {"trainer": "CoOp", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0}).cuda()
        pl = promptsrcfit.init_params(model, seed=0)
        teacher = plain.text_features_f32(ids.cuda())
        del plain
        lr = torch.full((1,), SRC["lr"], device="cuda")
        st = promptsrcfit.PromptSRCFitState(model, ids, pl, teacher)
        r = {"fit": "PromptSRC", **SRC, "weights": [25.0, 10.0, 1.0]}
    r["rows_per_image"] = tokens + n
    r["device_step"] = timed_ms(lambda: st.step(images, labels, lr), iters, warmup)
    r["vision_stash_bytes"], r["vision_workspace_bytes"] = st.towers.vision.stash.numel(), st.towers.vision.ws.numel()
    ws1, st1 = vptfit.stash_bytes(model, 1, n)
    r["vision_train_bytes_per_image"] = {"workspace": ws1, "stash": st1}
    del st, model
    torch.cuda.empty_cache()
    return r, pl, teacher


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--op-iters", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--operator", action="store_true")
    ap.add_argument("--only", type=int, choices=sorted(RUNS), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    _lib.set_option("vision_train_long", 1)
    out = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)      # the entries of earlier runs stay
    new = out.setdefault("vit_l14", {})
    new.update({"classes": CLASSES, "batch": BATCH, "device": torch.cuda.get_device_name(0), "option": {"vision_train_long": 1}})
    runs = new.setdefault("runs", {})

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")

    if a.operator:
        out["operator"] = operator_times(a.op_iters, 3)
        save()
    for res in sorted(RUNS) if a.only is None else [a.only]:
        name, sp, sr = RUNS[res]
        geom = syn.GEOMETRIES[name]
        standin = dataclasses.replace(geom, vision_patch_size=sp, image_resolution=sr)
        assert standin.grid == geom.grid
        run = {"geometry": f"{name}, patch {geom.vision_patch_size} at {geom.image_resolution} px",
               "standin": f"{name} towers, patch {sp} at {sr} px", "tokens": geom.vision_tokens, "steps": []}
        run["front_end"] = front_end_times(geom, standin, a.op_iters, 3)
        print(json.dumps(run["front_end"]), flush=True)
        sd = syn.synthetic_state_dict(geom, seed=0)
        gen = torch.Generator().manual_seed(1)
        sd_standin = dict(sd)       # the same tower behind conv1
        sd_standin["visual.conv1.weight"] = (torch.randn(geom.vision_width, 3, sp, sp, generator=gen) * (3 * sp * sp) ** -0.5).half().float()
        images = torch.randn(BATCH, 3, geom.image_resolution, geom.image_resolution, generator=gen).half().cuda()
        images_standin = torch.randn(BATCH, 3, sr, sr, generator=gen).half().cuda()
        ids = syn.synthetic_token_ids(CLASSES, geom, seed=0)
        labels = torch.randint(0, CLASSES, (BATCH,), generator=gen).cuda()
        sd16 = None if a.no_torch else {k: (v.cuda().half() if v.is_floating_point() else v.cuda()) for k, v in sd.items()}
        for fit in ("MaPLe", "PromptSRC"):
            r, pl, teacher = device_fit(sd, ids, images, labels, fit, geom.vision_tokens, a.iters, a.warmup)
            s, _, _ = device_fit(sd_standin, ids, images_standin, labels, fit, geom.vision_tokens, a.iters, a.warmup)
            r["standin_step"] = s["device_step"]
            r["standin_vision_train_bytes_per_image"] = s["vision_train_bytes_per_image"]
            r["device_over_standin"] = r["device_step"]["median_ms"] / s["device_step"]["median_ms"]
            if not a.no_torch:
                if fit == "MaPLe":
                    r["torch_step"] = torch_maple(sd16, ids, pl, images, labels, a.iters, a.warmup)
                else:
                    r["torch_step"] = torch_promptsrc(sd16, ids, pl, images, labels, teacher, a.iters, a.warmup)
                r["torch_over_device"] = r["torch_step"]["median_ms"] / r["device_step"]["median_ms"]
                torch.cuda.empty_cache()
            print(json.dumps(r), flush=True)
            run["steps"].append(r)
            runs[str(res)] = run
            save()
        del sd16
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
