"""SHA-256 of what the training kernels write, from fixed seeds: one case per kernel family that shares train_rules.h -- the TaskRes step
(SGD and Adam), the adapter step, the loss heads of the three prompt learners, the context step, ProGrad's step, the one-call steps (static, under the
dynamic loss scale and with the class token at the front or in the middle) and the TempScaling fit.  Two builds of the library compute the same thing exactly when every digest is equal.

The library is whichever build CLIPMI_LIBRARY names (default: the in-tree one).  Run it once per build, each in a process of its own,
and compare the files:

    CLIPMI_LIBRARY=/path/to/other/libclipmi.so python tools/train_bits.py --out before.txt
    python tools/train_bits.py --out after.txt
    python tools/train_bits.py --compare before.txt after.txt     # exit status 1 if a digest differs

Every case is small (a few rows, C on both sides of a workgroup's stride, odd E); a row with a label outside [0, C) is part of the
head cases.

``--group fits`` adds the fit states (CoOp, KgCoOp and ProGrad with a generic and CoOp with a class-specific context, ProDA, CoCoOp, VPT,
MaPLe, PromptSRC) on the tests' tiny cases: three steps on every route a state accepts -- static SGD, one call, the dynamic loss scale
(started above fp16's overflow point, so that the first step is skipped), dynamic in one call, Adam, AdamW, Adam under the dynamic scale,
and the sharded step over a local gather with one rank and with two.  A digest covers the losses, the master block, the momentum buffer
or Adam's moments and the scaler's block: two checkouts of the package Python on one library issue the same launches exactly when every
digest is equal.  Measurement only; bench.py does not run it."""
import argparse
import ctypes as C
import hashlib
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))     # the fit states' cases are the tests' (coopfit_ref.make_case and its siblings)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def randn(gen, *shape):
    return torch.randn(*shape, generator=gen).cuda()


def prompt_ids(geom, n_cls, n_ctx):
    """[SOT, X * n_ctx, 0 .. 7 name tokens, EOT, 0 ..]"""
    from clip_calibration_amd import synthetic as syn
    g = syn.GEOMETRIES[geom]
    rng = np.random.RandomState(100)
    ids = np.zeros((n_cls, g.context_length), np.int64)
    for c in range(n_cls):
        k = c % 8
        ids[c, 0] = g.vocab_size - 2
        ids[c, 1:1 + n_ctx] = 1
        ids[c, 1 + n_ctx:1 + n_ctx + k] = rng.randint(2, g.vocab_size - 2, size=k)
        ids[c, 1 + n_ctx + k] = g.vocab_size - 1
    return torch.from_numpy(ids)


def cases():
    """Yields (name, digest)."""
    from clip_calibration_amd import coopfit, fitoptim, ops, synthetic as syn
    from clip_calibration_amd._lib import check, lib
    from clip_calibration_amd.model import build_model

    lr = torch.tensor([0.01], dtype=torch.float32).cuda()
    # TaskRes: rows 5, E 65, C below and above the 256-thread stride
    for Cn in (3, 257):
        for opt in ("sgd", "adam"):
            g = torch.Generator().manual_seed(1)
            f, base, res = randn(g, 5, 65), randn(g, Cn, 65), 0.1 * randn(g, Cn, 65)
            y = torch.randint(0, Cn, (5,), generator=g).cuda()
            s1, s2 = torch.zeros_like(res), torch.zeros_like(res)
            losses = [ops.taskres_train_step(f, y, base, res, s1, s2, lr, 0.5, 100.0, k, opt, 5e-4, 0.9 if opt == "sgd" else 0.0, want_loss=True)
                      for k in range(2)]
            yield f"taskres_step {opt} C={Cn}", digest(res, s1, s2, *losses)
    # the adapter: rows 5, E 64, H 16; C = 1025 takes the 1024-thread stride a second time
    for Cn in (3, 1025):
        g = torch.Generator().manual_seed(2)
        f, text = randn(g, 5, 64), torch.nn.functional.normalize(randn(g, Cn, 64), dim=1)
        w1, w2 = 0.1 * randn(g, 16, 64), 0.1 * randn(g, 64, 16)
        y = torch.randint(0, Cn, (5,), generator=g).cuda()
        m1, m2 = torch.zeros_like(w1), torch.zeros_like(w2)
        losses = [ops.adapter_train_step(f, y, text, w1, w2, m1, m2, lr, 0.2, 100.0, k == 0, 0.9, 0.0, 5e-4, False, want_loss=True) for k in range(2)]
        yield f"adapter_step C={Cn}", digest(w1, w2, m1, m2, *losses)
    # the heads: every mode, B and C on both sides of a stride, E even and odd, the last row's label outside [0, C) where B > 1
    for B in (1, 5):
        for Cn in (2, 257):
            for E in (64, 65):
                g = torch.Generator().manual_seed(3)
                f, text, tea = randn(g, B, E), randn(g, Cn, E), randn(g, Cn, E)
                y = torch.randint(0, Cn, (B,), generator=g)
                if B > 1:
                    y[B - 1] = Cn
                y = y.cuda()
                yield f"coop_head B={B} C={Cn} E={E}", digest(*ops.coop_head(f, y, text, 100.0, 256.0, want16=True))
                for method in ("coop", "kgcoop", "prograd"):
                    losses, d_text, d_kl = ops.prompt_head(f, y, text, 100.0, 256.0, method, None if method == "coop" else tea, 8.0, 2.0)
                    yield f"prompt_head {method} B={B} C={Cn} E={E}", digest(losses, d_text, *(() if d_kl is None else (d_kl,)))
    # the context step and ProGrad's: generic and per-class context, with and without Nesterov
    Cn, L, D, n_ctx = 5, 8, 65, 4
    for per_class in (False, True):
        for nesterov in (False, True):
            g = torch.Generator().manual_seed(4)
            da, db = randn(g, Cn * L, D), -randn(g, Cn * L, D)
            shape = (Cn, n_ctx, D) if per_class else (n_ctx, D)
            tag = f"per_class={int(per_class)} nesterov={int(nesterov)}"
            ctx, buf = randn(g, *shape), torch.zeros(*shape).cuda()
            grads = [ops.ctx_step(da, Cn, n_ctx, per_class, 256.0, ctx, buf, lr, k == 0, 0.9, 0.0, 5e-4, nesterov) for k in range(2)]
            yield "ctx_step " + tag, digest(ctx, buf, *grads)
            ctx, buf = randn(g, *shape), torch.zeros(*shape).cuda()
            out = []
            for k, b in enumerate((db, da - 3.0 * db)):     # a.b > 0, then < 0: the plain gradient and the projected one
                out += list(ops.prograd_step(da, b, Cn, n_ctx, per_class, 256.0, 0.8, ctx, buf, lr, k == 0, 0.9, 0.0, 5e-4, nesterov))
            yield "prograd_step " + tag, digest(ctx, buf, *out)
    # the one-call steps on `tiny`, 3 classes: CoOp's own symbol and every mode of clipmi_prompt_train_step, two steps each
    model = build_model(dict(syn.synthetic_state_dict("tiny", seed=0)), {"trainer": "CoOp"}).cuda()
    ids = prompt_ids("tiny", 3, 4)
    g = torch.Generator().manual_seed(5)
    E = syn.GEOMETRIES["tiny"].embed_dim
    ctx0 = 0.02 * torch.randn(4, syn.GEOMETRIES["tiny"].transformer_width, generator=g)
    f, tea = randn(g, 4, E), randn(g, 3, E)
    y = torch.randint(0, 3, (4,), generator=g).cuda()
    for name, mode in (("coop_train_step", None), ("prompt_train_step coop", 0), ("prompt_train_step kgcoop", 1), ("prompt_train_step prograd", 2)):
        st = coopfit.CoOpFitState(model, ids, ctx0, momentum=0.9, weight_decay=5e-4, grad_scale=256.0)
        t, h = st.tower, model._handle
        losses, grad = torch.zeros(2, 3).cuda(), torch.zeros(2, *ctx0.shape).cuda()
        need = lib.clipmi_prompt_train_step_bytes(h, t.C, t.rows, 4, 2, t.n_ctx, 0)      # ProGrad's: the largest
        ws = torch.empty(need, dtype=torch.uint8).cuda()
        head = (h, C.byref(t.dgrad[0]), t.base.data_ptr(), coopfit._DT[t.base.dtype], st.ctx.data_ptr(), st.buf.data_ptr(), t.n_ctx, 0, t.eot.data_ptr(),
                t.C, t.rows, f.data_ptr(), f.stride(0), y.data_ptr(), 4, st.scale, 256.0)
        tail = (ws.data_ptr(), ws.numel(), t.stash.data_ptr(), t.stash.numel(), ops._stream())
        for k in range(2):
            sgd = (lr.data_ptr(), int(k == 0), 0.9, 0.0, 5e-4, 0)
            with model._launch_lock:
                if mode is None:
                    check(lib.clipmi_coop_train_step(*head, *sgd, losses[k].data_ptr(), grad[k].data_ptr(), *tail), name)
                else:
                    check(lib.clipmi_prompt_train_step(*head, mode, tea.data_ptr(), 8.0, 2.0, 0.8, *sgd, losses[k].data_ptr(), grad[k].data_ptr(), None,
                                                       None, *tail), name)
        yield name, digest(st.ctx, st.buf, losses, grad)
    # the scaled and the placed one-call steps at the same size: generic and class-specific context, uneven name lengths with a 0 among them
    # (prompt_ids gives class c a name of c tokens), a first step that overflows fp16 and is skipped.  ProGrad's digests add projected and dots
    ctx0c = 0.02 * torch.randn(3, 4, syn.GEOMETRIES["tiny"].transformer_width, generator=g)
    plain, skip = {"init_scale": 256.0, "growth_interval": 1}, {"init_scale": 2.0 ** 40, "backoff_factor": 2.0 ** -28}
    runs = [(f"prompt_train_step_scaled {method} per_class={pc}", method, pc, None, plain) for method in ("coop", "kgcoop") for pc in (0, 1)]
    runs += [("prompt_train_step_scaled coop first step skipped", "coop", 0, None, skip)]
    runs += [(f"prompt_train_step_placed {method} {pos}", method, 0, pos, None) for method in ("coop", "kgcoop", "prograd") for pos in ("middle", "front")]
    runs += [(f"prompt_train_step_scaled_placed {method} {pos}", method, 0, pos, plain) for method in ("coop", "kgcoop") for pos in ("middle", "front")]
    for name, method, pc, pos, scaler in runs:
        kw = {"grad_scale": "dynamic", "scaler": scaler} if scaler else {"grad_scale": 256.0}
        st = coopfit.CoOpFitState(model, ids, ctx0c if pc else ctx0, momentum=0.9, weight_decay=5e-4, method=method, teacher=None if method == "coop" else tea,
                                  T=2.0, lam=0.8, class_token_position=pos or "end", name_lens=[0, 1, 2] if pos else None, **kw)
        t, h, mode = st.tower, model._handle, ops.PROMPT_MODES[method]
        block = ops.new_scaler_state(scaler["init_scale"], "cuda") if scaler else None
        cfg = fitoptim._check_scaler(name, scaler)
        sizer = getattr(lib, "clipmi_prompt_train_step" + ("_scaled" if scaler else "") + ("_placed" if pos else "") + "_bytes")
        ws = torch.empty(sizer(h, t.C, t.rows, 4, mode, t.n_ctx, pc), dtype=torch.uint8).cuda()
        losses, grad = torch.zeros(2, 3).cuda(), torch.zeros(2, *st.ctx.shape).cuda()
        projected, dots = torch.zeros(2, dtype=torch.int32).cuda(), torch.zeros(2, 3, dtype=torch.float64).cuda()
        head = (h, C.byref(t.dgrad[0]), t.base.data_ptr(), coopfit._DT[t.base.dtype], st.ctx.data_ptr(), st.buf.data_ptr(), t.n_ctx, pc,
                *((t.position, t.name_lens.data_ptr()) if pos else ()), t.eot.data_ptr(), t.C, t.rows, f.data_ptr(), f.stride(0), y.data_ptr(), 4, st.scale)
        tail = (ws.data_ptr(), ws.numel(), t.stash.data_ptr(), t.stash.numel(), ops._stream())
        for k in range(2):
            out = (losses[k].data_ptr(), grad[k].data_ptr())
            with model._launch_lock:
                if scaler:
                    fn = lib.clipmi_prompt_train_step_scaled_placed if pos else lib.clipmi_prompt_train_step_scaled
                    check(fn(*head, block.data_ptr(), cfg["growth_factor"], cfg["backoff_factor"], cfg["growth_interval"], mode, tea.data_ptr(), 8.0,
                             lr.data_ptr(), 0.9, 0.0, 5e-4, 0, *out, *tail), name)
                else:
                    check(lib.clipmi_prompt_train_step_placed(*head, 256.0, mode, tea.data_ptr(), 8.0, 2.0, 0.8, lr.data_ptr(), int(k == 0), 0.9, 0.0, 5e-4, 0,
                                                              *out, projected[k:].data_ptr(), dots[k].data_ptr(), *tail), name)
        if scaler is skip:
            assert ops.scaler_state_dict(block)["skipped_steps"] == 1 and ops.scaler_state_dict(block)["applied_steps"] == 1, ops.scaler_state_dict(block)
        yield name, digest(st.ctx, st.buf, losses, grad, *((block,) if scaler else ()), *((projected, dots) if method == "prograd" else ()))
    # TempScaling: 37 rows in batches of 16, two epochs, momentum and weight decay
    g = torch.Generator().manual_seed(6)
    cos = torch.tanh(randn(g, 37, 11))
    y = torch.randint(0, 11, (37,), generator=g).cuda()
    state = torch.tensor([math.log(1 / 0.07), 0.0, 0.0, 0.0], dtype=torch.float32).cuda()
    rates = torch.full((6,), 0.01, dtype=torch.float32).cuda()
    losses = ops.tempscale_fit(cos, y, state, rates, 16, 2, 0.9, 0.0, 5e-4, False, want_losses=True)
    yield "tempscale_fit", digest(state, losses)


# the dynamic routes start above fp16's overflow point and fall to 2^8 or 2^11 with the first, skipped step (tests/test_gpu_cocoopshard_ranks.py ROUTES
# has CoCoOp's values, measured on its case; 2^40 overflows whatever the case)
OVER = {"init_scale": 2.0 ** 40, "backoff_factor": 2.0 ** -32}
COCOOP_OVER = {"init_scale": 2.0 ** 16, "backoff_factor": 2.0 ** -5}


def fit_routes(dynamic=True, one_call=True, shard_adam=False, shard_dynamic=False, over=OVER):
    """(route name, constructor arguments, one_call, world) of every route a state accepts."""
    dyn = dict(grad_scale="dynamic", scaler=over)
    routes = [("static", {}, False, 0), ("adam", dict(optimizer="adam"), False, 0), ("adamw", dict(optimizer="adamw"), False, 0)]
    if one_call:
        routes.append(("one_call", {}, True, 0))
    if dynamic:
        routes += [("dynamic", dyn, False, 0), ("adam+dynamic", dict(dyn, optimizer="adam"), False, 0)]
        if one_call:
            routes.append(("dynamic+one_call", dyn, True, 0))
    for world in (1, 2):
        routes.append((f"shard{world}", {}, False, world))
        if shard_dynamic:
            routes.append((f"shard{world} dynamic", dyn, False, world))
        if shard_adam:
            routes.append((f"shard{world} adam", dict(optimizer="adam"), False, world))
    return routes


def fit_cases():
    """Yields (name, digest): three steps of every fit state on every route."""
    import cocoopfit_ref
    import coopfit_ref
    import maplefit_ref
    import prodafit_ref
    import promptsrcfit_ref
    import vptfit_ref
    from clip_calibration_amd import cocoopfit, coopfit, maplefit, prodafit, promptsrcfit, vptfit
    from clip_calibration_amd.model import build_model

    Cn, B, gs = 5, 4, 256.0     # the tests' grad_scale: the synthetic weights give gradients far larger than ViT-B/16's
    fits = []                   # (name, make(**kw), batch, step arguments, routes)
    text_model = {g: build_model(dict(coopfit_ref.state_dict(g)), {"trainer": "CoOp"}).cuda() for g in ("tiny", "tiny3")}
    for name in ("coop", "coop_csc", "kgcoop", "prograd"):
        c, m = coopfit_ref.make_case("tiny", Cn, 4, B, csc=name == "coop_csc"), text_model["tiny"]
        extra = {}
        if name in ("kgcoop", "prograd"):
            extra = dict(method=name, teacher=(torch.randn(Cn, m.geometry.embed_dim, generator=torch.Generator().manual_seed(3)) * 2.0).cuda())
        make = lambda c=c, m=m, extra=extra, **kw: coopfit.CoOpFitState(m, c["ids"], c["ctx"], coopfit_ref.LOGIT_SCALE, **dict(dict(grad_scale=gs), **kw), **extra)
        fits.append((name, make, (c["feats"].cuda(), c["labels"].cuda()), {}, fit_routes(dynamic=name != "prograd")))
    c, m = prodafit_ref.make_case("tiny", Cn, 4, 8, 4, B), text_model["tiny"]
    make = lambda c=c, m=m, **kw: prodafit.ProDAFitState(m, c["ids"], c["ctx"], prompt_bs=4, logit_scale=prodafit_ref.LOGIT_SCALE, **dict(dict(grad_scale=gs), **kw))
    fits.append(("proda", make, (c["feats"].cuda(), c["labels"].cuda()), {"sel": np.array([0, 3, 5, 6])}, fit_routes(shard_dynamic=True)))
    c, m = cocoopfit_ref.make_case("tiny3", 3, 4, 3), text_model["tiny3"]
    make = lambda c=c, m=m, **kw: cocoopfit.CoCoOpFitState(m, c["ids"], c["params"], logit_scale=cocoopfit_ref.LOGIT_SCALE, **dict(dict(grad_scale=gs), **kw))
    fits.append(("cocoop", make, (c["feats"].cuda(), c["labels"].cuda()), {}, fit_routes(shard_adam=True, shard_dynamic=True, over=COCOOP_OVER)))
    c = vptfit_ref.make_case("tiny", 2, 2, B, Cn)
    m = build_model(dict(c["sd"]), {"trainer": "VPT", "vision_depth": 2, "vision_ctx": 2, "language_depth": 0, "language_ctx": 0}).cuda()
    make = lambda c=c, m=m, text=c["text"].cuda(), **kw: vptfit.VPTFitState(m, text, vptfit_ref.LOGIT_SCALE, c["prompts"], **dict(dict(grad_scale=gs), **kw))
    fits.append(("vpt", make, (c["images"].cuda(), c["labels"].cuda()), {}, fit_routes(shard_adam=True, shard_dynamic=True)))
    c = maplefit_ref.make_case("tiny3", 2, 1, Cn, B)
    m = build_model(dict(c["sd"]), maplefit_ref.design(1)).cuda()
    make = lambda c=c, m=m, **kw: maplefit.MaPLeFitState(m, c["ids"], c["pl"], maplefit_ref.LOGIT_SCALE, seq_rows=maplefit_ref.live_rows(c["ids"], False),
                                                         **dict(dict(grad_scale=gs), **kw))
    fits.append(("maple", make, (c["images"].cuda(), c["labels"].cuda()), {}, fit_routes(shard_adam=True, shard_dynamic=True)))
    c = promptsrcfit_ref.make_case("tiny", 2, 2, 3, 2, Cn, B)
    m = build_model(dict(c["sd"]), promptsrcfit_ref.design(3, 2, 2, 2)).cuda()
    make = lambda c=c, m=m, teacher=c["teacher"].cuda(), **kw: promptsrcfit.PromptSRCFitState(
        m, c["ids"], c["p"], teacher, promptsrcfit_ref.LOGIT_SCALE, seq_rows=promptsrcfit_ref.live_rows(c["ids"], True), **dict(dict(grad_scale=gs), **kw))
    fits.append(("promptsrc", make, (c["images"].cuda(), c["labels"].cuda()), {}, fit_routes(shard_adam=True, shard_dynamic=True)))

    lr = torch.tensor([2e-3, 1e-3, 5e-4], dtype=torch.float32).cuda()
    for name, make, batch, step_kw, routes in fits:
        for route, kw, one_call, world in routes:
            if world:
                local = coopfit.LocalGather(world)
                st = [make(shard=coopfit.Shard(world, r, local), **kw) for r in range(world)][0]      # a step of one steps them all
            else:
                st = make(**kw)
            call = dict(step_kw, want_loss=True, **({"one_call": True} if one_call else {}))
            losses = torch.cat([st.step(*batch, lr[k:k + 1], **call) for k in range(3)])
            torch.cuda.synchronize()
            if st.dynamic:
                assert st.scaler_state()["skipped_steps"] >= 1 and st.scaler_state()["applied_steps"] >= 1, (name, route, st.scaler_state())
            moments = (st.buf,) if st._adam is None else (st._adam.exp_avg, st._adam.exp_avg_sq)
            yield f"fit {name} {route}", digest(losses, st._master(), *moments, *((st._scaler.block,) if st.dynamic else ()))


def read(path):
    return dict(line.rstrip("\n").rsplit("  ", 1) for line in open(path) if line.strip())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--group", choices=("kernels", "fits", "all"), default="kernels", help="the kernel families (the default), the fit states, or both")
    ap.add_argument("--compare", nargs=2, metavar=("BEFORE", "AFTER"))
    a = ap.parse_args()
    if a.compare:
        before, after = read(a.compare[0]), read(a.compare[1])
        names = list(before) + [n for n in after if n not in before]
        equal = [n for n in names if before.get(n) == after.get(n)]
        for n in names:
            print(f"{'equal ' if n in equal else 'DIFFER'}  {n}  {before.get(n, '-')}  {after.get(n, '-')}")
        print(f"{len(equal)} of {len(names)} digests equal")
        sys.exit(0 if len(equal) == len(names) else 1)
    groups = [g for g, on in ((cases, a.group != "fits"), (fit_cases, a.group != "kernels")) if on]
    lines = [f"{name}  {value}" for group in groups for name, value in group()]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
