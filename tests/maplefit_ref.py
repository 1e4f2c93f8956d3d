"""Reference of MaPLe's training path (clip_calibration_amd/maplefit.py, csrc/maple_train.hip, the deep-prompt entry points of
csrc/text_backward.hip, the joint head of csrc/prompt_train.hip).  It does not import the package's library.

(1) A hand-written torch restatement, in whatever dtype it is given (float64 in the tests), of what the kernels implement beyond
coopfit_ref's text blocks and vptfit_ref's image tower: the text tower's deep-prompt splice and its reduction, the coupling functions
forward and backward, the joint head and the master block's layout -- no autograd inside.  (2) The truth: torch autograd through
``oracle.clip_oracle.maple_prompt_learner`` + ``text_encoder(deep_prompts=...)`` + ``encode_image(shared_ctx, deep_prompts)``; every
``.half()`` cast is applied to the VALUE and the gradient passes straight through.  The case list is at the bottom."""
import math

import torch

import coopfit_ref as cref
import prodafit_ref as dref
import vptfit_ref as vref
from clip_calibration_amd import synthetic as syn     # weights and geometry only (no library call)
from oracle import clip_oracle as orc

LOGIT_SCALE = 4.6052
rel_fro = cref.rel_fro


def h(t):
    """The value rounded through fp16, in t's dtype."""
    return t.half().to(t.dtype)


# --------------------------------------------------------------------------------------------------------------------- the master block
def param_names(depth):
    return (["ctx"] + [f"compound_prompts_text.{i}" for i in range(depth - 1)] + ["proj.weight", "proj.bias"]
            + [f"compound_prompt_projections.{i}.weight" for i in range(depth - 1)] + [f"compound_prompt_projections.{i}.bias" for i in range(depth - 1)])


def depth_of(pl):
    return 1 + len([k for k in pl if k.startswith("compound_prompts_text.")])


def block_floats(n_ctx, depth, Dt, Dv):
    return depth * n_ctx * Dt + depth * Dv * Dt + depth * Dv


def pack(pl, dtype=torch.float32):
    return torch.cat([pl[n].to(dtype).reshape(-1) for n in param_names(depth_of(pl))])


def unpack(block, n_ctx, depth, Dt, Dv):
    shapes = [(n_ctx, Dt)] * depth + [(Dv, Dt), (Dv,)] + [(Dv, Dt)] * (depth - 1) + [(Dv,)] * (depth - 1)
    out, at = {}, 0
    for name, shape in zip(param_names(depth), shapes):
        n = math.prod(shape)
        out[name] = block[at:at + n].reshape(shape)
        at += n
    assert at == block.numel()
    return out


def linear_names(i):
    return ("proj.weight", "proj.bias") if i == 0 else (f"compound_prompt_projections.{i - 1}.weight", f"compound_prompt_projections.{i - 1}.bias")


def text_name(i):
    return "ctx" if i == 0 else f"compound_prompts_text.{i - 1}"


# ------------------------------------------------------------------------------------------------------------------ (1) the restatement
def couple_forward(pl, dtype=torch.float64):
    """vis [depth, n_ctx, Dv]: slot 0 = h(ctx) h(W0)^T + h(b0) (proj is a half Linear), slot i = t_i W_i^T + b_i."""
    out = []
    for i in range(depth_of(pl)):
        wn, bn = linear_names(i)
        t, w, b = pl[text_name(i)].to(dtype), pl[wn].to(dtype), pl[bn].to(dtype)
        if i == 0:
            t, w, b = h(t), h(w), h(b)
        out.append(t @ w.t() + b)
    return torch.stack(out)


def couple_backward(pl, d_vis, dtype=torch.float64):
    """{name: gradient} of the coupling functions from d_vis [depth, n_ctx, Dv]: d_t_i = d_vis[i] W_i, db_i = sum_j d_vis[i][j],
    dW_i = d_vis[i]^T t_i; the roundings of slot 0 pass the gradient straight through and multiply the rounded values."""
    out = {}
    for i in range(depth_of(pl)):
        wn, bn = linear_names(i)
        t, w = pl[text_name(i)].to(dtype), pl[wn].to(dtype)
        if i == 0:
            t, w = h(t), h(w)
        out[text_name(i)] = d_vis[i] @ w
        out[bn] = d_vis[i].sum(0)
        out[wn] = d_vis[i].t() @ t
    return out


def text_forward(sd, ids, ctx, deep, dtype=torch.float64, rows=None):
    """(text features [C, E], stash) of the text tower with ``ctx`` on rows 1 .. n_ctx and h(deep[i - 1]) spliced over them in front of
    block i.  ``rows``: the live token rows per prompt (None: the whole context)."""
    C, Lc = ids.shape
    L = Lc if rows is None else rows
    D = sd["ln_final.weight"].shape[0]
    H, n_ctx, layers = D // 64, ctx.shape[0], cref.n_layers(sd)
    x = (cref.prompts_of(sd, ids, ctx, dtype) + sd["positional_embedding"].to(dtype))[:, :L].reshape(C * L, D)
    ws = [cref.block_weights(sd, i, dtype) for i in range(layers)]
    stashes = []
    for i in range(layers):
        if 1 <= i <= len(deep):
            x = splice(x, deep[i - 1].to(dtype), C, L, n_ctx)
        x, st = cref.block_forward(x, ws[i], C, L, H)
        stashes.append(st)
    eot_rows = torch.arange(C) * L + ids.argmax(dim=-1)
    gamma, beta, proj = sd["ln_final.weight"].to(dtype), sd["ln_final.bias"].to(dtype), sd["text_projection"].to(dtype)
    text = cref.ln_forward(x[eot_rows], gamma, beta) @ proj
    return text, {"blocks": stashes, "ws": ws, "x_final": x, "eot_rows": eot_rows, "C": C, "L": L, "H": H, "n_ctx": n_ctx, "n_deep": len(deep)}


def splice(x, deep, C, L, n_ctx):
    """Rows 1 .. n_ctx of every prompt of x [C L, D] overwritten with h(deep) [n_ctx, D]."""
    x = x.reshape(C, L, -1).clone()
    x[:, 1:1 + n_ctx] = h(deep)
    return x.reshape(C * L, -1)


def splice_reduce(g, C, L, n_ctx):
    """(sum over the prompts of g's rows 1 .. n_ctx, g with those rows zeroed)."""
    g = g.reshape(C, L, -1).clone()
    out = g[:, 1:1 + n_ctx].sum(0)
    g[:, 1:1 + n_ctx] = 0
    return out, g.reshape(C * L, -1)


def text_backward(sd, st, d_text, dtype=torch.float64):
    """(d_ctx [n_ctx, D], [d_deep_i]) from d_text [C, E]: the tail, the blocks last to first with the splice reduction behind block i's
    backward, ctx from the rows 1 .. n_ctx of the input's gradient."""
    C, L, H, n_ctx = st["C"], st["L"], st["H"], st["n_ctx"]
    gamma, proj = sd["ln_final.weight"].to(dtype), sd["text_projection"].to(dtype)
    g = torch.zeros_like(st["x_final"])
    g[st["eot_rows"]] = cref.ln_backward(st["x_final"][st["eot_rows"]], gamma, d_text.to(dtype) @ proj.t())
    d_deep = [None] * st["n_deep"]
    for i in reversed(range(len(st["blocks"]))):
        g = cref.block_backward(g, st["blocks"][i], st["ws"][i], C, L, H)
        if 1 <= i <= st["n_deep"]:
            d_deep[i - 1], g = splice_reduce(g, C, L, n_ctx)
    return cref.ctx_gradient(g, C, L, n_ctx, False), d_deep


def joint_head(feats, labels, text, scale):
    """(loss, d loss / d feats, d loss / d text) of mean CE(scale normalise(f) normalise(t)^T, y), the logits formed once."""
    nf, nt = feats.norm(dim=-1, keepdim=True), text.norm(dim=-1, keepdim=True)
    x, u = feats / nf, text / nt
    z = scale * x @ u.t()
    rows = torch.logsumexp(z, dim=-1) - z[torch.arange(z.shape[0]), labels]
    dz = torch.softmax(z, dim=-1)
    dz[torch.arange(z.shape[0]), labels] -= 1.0
    dz = dz / z.shape[0]
    dx, du = scale * dz @ u, scale * dz.t() @ x
    return rows.mean(), (dx - x * (x * dx).sum(-1, keepdim=True)) / nf, (du - u * (u * du).sum(-1, keepdim=True)) / nt


# The oracle keeps two islands of fp32 arithmetic inside a float64 run (its LayerNorm and the softmax of its attention); prodafit_ref
# restates them for the text blocks.  The two towers below run on those island blocks, the splice between them unchanged, so that the
# restatement meets the oracle's float64 autograd at float64 rounding; the image tower's attention is the same island without a mask.
def island_text(sd, ids, ctx, deep, dtype=torch.float64):
    """(text features, d_text -> (d_ctx, [d_deep_i])) on prodafit_ref's island blocks, on the context cut behind the last EOT as the truth
    runs it (coopfit_ref.cut); the oracle normalises every row with ln_final and then takes the EOT rows."""
    sd, ids = cref.cut(sd, ids)
    C, L = ids.shape
    D = sd["ln_final.weight"].shape[0]
    H, n_ctx, layers = D // 64, ctx.shape[0], cref.n_layers(sd)
    x = (cref.prompts_of(sd, ids, ctx, dtype) + sd["positional_embedding"].to(dtype)).reshape(C * L, D)
    ws = [cref.block_weights(sd, i, dtype) for i in range(layers)]
    stashes = []
    for i in range(layers):
        if 1 <= i <= len(deep):
            x = splice(x, deep[i - 1].to(dtype), C, L, n_ctx)
        x, st = dref.island_block_forward(x, ws[i], C, L, H)
        stashes.append(st)
    eot_rows = torch.arange(C) * L + ids.argmax(dim=-1)
    gamma, beta, proj = sd["ln_final.weight"].to(dtype), sd["ln_final.bias"].to(dtype), sd["text_projection"].to(dtype)
    y, ln_f = dref.island_ln_forward(x, gamma, beta)

    def backward(d_text):
        g = torch.zeros_like(x)
        g[eot_rows] = d_text @ proj.t()
        g = dref.island_ln_backward(ln_f, gamma, g)
        d_deep = [None] * len(deep)
        for i in reversed(range(layers)):
            g = dref.island_block_backward(g, stashes[i], ws[i], C, L, H)
            if 1 <= i <= len(deep):
                d_deep[i - 1], g = splice_reduce(g, C, L, n_ctx)
        return cref.ctx_gradient(g, C, L, n_ctx, False), d_deep

    return y[eot_rows] @ proj, backward


def island_vblock_forward(x, w, N, L, H):
    """prodafit_ref.island_block_forward without the causal mask (the image tower's blocks)."""
    D = 64 * H
    h1, ln1 = dref.island_ln_forward(x, w["ln_1.weight"], w["ln_1.bias"])
    qkv = h1 @ w["attn.in_proj_weight"].t() + w["attn.in_proj_bias"]
    q, k, v = (cref.split_heads(t, N, L, H) for t in qkv.reshape(N * L, 3 * D).split(D, dim=-1))
    p32 = torch.softmax(((q @ k.transpose(-1, -2)) / 8.0).float(), dim=-1)
    att = (p32.to(qkv.dtype) @ v).transpose(1, 2).reshape(N * L, D)
    x_mid = x + (att @ w["attn.out_proj.weight"].t() + w["attn.out_proj.bias"])
    h2, ln2 = dref.island_ln_forward(x_mid, w["ln_2.weight"], w["ln_2.bias"])
    h_ = h2 @ w["mlp.c_fc.weight"].t() + w["mlp.c_fc.bias"]
    out = x_mid + (cref.quickgelu(h_) @ w["mlp.c_proj.weight"].t() + w["mlp.c_proj.bias"])
    return out, {"ln1": ln1, "ln2": ln2, "qkv": qkv, "p32": p32, "h": h_}


def island_image(sd, images, vis, dtype=torch.float64):
    """(image features, d_feats -> d_vis [depth, n_ctx, D]) of vptfit_ref's tower on island blocks: ln_pre on every row, ln_post on the
    class rows, the prompt rows' values rounded through fp16; the backward of a block is prodafit_ref's (it never reads the mask)."""
    pr = h(vis.to(dtype))
    depth, n_ctx, D = pr.shape
    x = orc.patch_embed(images.to(dtype), sd["visual.conv1.weight"])
    B = x.shape[0]
    x = torch.cat([sd["visual.class_embedding"].to(dtype).expand(B, 1, -1), x], dim=1) + sd["visual.positional_embedding"].to(dtype)
    L0 = x.shape[1]
    x = torch.cat([x, pr[0].expand(B, -1, -1)], dim=1)
    L, H, layers = L0 + n_ctx, D // 64, vref.n_layers(sd)
    x, ln_pre = dref.island_ln_forward(x, sd["visual.ln_pre.weight"].to(dtype), sd["visual.ln_pre.bias"].to(dtype))
    x = x.reshape(B * L, D)
    ws = [vref.vblock_weights(sd, i, dtype) for i in range(layers)]
    stashes = []
    for i in range(layers):
        if 0 < i < depth:
            x = x.reshape(B, L, D).clone()
            x[:, L0:] = pr[i]
            x = x.reshape(B * L, D)
        x, st = island_vblock_forward(x, ws[i], B, L, H)
        stashes.append(st)
    gamma_post, proj = sd["visual.ln_post.weight"].to(dtype), sd["visual.proj"].to(dtype)
    y, ln_post = dref.island_ln_forward(x.reshape(B, L, D)[:, 0, :], gamma_post, sd["visual.ln_post.bias"].to(dtype))

    def backward(d_feats):
        g = torch.zeros(B, L, D, dtype=dtype)
        g[:, 0] = dref.island_ln_backward(ln_post, gamma_post, d_feats @ proj.t())
        g = g.reshape(B * L, D)
        d_vis = torch.zeros(depth, n_ctx, D, dtype=dtype)
        for i in reversed(range(layers)):
            g = dref.island_block_backward(g, stashes[i], ws[i], B, L, H)
            if 1 <= i < depth:
                g3 = g.reshape(B, L, D).clone()
                d_vis[i] = g3[:, L0:].sum(0)
                g3[:, L0:] = 0
                g = g3.reshape(B * L, D)
        d_vis[0] = dref.island_ln_backward(ln_pre, sd["visual.ln_pre.weight"].to(dtype), g.reshape(B, L, D))[:, L0:].sum(0)
        return d_vis

    return y @ proj, backward


def loss_and_grads(sd, ids, pl, images, labels, logit_scale=LOGIT_SCALE, dtype=torch.float64, rows=None, islands=False):
    """(loss, {name: gradient}) by the restatement: couple, both towers forward, the joint head, both backwards, the coupling backward.
    ``islands``: on the towers that restate the oracle's two fp32 islands (``rows`` is then the truth's own cut)."""
    depth = depth_of(pl)
    deep = [pl[text_name(i)] for i in range(1, depth)]
    vis = couple_forward(pl, dtype)
    if islands:
        text, tback = island_text(sd, ids, pl["ctx"], deep, dtype)
        feats, vback = island_image(sd, images, vis, dtype)
        loss, d_feats, d_text = joint_head(feats, labels, text, math.exp(logit_scale))
        d_ctx, d_deep = tback(d_text)
        grads = couple_backward(pl, vback(d_feats), dtype)
    else:
        text, tst = text_forward(sd, ids, pl["ctx"], deep, dtype, rows)
        feats, vst = vref.forward(sd, images, vis, dtype)
        loss, d_feats, d_text = joint_head(feats, labels, text, math.exp(logit_scale))
        d_ctx, d_deep = text_backward(sd, tst, d_text, dtype)
        grads = couple_backward(pl, vref.backward(sd, vst, d_feats, dtype), dtype)
    grads["ctx"] = grads["ctx"] + d_ctx
    for i in range(1, depth):
        grads[text_name(i)] = grads[text_name(i)] + d_deep[i - 1]
    return loss, grads


# ----------------------------------------------------------------------------------------------------------------------- (2) the truth
def oracle_loss_grads(sd, ids, pl, images, labels, logit_scale=LOGIT_SCALE, dtype=torch.float64, return_logits=False):
    """(loss, {name: gradient}) by torch autograd through the oracle's MaPLe functions in ``dtype``; ``return_logits`` adds the logits [B, C].  The oracle applies ``.half()`` to
    every prompt tensor through its ``_h`` (whose own backward would round the gradient too): the values are rounded here by a function
    whose gradient passes straight through, and ``_h`` is taken out for the call, as vptfit_ref does.  ``proj`` is a half Linear: its
    operands are rounded the same way for ``shared_ctx``; the text side reads ``ctx`` as it is."""
    sd_c, ids_c = cref.cut(sd, ids)
    depth = depth_of(pl)
    p = {n: pl[n].detach().to(dtype).clone().requires_grad_(True) for n in param_names(depth)}
    hv = vref._HalfValue.apply
    half_proj = dict(p, **{n: hv(p[n]) for n in ("ctx", "proj.weight", "proj.bias")})
    assert callable(getattr(orc, "_h", None)), "oracle.clip_oracle._h is gone: restate how the prompts' cast is made transparent"
    keep, orc._h = orc._h, (lambda t, dt: t.to(dt))
    try:
        prompts, _, deep_t, deep_v = orc.maple_prompt_learner(sd_c, ids_c, p, dtype)
        _, shared, _, _ = orc.maple_prompt_learner(sd_c, ids_c, half_proj, dtype)
        tf = orc.text_encoder(sd_c, prompts, ids_c, dtype, [hv(t) for t in deep_t] or None, p["ctx"].shape[0])
        f = orc.encode_image(sd, images.to(dtype), dtype, hv(shared), [hv(v) for v in deep_v])
    finally:
        orc._h = keep
    logits = math.exp(logit_scale) * (f / f.norm(dim=-1, keepdim=True)) @ (tf / tf.norm(dim=-1, keepdim=True)).t()
    loss = torch.nn.functional.cross_entropy(logits.float() if dtype == torch.float16 else logits, labels)
    loss.backward()
    grads = {n: (t.grad.detach() if t.grad is not None else torch.zeros_like(t)) for n, t in p.items()}
    return (loss.detach(), grads, logits.detach()) if return_logits else (loss.detach(), grads)


def yardstick(sd, ids, pl, images, labels, logit_scale=LOGIT_SCALE):
    """(loss, grads, how, logits) of the reference's own precision: the oracle's autograd at float16 on the CPU, or, where this torch build lacks
    an fp16 CPU op of it, the fp32 oracle with weights and inputs rounded through fp16 (coopfit_ref.yardstick_grad's fallback)."""
    try:
        l, g, z = oracle_loss_grads(sd, ids, {k: v.half() for k, v in pl.items()}, images.half(), labels, logit_scale, torch.float16, True)
        if all(torch.isfinite(t.float()).all() for t in g.values()):
            return l.double(), {k: v.double() for k, v in g.items()}, "fp16", z.double()
    except RuntimeError:
        pass
    sd16 = {k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()}
    l, g, z = oracle_loss_grads(sd16, ids, {k: v.half().float() for k, v in pl.items()}, images.half().float(), labels, logit_scale, torch.float32, True)
    return l.double(), {k: v.double() for k, v in g.items()}, "fp32-rounded", z.double()


def logits_of(feats, text, logit_scale=LOGIT_SCALE):
    """exp(logit_scale) normalise(feats) normalise(text)^T in float64."""
    f, t = feats.double(), text.double()
    return math.exp(logit_scale) * (f / f.norm(dim=-1, keepdim=True)) @ (t / t.norm(dim=-1, keepdim=True)).t()


# ------------------------------------------------------------------------------------------------------------------------------- cases
def make_params(geom, n_ctx, depth, seed=0):
    """The prompt learner's parameters, fp32: prompts from N(0, 0.02^2), the Linears as nn.Linear draws them, proj already fp16 values."""
    g = syn.GEOMETRIES[geom]
    Dt, Dv = g.transformer_width, g.vision_width
    gen = torch.Generator().manual_seed(900 + seed)
    pl = {"ctx": 0.02 * torch.randn(n_ctx, Dt, generator=gen)}
    for i in range(depth - 1):
        pl[f"compound_prompts_text.{i}"] = 0.02 * torch.randn(n_ctx, Dt, generator=gen)
    bound = 1.0 / math.sqrt(Dt)
    for i in range(depth):
        wn, bn = linear_names(i)
        pl[wn] = (torch.rand(Dv, Dt, generator=gen) * 2 - 1) * bound
        pl[bn] = (torch.rand(Dv, generator=gen) * 2 - 1) * bound
    pl["proj.weight"], pl["proj.bias"] = pl["proj.weight"].half().float(), pl["proj.bias"].half().float()
    return pl


def make_case(geom, depth, n_ctx, C, B, seed=0):
    """dict: sd, ids [C, context] (prompt 0's EOT directly behind the context rows), pl, images fp32 [B, 3, R, R], labels int64 [B]."""
    g = syn.GEOMETRIES[geom]
    gen = torch.Generator().manual_seed(950 + seed)
    images = torch.randn(B, 3, g.image_resolution, g.image_resolution, generator=gen)
    labels = torch.randint(0, C, (B,), generator=gen)
    return {"geom": geom, "sd": cref.state_dict(geom, seed), "ids": cref.prompt_ids(geom, C, n_ctx, seed), "pl": make_params(geom, n_ctx, depth, seed),
            "images": images, "labels": labels}


def design(n_ctx):
    return {"trainer": "MaPLe", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0, "maple_length": n_ctx}


def live_rows(ids, cut):
    """The library's seq_rows for a case: behind the last EOT rounded up to 8 with the cut, the whole context (0) without."""
    return min(ids.shape[1], (int(ids.argmax(dim=-1).max()) + 1 + 7) // 8 * 8) if cut else 0


# (geometry, depth, n_ctx, C, B, live-row cut): depth 1 (no deep prompt), 2 (one block without a splice on each side) and 3 (full) on tiny3;
# n_ctx 1, 2, 3; C 3 and 5; B 1 and 3; with and without the cut; tiny for Dt = Dv and two text heads
CASES = [
    ("tiny3", 1, 2, 3, 1, True),
    ("tiny3", 2, 1, 5, 3, False),
    ("tiny3", 3, 3, 3, 3, True),
    ("tiny3", 3, 2, 5, 1, False),
    ("tiny", 2, 2, 5, 3, True),
]
