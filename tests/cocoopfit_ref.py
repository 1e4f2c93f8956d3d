"""Reference of CoCoOp's training path (clip_calibration_amd/cocoopfit.py, csrc/cocoop_train.hip).  It imports none of the package's kernels.

(1) A no-autograd restatement, in whatever dtype it is given, of the meta-net, the per-image prompt assembly, the per-pair loss head with
its backward, and the reduce of the tower's input gradient into the five gradients with the meta-net's backward written out by hand -- on
``coopfit_ref``'s tower or, for the comparison with (2) at 1e-9, on ``prodafit_ref.island_tower``, which keeps the oracle's two fp32
islands.  (2) The truth: torch autograd through ``oracle.clip_oracle.coop_prompts`` and ``text_encoder``, composed image by image as
``oracle.clip_oracle.cocoop_forward`` composes them, with the cross-entropy of the reference's train mode (cocoop.py:186-202).  The cases
of the test files are at the bottom."""
import functools
import math

import torch

import coopfit_ref as ref
import prodafit_ref as dref
from clip_calibration_amd import synthetic as syn     # weights and geometry only (no library call)
from oracle import clip_oracle as orc

LOGIT_SCALE = ref.LOGIT_SCALE
NAMES = ("ctx", "meta_net.linear1.weight", "meta_net.linear1.bias", "meta_net.linear2.weight", "meta_net.linear2.bias")
MARGIN = 1e-2      # every float64 pre-activation of a case has |a| >= MARGIN max|a|: no ReLU flips between precisions


def unit(t):
    return t / t.norm(dim=-1, keepdim=True)


# ------------------------------------------------------------------------------------------------------------------ (1) the restatement
def meta(feats, p):
    """(x [B, E], a [B, H], hid [B, H], pi [B, D]) of the meta-net on raw features."""
    x = unit(feats)
    a = x @ p[NAMES[1]].t() + p[NAMES[2]]
    hid = a.clamp(min=0)
    return x, a, hid, hid @ p[NAMES[3]].t() + p[NAMES[4]]


def assemble(emb, ctx, pi):
    """prompts [B C, L, D], image-major: row 0 and the rows behind the context from emb [C, L, D], rows 1 .. n_ctx = ctx + pi[b]."""
    C, L, D = emb.shape
    B, n_ctx = pi.shape[0], ctx.shape[0]
    out = emb.to(ctx.dtype).unsqueeze(0).repeat(B, 1, 1, 1)
    for b in range(B):
        for c in range(C):
            for j in range(n_ctx):
                out[b, c, 1 + j] = ctx[j] + pi[b]
    return out.reshape(B * C, L, D)


def head(feats, labels, text, scale):
    """(loss, d loss / d text [B C, E], row losses [B], logits [B, C]) for raw text features [B C, E]: every pair has its own text row."""
    B, E = feats.shape
    C = text.shape[0] // B
    x = unit(feats)
    t = text.reshape(B, C, E)
    nt = t.norm(dim=-1, keepdim=True)
    u = t / nt
    z = scale * (x[:, None] * u).sum(-1)
    ar = torch.arange(B)
    rows = torch.logsumexp(z, dim=-1) - z[ar, labels]
    dz = torch.softmax(z, dim=-1)
    dz[ar, labels] -= 1.0
    dz = dz / B
    v = scale * dz[:, :, None] * x[:, None]
    d = (v - u * (u * v).sum(-1, keepdim=True)) / nt
    return rows.mean(), d.reshape(B * C, E), rows, z


def reduce(d_embed, x, hid, w2, B, C, n_ctx):
    """The five gradients from d_embed [B C, L, D]: classes, images and context rows in ascending order; torch's relu backward is zero
    where the OUTPUT is zero."""
    D = d_embed.shape[-1]
    g = d_embed.reshape(B, C, -1, D)
    dcs = torch.zeros(B, n_ctx, D, dtype=d_embed.dtype)
    for c in range(C):
        dcs = dcs + g[:, c, 1:1 + n_ctx]
    dctx, dpi = torch.zeros(n_ctx, D, dtype=d_embed.dtype), torch.zeros(B, D, dtype=d_embed.dtype)
    for b in range(B):
        dctx = dctx + dcs[b]
    for j in range(n_ctx):
        dpi = dpi + dcs[:, j]
    db2, dw2 = torch.zeros(D, dtype=d_embed.dtype), torch.zeros(D, hid.shape[1], dtype=d_embed.dtype)
    for b in range(B):
        db2 = db2 + dpi[b]
        dw2 = dw2 + dpi[b][:, None] * hid[b][None, :]
    dhid = (hid > 0).to(d_embed.dtype) * (dpi @ w2)
    db1, dw1 = torch.zeros(hid.shape[1], dtype=d_embed.dtype), torch.zeros(hid.shape[1], x.shape[1], dtype=d_embed.dtype)
    for b in range(B):
        db1 = db1 + dhid[b]
        dw1 = dw1 + dhid[b][:, None] * x[b][None, :]
    return dict(zip(NAMES, (dctx, dw1, db1, dw2, db2)))


def restated(sd, ids, params, feats, labels, logit_scale=LOGIT_SCALE, dtype=torch.float64, islands=False):
    """loss, the five gradients, logits, text and the meta-net's parts by the restatement; ``islands``: on ``prodafit_ref.island_tower``."""
    sd_c, ids_c = ref.cut(sd, ids)
    p = {k: params[k].to(dtype) for k in NAMES}
    f = feats.to(dtype)
    B, C, n_ctx = f.shape[0], ids.shape[0], p["ctx"].shape[0]
    x, a, hid, pi = meta(f, p)
    emb = sd["token_embedding.weight"][ids_c].to(dtype)
    eot = ids_c.argmax(dim=-1).repeat(B)
    text, backward = (dref.island_tower if islands else dref.tower)(sd_c, assemble(emb, p["ctx"], pi), eot, dtype)
    loss, d_text, rows, z = head(f, labels, text, math.exp(logit_scale))
    grads = reduce(backward(d_text), x, hid, p[NAMES[3]], B, C, n_ctx)
    return {"loss": float(loss), "grads": grads, "logits": z, "text": text, "x": x, "a": a, "hid": hid, "pi": pi, "rows": rows}


def sgd_steps(params, grads_per_step, rates, momentum, dampening, weight_decay, nesterov):
    """torch.optim.SGD over the five tensors with one set of hyper-parameters, by ``coopfit_ref.sgd_step`` on each."""
    w = {k: params[k].clone() for k in NAMES}
    buf = {k: None for k in NAMES}
    for step, (g, lr) in enumerate(zip(grads_per_step, rates)):
        for k in NAMES:
            w[k], buf[k] = ref.sgd_step(w[k], buf[k], g[k], lr, momentum, dampening, weight_decay, nesterov, step == 0)
    return w


# ------------------------------------------------------------------------------------------------------------------------- (2) the truth
def oracle_parts(sd, ids, params, feats, labels, logit_scale=LOGIT_SCALE, dtype=torch.float64):
    """loss, the five gradients and the logits by torch autograd through the oracle's pieces in ``dtype``, composed as
    ``oracle.clip_oracle.cocoop_forward`` composes them (the image features given instead of encoded), in train mode with labels."""
    sd_c, ids_c = ref.cut(sd, ids)
    p = {k: params[k].detach().to(dtype).clone().requires_grad_(True) for k in NAMES}
    f = orc.l2_normalize(feats.to(dtype))
    hid = torch.relu(f @ p[NAMES[1]].t() + p[NAMES[2]])
    bias = hid @ p[NAMES[3]].t() + p[NAMES[4]]
    logits = []
    for b in range(f.shape[0]):
        tf = orc.text_encoder(sd_c, orc.coop_prompts(sd_c, ids_c, p["ctx"] + bias[b], dtype), ids_c, dtype)
        logits.append(math.exp(logit_scale) * f[b] @ orc.l2_normalize(tf).t())
    z = torch.stack(logits)
    loss = torch.nn.functional.cross_entropy(z.float() if dtype == torch.float16 else z, labels)
    loss.backward()
    return {"loss": float(loss.detach()), "grads": {k: p[k].grad.detach() for k in NAMES}, "logits": z.detach()}


def yardstick_parts(sd, ids, params, feats, labels, logit_scale=LOGIT_SCALE):
    """The same at the reference's own precision (PREC fp16: the meta-net in half as well): the oracle's autograd at float16 on the CPU
    or, where this torch build lacks an fp16 CPU op of that backward (or the result is not finite), the fp32 oracle with weights and
    inputs rounded through fp16.  Returns (parts, how)."""
    half = {k: params[k].half() for k in NAMES}
    try:
        got = oracle_parts(sd, ids, half, feats.half(), labels, logit_scale, torch.float16)
        if all(torch.isfinite(g.float()).all() for g in got["grads"].values()) and math.isfinite(got["loss"]):
            return dict(got, grads={k: g.double() for k, g in got["grads"].items()}), "fp16"
    except RuntimeError:
        pass
    sd16 = {k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()}
    got = oracle_parts(sd16, ids, {k: v.float() for k, v in half.items()}, feats.half().float(), labels, logit_scale, torch.float32)
    return dict(got, grads={k: g.double() for k, g in got["grads"].items()}), "fp32-rounded"


# ------------------------------------------------------------------------------------------------------------------------------- cases
def draw_meta_net(feats, E, H, D, seed):
    """W1, b1, W2, b2 fp32 with every float64 pre-activation |a| >= MARGIN max|a| (redrawn under the next seed until it holds), both
    signs present: some hidden units are off, some on.  pi comes out at the context's own size (0.02)."""
    x = unit(feats.double())
    for k in range(64):
        g = torch.Generator().manual_seed(900 + 64 * seed + k)
        w1 = torch.randn(H, E, generator=g) * (4.0 / math.sqrt(E))
        b1 = 0.1 * torch.randn(H, generator=g)
        w2 = 0.02 * torch.randn(D, H, generator=g)
        b2 = 0.02 * torch.randn(D, generator=g)
        a = x @ w1.double().t() + b1.double()
        if float(a.abs().min()) >= MARGIN * float(a.abs().max()) and bool((a > 0).any()) and bool((a < 0).any()):
            return w1, b1, w2, b2
    raise AssertionError("no meta-net with the margin found")


@functools.lru_cache(maxsize=None)
def make_case(geom, C, n_ctx, B, seed=0, separable=False):
    """dict: sd, ids, params (the five fp32 tensors), feats fp32 [B, E], labels int64 [B]: ``coopfit_ref.make_case`` plus a meta-net."""
    c = ref.make_case(geom, C, n_ctx, B, False, seed, separable=separable)
    g = syn.GEOMETRIES[geom]
    E, D = g.embed_dim, g.transformer_width
    w1, b1, w2, b2 = draw_meta_net(c["feats"], E, max(E // 16, 1), D, seed)
    return {"sd": c["sd"], "ids": c["ids"], "feats": c["feats"], "labels": c["labels"], "params": dict(zip(NAMES, (c["ctx"], w1, b1, w2, b2)))}


# (geometry, C, n_ctx, B): at most 15 prompts
CASES = [("tiny", 3, 4, 1), ("tiny", 5, 4, 3), ("tiny3", 3, 4, 3), ("tiny3", 5, 4, 1)]


def head_case(B, C, E, seed=0):
    """Synthetic rows for the head: B C text rows near C class directions, features whose softmax is not saturated, a wide feature
    matrix to slice a strided view from."""
    g = torch.Generator().manual_seed(B * 1000 + C * 10 + seed)
    wide = torch.randn(B, E + 24, generator=g)
    base = torch.randn(1, C, E, generator=g)
    text = (base + 0.1 * torch.randn(B, C, E, generator=g)).reshape(B * C, E) * 0.3
    y = torch.randint(0, C, (B,), generator=g)
    return wide, text, y


HEAD_SCALE = 10.0
