"""Reference of CoOp's training path (clip_calibration_amd/coopfit.py, csrc/text_backward.hip, csrc/prompt_train.hip).  It does not import the package.

Two things live here.  (1) A hand-written torch restatement, in whatever dtype it is given (float64 in the tests), of every backward
formula the kernels implement: LayerNorm, QuickGELU, causal attention, the loss head through both normalisations, the tail (projection,
ln_final, the EOT scatter), one block, the context reduction and torch.optim.SGD's rule -- no autograd inside.  (2) The truth: torch
autograd through ``oracle.clip_oracle.coop_prompts`` and ``text_encoder``, which tests/test_coopfit_cpu.py holds (1) against and the GPU
tests hold the device against.  The case lists of the three test files are at the bottom."""
import math

import numpy as np
import torch

from clip_calibration_amd import synthetic as syn     # weights and geometry only (no library call)
from oracle import clip_oracle as orc

LOGIT_SCALE = 4.6052


# ------------------------------------------------------------------------------------------------------------------ (1) the restatement
def ln_forward(x, gamma, beta, eps=1e-5):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps) * gamma + beta


def ln_backward(x, gamma, dy, eps=1e-5):
    """dX of y = LayerNorm(x) gamma + beta for the upstream dy, row by row."""
    mean = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    xhat = (x - mean) * rstd
    t = dy * gamma
    return rstd * (t - t.mean(-1, keepdim=True) - xhat * (t * xhat).mean(-1, keepdim=True))


def quickgelu(h):
    return h * torch.sigmoid(1.702 * h)


def quickgelu_backward(h, d_a):
    s = torch.sigmoid(1.702 * h)
    return d_a * (s + 1.702 * h * s * (1 - s))


def split_heads(t, N, L, H):
    return t.reshape(N, L, H, 64).transpose(1, 2)          # [N, H, L, 64]


def attention_probs(q, k):
    L = q.shape[-2]
    s = q @ k.transpose(-1, -2) / 8.0
    mask = torch.ones(L, L, dtype=torch.bool).tril()
    return torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1)


def attention_forward(qkv, N, L, H):
    D = 64 * H
    q, k, v = (split_heads(t, N, L, H) for t in qkv.reshape(N * L, 3 * D).split(D, dim=-1))
    return (attention_probs(q, k) @ v).transpose(1, 2).reshape(N * L, D)


def attention_backward(qkv, d_out, N, L, H):
    """dqkv [N L, 3 D] of the causal attention for the upstream d_out [N L, D]: dV = P^T dO, dP = dO V^T,
    dS = P o (dP - rowsum(dP o P)), dQ = dS K / 8, dK = dS^T Q / 8."""
    D = 64 * H
    q, k, v = (split_heads(t, N, L, H) for t in qkv.reshape(N * L, 3 * D).split(D, dim=-1))
    do = split_heads(d_out, N, L, H)
    p = attention_probs(q, k)
    dv = p.transpose(-1, -2) @ do
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    dq = ds @ k / 8.0
    dk = ds.transpose(-1, -2) @ q / 8.0
    return torch.cat([t.transpose(1, 2).reshape(N * L, D) for t in (dq, dk, dv)], dim=-1)


def head(feats, labels, text, scale):
    """(loss, d loss / d text, row losses) of mean CE(scale normalise(f) normalise(t)^T, y)."""
    nf, nt = feats.norm(dim=-1, keepdim=True), text.norm(dim=-1, keepdim=True)
    x, u = feats / nf, text / nt
    z = scale * x @ u.t()
    lse = torch.logsumexp(z, dim=-1)
    rows = lse - z[torch.arange(z.shape[0]), labels]
    dz = torch.softmax(z, dim=-1)
    dz[torch.arange(z.shape[0]), labels] -= 1.0
    dz = dz / z.shape[0]
    du = scale * dz.t() @ x
    d_text = (du - u * (u * du).sum(-1, keepdim=True)) / nt
    return rows.mean(), d_text, rows


def block_weights(sd, i, dtype):
    p = f"transformer.resblocks.{i}."
    names = ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
             "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")
    return {n: sd[p + n].to(dtype) for n in names}


def block_forward(x, w, N, L, H):
    """One residual block on rows [N L, D]; returns (output, stash)."""
    qkv = ln_forward(x, w["ln_1.weight"], w["ln_1.bias"]) @ w["attn.in_proj_weight"].t() + w["attn.in_proj_bias"]
    x_mid = x + attention_forward(qkv, N, L, H) @ w["attn.out_proj.weight"].t() + w["attn.out_proj.bias"]
    h = ln_forward(x_mid, w["ln_2.weight"], w["ln_2.bias"]) @ w["mlp.c_fc.weight"].t() + w["mlp.c_fc.bias"]
    out = x_mid + quickgelu(h) @ w["mlp.c_proj.weight"].t() + w["mlp.c_proj.bias"]
    return out, {"x_in": x, "x_mid": x_mid, "qkv": qkv, "h": h}


def block_backward(g, st, w, N, L, H):
    """The gradient of the block's input rows from the gradient g of its output rows: the eight steps of the device driver."""
    d_a = g @ w["mlp.c_proj.weight"]
    d_h = quickgelu_backward(st["h"], d_a)
    g = g + ln_backward(st["x_mid"], w["ln_2.weight"], d_h @ w["mlp.c_fc.weight"])
    d_att = g @ w["attn.out_proj.weight"]
    dqkv = attention_backward(st["qkv"], d_att, N, L, H)
    return g + ln_backward(st["x_in"], w["ln_1.weight"], dqkv @ w["attn.in_proj_weight"])


def n_layers(sd):
    return len([k for k in sd if k.startswith("transformer.resblocks.") and k.endswith(".attn.in_proj_weight")])


def prompts_of(sd, ids, ctx, dtype):
    emb = sd["token_embedding.weight"][ids].to(dtype)
    n_ctx = ctx.shape[-2]
    c = ctx.to(dtype)
    if c.dim() == 2:
        c = c.unsqueeze(0).expand(ids.shape[0], -1, -1)
    return torch.cat([emb[:, :1], c, emb[:, 1 + n_ctx:]], dim=1)


def loss_and_grad(sd, ids, ctx, feats, labels, logit_scale=LOGIT_SCALE, dtype=torch.float64, rows=None):
    """(loss, d loss / d ctx) by the restatement: forward with a stash, head, tail backward, block backwards, context reduction.
    ``rows``: the live token rows per prompt (None: the whole context)."""
    C, Lc = ids.shape
    L = Lc if rows is None else rows
    D = sd["ln_final.weight"].shape[0]
    H = D // 64
    n_ctx = ctx.shape[-2]
    x = (prompts_of(sd, ids, ctx, dtype) + sd["positional_embedding"].to(dtype))[:, :L].reshape(C * L, D)
    stashes = []
    layers = n_layers(sd)
    ws = [block_weights(sd, i, dtype) for i in range(layers)]
    for i in range(layers):
        x, st = block_forward(x, ws[i], C, L, H)
        stashes.append(st)
    eot_rows = torch.arange(C) * L + ids.argmax(dim=-1)
    gamma, beta, proj = sd["ln_final.weight"].to(dtype), sd["ln_final.bias"].to(dtype), sd["text_projection"].to(dtype)
    text = ln_forward(x[eot_rows], gamma, beta) @ proj
    loss, d_text, _ = head(feats.to(dtype), labels, text, math.exp(logit_scale))
    g = torch.zeros_like(x)                                                   # tail: projection, ln_final, scatter
    g[eot_rows] = ln_backward(x[eot_rows], gamma, d_text @ proj.t())
    for i in reversed(range(layers)):
        g = block_backward(g, stashes[i], ws[i], C, L, H)
    return loss, ctx_gradient(g, C, L, n_ctx, ctx.dim() == 3)


def ctx_gradient(g, C, L, n_ctx, per_class):
    rows = g.reshape(C, L, -1)[:, 1:1 + n_ctx]
    return rows if per_class else rows.sum(0)


def sgd_step(w, buf, grad, lr, momentum, dampening, weight_decay, nesterov, first):
    """torch.optim.SGD's rule in the dtype of its arguments: (w', buf')."""
    if weight_decay != 0:
        grad = grad + weight_decay * w
    if momentum != 0:
        buf = grad.clone() if first else momentum * buf + (1 - dampening) * grad
        grad = grad + momentum * buf if nesterov else buf
    return w - lr * grad, buf


# ------------------------------------------------------------------------------------------------------------------------- (2) the truth
def cut(sd, ids):
    """The same model on a context cut behind the last EOT: the blocks mask causally and only the EOT rows are read (tests/conftest.py
    oracle_text_features), so loss and gradient are those of the whole context, at a fraction of the CPU time."""
    L = int(ids.argmax(dim=-1).max()) + 1
    out = dict(sd)
    out["positional_embedding"] = sd["positional_embedding"][:L].clone()
    return out, ids[:, :L]


def oracle_loss_grad(sd, ids, ctx, feats, labels, logit_scale=LOGIT_SCALE, dtype=torch.float64):
    """(loss, d loss / d ctx) by torch autograd through oracle.clip_oracle.coop_prompts and text_encoder in ``dtype``."""
    sd_c, ids_c = cut(sd, ids)
    c = ctx.detach().to(dtype).clone().requires_grad_(True)
    tf = orc.text_encoder(sd_c, orc.coop_prompts(sd_c, ids_c, c, dtype), ids_c, dtype)
    f = feats.to(dtype)
    logits = math.exp(logit_scale) * (f / f.norm(dim=-1, keepdim=True)) @ (tf / tf.norm(dim=-1, keepdim=True)).t()
    loss = torch.nn.functional.cross_entropy(logits.float() if dtype == torch.float16 else logits, labels)
    loss.backward()
    return loss.detach(), c.grad.detach()


def yardstick_grad(sd, ids, ctx, feats, labels, logit_scale=LOGIT_SCALE):
    """The gradient of the reference's own precision (PREC fp16): the oracle's autograd at dtype float16 on the CPU.  Returns
    (grad, how): how == "fp16" or, where this torch build lacks an fp16 CPU op of that backward, "fp32-rounded" -- the fp32 oracle with the
    weights and the context rounded through fp16."""
    try:
        _, g = oracle_loss_grad(sd, ids, ctx.half(), feats.half(), labels, logit_scale, torch.float16)
        if torch.isfinite(g.float()).all():
            return g.double(), "fp16"
    except RuntimeError:
        pass
    sd16 = {k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()}
    _, g = oracle_loss_grad(sd16, ids, ctx.half().float(), feats.half().float(), labels, logit_scale, torch.float32)
    return g.double(), "fp32-rounded"


def rel_fro(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------------------------------------------------------------------- cases
def state_dict(geom, seed=0):
    return {k: v for k, v in syn.synthetic_state_dict(geom, seed=seed).items()}


def prompt_ids(geom, C, n_ctx, seed=0, far=False):
    """ids [C, context] = [SOT, X * n_ctx, name tokens, EOT, 0 ..]: the names are 0 .. 7 tokens long, prompt 0's EOT sits directly
    behind the context; ``far`` puts the last prompt's EOT on the last token of the context."""
    g = syn.GEOMETRIES[geom]
    V, Lc = g.vocab_size, g.context_length
    rng = np.random.RandomState(100 + seed)
    ids = np.zeros((C, Lc), np.int64)
    for c in range(C):
        k = c % 8
        if far and c == C - 1:
            k = Lc - 2 - n_ctx
        ids[c, 0] = V - 2
        ids[c, 1:1 + n_ctx] = 1
        ids[c, 1 + n_ctx:1 + n_ctx + k] = rng.randint(2, V - 2, size=k)
        ids[c, 1 + n_ctx + k] = V - 1
    return torch.from_numpy(ids)


def make_case(geom, C, n_ctx, B, csc=False, seed=0, far=False, separable=False):
    """dict: sd, ids, ctx fp32, feats fp32 [B, E], labels int64 [B]."""
    g = syn.GEOMETRIES[geom]
    gen = torch.Generator().manual_seed(500 + seed)
    shape = (C, n_ctx, g.transformer_width) if csc else (n_ctx, g.transformer_width)
    ctx = 0.02 * torch.randn(*shape, generator=gen)
    feats = torch.randn(B, g.embed_dim, generator=gen)
    labels = torch.randint(0, C, (B,), generator=gen)
    return {"sd": state_dict(geom), "ids": prompt_ids(geom, C, n_ctx, seed, far), "ctx": ctx, "feats": feats, "labels": labels}


# (geometry, C, n_ctx, B, class-specific): the CPU test runs all of them, the GPU test the same list
GRADIENT_CASES = [
    ("tiny", 3, 4, 1, False),
    ("tiny", 3, 16, 8, True),
    ("tiny", 37, 4, 33, False),
    ("tiny3", 3, 16, 33, False),
    ("tiny3", 37, 16, 8, False),
    ("tiny3", 37, 4, 1, True),
]
LN_CASES = [(D, rows) for D in (64, 128, 512) for rows in (1, 77, 3 * 77 + 5)]
ATTENTION_CASES = [(n, h, L) for (n, h) in ((1, 1), (3, 2), (37, 8)) for L in (1, 2, 20, 33, 77)]
HEAD_CASES = [(1, 2, 64), (8, 3, 128), (33, 37, 512), (8, 37, 64), (33, 2, 128)]
