"""Reference of ProDA's training path (clip_calibration_amd/prodafit.py, csrc/proda_train.hip).  It imports none of the package's kernels.

(1) A no-autograd restatement, in whatever dtype it is given, of the prompt assembly (by the row formulas), of the loss head with its
backward (sigma in the difference form) and of the context reduce, on top of ``coopfit_ref``'s restatement of the tower -- and, for the
comparison with (2) at 1e-9, on a second restatement of the tower that keeps the oracle's two fp32 islands (``tower``).  (2) The truth:
torch autograd through ``oracle.clip_oracle.text_encoder`` on prompts assembled by one ``torch.cat`` per class and context (proda.py:162-228),
with the loss in the reference's form (proda.py:272-302) -- the three-term sigma through the [E, C, C] product.  The cases of the
test files are at the bottom."""
import functools
import math

import numpy as np
import torch

import coopfit_ref as ref
from clip_calibration_amd import synthetic as syn     # weights and geometry only (no library call)
from oracle import clip_oracle as orc

LOGIT_SCALE = ref.LOGIT_SCALE
ALPHA = 0.1


def unit(t):
    return t / t.norm(dim=-1, keepdim=True)


def positions(P):
    """proda.py:110-114."""
    return np.array([0] * (P // 4) + [1] * (P // 4) + [2] * (P // 2), np.int64)


def ordered(sel, pos):
    """end | middle | front, the draw order kept inside a group."""
    sel = np.asarray(sel, np.int64)
    return np.concatenate([sel[pos[sel] == k] for k in (2, 1, 0)])


def name_lens_of(ids, n_ctx):
    return (ids.argmax(dim=-1) - n_ctx - 2).numpy()


def nc_ids_of(ids, n_ctx):
    """The ids of "X .. X .": class 0 of these cases has an empty name."""
    assert int(ids[0].argmax()) == n_ctx + 2
    return ids[:1].clone()


# ------------------------------------------------------------------------------------------------------------------ (1) the restatement
def ctx_row(ps, j, nl, h):
    if ps == 0:
        return 1 + nl + j
    if ps == 1:
        return 1 + j if j < h else 1 + nl + j
    return 1 + j


def assemble(emb, nc_emb, ctx, sel, pos, name_lens, cls_eot=None):
    """(prompts [C Pb + P, L, D], eot [C Pb + P]) by the row formulas: ``sel`` already ordered; emb [C, L, D], nc_emb [1, L, D].
    ``cls_eot``: the classes' EOT rows (None: n_ctx + 2 + name length, the layout [SOT, X * n_ctx, name, '.', EOT])."""
    C, L, D = emb.shape
    P, n_ctx, _ = ctx.shape
    Pb, h = len(sel), n_ctx // 2
    out = torch.empty(C * Pb + P, L, D, dtype=ctx.dtype)
    eot = np.empty(C * Pb + P, np.int32)
    for c in range(C):
        nl = int(name_lens[c])
        for q, p in enumerate(sel):
            rows = [ctx_row(int(pos[p]), j, nl, h) for j in range(n_ctx)]
            free = [r for r in range(1, 1 + n_ctx + nl) if r not in rows]
            x = emb[c].to(ctx.dtype).clone()
            x[rows] = ctx[p]
            x[free] = emb[c, 1 + n_ctx:1 + n_ctx + nl].to(ctx.dtype)
            out[c * Pb + q] = x
            eot[c * Pb + q] = n_ctx + 2 + nl if cls_eot is None else cls_eot[c]
    for p in range(P):
        x = nc_emb[0].to(ctx.dtype).clone()
        x[1:1 + n_ctx] = ctx[p]
        out[C * Pb + p] = x
        eot[C * Pb + p] = n_ctx + 2
    return out, eot


def ctx_reduce(d_embed, sel, pos, name_lens, C, P, n_ctx):
    """d ctx [P, n_ctx, D] from d_embed [C Pb + P, L, D]: a selected context's class rows in ascending class order, then the no-class row."""
    Pb, h = len(sel), n_ctx // 2
    g = torch.zeros(P, n_ctx, d_embed.shape[-1], dtype=d_embed.dtype)
    for q, p in enumerate(sel):
        for c in range(C):
            rows = [ctx_row(int(pos[p]), j, int(name_lens[c]), h) for j in range(n_ctx)]
            g[p] = g[p] + d_embed[c * Pb + q, rows]
    return g + d_embed[C * Pb:, 1:1 + n_ctx]


def head(feats, labels, text, C, Pb, scale, alpha):
    """(total, upper, m, d total / d text [N, E]) of ProDA's loss on raw text features [C Pb + P, E], sigma in the difference form."""
    N, E = text.shape
    P, B = N - C * Pb, feats.shape[0]
    ar = torch.arange(B)
    x = unit(feats)
    x2 = x * x
    tc = text[:C * Pb].reshape(C, Pb, E)
    nt = tc.norm(dim=-1, keepdim=True)
    u = tc / nt
    m = u.mean(1)
    v = u - m[:, None]
    diff = v[labels][:, None] - v[None]                                   # [B, C, Pb, E]: v_y - v_c
    sigma = (x2[:, None, None, :] * diff ** 2).sum((-1, -2)) / (Pb + 1)
    z = scale * x @ m.t() + 0.5 * scale ** 2 * sigma
    upper = (torch.logsumexp(z, dim=-1) - z[ar, labels]).mean()
    dz = torch.softmax(z, dim=-1)
    dz[ar, labels] -= 1.0
    dz = dz / B
    dm = scale * dz.t() @ x
    w = 0.5 * scale ** 2 * dz
    t1 = torch.einsum("bk,bd,bkqd->kqd", w, x2, -diff)
    t2 = torch.zeros_like(t1).index_add_(0, labels, torch.einsum("bc,bd,bcqd->bqd", w, x2, diff))
    dv = 2.0 / (Pb + 1) * (t1 + t2)
    du = dv - dv.mean(1, keepdim=True) + dm[:, None] / Pb
    d_cls = (du - u * (u * du).sum(-1, keepdim=True)) / nt
    nc = text[C * Pb:]
    nn = nc.norm(dim=-1, keepdim=True)
    n = nc / nn
    G = n @ n.t()
    off = ~torch.eye(P, dtype=torch.bool)
    lm = G[off].abs().mean()
    dn = alpha * 2.0 / (P * (P - 1)) * (torch.sign(G) * off) @ n
    d_nc = (dn - n * (n * dn).sum(-1, keepdim=True)) / nn
    return upper + alpha * lm, upper, lm, torch.cat([d_cls.reshape(C * Pb, E), d_nc]), z


# The oracle's encoder (the truth below) keeps two islands of fp32 arithmetic whatever the activation dtype: oracle.clip_oracle.layer_norm
# computes in fp32 from elementary operations and casts back, and multi_head_attention takes the softmax of the fp32 scores.  Its float64
# run therefore carries fp32 rounding, forward and backward (tests/test_coopfit_cpu.py holds CoOp's float64 restatement to 1e-4 of it).
# ``island_tower`` restates exactly that: the same fp32 operations in the same order in the forward, and in the backward the derivative
# of every one of those elementary operations, in fp32, accumulated in the order in which they were applied -- written out by hand,
# with no autograd graph.  Everything outside the two islands stays in ``dtype``.
def island_ln_forward(x, gamma, beta, eps=1e-5):
    """(oracle.clip_oracle.layer_norm(x), what its backward needs): d = x - mean and r = rsqrt(var + eps), fp32."""
    xf = x.float()
    d = xf - xf.mean(dim=-1, keepdim=True)
    r = torch.rsqrt((d ** 2).mean(dim=-1, keepdim=True) + eps)
    return ((d * r) * gamma.float() + beta.float()).to(x.dtype), (d, r)


def island_ln_backward(st, gamma, dy):
    """dX of that LayerNorm in fp32, term by term: through the normalised row, through r = rsqrt(mean(d^2) + eps), through the mean."""
    d, r = st
    D = d.shape[-1]
    t = dy.float() * gamma.float()
    g_row = t * r
    g_var = -0.5 * (t * d).sum(-1, keepdim=True) * r.pow(3)
    g_sq = (g_var.expand_as(d) / D) * (d * 2.0)
    g_mean = (-g_row).sum(-1, keepdim=True) + (-g_sq).sum(-1, keepdim=True)
    return ((g_row + g_sq) + g_mean.expand_as(d) / D).to(dy.dtype)


def island_attention(qkv, N, L, H):
    """(attention output [N L, D], the fp32 probabilities): scores in the activation dtype, softmax of their fp32 copy, cast back."""
    D = 64 * H
    q, k, v = (ref.split_heads(t, N, L, H) for t in qkv.reshape(N * L, 3 * D).split(D, dim=-1))
    s = (q @ k.transpose(-1, -2)) / 8.0 + orc.causal_mask(L).to(qkv.dtype)
    p32 = torch.softmax(s.float(), dim=-1)
    return (p32.to(qkv.dtype) @ v).transpose(1, 2).reshape(N * L, D), p32


def island_attention_backward(qkv, p32, d_out, N, L, H):
    """coopfit_ref.attention_backward with dS = P o (dP - rowsum(dP o P)) evaluated in fp32 on the fp32 probabilities, by the one
    primitive that evaluates it for torch.softmax (its summation order is the primitive's own)."""
    D = 64 * H
    q, k, v = (ref.split_heads(t, N, L, H) for t in qkv.reshape(N * L, 3 * D).split(D, dim=-1))
    do = ref.split_heads(d_out, N, L, H)
    p = p32.to(qkv.dtype)
    dv = p.transpose(-1, -2) @ do
    dp = do @ v.transpose(-1, -2)
    ds = torch.ops.aten._softmax_backward_data(dp.float(), p32, -1, torch.float32).to(qkv.dtype) / 8.0
    dq = ds @ k
    dk = ds.transpose(-1, -2) @ q
    return torch.cat([t.transpose(1, 2).reshape(N * L, D) for t in (dq, dk, dv)], dim=-1)


def island_block_forward(x, w, N, L, H):
    h1, ln1 = island_ln_forward(x, w["ln_1.weight"], w["ln_1.bias"])
    qkv = h1 @ w["attn.in_proj_weight"].t() + w["attn.in_proj_bias"]
    att, p32 = island_attention(qkv, N, L, H)
    x_mid = x + (att @ w["attn.out_proj.weight"].t() + w["attn.out_proj.bias"])
    h2, ln2 = island_ln_forward(x_mid, w["ln_2.weight"], w["ln_2.bias"])
    h = h2 @ w["mlp.c_fc.weight"].t() + w["mlp.c_fc.bias"]
    out = x_mid + (ref.quickgelu(h) @ w["mlp.c_proj.weight"].t() + w["mlp.c_proj.bias"])
    return out, {"ln1": ln1, "ln2": ln2, "qkv": qkv, "p32": p32, "h": h}


def island_block_backward(g, st, w, N, L, H):
    d_h = ref.quickgelu_backward(st["h"], g @ w["mlp.c_proj.weight"])
    g = g + island_ln_backward(st["ln2"], w["ln_2.weight"], d_h @ w["mlp.c_fc.weight"])
    dqkv = island_attention_backward(st["qkv"], st["p32"], g @ w["attn.out_proj.weight"], N, L, H)
    return g + island_ln_backward(st["ln1"], w["ln_1.weight"], dqkv @ w["attn.in_proj_weight"])


def _tower_input(sd, prompts, eot, dtype):
    N, L, D = prompts.shape
    x = (prompts.to(dtype) + sd["positional_embedding"][:L].to(dtype)).reshape(N * L, D)
    ws = [ref.block_weights(sd, i, dtype) for i in range(ref.n_layers(sd))]
    eot_rows = torch.arange(N) * L + torch.as_tensor(eot, dtype=torch.int64)
    return x, ws, eot_rows, sd["ln_final.weight"].to(dtype), sd["ln_final.bias"].to(dtype), sd["text_projection"].to(dtype)


def tower(sd, prompts, eot, dtype):
    """(text features [N, E], a function d_text -> d_embed [N, L, D]) by coopfit_ref's restatement of the tower on assembled prompts."""
    N, L, D = prompts.shape
    H = D // 64
    x, ws, eot_rows, gamma, beta, proj = _tower_input(sd, prompts, eot, dtype)
    stashes = []
    for w in ws:
        x, st = ref.block_forward(x, w, N, L, H)
        stashes.append(st)
    text = ref.ln_forward(x[eot_rows], gamma, beta) @ proj

    def backward(d_text):
        g = torch.zeros_like(x)
        g[eot_rows] = ref.ln_backward(x[eot_rows], gamma, d_text @ proj.t())
        for w, st in zip(reversed(ws), reversed(stashes)):
            g = ref.block_backward(g, st, w, N, L, H)
        return g.reshape(N, L, D)

    return text, backward


def island_tower(sd, prompts, eot, dtype):
    """``tower`` with the oracle's two fp32 islands (above).  The oracle normalises every row with ln_final and then takes the EOT rows."""
    N, L, D = prompts.shape
    H = D // 64
    x, ws, eot_rows, gamma, beta, proj = _tower_input(sd, prompts, eot, dtype)
    stashes = []
    for w in ws:
        x, st = island_block_forward(x, w, N, L, H)
        stashes.append(st)
    y, ln_f = island_ln_forward(x, gamma, beta)
    text = y[eot_rows] @ proj

    def backward(d_text):
        g = torch.zeros_like(x)
        g[eot_rows] = d_text @ proj.t()
        g = island_ln_backward(ln_f, gamma, g)
        for w, st in zip(reversed(ws), reversed(stashes)):
            g = island_block_backward(g, st, w, N, L, H)
        return g.reshape(N, L, D)

    return text, backward


def restated(sd, ids, ctx, feats, labels, sel=None, alpha=ALPHA, logit_scale=LOGIT_SCALE, dtype=torch.float64, islands=False, name_lens=None):
    """What ``oracle_parts`` returns, by the restatement; ``islands``: on ``island_tower``.  ``name_lens``: None takes the prompts' own."""
    sd_c, ids_c = ref.cut(sd, ids)
    C = ids.shape[0]
    P, n_ctx, _ = ctx.shape
    pos = positions(P)
    sel = ordered(np.arange(P) if sel is None else sel, pos)
    nl = name_lens_of(ids, n_ctx) if name_lens is None else np.asarray(name_lens)
    emb = sd["token_embedding.weight"][ids_c].to(dtype)
    prompts, eot = assemble(emb, emb[:1], ctx.to(dtype), sel, pos, nl, ids_c.argmax(dim=-1).numpy())
    text, backward = (island_tower if islands else tower)(sd_c, prompts, eot, dtype)
    total, upper, lm, d_text, _ = head(feats.to(dtype), labels, text, C, len(sel), math.exp(logit_scale), alpha)
    return {"loss": float(total), "upper": float(upper), "m": float(lm), "grad": ctx_reduce(backward(d_text), sel, pos, nl, C, P, n_ctx), "text": text}


# ------------------------------------------------------------------------------------------------------------------------- (2) the truth
def truth_prompts(emb, nc_emb, ctx, drawn, pos, name_lens):
    """(class prompts [C Pb, L, D], no-class prompts [P, L, D]) as ProDA's prompt learner builds them (proda.py:146-228), one
    ``torch.cat`` per class and context: the class name in front of the context vectors, between their two halves, or behind them.  The
    reference groups a step's contexts by position before it lays them out, so a class's prompts come end | middle | front with the draw
    order kept inside a group; ``drawn`` is the step's selection in any order."""
    n_ctx = ctx.shape[1]
    split = n_ctx // 2
    order = [int(p) for want in (2, 1, 0) for p in drawn if int(pos[p]) == want]
    rows = []
    for c in range(emb.shape[0]):
        nl = int(name_lens[c])
        sos, name, tail = emb[c, :1], emb[c, 1 + n_ctx:1 + n_ctx + nl], emb[c, 1 + n_ctx + nl:]
        for p in order:
            if pos[p] == 0:
                parts = [sos, name, ctx[p], tail]
            elif pos[p] == 1:
                parts = [sos, ctx[p, :split], name, ctx[p, split:], tail]
            else:
                parts = [sos, ctx[p], name, tail]
            rows.append(torch.cat(parts))
    no_class = [torch.cat([nc_emb[0, :1], ctx[p], nc_emb[0, 1 + n_ctx:]]) for p in range(ctx.shape[0])]
    return torch.stack(rows), torch.stack(no_class)


def truth_loss(x, text, nc_text, labels, C, scale, alpha, up=lambda t: t):
    """(total, upper, m) of ProDA's training loss (proda.py:272-302) on normalised image features x [B, E] and raw text features.  The
    variance term is formed the reference's way, not the kernels': the per-dimension covariance of a class pair over the prompts,
    cov[e, i, k] = sum_q v_iqe v_kqe / (Pb + 1), an [E, C, C] tensor; R[b, i, k] = sum_e x_be^2 cov[e, i, k]; and
    sigma[b, c] = R[b, y, y] + R[b, c, c] - 2 R[b, y, c].  ``up`` widens the logits and the cosines before the loss functions (the
    float16 yardstick evaluates those on fp32 copies, as promptfit_ref does)."""
    Pb, B = text.shape[0] // C, labels.shape[0]
    u = unit(text).reshape(C, Pb, -1)
    centre = u.mean(dim=1)
    v = (u - centre[:, None]).permute(2, 0, 1)                         # [E, C, Pb]
    cov = (v @ v.transpose(1, 2)) / (Pb + 1)                           # [E, C, C]
    R = torch.einsum("be,eik->bik", x * x, cov)
    b, k = torch.arange(B), torch.arange(C)
    sigma = R[b, labels, labels][:, None] + R[:, k, k] - 2.0 * R[b, labels]
    z = scale * (x @ centre.t()) + 0.5 * scale ** 2 * sigma
    upper = torch.nn.functional.cross_entropy(up(z), labels)
    n = unit(nc_text)
    cos = n @ n.t()
    off_diagonal = ~torch.eye(cos.shape[0], dtype=torch.bool)
    m = up(cos[off_diagonal]).abs().mean()
    return upper + alpha * m, upper, m


def restated_encoder(sd, prompts, tokenized, dtype):
    """oracle.clip_oracle.text_encoder's signature on coopfit_ref's forward formulas: plain torch operations in ``dtype`` throughout
    (the oracle's LayerNorm and softmax work in fp32 whatever the dtype), differentiable by autograd."""
    return tower(sd, prompts, tokenized.argmax(dim=-1), dtype)[0]


def oracle_parts(sd, ids, ctx, feats, labels, sel=None, alpha=ALPHA, logit_scale=LOGIT_SCALE, dtype=torch.float64, encoder=orc.text_encoder,
                 name_lens=None):
    """loss, upper, m, grad [P, n_ctx, D] and the raw text features by torch autograd through the oracle in ``dtype``.  ``sel`` as drawn
    (any order): the reference's forward groups it.  ``name_lens``: None takes the prompts' own.  ``encoder=restated_encoder``: the same autograd through a tower without the
    oracle's fp32 islands."""
    sd_c, ids_c = ref.cut(sd, ids)
    C = ids.shape[0]
    P, n_ctx, _ = ctx.shape
    pos = positions(P)
    sel = np.arange(P) if sel is None else np.asarray(sel)
    nl = name_lens_of(ids, n_ctx) if name_lens is None else np.asarray(name_lens)
    c = ctx.detach().to(dtype).clone().requires_grad_(True)
    emb = sd_c["token_embedding.weight"][ids_c].to(dtype)
    nc_ids = nc_ids_of(ids_c, n_ctx)
    prompts, nc_prompts = truth_prompts(emb, emb[:1], c, sel, pos, nl)
    tokenized = ids_c.unsqueeze(1).repeat(1, len(sel), 1).view(C * len(sel), -1)
    tf = encoder(sd_c, prompts, tokenized, dtype)
    nc_tf = encoder(sd_c, nc_prompts, nc_ids.repeat(P, 1), dtype)
    up = (lambda t: t.float()) if dtype == torch.float16 else (lambda t: t)
    total, upper, lm = truth_loss(unit(feats.to(dtype)), tf, nc_tf, labels, C, math.exp(logit_scale), alpha, up)
    total.backward()
    return {"loss": float(total.detach()), "upper": float(upper.detach()), "m": float(lm.detach()), "grad": c.grad.detach(),
            "text": torch.cat([tf, nc_tf]).detach()}


def yardstick_parts(sd, ids, ctx, feats, labels, sel=None, alpha=ALPHA, logit_scale=LOGIT_SCALE, name_lens=None):
    """The same at the reference's own precision, as promptfit_ref.yardstick_parts makes it: the oracle's autograd at float16 on the CPU
    or, where this torch build lacks an fp16 CPU op of that backward (or the result is not finite), the fp32 oracle with weights and
    inputs rounded through fp16.  Returns (parts, how)."""
    try:
        got = oracle_parts(sd, ids, ctx.half(), feats.half(), labels, sel, alpha, logit_scale, torch.float16, name_lens=name_lens)
        if torch.isfinite(got["grad"].float()).all() and math.isfinite(got["loss"]):
            return dict(got, grad=got["grad"].double()), "fp16"
    except RuntimeError:
        pass
    sd16 = {k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()}
    got = oracle_parts(sd16, ids, ctx.half().float(), feats.half().float(), labels, sel, alpha, logit_scale, torch.float32, name_lens=name_lens)
    return dict(got, grad=got["grad"].double()), "fp32-rounded"


# ------------------------------------------------------------------------------------------------------------------------------- cases
def prompt_ids(geom, C, n_ctx, seed=0):
    """ids [C, context] = [SOT, X * n_ctx, name, '.', EOT, 0 ..]: class c's name is c % 7 tokens long (class 0's is empty: the three
    positions coincide there), except the last class, whose name is as long as puts its EOT on the last live row of the cut (the row
    count is the EOT's row + 1 rounded up to a multiple of 8)."""
    g = syn.GEOMETRIES[geom]
    V, Lc = g.vocab_size, g.context_length
    rng = np.random.RandomState(300 + seed)
    far = (n_ctx + 2 + 6 + 1 + 7) // 8 * 8 - 1
    ids = np.zeros((C, Lc), np.int64)
    for c in range(C):
        k = c % 7 if c < C - 1 else far - n_ctx - 2
        ids[c, 0] = V - 2
        ids[c, 1:1 + n_ctx] = 1
        ids[c, 1 + n_ctx:1 + n_ctx + k] = rng.randint(3, V - 2, size=k)
        ids[c, 1 + n_ctx + k] = 2          # '.'
        ids[c, 2 + n_ctx + k] = V - 1
    return torch.from_numpy(ids)


@functools.lru_cache(maxsize=None)
def make_case(geom, C, n_ctx, P, Pb, B, seed=0):
    """dict: sd, ids, ctx fp32 [P, n_ctx, D], feats fp32 [B, E], labels int64 [B]."""
    g = syn.GEOMETRIES[geom]
    gen = torch.Generator().manual_seed(700 + seed)
    ctx = 0.02 * torch.randn(P, n_ctx, g.transformer_width, generator=gen)
    feats = torch.randn(B, g.embed_dim, generator=gen)
    labels = torch.randint(0, C, (B,), generator=gen)
    return {"sd": ref.state_dict(geom), "ids": prompt_ids(geom, C, n_ctx, seed), "ctx": ctx, "feats": feats, "labels": labels}


# (geometry, C, n_ctx, P, Pb, B) -> the selections tried on it, as drawn (None: all contexts).  pos is [front] * (P // 4) + [middle] *
# (P // 4) + [end] * (P // 2): for P = 8 contexts 0, 1 are front, 2, 3 middle, 4 .. 7 end.
CASES = {
    ("tiny", 2, 4, 4, 4, 1): [None],                                   # all four contexts in natural order, one sample
    ("tiny", 3, 5, 8, 2, 8): [(0, 1), (3, 6), (7, 4)],                 # odd n_ctx (h = 2): {front, front}, {middle, end}, {end, end}
    ("tiny", 37, 4, 8, 4, 33): [(1, 6, 2, 5)],                         # off the wave and workgroup multiples, classes absent from the batch
    ("tiny3", 3, 16, 4, 1, 8): [(1,)],                                 # Pb = 1: v = 0 and sigma = 0 exactly
    ("tiny3", 37, 4, 8, 4, 1): [(7, 0, 3, 4)],
}
CASE_LIST = [(k, s) for k, sels in CASES.items() for s in sels]
SEQ_ROWS_CASES = [(("tiny", 3, 5, 8, 2, 8), (3, 6)), (("tiny3", 37, 4, 8, 4, 1), (7, 0, 3, 4))]


def head_case(B, C, E, Pb, P, seed=0):
    """Synthetic text rows for the head: text_{c,q} = base_c + 0.1 noise, raw no-class rows, features whose softmax is not saturated."""
    g = torch.Generator().manual_seed(B * 1000 + C * 10 + Pb + seed)
    wide = torch.randn(B, E + 24, generator=g)
    base = torch.randn(C, 1, E, generator=g)
    text = (base + 0.1 * torch.randn(C, Pb, E, generator=g)).reshape(C * Pb, E) * 0.3
    nc = torch.randn(P, E, generator=g) * 2.0
    y = torch.randint(0, C, (B,), generator=g)
    return wide, torch.cat([text, nc]), y


HEAD_SCALE = 10.0
HEAD_CASES = [(B, C, E, Pb, P) for (B, C, E) in ref.HEAD_CASES for (Pb, P) in ((1, 4), (2, 8), (4, 4))]
