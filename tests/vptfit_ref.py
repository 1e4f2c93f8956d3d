"""Reference of VPT's training path (clip_calibration_amd/vptfit.py, csrc/vision_backward.hip, csrc/prompt_train.hip, the unmasked attention
backward of csrc/attention.hip).  It does not import the package.

(1) A hand-written torch restatement, in whatever dtype it is given (float64 in the tests), of what the kernels implement beyond
coopfit_ref's LayerNorm, QuickGELU and block formulas: attention's backward without a mask, the image-side loss head, the splice
reduction of the deep prompts and the ln_pre tail of slot 0 -- no autograd inside.  (2) The truth: torch autograd through
``oracle.clip_oracle.encode_image(sd, image, dtype, shared_ctx, deep_prompts)``; its ``.half()`` cast is applied to the VALUE and the
gradient passes straight through.  The case lists are at the bottom."""
import math

import torch

import coopfit_ref as cref
from clip_calibration_amd import synthetic as syn     # weights and geometry only (no library call)
from oracle import clip_oracle as orc

LOGIT_SCALE = 4.6052
CUSTOM = syn.ClipGeometry(128, 112, 2, 128, 8, 77, 256, 128, 2, 2)     # 196 patches + class = 197 tokens at width 128


def geometry(name):
    return CUSTOM if name == "custom" else syn.GEOMETRIES[name]


# ------------------------------------------------------------------------------------------------------------------ (1) the restatement
def attention_probs_full(q, k):
    return torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)


def attention_forward_full(qkv, N, L, H):
    D = 64 * H
    q, k, v = (cref.split_heads(t, N, L, H) for t in qkv.reshape(N * L, 3 * D).split(D, dim=-1))
    return (attention_probs_full(q, k) @ v).transpose(1, 2).reshape(N * L, D)


def attention_backward_full(qkv, d_out, N, L, H, lo=None):
    """dqkv [N L, 3 D] of attention without a mask.  ``lo``: the kernel's rounding points -- P and dS rounded to ``lo`` in front of their
    products and one rounding of dqkv (None: none)."""
    D = 64 * H
    r = (lambda t: t) if lo is None else (lambda t: t.to(lo).to(qkv.dtype))
    q, k, v = (cref.split_heads(t, N, L, H) for t in qkv.reshape(N * L, 3 * D).split(D, dim=-1))
    do = cref.split_heads(d_out, N, L, H)
    p = attention_probs_full(q, k)
    dv = r(p).transpose(-1, -2) @ do
    dp = do @ v.transpose(-1, -2)
    ds = r(p * (dp - (dp * p).sum(-1, keepdim=True)))
    dq = ds @ k / 8.0
    dk = ds.transpose(-1, -2) @ q / 8.0
    return r(torch.cat([t.transpose(1, 2).reshape(N * L, D) for t in (dq, dk, dv)], dim=-1))


def head_image(feats, labels, text, scale):
    """(loss, d loss / d feats, row losses) of mean CE(scale normalise(f) normalise(t)^T, y)."""
    nf, nt = feats.norm(dim=-1, keepdim=True), text.norm(dim=-1, keepdim=True)
    x, u = feats / nf, text / nt
    z = scale * x @ u.t()
    rows = torch.logsumexp(z, dim=-1) - z[torch.arange(z.shape[0]), labels]
    dz = torch.softmax(z, dim=-1)
    dz[torch.arange(z.shape[0]), labels] -= 1.0
    dz = dz / z.shape[0]
    dx = scale * dz @ u
    return rows.mean(), (dx - x * (x * dx).sum(-1, keepdim=True)) / nf, rows


def vblock_weights(sd, i, dtype):
    p = f"visual.transformer.resblocks.{i}."
    names = ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
             "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")
    return {n: sd[p + n].to(dtype) for n in names}


def block_forward(x, w, N, L, H):
    qkv = cref.ln_forward(x, w["ln_1.weight"], w["ln_1.bias"]) @ w["attn.in_proj_weight"].t() + w["attn.in_proj_bias"]
    x_mid = x + attention_forward_full(qkv, N, L, H) @ w["attn.out_proj.weight"].t() + w["attn.out_proj.bias"]
    h = cref.ln_forward(x_mid, w["ln_2.weight"], w["ln_2.bias"]) @ w["mlp.c_fc.weight"].t() + w["mlp.c_fc.bias"]
    out = x_mid + cref.quickgelu(h) @ w["mlp.c_proj.weight"].t() + w["mlp.c_proj.bias"]
    return out, {"x_in": x, "x_mid": x_mid, "qkv": qkv, "h": h}


def block_backward(g, st, w, N, L, H):
    d_h = cref.quickgelu_backward(st["h"], g @ w["mlp.c_proj.weight"])
    g = g + cref.ln_backward(st["x_mid"], w["ln_2.weight"], d_h @ w["mlp.c_fc.weight"])
    dqkv = attention_backward_full(st["qkv"], g @ w["attn.out_proj.weight"], N, L, H)
    return g + cref.ln_backward(st["x_in"], w["ln_1.weight"], dqkv @ w["attn.in_proj_weight"])


def n_layers(sd):
    return len([k for k in sd if k.startswith("visual.transformer.resblocks.") and k.endswith(".attn.in_proj_weight")])


def forward(sd, images, prompts, dtype=torch.float64):
    """(features [B, E], stash) of the image tower with the prompt block [depth, n_ctx, D] (values rounded through fp16)."""
    pr = prompts.half().to(dtype)
    depth, n_ctx, D = pr.shape
    x = orc.patch_embed(images.to(dtype), sd["visual.conv1.weight"])
    B = x.shape[0]
    x = torch.cat([sd["visual.class_embedding"].to(dtype).expand(B, 1, -1), x], dim=1) + sd["visual.positional_embedding"].to(dtype)
    L0 = x.shape[1]
    x = torch.cat([x, pr[0].expand(B, -1, -1)], dim=1)
    L, H, layers = L0 + n_ctx, D // 64, n_layers(sd)
    x = cref.ln_forward(x, sd["visual.ln_pre.weight"].to(dtype), sd["visual.ln_pre.bias"].to(dtype)).reshape(B * L, D)
    stash = []
    for i in range(layers):
        if 0 < i < depth:
            x = x.reshape(B, L, D).clone()
            x[:, L0:] = pr[i]
            x = x.reshape(B * L, D)
        x, st = block_forward(x, vblock_weights(sd, i, dtype), B, L, H)
        stash.append(st)
    cls = x.reshape(B, L, D)[:, 0]
    feats = cref.ln_forward(cls, sd["visual.ln_post.weight"].to(dtype), sd["visual.ln_post.bias"].to(dtype)) @ sd["visual.proj"].to(dtype)
    return feats, {"blocks": stash, "x_post": cls, "pr": pr, "B": B, "L": L, "L0": L0, "H": H}


def backward(sd, st, d_feats, dtype=torch.float64):
    """d_prompts [depth, n_ctx, D] from d_feats [B, E]: the tail, the blocks last to first with the splice reduction, slot 0 through ln_pre
    (the batch summed first: LayerNorm's backward is linear in dy and the pre-LN row is the prompt for every image)."""
    pr, B, L, L0, H = st["pr"], st["B"], st["L"], st["L0"], st["H"]
    depth, n_ctx, D = pr.shape
    g = torch.zeros(B, L, D, dtype=dtype)
    g[:, 0] = cref.ln_backward(st["x_post"], sd["visual.ln_post.weight"].to(dtype), d_feats.to(dtype) @ sd["visual.proj"].to(dtype).t())
    g = g.reshape(B * L, D)
    d_prompts = torch.zeros(depth, n_ctx, D, dtype=dtype)
    for i in range(len(st["blocks"]) - 1, -1, -1):
        g = block_backward(g, st["blocks"][i], vblock_weights(sd, i, dtype), B, L, H)
        if 1 <= i < depth:
            g3 = g.reshape(B, L, D).clone()
            d_prompts[i] = g3[:, L0:].sum(0)
            g3[:, L0:] = 0
            g = g3.reshape(B * L, D)
    d_prompts[0] = cref.ln_backward(pr[0], sd["visual.ln_pre.weight"].to(dtype), g.reshape(B, L, D)[:, L0:].sum(0))
    return d_prompts


def loss_and_grad(sd, images, prompts, text, labels, logit_scale=LOGIT_SCALE, dtype=torch.float64):
    feats, st = forward(sd, images, prompts, dtype)
    loss, d_feats, _ = head_image(feats, labels, text.to(dtype), math.exp(logit_scale))
    return loss, backward(sd, st, d_feats, dtype)


# ----------------------------------------------------------------------------------------------------------------------- (2) the truth
class _HalfValue(torch.autograd.Function):
    """x.half() as the oracle applies it, the gradient passed straight through."""

    @staticmethod
    def forward(ctx, x):
        return x.half().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def oracle_loss_grad(sd, images, prompts, text, labels, logit_scale=LOGIT_SCALE, dtype=torch.float64):
    """(loss, d loss / d prompts) by torch autograd through oracle.clip_oracle.encode_image in ``dtype``."""
    p = prompts.detach().to(dtype).clone().requires_grad_(True)
    ph = _HalfValue.apply(p)
    # torch's own backward of .half() rounds the GRADIENT to fp16 as well; the values are rounded above, so the oracle's cast is taken out
    # for the call and the gradient passes straight through.  This leans on one internal name of the oracle, ``_h(t, dtype)``, the cast it
    # applies to every prompt tensor and to nothing else (oracle/clip_oracle.py); the assertion below fails loudly if that name goes away,
    # and test_vptfit_cpu.py holds this truth to the autograd-free restatement, which never touches it.
    assert callable(getattr(orc, "_h", None)), "oracle.clip_oracle._h is gone: restate how the prompts' cast is made transparent"
    keep, orc._h = orc._h, (lambda t, dt: t.to(dt))
    try:
        f = orc.encode_image(sd, images.to(dtype), dtype, ph[0], [ph[i] for i in range(1, p.shape[0])])
    finally:
        orc._h = keep
    t = text.to(dtype)
    logits = math.exp(logit_scale) * (f / f.norm(dim=-1, keepdim=True)) @ (t / t.norm(dim=-1, keepdim=True)).t()
    loss = torch.nn.functional.cross_entropy(logits.float() if dtype == torch.float16 else logits, labels)
    loss.backward()
    return loss.detach(), p.grad.detach()


def yardstick(sd, images, prompts, text, labels, logit_scale=LOGIT_SCALE):
    """(loss, grad, how) of the reference's own precision: the oracle's autograd at float16 on the CPU, or, where this torch build lacks an
    fp16 CPU op of it, the fp32 oracle with weights and inputs rounded through fp16 (coopfit_ref.yardstick_grad's fallback)."""
    try:
        l, g = oracle_loss_grad(sd, images.half(), prompts.half(), text.half(), labels, logit_scale, torch.float16)
        if torch.isfinite(g.float()).all():
            return l.double(), g.double(), "fp16"
    except RuntimeError:
        pass
    sd16 = {k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()}
    l, g = oracle_loss_grad(sd16, images.half().float(), prompts.half().float(), text.half().float(), labels, logit_scale, torch.float32)
    return l.double(), g.double(), "fp32-rounded"


rel_fro = cref.rel_fro


# ------------------------------------------------------------------------------------------------------------------------------- cases
def make_case(geom, n_ctx, depth, B, C, seed=0, separable=False):
    """dict: sd, images fp32 [B, 3, R, R], prompts fp32 [depth, n_ctx, D], text fp32 [C, E], labels int64 [B]."""
    g = geometry(geom)
    gen = torch.Generator().manual_seed(700 + seed)
    sd = {k: v for k, v in syn.synthetic_state_dict(g, seed=seed).items()}
    prompts = 0.02 * torch.randn(depth, n_ctx, g.vision_width, generator=gen)
    images = torch.randn(B, 3, g.image_resolution, g.image_resolution, generator=gen)
    text = torch.randn(C, g.embed_dim, generator=gen)
    labels = torch.randint(0, C, (B,), generator=gen)
    if separable:      # the classes' text rows are the images' own zero-prompt features: a loss that can go down
        with torch.no_grad():
            f = orc.encode_image(sd, images, torch.float32)
        labels = torch.arange(B) % C
        text = torch.stack([f[labels == c].mean(0) for c in range(C)])
    return {"geom": geom, "sd": sd, "images": images, "prompts": prompts, "text": text, "labels": labels}


# (geometry, n_ctx, depth, B, C): n_ctx in {1, 8}; depth 1, in between, and the tower's layers
GRADIENT_CASES = [
    ("tiny", 1, 1, 3, 5),
    ("tiny", 8, 2, 4, 7),
    ("tiny3", 8, 1, 2, 3),
    ("tiny3", 1, 2, 5, 4),
    ("tiny3", 8, 3, 3, 37),
]
GPU_CASES = GRADIENT_CASES + [("custom", 8, 2, 2, 5)]     # 197 + 8 = 205 rows: the real length at toy width
ATTENTION_LENGTHS = (1, 15, 16, 17, 25, 33, 96, 97, 197, 205, 213, 224)
