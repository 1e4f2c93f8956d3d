"""Reference of PromptSRC's / IVLP's training path (clip_calibration_amd/promptsrcfit.py, csrc/promptsrc_train.hip, the four-term head of
csrc/prompt_train.hip).  It does not import the package's library.

(1) A hand-written torch restatement, in whatever dtype it is given (float64 in the tests), of what the kernels implement beyond
maplefit_ref's two towers: the four-term head against a frozen teacher, the master block's layout, SGD over it and the Gaussian-weighted
prompt aggregation -- no autograd inside.  (2) The truth: torch autograd through the oracle's ``coop_prompts`` +
``text_encoder(deep_prompts=...)`` + ``encode_image(shared_ctx, deep_prompts)`` and the reference's loss expression; every ``.half()``
cast is applied to the VALUE and the gradient passes straight through.  The case list is at the bottom."""
import math

import numpy as np
import torch

import coopfit_ref as cref
import maplefit_ref as mref
import vptfit_ref as vref
from clip_calibration_amd import synthetic as syn     # weights and geometry only (no library call)
from oracle import clip_oracle as orc

LOGIT_SCALE = 4.6052
WEIGHTS = (25.0, 10.0, 1.0)      # w_text, w_image, w_logit of the reference
rel_fro = cref.rel_fro
h = mref.h


# --------------------------------------------------------------------------------------------------------------------- the master block
def param_names(dt, dv):
    return (["ctx"] + [f"transformer.resblocks.{i}.VPT_shallow" for i in range(1, dt)] + ["visual.VPT"]
            + [f"visual.transformer.resblocks.{i}.VPT_shallow" for i in range(1, dv)])


def depths_of(p):
    return (1 + len([k for k in p if k.startswith("transformer.resblocks.")]), 1 + len([k for k in p if k.startswith("visual.transformer.resblocks.")]))


def block_floats(nt, dt, Dt, nv, dv, Dv):
    return dt * nt * Dt + dv * nv * Dv


def pack(p, dtype=torch.float32):
    return torch.cat([p[n].to(dtype).reshape(-1) for n in param_names(*depths_of(p))])


def unpack(block, nt, dt, Dt, nv, dv, Dv):
    out, at = {}, 0
    for name, shape in zip(param_names(dt, dv), [(nt, Dt)] * dt + [(nv, Dv)] * dv):
        n = math.prod(shape)
        out[name] = block[at:at + n].reshape(shape)
        at += n
    assert at == block.numel()
    return out


def text_prompts(p):
    dt, _ = depths_of(p)
    return p["ctx"], [p[f"transformer.resblocks.{i}.VPT_shallow"] for i in range(1, dt)]


def vis_block(p, dtype=torch.float64):
    _, dv = depths_of(p)
    return torch.stack([p["visual.VPT"].to(dtype)] + [p[f"visual.transformer.resblocks.{i}.VPT_shallow"].to(dtype) for i in range(1, dv)])


# ------------------------------------------------------------------------------------------------------------------ (1) the restatement
def sign0(d):
    return torch.sign(d)          # sign(0) = 0


def head(feats, zs, text, teacher, labels, scale, weights=WEIGHTS):
    """(losses [5] = total, CE, text L1, image L1, logit KL; d loss / d feats; d loss / d text), everything in the inputs' dtype:
    dz = (p - onehot) / B + w_logit (p - q) / (B C); the L1 terms add w_text sign(u - o) / (C E) to du and w_image sign(x - y) / (B E)
    to dx in front of the two normalisation backwards."""
    w_text, w_image, w_logit = weights
    B, E = feats.shape
    Cn = text.shape[0]
    nf, nt = feats.norm(dim=-1, keepdim=True), text.norm(dim=-1, keepdim=True)
    x, u = feats / nf, text / nt
    y, o = zs / zs.norm(dim=-1, keepdim=True), teacher / teacher.norm(dim=-1, keepdim=True)
    z, zz = scale * x @ u.t(), scale * y @ o.t()
    logp, logq = torch.log_softmax(z, dim=-1), torch.log_softmax(zz, dim=-1)
    p, q = logp.exp(), logq.exp()
    ce = -logp[torch.arange(B), labels].mean()
    lt, li = (u - o).abs().mean(), (x - y).abs().mean()
    kl = (q * (logq - logp)).sum() / (B * Cn)
    dz = p.clone()
    dz[torch.arange(B), labels] -= 1.0
    dz = dz / B + w_logit * (p - q) / (B * Cn)
    dx = scale * dz @ u + w_image * sign0(x - y) / (B * E)
    du = scale * dz.t() @ x + w_text * sign0(u - o) / (Cn * E)
    losses = torch.stack([ce + w_text * lt + w_image * li + w_logit * kl, ce, lt, li, kl])
    return losses, (dx - x * (x * dx).sum(-1, keepdim=True)) / nf, (du - u * (u * du).sum(-1, keepdim=True)) / nt


def margins(feats, zs, text, teacher):
    """(min |u - o|, min |x - y|) over every element, in the inputs' dtype: how far the L1 terms' signs are from flipping."""
    x, u = feats / feats.norm(dim=-1, keepdim=True), text / text.norm(dim=-1, keepdim=True)
    y, o = zs / zs.norm(dim=-1, keepdim=True), teacher / teacher.norm(dim=-1, keepdim=True)
    return float((u - o).abs().min()), float((x - y).abs().min())


def frozen_features(sd, images, dtype=torch.float64, islands=False):
    """The frozen plain image tower's features: vptfit_ref's tower (or maplefit_ref's island tower) with no prompt row."""
    D = sd["visual.ln_post.weight"].shape[0]
    none = torch.zeros(1, 0, D, dtype=dtype)
    if islands:
        return mref.island_image(sd, images, none, dtype)[0]
    return vref.forward(sd, images, none, dtype)[0]


def loss_and_grads(sd, ids, p, images, labels, teacher, weights=WEIGHTS, logit_scale=LOGIT_SCALE, dtype=torch.float64, rows=None, islands=False,
                   return_features=False):
    """(losses [5], {name: gradient}) by the restatement: the frozen tower, both prompted towers forward, the head, both backwards, the
    block's layout.  ``islands``: on the towers that restate the oracle's two fp32 islands (``rows`` is then the truth's own cut)."""
    dt, dv = depths_of(p)
    ctx, deep = text_prompts(p)
    vis = vis_block(p, dtype)
    zs = frozen_features(sd, images, dtype, islands)
    if islands:
        text, tback = mref.island_text(sd, ids, ctx, deep, dtype)
        feats, vback = mref.island_image(sd, images, vis, dtype)
    else:
        text, tst = mref.text_forward(sd, ids, ctx, deep, dtype, rows)
        feats, vst = vref.forward(sd, images, vis, dtype)
    losses, d_feats, d_text = head(feats, zs, text, teacher.to(dtype), labels, math.exp(logit_scale), weights)
    if islands:
        d_ctx, d_deep = tback(d_text)
        d_vis = vback(d_feats)
    else:
        d_ctx, d_deep = mref.text_backward(sd, tst, d_text, dtype)
        d_vis = vref.backward(sd, vst, d_feats, dtype)
    grads = dict(zip(param_names(dt, dv), [d_ctx] + list(d_deep) + [d_vis[i] for i in range(dv)]))
    if return_features:
        return losses, grads, {"text": text, "feats": feats, "zs": zs}
    return losses, grads


def sgd_step(block, grad, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    """torch.optim.SGD's rule on the block; returns (block, buf); buf None on the first step."""
    g = grad + weight_decay * block
    if momentum:
        buf = g.clone() if buf is None else momentum * buf + (1 - dampening) * g
        g = g + momentum * buf if nesterov else buf
    return block - lr * g, buf


def gpa_weights(epochs, mean, std):
    """The closed form: exp(-(e - mean)^2 / (2 std^2)) over e = 1 .. epochs, normalised (the density's constant cancels)."""
    w = np.array([math.exp(-0.5 * ((e - mean) / std) ** 2) for e in range(1, epochs + 1)], dtype=np.float64)
    return w / w.sum()


def gpa(blocks, weights):
    """sum_e weights[e] * blocks[e] in float64."""
    return sum(float(w) * b.double() for w, b in zip(weights, blocks))


# ----------------------------------------------------------------------------------------------------------------------- (2) the truth
def oracle_loss_grads(sd, ids, p, images, labels, teacher, weights=WEIGHTS, logit_scale=LOGIT_SCALE, dtype=torch.float64, return_logits=False):
    """(losses [5], {name: gradient}) by torch autograd through the oracle in ``dtype`` and the reference's loss expression
    (promptsrc.py:186-210, 298-317): F.cross_entropy, two F.l1_loss(reduction='mean') and F.kl_div(log_softmax(z), log_softmax(zz),
    reduction='sum', log_target=True) / numel.  The prompts' ``.half()`` is applied to the value, the gradient passes straight through
    (maplefit_ref.oracle_loss_grads); ``ctx`` is read as it is."""
    w_text, w_image, w_logit = weights
    sd_c, ids_c = cref.cut(sd, ids)
    dt, dv = depths_of(p)
    q = {n: p[n].detach().to(dtype).clone().requires_grad_(True) for n in param_names(dt, dv)}
    hv = vref._HalfValue.apply
    ctx, deep_t = text_prompts(q)
    deep_v = [q[f"visual.transformer.resblocks.{i}.VPT_shallow"] for i in range(1, dv)]
    assert callable(getattr(orc, "_h", None)), "oracle.clip_oracle._h is gone: restate how the prompts' cast is made transparent"
    keep, orc._h = orc._h, (lambda t, d: t.to(d))
    try:
        prompts = orc.coop_prompts(sd_c, ids_c, ctx, dtype)
        tf = orc.text_encoder(sd_c, prompts, ids_c, dtype, [hv(t) for t in deep_t] or None, ctx.shape[0])
        f = orc.encode_image(sd, images.to(dtype), dtype, hv(q["visual.VPT"]), [hv(v) for v in deep_v])
        with torch.no_grad():
            zs = orc.encode_image(sd, images.to(dtype), dtype)
    finally:
        orc._h = keep
    F = torch.nn.functional
    up = (lambda t: t.float()) if dtype == torch.float16 else (lambda t: t)
    x, u = f / f.norm(dim=-1, keepdim=True), tf / tf.norm(dim=-1, keepdim=True)
    tea = teacher.to(dtype)
    y, o = zs / zs.norm(dim=-1, keepdim=True), tea / tea.norm(dim=-1, keepdim=True)
    s = math.exp(logit_scale)
    z, zz = s * x @ u.t(), s * y @ o.t()
    ce = F.cross_entropy(up(z), labels)
    lt, li = F.l1_loss(up(u), up(o), reduction="mean"), F.l1_loss(up(x), up(y), reduction="mean")
    kl = F.kl_div(F.log_softmax(up(z), dim=1), F.log_softmax(up(zz), dim=1), reduction="sum", log_target=True) / z.numel()
    total = ce + w_text * lt + w_image * li + w_logit * kl
    total.backward()
    grads = {n: (t.grad.detach() if t.grad is not None else torch.zeros_like(t)) for n, t in q.items()}
    losses = torch.stack([total, ce, lt, li, kl]).detach()
    if return_logits:      # the logits and the four normalised operands of the two L1 terms
        return losses, grads, {"z": z.detach().double(), "u": u.detach().double(), "x": x.detach().double(), "o": o.double(), "y": y.double()}
    return losses, grads


def yardstick(sd, ids, p, images, labels, teacher, weights=WEIGHTS, logit_scale=LOGIT_SCALE):
    """(losses, grads, how, {z, u, x, o, y}) of the reference's own precision: the oracle's autograd at float16 on the CPU, or, where this torch build
    lacks an fp16 CPU op of it, the fp32 oracle with weights and inputs rounded through fp16 (maplefit_ref.yardstick's fallback)."""
    try:
        l, g, z = oracle_loss_grads(sd, ids, {k: v.half() for k, v in p.items()}, images.half(), labels, teacher.half(), weights, logit_scale,
                                    torch.float16, True)
        if all(torch.isfinite(t.float()).all() for t in g.values()):
            return l.double(), {k: v.double() for k, v in g.items()}, "fp16", z
    except RuntimeError:
        pass
    sd16 = {k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()}
    l, g, z = oracle_loss_grads(sd16, ids, {k: v.half().float() for k, v in p.items()}, images.half().float(), labels, teacher.half().float(), weights,
                                logit_scale, torch.float32, True)
    return l.double(), {k: v.double() for k, v in g.items()}, "fp32-rounded", z


# ------------------------------------------------------------------------------------------------------------------------------- cases
def make_params(geom, nt, dt, nv, dv, seed=0, vision_std=0.02):
    """The prompts, fp32, from N(0, 0.02^2) (the image prompts from N(0, vision_std^2))."""
    g = syn.GEOMETRIES[geom]
    gen = torch.Generator().manual_seed(1900 + seed)
    p = {}
    for name in param_names(dt, dv):
        vis = name.startswith("visual.")
        p[name] = (vision_std if vis else 0.02) * torch.randn(nv if vis else nt, g.vision_width if vis else g.transformer_width, generator=gen)
    return p


def make_case(geom, dt, dv, nt, nv, C, B, seed=0, vision_std=0.02):
    """dict: sd, ids [C, context], p, images fp32 [B, 3, R, R], labels int64 [B], teacher fp32 [C, E] (the plain text features of the
    prompts' own ids plus noise: a teacher near the student, as the reference's is, but equal to it nowhere)."""
    g = syn.GEOMETRIES[geom]
    gen = torch.Generator().manual_seed(1950 + seed)
    images = torch.randn(B, 3, g.image_resolution, g.image_resolution, generator=gen)
    labels = torch.randint(0, C, (B,), generator=gen)
    sd, ids = cref.state_dict(geom, seed), cref.prompt_ids(geom, C, nt, seed)
    with torch.no_grad():
        plain = orc.encode_text(sd, ids).float()
    teacher = plain + 0.25 * float(plain.abs().mean()) * torch.randn(plain.shape, generator=gen)
    return {"geom": geom, "sd": sd, "ids": ids, "p": make_params(geom, nt, dt, nv, dv, seed, vision_std), "images": images, "labels": labels,
            "teacher": teacher}


def e2e_case(geom, dt, dv, nt, nv, C, B, weights, seed=0, vision_std=0.5, offset=0.02):
    """A case for the end-to-end comparison with a half-precision yardstick.  The image prompts are drawn from N(0, vision_std^2), 25
    times the usual scale.  The teacher is the float64 student's own normalised text features moved by +-``offset`` in every element:
    |u - o| is then about ``offset`` everywhere.  The frozen tower's y is not ours to choose: ``seed`` (weights, images, prompts) is.
    Adds the float64 truth (loss64, grad64, ex64), the yardstick (loss16, grad16, how, ex16), ``feature_error`` -- the yardstick's largest
    error on u and x -- and ``margin``, the smallest float64 |u - o| (with w_text > 0) or |x - y| (with w_image > 0), inf with neither.
    The caller asserts margin >= 4 feature_error: no L1 sign that any precision in play can flip."""
    c = make_case(geom, dt, dv, nt, nv, C, B, seed, vision_std)
    ctx, deep = text_prompts(c["p"])
    with torch.no_grad():
        u = mref.text_forward(c["sd"], c["ids"], ctx, deep, torch.float64)[0]
    u = u / u.norm(dim=-1, keepdim=True)
    sign = torch.randint(0, 2, u.shape, generator=torch.Generator().manual_seed(7 + seed)).double() * 2 - 1
    c["teacher"] = (u + offset * sign).float()
    c["seed"], c["weights"] = seed, weights
    args = (c["sd"], c["ids"], c["p"], c["images"], c["labels"], c["teacher"], weights)
    c["loss64"], c["grad64"], c["ex64"] = oracle_loss_grads(*args, return_logits=True)
    c["loss16"], c["grad16"], c["how"], c["ex16"] = yardstick(*args)
    c["feature_error"] = max(float((c["ex16"][k] - c["ex64"][k]).abs().max()) for k in ("u", "x"))
    e = c["ex64"]
    c["margin"] = min(float((e["u"] - e["o"]).abs().min()) if weights[0] > 0 else math.inf, float((e["x"] - e["y"]).abs().min()) if weights[1] > 0 else math.inf)
    return c


def design(nt, dt, nv, dv):
    return {"trainer": "IVLP", "vision_depth": dv, "language_depth": dt, "vision_ctx": nv, "language_ctx": nt}


live_rows = mref.live_rows

# the end-to-end cases of the GPU test, (geometry, text depth, image depth, nt, nv, C, B, live-row cut): tiny (two layers) and tiny3,
# depths (1, 1) and (3, 2) -- (2, 2) where the tower has two layers --, batches 1 and 3
E2E_CASES = [
    ("tiny", 1, 1, 2, 2, 3, 1, True),
    ("tiny", 2, 2, 2, 3, 5, 3, False),
    ("tiny3", 1, 1, 3, 2, 5, 3, False),
    ("tiny3", 3, 2, 2, 1, 3, 3, True),
    ("tiny3", 3, 2, 1, 2, 3, 1, False),
]
# the loss weights they run with: IVLP, the logit term alone, the text L1 term beside it, and the reference's three
E2E_WEIGHTS = {"ivlp": (0.0, 0.0, 0.0), "logit": (0.0, 0.0, 1.0), "text": (25.0, 0.0, 1.0), "full": WEIGHTS}

# (geometry, text depth, image depth, nt, nv, C, B, live-row cut): depths (1, 1) -- no deep slot on either side -- and (3, 2) on tiny3,
# nt != nv, batches 1 and 3; tiny for Dt = Dv and two text heads
CASES = [
    ("tiny3", 1, 1, 2, 3, 3, 1, True),
    ("tiny3", 3, 2, 2, 1, 5, 3, False),
    ("tiny", 2, 2, 3, 2, 3, 3, True),
    ("tiny", 1, 2, 1, 2, 5, 1, False),
]
