"""Plain references of the ModifiedResNet glue kernels (csrc/resnet.hip), the two convolution epilogues of clipmi_gemm_f16 and the
prompt-learner glue (csrc/cocoop.hip, clipmi_group_mean) -- the oracle of tests/test_glue_ref_cpu.py and tests/test_gpu_glue_ops.py.
numpy / torch-CPU, float64 wherever there is arithmetic, written from the formulas of include/clipmi.h and the reference lines it cites:

* clip/model.py:106-112, 20-37 (3x3 convolutions with padding 1, nn.AvgPool2d(k)), :69-71 (AttentionPool2d's token build), :72-90
  (its attention: the mean token is the only query, head_dim 64, scale 1/8);
* trainers/classification/cocoop.py:154-161 (meta-net and shift), :163-171 (construct_prompts), :193-199 (the per-image logits);
* trainers/classification/clip_adapter.py:138-172, taskres.py:105-106, proda.py:316-333.

Data movers return the exact fp16 result (a copy, or one IEEE round-to-nearest-even rounding, which torch's .half() is).  Arithmetic
ones return ``(value, bound)``, both float64: ``bound`` is the data-dependent part of the forward error bound the GPU test allows,
evaluated on absolute values; the ``tol_*`` functions below turn it into the tolerance.  The case lists and input generators at the
end are shared by the CPU test (which holds a float32 evaluation of every formula to the same tolerance) and the GPU test: same
seeds, same tensors.
"""
from __future__ import annotations

import torch

U16 = 2.0 ** -11      # unit roundoff of fp16
U32 = 2.0 ** -24      # unit roundoff of fp32; also the smallest fp16 subnormal


def _f64(t):
    return t.detach().cpu().to(torch.float64)


# ---------------------------------------------------------------------------------------------------------------- csrc/resnet.hip
def conv_out(n, stride):
    return (n + 2 - 3) // stride + 1


def im2col3x3_nchw(img, stride, kpad):
    """img [B,Cin,H,W] fp32|fp16 -> fp16 [B*Ho*Wo, kpad]: column c*9 + ky*3 + kx = fp16(img[b, c, yo*stride + ky - 1, xo*stride + kx - 1]),
    zero outside the image and in the padding columns."""
    B, Cin, H, W = img.shape
    Ho, Wo = conv_out(H, stride), conv_out(W, stride)
    src = img.detach().cpu().half()
    col = torch.zeros(B, Ho, Wo, kpad, dtype=torch.float16)
    for ky in range(3):
        ys = torch.arange(Ho) * stride + ky - 1
        yo = torch.nonzero((ys >= 0) & (ys < H)).flatten()
        for kx in range(3):
            xs = torch.arange(Wo) * stride + kx - 1
            xo = torch.nonzero((xs >= 0) & (xs < W)).flatten()
            if len(yo) and len(xo):
                tap = src[:, :, ys[yo]][:, :, :, xs[xo]]                                     # [B, Cin, ny, nx]
                col[:, yo[:, None], xo[None, :], ky * 3 + kx:Cin * 9:9] = tap.permute(0, 2, 3, 1)
    return col.reshape(B * Ho * Wo, kpad)


def im2col3x3_nhwc(x, kpad):
    """x [B,H,W,C] fp16 -> fp16 [B*H*W, kpad]: column (ky*3 + kx)*C + c = x[b, y + ky - 1, x + kx - 1, c], zero outside and in the padding."""
    B, H, W, C = x.shape
    src = x.detach().cpu()
    col = torch.zeros(B, H, W, kpad, dtype=torch.float16)
    for ky in range(3):
        for kx in range(3):
            t = ky * 3 + kx
            y0, y1 = max(0, 1 - ky), min(H, H + 1 - ky)       # output rows whose tap row y + ky - 1 is inside
            x0, x1 = max(0, 1 - kx), min(W, W + 1 - kx)
            if y0 < y1 and x0 < x1:
                col[:, y0:y1, x0:x1, t * C:(t + 1) * C] = src[:, y0 + ky - 1:y1 + ky - 1, x0 + kx - 1:x1 + kx - 1, :]
    return col.reshape(B * H * W, kpad)


def avgpool_nhwc(x, k):
    """x [B,H,W,C] fp16 -> float64 [B,H/k,W/k,C], the mean of each k x k window."""
    B, H, W, C = x.shape
    v = _f64(x).reshape(B, H // k, k, W // k, k, C)
    out = torch.zeros(B, H // k, W // k, C, dtype=torch.float64)
    for dy in range(k):
        for dx in range(k):
            out += v[:, :, dy, :, dx, :]
    return out / (k * k)


def tol_avgpool(ref):
    """One fp16 rounding (2^-11) of an fp32 sum whose own error is orders below, times 2; 2^-24 is the smallest fp16 subnormal."""
    return 2.0 ** -10 * ref.abs() + U32


def attnpool_tokens(x, pos):
    """x [B,HW,C] fp16, pos [HW+1,C] fp32 -> (rows fp16 [B,HW+1,C], mean float64 [B,C], tol float64 [B,C]).  rows[:, 1:] is exact
    (one fp32 add, one rounding); rows[:, 0] is only the float64 mean rounded, for the eye: compare row 0 with ``mean`` within ``tol``."""
    B, HW, C = x.shape
    xs, ps = x.detach().cpu(), pos.detach().cpu()
    rows = torch.empty(B, HW + 1, C, dtype=torch.float16)
    rows[:, 1:] = (xs.float() + ps[1:].float()[None]).half()
    mean = _f64(xs).mean(dim=1) + _f64(ps[0])[None]
    rows[:, 0] = mean.half()
    tol = tol_avgpool(mean) + HW * U32 * _f64(xs).abs().mean(dim=1)
    return rows, mean, tol


def attnpool(q, kv, B, T, heads):
    """q [B,C] fp16, kv [B*T,2C] fp16 (k | v), C = 64*heads -> (out float64 [B,C], tol float64 [B,C]): per (image, head)
    softmax_t(q . k_t / 8) applied to v.  The output is a convex combination of v[b,:,h,d] rounded once to fp16: tol = 2^-10 max_t |v|."""
    C = heads * 64
    qq = _f64(q).reshape(B, heads, 64)
    kk = _f64(kv)[:, :C].reshape(B, T, heads, 64)
    vv = _f64(kv)[:, C:].reshape(B, T, heads, 64)
    s = torch.einsum("bhd,bthd->bht", qq, kk) * 0.125
    p = torch.softmax(s, dim=-1)
    out = torch.einsum("bht,bthd->bhd", p, vv).reshape(B, C)
    tol = 2.0 ** -10 * vv.abs().amax(dim=1).reshape(B, C)
    return out, tol


# ------------------------------------------------------------------------------------------------ clipmi_gemm_f16, convolution epilogues
def gemm_relu(a, w, bias, res16=None):
    """relu(a @ w^T + bias [+ res16]) in float64 from the fp16-rounded operands (a 1x1 convolution with the folded BatchNorm as bias,
    clip/model.py:27-45)."""
    y = _f64(a) @ _f64(w).t() + _f64(bias)[None]
    if res16 is not None:
        y = y + _f64(res16)
    return torch.relu(y)


# ---------------------------------------------------------------------------------------------------------------- csrc/cocoop.hip
def _chain_tol(n, S):
    """2 n 2^-24 S: n the longest chain of fp32 additions behind an output, S the same expression on absolute values."""
    return 2.0 * n * U32 * S


def cocoop_ctx(img_n, w1, b1, w2, b2, ctx):
    """cocoop.py:154-161: ctx_shifted[b,t,:] = ctx[t,:] + W2 relu(W1 img_n[b] + b1) + b2 -> (float64 [B,n_ctx,D], tol).  ReLU is
    1-Lipschitz, so the bound of its argument carries through it."""
    f, W1, B1, W2, B2, cx = (_f64(t) for t in (img_n, w1, b1, w2, b2, ctx))
    bias = torch.relu(f @ W1.t() + B1) @ W2.t() + B2
    val = cx[None] + bias[:, None, :]
    S = (f.abs() @ W1.abs().t() + B1.abs()) @ W2.abs().t() + B2.abs()
    S = cx.abs()[None] + S[:, None, :]
    return val, _chain_tol(w1.shape[1] + w1.shape[0] + 2, S)


def cocoop_prompts(base, ctx_shifted):
    """cocoop.py:163-171: prompts[(b,c),l,:] = ctx_shifted[b,l-1,:] for 1 <= l <= n_ctx, else base[c,l,:]; fp16 [nb*C, L, D]."""
    C, L, D = base.shape
    nb, n_ctx, _ = ctx_shifted.shape
    out = base.detach().cpu().half()[None].repeat(nb, 1, 1, 1)
    out[:, :, 1:1 + n_ctx, :] = ctx_shifted.detach().cpu().half()[:, None]
    return out.reshape(nb * C, L, D)


def logits_per_image(img_n, txt, scale):
    """cocoop.py:193-199: logits[b,c] = scale <img_n[b], txt[b,c] / ||txt[b,c]||> -> (logits float64 [B,C], tol, txt_n_last float64 [C,E])."""
    f, t = _f64(img_n), _f64(txt)
    norm = t.norm(dim=-1)
    val = scale * torch.einsum("be,bce->bc", f, t) / norm
    S = abs(scale) * torch.einsum("be,bce->bc", f.abs(), t.abs()) / norm
    return val, _chain_tol(txt.shape[2] + 2, S), t[-1] / norm[-1][:, None]


def adapter_blend(f, w1, w2, ratio):
    """clip_adapter.py:138-172: ratio relu(W2 relu(W1 f)) + (1 - ratio) f -> (float64 [B,E], tol)."""
    x, W1, W2 = _f64(f), _f64(w1), _f64(w2)
    val = ratio * torch.relu(torch.relu(x @ W1.t()) @ W2.t()) + (1.0 - ratio) * x
    S = abs(ratio) * ((x.abs() @ W1.abs().t()) @ W2.abs().t()) + abs(1.0 - ratio) * x.abs()
    return val, _chain_tol(w1.shape[1] + w1.shape[0] + 2, S)


def scale_add(a, b, alpha):
    """taskres.py:105-106: a + alpha b -> (float64, tol)."""
    A, Bb = _f64(a), _f64(b)
    return A + alpha * Bb, _chain_tol(2, A.abs() + abs(alpha) * Bb.abs())


def group_mean(x, P):
    """proda.py:328-332: [G*P, E] -> the mean over the P prompts of each class, (float64 [G,E], tol)."""
    v = _f64(x).reshape(-1, P, x.shape[1])
    return v.mean(dim=1), _chain_tol(P, v.abs().mean(dim=1))


# ----------------------------------------------------------------------------------------- cases and inputs (CPU and GPU tests share them)
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 1000003 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# (B, H, W, C, k, input offset in elements): C % 8 == 0 takes 16-byte vectors, the rest -- and a vector-width C behind an 8-byte-offset
# input pointer -- one channel per thread
AVGPOOL_CASES = [(2, 112, 112, 64, 2, 0), (1, 144, 144, 80, 2, 0), (1, 24, 24, 768, 2, 0), (1, 14, 14, 2048, 2, 0), (2, 14, 14, 2048, 7, 0),
                 (1, 9, 6, 64, 3, 0), (3, 5, 7, 64, 1, 0), (1, 7, 21, 2048, 7, 0), (2, 6, 4, 3, 2, 0), (1, 7, 14, 12, 7, 0), (3, 9, 3, 100, 3, 0),
                 (1, 1, 1, 100, 1, 0), (1, 1, 5, 12, 1, 0), (5, 2, 2, 3, 1, 0), (2, 8, 6, 64, 2, 4)]


def avgpool_input(B, H, W, C, k, off):
    return torch.randn(B, H, W, C, generator=_gen(B, H, W, C, k, off)).half()


# (B, HW, C): RN50 / RN101 224 px, RN50x4 288 px, RN50x16 384 px, then ragged
TOKENS_CASES = [(2, 49, 2048), (1, 81, 2560), (1, 144, 3072), (3, 1, 64), (1, 5, 100), (5, 7, 264)]


def tokens_input(B, HW, C):
    g = _gen(B, HW, C)
    return torch.randn(B, HW, C, generator=g).half(), torch.randn(HW + 1, C, generator=g) * 0.5


# (B, T, heads, kind): T of RN50 (50), RN50x4 (82), RN50x16 (145), RN50x64 (197); B * heads in {1, 5, 32, 120} and a few more
ATTNPOOL_SHAPES = [(1, 2, 1), (5, 50, 1), (1, 50, 32), (3, 82, 40), (1, 145, 48), (1, 197, 5), (2, 197, 16)]
ATTNPOOL_KINDS = ("random", "peaked", "flat")
ATTNPOOL_CASES = [s + (kind,) for s in ATTNPOOL_SHAPES for kind in ATTNPOOL_KINDS]


def attnpool_input(B, T, heads, kind):
    """random: N(0, 1.5) as test_attention; peaked: equal keys but one per row, whose score is 30 above the rest; flat: equal keys."""
    C = heads * 64
    g = _gen(B, T, heads, ATTNPOOL_KINDS.index(kind))
    q = (torch.randn(B, C, generator=g) * 1.5).half()
    kv = torch.randn(B, T, 2 * C, generator=g) * 1.5
    if kind != "random":
        kv[:, :, :C] = kv[:, :1, :C]
        if kind == "peaked":
            qh = q.double().reshape(B, heads, 64)
            lift = (240.0 * qh / (qh * qh).sum(-1, keepdim=True)).reshape(B, C)       # q . lift / 8 = 30 per head
            peak = torch.randint(0, T, (B,), generator=g)
            kv[torch.arange(B), peak, :C] += lift.float()
    return q, kv.reshape(B * T, 2 * C).half()


# (M, N, K): the 1x1 convolutions of RN50 at batch 2 (56, 28, 14, 7 px maps), the stem GEMM, ragged ones.  N % 8 == 0 takes the LDS-staged
# fp16 epilogue, other N (260, 4) the direct one.  A forced gemm_variant 'a' (the 320-row ping-pong kernel) needs two K-steps: shapes with
# K = 64 run the 256-row kernel again under it (pick_variant, csrc/gemm.hip), so the two ragged K = 128 shapes are what takes the direct
# epilogue into the ping-pong kernel, and the K >= 128 convolution shapes the staged one (tests/test_glue_ref_cpu.py holds this list to that).
GEMM_SHAPES = [(6272, 64, 64), (6272, 256, 64), (6272, 64, 256), (6272, 128, 256), (1568, 512, 128), (1568, 128, 512), (1568, 256, 512),
               (392, 1024, 256), (392, 256, 1024), (392, 512, 1024), (98, 2048, 512), (98, 512, 2048), (25088, 64, 64),
               (513, 260, 64), (7, 64, 64), (1, 4, 64), (3000, 520, 640), (513, 260, 128), (321, 4, 128)]
GEMM_TILE_ROWS = {"0": 128, "1": 256, "a": 320}     # gemm_variant -> tile height (T128, T256w16, T320w8)
GEMM_PINGPONG_MIN_K = 128                            # below it a forced 'a' falls back to '1'
GEMM_STEM = (25088, 64, 64)        # K = 64 padded from 3 * 9 = 27: columns 27.. of both operands are zero
GEMM_EPILOGUES = ["relu16", "relu32", "res16relu"]
GEMM_TOL = {"relu16": 2e-3, "relu32": 2e-4, "res16relu": 2e-3}     # test_gemm's: fp16 out / fp32 out, times max |ref|


def gemm_input(M, N, K):
    """test_gemm's operands (zero-mean, so about half of the pre-activations are negative) + an fp16 residual."""
    g = _gen(M, N, K)
    a = torch.randn(M, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    if (M, N, K) == GEMM_STEM:
        a[:, 27:] = 0
        w[:, 27:] = 0
    bias = torch.randn(N, generator=g) * 0.1
    res = torch.randn(M, N, generator=g).half()
    return a, w, bias, res


# (B, E, H, D, n_ctx): H = E/16, H = 1, H = 4096 (the limit: 16 KiB of LDS)
CTX_CASES = [(1, 512, 32, 512, 4), (3, 1024, 64, 768, 16), (64, 640, 40, 300, 1), (3, 16, 1, 512, 4), (1, 512, 1, 300, 16),
             (3, 512, 4096, 768, 4), (64, 1024, 64, 512, 4), (3, 640, 40, 768, 16)]


def ctx_input(B, E, H, D, n_ctx):
    g = _gen(B, E, H, D, n_ctx)
    f = torch.randn(B, E, generator=g)
    f = f / f.norm(dim=-1, keepdim=True)
    return (f, torch.randn(H, E, generator=g) * E ** -0.5 * 4, torch.randn(H, generator=g) * 0.1, torch.randn(D, H, generator=g) * H ** -0.5,
            torch.randn(D, generator=g) * 0.1, torch.randn(n_ctx, D, generator=g) * 0.02)


# (B, E, H)
ADAPTER_CASES = [(1, 512, 32), (3, 1024, 64), (64, 640, 40), (3, 16, 1), (1, 512, 1), (3, 512, 4096), (64, 1024, 256)]


def adapter_input(B, E, H):
    g = _gen(B, E, H)
    return torch.randn(B, E, generator=g), torch.randn(H, E, generator=g) * E ** -0.5, torch.randn(E, H, generator=g) * H ** -0.5, 0.2


# (G, P, E)
GROUP_MEAN_CASES = [(1, 1, 512), (1000, 4, 512), (1, 32, 300), (1000, 32, 16), (37, 4, 1024), (1000, 1, 640)]


def group_mean_input(G, P, E):
    x = torch.randn(G * P, E, generator=_gen(G, P, E))
    return x / x.norm(dim=-1, keepdim=True)


SCALE_ADD_CASES = [1, 255, 775, 1000 * 512]


def scale_add_input(n):
    g = _gen(n)
    return torch.randn(n, generator=g), torch.randn(n, generator=g), 0.5


# (B, C, E)
LOGITS_CASES = [(1, 1, 512), (3, 37, 1024), (64, 37, 640), (3, 1000, 512), (5, 37, 16), (1, 1000, 300), (5, 1, 768)]


def logits_input(B, C, E):
    g = _gen(B, C, E)
    f = torch.randn(B, E, generator=g)
    f = f / f.norm(dim=-1, keepdim=True)
    txt = torch.randn(B, C, E, generator=g) * 3.0          # a different text matrix per image, un-normalised
    dac = torch.rand(C, generator=g) + 0.5
    return f, txt, dac


# (B, Cin, H, W, stride, Kpad, image dtype): the stems of RN50 224 px, RN50x4 288 px, RN50x16 384 px; odd and non-square inputs (stride 2:
# Ho = (H - 1) / 2 + 1), 1x1 and 1xN maps, Cin * 9 not a multiple of 8, Kpad one step larger than needed
IM2COL_NCHW_CASES = [(2, 3, 224, 224, 2, 64, torch.float32), (1, 3, 288, 288, 2, 64, torch.float16), (1, 3, 384, 384, 2, 64, torch.float32),
                     (1, 3, 65, 37, 2, 64, torch.float32), (3, 3, 9, 12, 1, 64, torch.float16), (1, 5, 7, 7, 2, 64, torch.float32),
                     (2, 5, 6, 11, 1, 128, torch.float32), (1, 5, 8, 5, 2, 64, torch.float16), (1, 3, 1, 1, 1, 64, torch.float32),
                     (1, 3, 1, 1, 2, 64, torch.float16), (1, 3, 1, 9, 2, 128, torch.float16), (3, 3, 5, 5, 2, 64, torch.float32),
                     (1, 3, 6, 1, 1, 64, torch.float32)]


def im2col_nchw_input(B, Cin, H, W, stride, kpad, dtype):
    return torch.randn(B, Cin, H, W, generator=_gen(B, Cin, H, W, stride, kpad)).to(dtype)


# (B, H, W, C, Kpad): stem conv2 / layer1 / layer4 of RN50, RN50x4, RN50x16; then small maps with C in {8, 24, 32, 64, 72}: with 24
# and 72 a tap starts in the middle of a 64-column group
IM2COL_NHWC_CASES = [(2, 112, 112, 32, 320), (1, 56, 56, 64, 576), (2, 7, 7, 512, 4608), (1, 144, 144, 40, 384), (1, 9, 9, 640, 5760),
                     (1, 192, 192, 48, 448), (1, 5, 7, 8, 128), (3, 3, 5, 24, 256), (1, 1, 1, 32, 320), (1, 1, 6, 72, 704), (2, 7, 4, 64, 640),
                     (5, 2, 3, 24, 256), (1, 4, 1, 72, 704)]


def im2col_nhwc_input(B, H, W, C, kpad):
    return torch.randn(B, H, W, C, generator=_gen(B, H, W, C, kpad)).half()


# (n_images, C, L, D, n_ctx, base dtype): n_ctx in {1, 4, 16, L - 2}
PROMPTS_CASES = [(1, 1, 77, 512, 4, torch.float16), (3, 37, 77, 512, 16, torch.float16), (4, 100, 20, 512, 1, torch.float32),
                 (3, 37, 18, 24, 16, torch.float16), (1, 1, 6, 24, 4, torch.float32), (4, 100, 12, 24, 4, torch.float16),
                 (3, 37, 77, 512, 75, torch.float32), (1, 1, 77, 24, 1, torch.float32), (4, 100, 3, 512, 1, torch.float16)]


def prompts_input(nb, C, L, D, n_ctx, dtype):
    g = _gen(nb, C, L, D, n_ctx)
    return torch.randn(C, L, D, generator=g).to(dtype), torch.randn(nb, n_ctx, D, generator=g)
