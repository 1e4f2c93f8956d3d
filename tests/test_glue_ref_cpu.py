"""CPU-only: (1) the references of tests/glue_ref.py against an independent torch formulation each, so that a failure of
tests/test_gpu_glue_ops.py points at the kernel; (2) for every toleranced case of the GPU test, with the same seeds, the float32
torch-CPU evaluation of the formula stays within the tolerance the GPU test allows (so the tolerance is attainable in the kernels' own
precision) and the GEMM inputs put the ReLU's share of zeros where the GPU test expects it; (3) the C-ABI argument contract of the
ResNet / prompt-learner entry points: every refusal below happens before any launch, so it needs no GPU."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import glue_ref as ref
from clip_calibration_amd import _lib


def _within(got, want, tol, what):
    err = (got.double() - want).abs()
    worst = (err - tol).max().item()
    assert worst <= 0, f"{what}: float32 evaluation exceeds the tolerance by {worst:.3e} (max err {err.max().item():.3e})"


# ---- (1) the references ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cin,H,W,stride", [(2, 3, 12, 12, 2), (1, 3, 9, 7, 2), (2, 5, 6, 11, 1), (1, 3, 1, 1, 2), (1, 3, 1, 9, 1), (3, 4, 5, 8, 2)])
def test_im2col_nchw_ref_vs_unfold_and_conv2d(B, Cin, H, W, stride):
    g = torch.Generator().manual_seed(H * 31 + W)
    img = torch.randn(B, Cin, H, W, generator=g)
    kpad = (Cin * 9 + 63) // 64 * 64 + 64
    col = ref.im2col3x3_nchw(img, stride, kpad)
    unf = F.unfold(img.half().float(), 3, padding=1, stride=stride)                     # [B, Cin*9, Ho*Wo], row c*9 + ky*3 + kx
    assert torch.equal(col[:, :Cin * 9].float(), unf.transpose(1, 2).reshape(-1, Cin * 9))
    assert torch.count_nonzero(col[:, Cin * 9:]) == 0
    w = torch.randn(7, Cin, 3, 3, generator=g).half()
    wk = torch.zeros(7, kpad, dtype=torch.float64)
    wk[:, :Cin * 9] = w.double().reshape(7, Cin * 9)
    conv = F.conv2d(img.half().double(), w.double(), stride=stride, padding=1)           # [B, 7, Ho, Wo]
    torch.testing.assert_close(col.double() @ wk.t(), conv.permute(0, 2, 3, 1).reshape(-1, 7), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("B,H,W,C", [(2, 6, 6, 8), (1, 5, 7, 24), (3, 1, 1, 8), (1, 1, 6, 72), (2, 4, 1, 16)])
def test_im2col_nhwc_ref_vs_unfold_and_conv2d(B, H, W, C):
    g = torch.Generator().manual_seed(H * 31 + W + C)
    x = torch.randn(B, H, W, C, generator=g).half()
    kpad = (9 * C + 63) // 64 * 64
    col = ref.im2col3x3_nhwc(x, kpad)
    unf = F.unfold(x.float().permute(0, 3, 1, 2), 3, padding=1)                          # rows c*9 + t -> columns t*C + c
    unf = unf.reshape(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * C)
    assert torch.equal(col[:, :9 * C].float(), unf)
    assert torch.count_nonzero(col[:, 9 * C:]) == 0
    w = torch.randn(5, C, 3, 3, generator=g).half()
    wk = torch.zeros(5, kpad, dtype=torch.float64)
    wk[:, :9 * C] = w.double().permute(0, 2, 3, 1).reshape(5, 9 * C)                     # tap-major, as resnet.py lays the weights out
    conv = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1)
    torch.testing.assert_close(col.double() @ wk.t(), conv.permute(0, 2, 3, 1).reshape(-1, 5), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", ref.AVGPOOL_CASES, ids=str)
def test_avgpool_ref_vs_torch_and_float32(case):
    B, H, W, C, k, _ = case
    x = ref.avgpool_input(*case)
    want = ref.avgpool_nhwc(x, k)
    torch.testing.assert_close(want, F.avg_pool2d(x.double().permute(0, 3, 1, 2), k).permute(0, 2, 3, 1), rtol=1e-14, atol=1e-15)
    got32 = F.avg_pool2d(x.float().permute(0, 3, 1, 2), k).permute(0, 2, 3, 1).half()
    _within(got32, want, ref.tol_avgpool(want), "avgpool")


@pytest.mark.parametrize("case", ref.TOKENS_CASES, ids=str)
def test_attnpool_tokens_ref_and_float32(case):
    x, pos = ref.tokens_input(*case)
    rows, mean, tol = ref.attnpool_tokens(x, pos)
    direct = torch.cat([x.double().mean(dim=1, keepdim=True), x.double()], dim=1) + pos.double()[None]   # clip/model.py:70-71
    torch.testing.assert_close(mean, direct[:, 0], rtol=1e-14, atol=1e-15)
    d = (rows[:, 1:].double() - direct[:, 1:]).abs()
    assert (d <= 2.0 ** -11 * direct[:, 1:].abs() * (1 + 2.0 ** -20) + 2.0 ** -25).all()   # an fp16 rounding of the fp32 sum
    _within((x.float().mean(dim=1) + pos[0]).half(), mean, tol, "attnpool_tokens row 0")


def test_tokens_and_attnpool_ref_vs_multi_head_attention_forward():
    """The token build and the one-query attention, chained with the q / k / v projections in float64, against torch's own
    multi-head attention called the way AttentionPool2d.forward calls it (separate projection weights, the mean token as the only
    query); the output projection is the identity here because clipmi_attnpool stops before c_proj."""
    g = torch.Generator().manual_seed(5)
    for B, HW, heads in [(2, 6, 2), (1, 1, 1), (3, 49, 3)]:
        C, T = heads * 64, HW + 1
        x = torch.randn(B, HW, C, generator=g).half()
        pos = torch.randn(T, C, generator=g) * 0.5
        wq, wk, wv = (torch.randn(C, C, generator=g, dtype=torch.float64) * C ** -0.5 for _ in range(3))
        bq, bk, bv = (torch.randn(C, generator=g, dtype=torch.float64) * 0.1 for _ in range(3))
        _, mean, _ = ref.attnpool_tokens(x, pos)
        tok = torch.cat([mean[:, None], x.double() + pos.double()[None, 1:]], dim=1)                   # [B, T, C]
        q = tok[:, 0] @ wq.t() + bq
        kv = torch.cat([tok @ wk.t() + bk, tok @ wv.t() + bv], dim=-1).reshape(B * T, 2 * C)
        got, _ = ref.attnpool(q, kv, B, T, heads)
        xt = x.double().permute(1, 0, 2)                                                               # [HW, B, C]
        xt = torch.cat([xt.mean(dim=0, keepdim=True), xt], dim=0) + pos.double()[:, None, :]
        want, _ = F.multi_head_attention_forward(
            query=xt[:1], key=xt, value=xt, embed_dim_to_check=C, num_heads=heads, q_proj_weight=wq, k_proj_weight=wk, v_proj_weight=wv,
            in_proj_weight=None, in_proj_bias=torch.cat([bq, bk, bv]), bias_k=None, bias_v=None, add_zero_attn=False, dropout_p=0.0,
            out_proj_weight=torch.eye(C, dtype=torch.float64), out_proj_bias=torch.zeros(C, dtype=torch.float64),
            use_separate_proj_weight=True, training=False, need_weights=False)
        torch.testing.assert_close(got, want[0], rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("case", ref.ATTNPOOL_CASES, ids=str)
def test_attnpool_float32_within_tolerance(case):
    B, T, heads, kind = case
    q, kv = ref.attnpool_input(*case)
    want, tol = ref.attnpool(q, kv, B, T, heads)
    C = heads * 64
    k32, v32 = kv.float()[:, :C].reshape(B, T, heads, 64), kv.float()[:, C:].reshape(B, T, heads, 64)
    s = torch.einsum("bhd,bthd->bht", q.float().reshape(B, heads, 64) * 0.125, k32)
    if kind == "peaked":
        top = s.sort(dim=-1).values
        if T > 1:
            assert ((top[..., -1] - top[..., -2]) > 25).all()
    if kind == "flat":
        torch.testing.assert_close(want, kv.double()[:, C:].reshape(B, T, C).mean(dim=1), rtol=1e-9, atol=1e-9)
    got32 = torch.einsum("bht,bthd->bhd", torch.softmax(s, dim=-1), v32).reshape(B, C).half()
    _within(got32, want, tol, "attnpool")


@pytest.mark.parametrize("shape", ref.GEMM_SHAPES, ids=str)
def test_gemm_relu_inputs_float32_and_zero_share(shape):
    M, N, K = shape
    a, w, bias, res = ref.gemm_input(M, N, K)
    for epi in ref.GEMM_EPILOGUES:
        r16 = res if epi == "res16relu" else None
        want = ref.gemm_relu(a, w, bias, r16)
        y = a.float() @ w.float().t() + bias
        got = torch.relu(y + res.float() if r16 is not None else y)
        if epi != "relu32":
            got = got.half()
        scale = want.abs().max().item() + 1e-6
        assert (got.double() - want).abs().max().item() <= ref.GEMM_TOL[epi] * scale
        if M * N >= 10000:
            share = (want == 0).double().mean().item()
            assert 0.48 <= share <= 0.52, (epi, share)


def test_gemm_shapes_reach_both_epilogues_under_every_tile_kernel():
    """What the GPU test's coverage rests on: under each forced gemm_variant that is honoured (the ping-pong kernel 'a' only from two
    K-steps on, else the 256-row kernel runs again), the shape list holds a large problem whose last row tile is ragged for the
    LDS-staged fp16 epilogue (N % 8 == 0) and for the direct one (N % 8 != 0)."""
    for variant, rows in ref.GEMM_TILE_ROWS.items():
        honoured = [(M, N, K) for M, N, K in ref.GEMM_SHAPES if variant != "a" or K >= ref.GEMM_PINGPONG_MIN_K]
        for staged in (True, False):
            hit = [(M, N, K) for M, N, K in honoured if (N % 8 == 0) == staged and M > rows and M % rows != 0]
            assert hit, f"no ragged shape with {'N % 8 == 0' if staged else 'N % 8 != 0'} reaches gemm_variant {variant}"


@pytest.mark.parametrize("case", ref.CTX_CASES, ids=str)
def test_cocoop_ctx_ref_and_float32(case):
    f, w1, b1, w2, b2, ctx = ref.ctx_input(*case)
    want, tol = ref.cocoop_ctx(f, w1, b1, w2, b2, ctx)
    H, E = w1.shape
    net = torch.nn.Sequential(torch.nn.Linear(E, H), torch.nn.ReLU(), torch.nn.Linear(H, w2.shape[0])).double()   # cocoop.py:96-100
    with torch.no_grad():
        net[0].weight.copy_(w1), net[0].bias.copy_(b1), net[2].weight.copy_(w2), net[2].bias.copy_(b2)
        direct = ctx.double().unsqueeze(0) + net(f.double()).unsqueeze(1)                                            # :154-161
        torch.testing.assert_close(want, direct, rtol=1e-12, atol=1e-13)
        _within(ctx[None] + (torch.relu(f @ w1.t() + b1) @ w2.t() + b2)[:, None], want, tol, "cocoop_ctx")


@pytest.mark.parametrize("case", ref.PROMPTS_CASES, ids=str)
def test_cocoop_prompts_ref_vs_cat(case):
    nb, C, L, D, n_ctx, dtype = case
    base, ctxs = ref.prompts_input(*case)
    got = ref.cocoop_prompts(base, ctxs)
    prefix, suffix = base[:, :1].half(), base[:, 1 + n_ctx:].half()
    want = torch.stack([torch.cat([prefix, ctxs[b].half().unsqueeze(0).expand(C, -1, -1), suffix], dim=1) for b in range(nb)])   # :163-171, 185-190
    assert got.shape == (nb * C, L, D) and torch.equal(got, want.reshape(nb * C, L, D))


@pytest.mark.parametrize("case", ref.LOGITS_CASES, ids=str)
def test_logits_per_image_ref_and_float32(case):
    f, txt, _ = ref.logits_input(*case)
    want, tol, last = ref.logits_per_image(f, txt, 100.0)
    rows = []
    for b in range(f.shape[0]):                                                                         # cocoop.py:193-199
        t = txt[b].double()
        t = t / t.norm(dim=-1, keepdim=True)
        rows.append(100.0 * f[b].double() @ t.t())
    torch.testing.assert_close(want, torch.stack(rows), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(last, t, rtol=1e-14, atol=1e-15)
    t32 = txt / txt.norm(dim=-1, keepdim=True)
    _within(100.0 * torch.einsum("be,bce->bc", f, t32), want, tol, "logits_per_image")
    torch.testing.assert_close(t32[-1].double(), last, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("case", ref.ADAPTER_CASES, ids=str)
def test_adapter_blend_ref_and_float32(case):
    f, w1, w2, ratio = ref.adapter_input(*case)
    want, tol = ref.adapter_blend(f, w1, w2, ratio)
    x = f.double()
    h = F.relu(F.linear(F.relu(F.linear(x, w1.double())), w2.double()))                                 # clip_adapter.py:138-150
    torch.testing.assert_close(want, ratio * h + (1 - ratio) * x, rtol=1e-12, atol=1e-13)               # :168-169
    _within(ratio * torch.relu(torch.relu(f @ w1.t()) @ w2.t()) + (1 - ratio) * f, want, tol, "adapter_blend")


@pytest.mark.parametrize("case", ref.GROUP_MEAN_CASES, ids=str)
def test_group_mean_ref_and_float32(case):
    G, P, E = case
    x = ref.group_mean_input(*case)
    want, tol = ref.group_mean(x, P)
    torch.testing.assert_close(want, x.double().view(G, P, E).mean(dim=1), rtol=1e-14, atol=1e-16)
    s = torch.zeros(G, E)
    for p in range(P):
        s = s + x.view(G, P, E)[:, p]
    _within(s / P, want, tol, "group_mean")


@pytest.mark.parametrize("n", ref.SCALE_ADD_CASES)
def test_scale_add_ref_and_float32(n):
    a, b, alpha = ref.scale_add_input(n)
    want, tol = ref.scale_add(a, b, alpha)
    torch.testing.assert_close(want, torch.add(a.double(), b.double(), alpha=alpha), rtol=1e-15, atol=0)
    _within(a + alpha * b, want, tol, "scale_add")


# ---- (3) the argument contract ---------------------------------------------------------------------------------------------------
P = ctypes.c_void_p(4096)          # fake but aligned: never dereferenced, every call below is refused (or empty) before a launch
P8 = ctypes.c_void_p(4096 + 8)     # 8-byte aligned only
OK, ARG, SHAPE = _lib.OK, _lib.ERR_ARG, _lib.ERR_SHAPE
F16, F32 = _lib.F16, _lib.F32


def test_contract_im2col3x3_nchw():
    f = _lib.lib.clipmi_im2col3x3_nchw
    assert f(P, F32, P, 1, 3, 8, 8, 2, 48, None) == SHAPE and "Kpad=48" in _lib.last_error()     # Kpad % 64
    assert f(P, F32, P, 1, 8, 8, 8, 2, 64, None) == SHAPE                                         # Kpad < 9 * Cin
    for stride in (0, 3):
        assert f(P, F32, P, 1, 3, 8, 8, stride, 64, None) == SHAPE
    assert f(P, F32, P, 1, 3, 0, 8, 2, 64, None) == SHAPE and f(P, F32, P, -1, 3, 8, 8, 2, 64, None) == SHAPE
    assert f(P, 7, P, 1, 3, 8, 8, 2, 64, None) == ARG and "dtype" in _lib.last_error()
    assert f(None, F32, P, 1, 3, 8, 8, 2, 64, None) == ARG and f(P, F32, None, 1, 3, 8, 8, 2, 64, None) == ARG
    assert f(P, F32, P8, 1, 3, 8, 8, 2, 64, None) == ARG                                          # col takes 16-byte stores
    assert f(None, F32, None, 0, 3, 8, 8, 2, 64, None) == OK


def test_contract_im2col3x3_nhwc():
    f = _lib.lib.clipmi_im2col3x3_nhwc
    assert f(P, P, 1, 4, 4, 12, 128, None) == SHAPE                                               # C % 8
    assert f(P, P, 1, 4, 4, 8, 72, None) == SHAPE and f(P, P, 1, 4, 4, 8, 64, None) == SHAPE      # Kpad % 64, Kpad < 9 * C
    assert f(P, P, 1, 0, 4, 8, 128, None) == SHAPE
    assert f(P, P8, 1, 4, 4, 8, 128, None) == ARG and f(P8, P, 1, 4, 4, 8, 128, None) == ARG      # unaligned col / x
    assert f(None, P, 1, 4, 4, 8, 128, None) == ARG and f(P, None, 1, 4, 4, 8, 128, None) == ARG
    assert f(None, None, 0, 4, 4, 8, 128, None) == OK


def test_contract_avgpool_nhwc():
    f = _lib.lib.clipmi_avgpool_nhwc
    assert f(P, P, 1, 7, 8, 64, 2, None) == SHAPE and f(P, P, 1, 8, 7, 64, 2, None) == SHAPE      # H % k, W % k
    assert f(P, P, 1, 8, 8, 64, 0, None) == SHAPE and f(P, P, 1, 8, 8, 0, 2, None) == SHAPE
    assert f(None, P, 1, 8, 8, 64, 2, None) == ARG and f(P, None, 1, 8, 8, 64, 2, None) == ARG
    assert f(None, None, 0, 8, 8, 64, 2, None) == OK


def test_contract_attnpool_tokens_and_attnpool():
    f = _lib.lib.clipmi_attnpool_tokens
    assert f(None, P, P, 1, 49, 64, None) == ARG and f(P, None, P, 1, 49, 64, None) == ARG and f(P, P, None, 1, 49, 64, None) == ARG
    assert f(P, P, P, 1, 0, 64, None) == ARG and f(P, P, P, 1, 49, 0, None) == ARG and f(P, P, P, -1, 49, 64, None) == ARG
    assert f(None, None, None, 0, 49, 64, None) == OK
    f = _lib.lib.clipmi_attnpool
    assert f(None, P, P, 1, 50, 32, None) == ARG and f(P, None, P, 1, 50, 32, None) == ARG and f(P, P, None, 1, 50, 32, None) == ARG
    assert f(P, P, P, 1, 0, 32, None) == ARG and f(P, P, P, 1, 50, 0, None) == ARG
    assert f(None, None, None, 0, 50, 32, None) == OK


def test_contract_gemm_f16_convolution_epilogues():
    f = _lib.lib.clipmi_gemm_f16
    relu, res16 = _lib.EPI_BIAS_RELU, _lib.EPI_BIAS_RESIDUAL16_RELU
    assert (relu, res16) == (4, 5)
    for epi in (relu, res16):
        assert f(P, 64, P, 64, None, P, P, 8, F16, 8, 8, 64, epi, None) == ARG and "bias" in _lib.last_error()
        assert f(P, 64, P, 64, P8, P, P, 8, F16, 8, 8, 64, epi, None) == ARG                      # bias is read 16 bytes at a time
        assert f(P, 48, P, 48, P, P, P, 8, F16, 8, 8, 48, epi, None) == SHAPE                      # K % 64
        assert f(P, 64, P, 64, P, P, P, 6, F16, 8, 6, 64, epi, None) == SHAPE                      # N % 4
        assert f(P, 64, P, 64, P, P, P, 8, 7, 8, 8, 64, epi, None) == ARG                          # out_dtype
        assert f(None, 64, None, 64, None, None, None, 8, F16, 0, 8, 64, epi, None) == OK           # M == 0
    assert f(P, 64, P, 64, P, P, P, 8, F32, 8, 8, 64, res16, None) == ARG and "RESIDUAL16" in _lib.last_error()   # fp32 output
    assert f(P, 64, P, 64, P, None, P, 8, F16, 8, 8, 64, res16, None) == ARG                       # no residual
    assert f(P, 64, P, 64, P, ctypes.c_void_p(4096 + 2), P, 8, F16, 8, 8, 64, res16, None) == ARG   # residual is read 8 bytes at a time


def test_contract_cocoop():
    f = _lib.lib.clipmi_cocoop_ctx
    good = [P] * 7
    assert f(*good, 1, 512, 4097, 512, 4, None) == SHAPE and "H=4097" in _lib.last_error()        # H floats of LDS, 16 KiB at most
    assert f(*good, 1, 512, 32, 512, 0, None) == SHAPE and f(*good, 1, 0, 32, 512, 4, None) == SHAPE and f(*good, 1, 512, 0, 512, 4, None) == SHAPE
    for i in range(7):
        assert f(*[None if j == i else P for j in range(7)], 1, 512, 32, 512, 4, None) == ARG
    assert f(*[None] * 7, 0, 512, 32, 512, 4, None) == OK
    f = _lib.lib.clipmi_cocoop_prompts
    assert f(P, F16, P, P, 1, 1, 77, 512, 76, None) == SHAPE and f(P, F16, P, P, 1, 1, 77, 512, 77, None) == SHAPE   # n_ctx >= L - 1
    assert f(P, F16, P, P, 1, 1, 77, 512, 0, None) == SHAPE
    assert f(P, F16, P, P, 1, 1, 77, 516, 4, None) == SHAPE and "D=516" in _lib.last_error()      # D % 8
    assert f(P, F16, P, P, 1, 1, 1, 512, 4, None) == SHAPE and f(P, F16, P, P, -1, 1, 77, 512, 4, None) == SHAPE
    assert f(P, 7, P, P, 1, 1, 77, 512, 4, None) == ARG and "dtype" in _lib.last_error()
    assert f(P, F16, P, P8, 1, 1, 77, 512, 4, None) == ARG                                        # prompts takes 16-byte stores
    assert f(None, F16, P, P, 1, 1, 77, 512, 4, None) == ARG and f(P, F16, None, P, 1, 1, 77, 512, 4, None) == ARG
    assert f(P, F16, P, None, 1, 1, 77, 512, 4, None) == ARG
    assert f(None, F16, None, None, 0, 5, 77, 512, 4, None) == OK and f(None, F16, None, None, 5, 0, 77, 512, 4, None) == OK
    f = _lib.lib.clipmi_logits_per_image
    assert f(None, P, 100.0, None, P, None, None, None, 1, 3, 16, None) == ARG and f(P, None, 100.0, None, P, None, None, None, 1, 3, 16, None) == ARG
    assert f(P, P, 100.0, None, None, None, None, None, 1, 3, 16, None) == ARG
    assert f(P, P, 100.0, None, P, None, None, None, 1, 0, 16, None) == SHAPE and f(P, P, 100.0, None, P, None, None, None, 1, 3, 0, None) == SHAPE
    assert f(None, None, 100.0, None, None, None, None, None, 0, 3, 16, None) == OK


def test_contract_adapter_blend_scale_add_group_mean():
    f = _lib.lib.clipmi_adapter_blend
    assert f(P, P, P, 0.2, P, 1, 512, 8193, None) == SHAPE and "H=8193" in _lib.last_error()     # H floats of LDS, 32 KiB at most
    assert f(P, P, P, 0.2, P, 1, 512, 0, None) == SHAPE and f(P, P, P, 0.2, P, 1, 0, 32, None) == SHAPE
    for i in range(4):
        ptrs = [None if j == i else P for j in range(4)]
        assert f(ptrs[0], ptrs[1], ptrs[2], 0.2, ptrs[3], 1, 512, 32, None) == ARG
    assert f(None, None, None, 0.2, None, 0, 512, 32, None) == OK
    f = _lib.lib.clipmi_scale_add
    assert f(None, P, 0.5, P, 4, None) == ARG and f(P, None, 0.5, P, 4, None) == ARG and f(P, P, 0.5, None, 4, None) == ARG
    assert f(P, P, 0.5, P, -1, None) == ARG
    assert f(None, None, 0.5, None, 0, None) == OK
    f = _lib.lib.clipmi_group_mean
    assert f(None, P, 2, 4, 16, None) == ARG and f(P, None, 2, 4, 16, None) == ARG
    assert f(P, P, 2, 0, 16, None) == SHAPE and f(P, P, 2, 4, 0, None) == SHAPE and f(P, P, -2, 4, 16, None) == SHAPE
    assert f(None, None, 0, 4, 16, None) == OK


def test_contract_l2_normalize_to():
    f = _lib.lib.clipmi_l2_normalize_to
    assert f(None, F32, P, F16, 4, 16, None) == ARG and f(P, F32, None, F16, 4, 16, None) == ARG
    assert f(P, F32, P, F16, 4, 0, None) == SHAPE and f(P, F32, P, F16, -4, 16, None) == SHAPE
    assert f(P, 7, P, F16, 4, 16, None) == ARG and f(P, 7, P, F32, 4, 16, None) == ARG and f(P, F32, P, 7, 4, 16, None) == ARG
    assert f(None, F32, None, F16, 0, 16, None) == OK
