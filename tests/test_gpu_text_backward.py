"""The kernels of CoOp's training path at operator level (csrc/text_backward.hip and csrc/prompt_train.hip through clip_calibration_amd.ops), one entry point at a
time against the float64 formulas of tests/coopfit_ref.py.  Every tolerance is derived where it is used, from the number formats and the
kernel's summation, never from what the kernel returns."""
import numpy as np
import pytest
import torch

import attention_ref
import coopfit_ref as ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import ops  # noqa: E402

U32, U16 = 2.0 ** -24, 2.0 ** -11     # unit roundoffs of fp32 and fp16


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------- LayerNorm backward
@pytest.mark.parametrize("dy_dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("D,rows", ref.LN_CASES)
def test_layernorm_backward(D, rows, dy_dtype):
    g = gen(D + rows)
    x = torch.randn(rows, D, generator=g) * 1.5 + 0.3
    gamma = 1.0 + 0.2 * torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g).to(dy_dtype)
    g0 = torch.randn(rows, D, generator=g)
    want_dx = ref.ln_backward(x.double(), gamma.double(), dy.double())
    want = g0.double() + want_dx
    gd, g16 = g0.cuda(), torch.full((rows, D), 7.0, dtype=torch.float16).cuda()
    ops.layernorm_backward(x.cuda(), gamma.cuda(), dy.cuda(), gd, g16)
    got = gd.cpu()
    # fp32 sums of D <= 512 terms by a lane-strided chain and a six-level tree: <= (D / 64 + 6 + 4) roundings, 18 u at most.  The terms
    # of dX = rstd (t - mean(t) - xhat mean(t xhat)) are bounded by rstd max|t| (2 + max|xhat|); the accumulation into g adds u |g|.
    xd = x.double()
    rstd = torch.rsqrt(xd.var(-1, unbiased=False, keepdim=True) + 1e-5)
    xhat = (xd - xd.mean(-1, keepdim=True)) * rstd
    t = (dy.double() * gamma.double()).abs().amax(-1, keepdim=True)
    tol = 32 * U32 * (rstd * t * (2 + xhat.abs().amax(-1, keepdim=True))) + 2 * U32 * want.abs()
    assert ((got.double() - want).abs() <= tol).all(), float(((got.double() - want).abs() / tol).max())
    assert torch.equal(g16.cpu(), got.half())       # the fp16 operand copy is the rounded stream, bit for bit


def test_layernorm_backward_scatter_and_strided_rows():
    """Row indices (the EOT scatter of the tail): only the indexed rows of g and g16 change; x rows may be a column slice."""
    D, R, rows = 128, 40, 5
    g = gen(9)
    wide = torch.randn(R, 2 * D, generator=g).cuda()
    x = wide[:, :D]
    gamma, dy = torch.rand(D, generator=g) + 0.5, torch.randn(rows, D, generator=g)
    idx = torch.tensor([3, 0, 39, 17, 8], dtype=torch.int32)
    gd, g16 = torch.zeros(R, D).cuda(), torch.zeros(R, D, dtype=torch.float16).cuda()
    ops.layernorm_backward(x, gamma.cuda(), dy.cuda(), gd, g16, row_idx=idx.cuda())
    want = torch.zeros(R, D, dtype=torch.float64)
    want[idx.long()] = ref.ln_backward(x.cpu().double()[idx.long()], gamma.double(), dy.double())
    got = gd.cpu()
    untouched = torch.ones(R, dtype=torch.bool)
    untouched[idx.long()] = False
    assert (got[untouched] == 0).all() and (g16.cpu()[untouched] == 0).all()
    assert (got.double() - want).abs().max() <= 64 * U32 * want.abs().max() * 8
    assert torch.equal(g16.cpu(), got.half())


# ------------------------------------------------------------------------------------------------------------------------ QuickGELU
def test_quickgelu_backward():
    g = gen(5)
    special = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 5.0, -5.0, 10.0, -10.0, 20.0, -20.0, 60.0, -60.0, 1e-4, -1e-4])
    h = torch.cat([special, 3.0 * torch.randn(4096 + 3, generator=g)]).half()         # not a multiple of 8: the tail path
    da = torch.cat([torch.ones(special.numel()), torch.randn(4096 + 3, generator=g)]).half()
    got = ops.quickgelu_backward(h.cuda(), da.cuda()).cpu()
    assert torch.isfinite(got.float()).all()
    want = ref.quickgelu_backward(h.double(), da.double())
    # fp32 arithmetic with a fast exponential (relative error of a few u32 in sigma, so < 1e-5 |d_a| (1 + |h|) on the derivative, which
    # decays like |h| exp(-1.7 |h|)), then one rounding to fp16: u16 relative, or half a subnormal step 2^-25 absolute.
    tol = U16 * want.abs() + 2.0 ** -25 + 1e-5 * da.double().abs()
    assert ((got.double() - want).abs() <= tol).all()
    assert got[0] == 0.5 and got[2] == 1.0 and got[3] == 0.0


# --------------------------------------------------------------------------------------------------------------- attention backward
def attention_inputs(N, H, L, seed=0):
    g = gen(1000 * N + 10 * H + L + seed)
    qkv = (0.7 * torch.randn(N * L, 3 * 64 * H, generator=g)).half()
    do = (0.5 * torch.randn(N * L, 64 * H, generator=g)).half()
    return qkv, do


def attention_tolerance(qkv, do, N, L, H):
    """The float64 restatement and its per-element bound: derived in tests/attention_ref.py (``attention_backward``), where the CPU suite
    holds an emulation of the kernel's rounding points to it.  These inputs are flat-softmax ones: the bound without the fp32 terms."""
    return attention_ref.attention_backward(qkv, do, N, L, H, True, fp32_terms=False)


@pytest.mark.parametrize("N,H,L", ref.ATTENTION_CASES)
def test_attention_backward(N, H, L):
    qkv, do = attention_inputs(N, H, L)
    want, tol = attention_tolerance(qkv, do, N, L, H)
    pad = 3                                                   # rows behind N * L: the kernel must leave them alone
    out = torch.full((N * L + pad, 3 * 64 * H), 3.0, dtype=torch.float16).cuda()
    ops.attention_backward(qkv.cuda(), do.cuda(), N, H, out=out)
    got = out.cpu()
    assert (got[N * L:] == 3.0).all()
    got = got[:N * L]
    assert torch.isfinite(got.float()).all()
    err = (got.double() - want).abs()
    assert (err <= tol).all(), float((err / tol).max())
    again = torch.empty_like(out)
    ops.attention_backward(qkv.cuda(), do.cuda(), N, H, out=again)
    assert torch.equal(again.cpu()[:N * L], got)              # the same inputs, the same bits


@pytest.mark.parametrize("L,j0", [(20, 7), (33, 16), (77, 33), (77, 76)])
def test_attention_backward_is_causal(L, j0):
    """Keys and values at or behind token j0 cannot reach an earlier query: dq of the rows before j0 keeps its bits when they change
    (the masked triangle contributes exact zeros); dq of the rows from j0 on moves."""
    N, H = 2, 2
    D = 64 * H
    qkv, do = attention_inputs(N, H, L, seed=1)
    base = ops.attention_backward(qkv.cuda(), do.cuda(), N, H).cpu().reshape(N, L, 3 * D)
    other = qkv.clone().reshape(N, L, 3 * D)
    other[:, j0:, D:] = (other[:, j0:, D:].float() * -1.5 + 0.25).half()      # k and v of the future tokens
    moved = ops.attention_backward(other.reshape(N * L, 3 * D).cuda(), do.cuda(), N, H).cpu().reshape(N, L, 3 * D)
    assert torch.equal(moved[:, :j0, :D], base[:, :j0, :D])
    assert not torch.equal(moved[:, j0:, :D], base[:, j0:, :D])


# ------------------------------------------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("B,C,E", ref.HEAD_CASES)
@pytest.mark.parametrize("strided", [False, True])
def test_coop_head(B, C, E, strided):
    g = gen(B * 100 + C)
    wide = torch.randn(B, E + 24, generator=g)
    f = wide[:, 8:8 + E]
    text = torch.randn(C, E, generator=g) * 0.3
    y = torch.randint(0, C, (B,), generator=g)
    scale = 100.0
    loss64, d64, _ = ref.head(f.double(), y, text.double(), scale)
    loss32, d32, _ = ref.head(f.float().contiguous(), y, text.float(), scale)
    fd = wide.cuda()[:, 8:8 + E] if strided else f.contiguous().cuda()
    loss, d_text, d16 = ops.coop_head(fd, y.cuda(), text.cuda(), scale, grad_scale=4.0, want16=True)
    # the yardstick is torch's own fp32 evaluation of the same formulas on the CPU: 4 x its distance from float64.  Its floor: a logit
    # z = scale * cosine carries about eight fp32 roundings (the dot's tree, two norms, two quotients, the scale), dz <= 8 u scale; the
    # loss moves by at most 2 dz and every probability, hence every gradient entry, by at most 2 dz of the largest entry.
    dz = 8 * U32 * scale
    tol_l = max(4 * abs(float(loss32) - float(loss64)), 2 * dz)
    tol_d = max(4 * float((d32.double() - d64).abs().max()), 2 * dz * float(d64.abs().max()))
    print(f"coopfit-parity: head B={B} C={C} E={E} strided={strided} dloss={abs(float(loss.cpu()) - float(loss64)):.3e} (tol {tol_l:.3e}) "
          f"dgrad={float((d_text.cpu().double() / 4.0 - d64).abs().max()):.3e} (tol {tol_d:.3e})")
    assert abs(float(loss.cpu()) - float(loss64)) <= tol_l
    assert float((d_text.cpu().double() / 4.0 - d64).abs().max()) <= tol_d          # grad_scale is an exact factor
    assert torch.equal(d16.cpu(), d_text.cpu().half())


def test_coop_head_bad_label_poisons_and_never_addresses():
    g = gen(2)
    f, text = torch.randn(4, 64, generator=g).cuda(), torch.randn(3, 64, generator=g).cuda()
    loss, d_text = ops.coop_head(f, torch.tensor([0, 5, 1, -1]).cuda(), text, 100.0)
    assert torch.isnan(loss.cpu()).all() and torch.isnan(d_text.cpu()).any()


# ---------------------------------------------------------------------------------------------------------------------- context step
@pytest.mark.parametrize("momentum,dampening,wd,nesterov", [(0.0, 0.0, 0.0, False), (0.9, 0.0, 5e-4, False), (0.9, 0.0, 0.0, True), (0.5, 0.25, 1e-2, False)])
def test_ctx_step_is_torch_sgd_bit_for_bit(momentum, dampening, wd, nesterov):
    """One prompt: no sum, so the update must equal torch.optim.SGD applied to the kernel's own reported gradient, bit for bit --
    three steps: the first initialises the momentum buffer."""
    L, D, n_ctx = 12, 64, 4
    g = gen(7)
    ctx = torch.randn(n_ctx, D, generator=g).cuda()
    buf = torch.zeros_like(ctx) if momentum else None
    p = torch.nn.Parameter(ctx.clone())
    opt = torch.optim.SGD([p], lr=0.05, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    lr = torch.tensor([0.05]).cuda()
    for k in range(3):
        d_embed = torch.randn(L, D, generator=g).cuda()
        grad = ops.ctx_step(d_embed, 1, n_ctx, False, 8.0, ctx, buf, lr, k == 0, momentum, dampening, wd, nesterov)
        assert torch.equal(grad, d_embed[1:1 + n_ctx] * 0.125)
        p.grad = grad.clone()
        opt.step()
        assert torch.equal(ctx, p.detach()), k


@pytest.mark.parametrize("C", [3, 37])
@pytest.mark.parametrize("per_class", [False, True])
def test_ctx_step_reduction(C, per_class):
    L, D, n_ctx = 9, 128, 4
    d_embed = torch.randn(C * L, D, generator=gen(C)).cuda()
    grad = ops.ctx_step(d_embed, C, n_ctx, per_class, 2.0).cpu()
    rows = d_embed.cpu().double().reshape(C, L, D)[:, 1:1 + n_ctx]
    if per_class:
        assert torch.equal(grad, (rows / 2.0).float())           # no sum: exact
        return
    # a serial fp32 sum of C terms: (C - 1) u sum |x|; the division by a power of two is exact
    tol = (C - 1) * U32 * rows.abs().sum(0) / 2.0
    assert ((grad.double() - rows.sum(0) / 2.0).abs() <= tol).all()
    before = d_embed.clone()
    assert torch.equal(ops.ctx_step(d_embed, C, n_ctx, per_class, 2.0).cpu(), grad) and torch.equal(before, d_embed)
