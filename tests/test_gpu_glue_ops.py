"""The ModifiedResNet glue kernels (csrc/resnet.hip), the two convolution epilogues of clipmi_gemm_f16 and the prompt-learner glue
(csrc/cocoop.hip, clipmi_group_mean, clipmi_l2_normalize_to with fp16 output), one entry point at a time against the plain references
of tests/glue_ref.py.  Data movers are compared bit for bit, arithmetic within the derived tolerances the references return
(tests/test_glue_ref_cpu.py holds a float32 CPU evaluation of every case to the same tolerances).  Every output is a slice out of the
middle of a larger buffer filled with a sentinel; the bytes around the slice must survive the launch (the vector kernels store 16
bytes at a time), and every launch is made twice: same input, same bits."""
import functools

import numpy as np
import pytest
import torch

import glue_ref as ref
from clip_calibration_amd import _lib

pytestmark = pytest.mark.gpu

from oracle import clip_oracle as orc  # noqa: E402  (checker only)

L = _lib.lib
F16, F32 = _lib.F16, _lib.F32
DT = {torch.float16: F16, torch.float32: F32}
PAD = 64                                    # guard elements on either side of an output
SENTINEL = {torch.float16: (torch.int16, 0x7C01), torch.float32: (torch.int32, 0x7FC00001), torch.int32: (torch.int32, -123456789)}   # NaNs


@pytest.fixture(scope="module")
def ops():
    from clip_calibration_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(SENTINEL[t.dtype][0])


class Guarded:
    """n elements in the middle of a sentinel-filled buffer."""

    def __init__(self, n, dtype, init=None):
        self.n, (self.idt, self.mark) = n, SENTINEL[dtype]
        self.buf = torch.empty(2 * PAD + n, dtype=dtype, device="cuda")
        self.buf.view(self.idt).fill_(self.mark)
        self.view = self.buf[PAD:PAD + n]
        if init is not None:
            self.view.copy_(init.reshape(-1))
        self.ptr = self.view.data_ptr() if n else self.buf.data_ptr() + PAD * self.buf.element_size()

    def result(self, what):
        torch.cuda.synchronize()
        b = self.buf.view(self.idt).cpu()
        assert (b[:PAD] == self.mark).all() and (b[PAD + self.n:] == self.mark).all(), f"{what}: wrote outside its output"
        return self.view.cpu().clone()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf.view(self.idt) == self.mark).all())


def _check(rc, what):
    _lib.check(rc, what)


def _twice(n, dtype, what, call, init=None):
    """Launch ``call(out_ptr)`` into two guarded buffers: guards intact, same bits both times; returns the output (CPU, flat)."""
    outs = []
    for _ in range(2):
        g = Guarded(n, dtype, init)
        _check(call(g.ptr), what)
        outs.append(g.result(what))
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), f"{what}: two launches on the same input differ"
    return outs[0]


def _assert_bits(got, want, what):
    got, want = got.reshape(want.shape), want.contiguous()
    bad = torch.nonzero(_bits(got) != _bits(want))
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {want.numel()} elements differ, first at {bad[0].tolist()}: got {got[tuple(bad[0].tolist())].item()}, want {want[tuple(bad[0].tolist())].item()}"


def _assert_within(got, want, tol, what):
    got = got.reshape(want.shape).double()
    over = (got - want).abs() - tol
    over[torch.isnan(over)] = float("inf")
    i = over.argmax()
    assert over.flatten()[i] <= 0, (f"{what}: worst at {np.unravel_index(int(i), tuple(want.shape))}: got {got.flatten()[i].item()!r}, want "
                                    f"{want.flatten()[i].item()!r}, tol {torch.as_tensor(tol).expand(want.shape).flatten()[i].item():.3e}")


# ---- csrc/resnet.hip -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.IM2COL_NCHW_CASES, ids=str)
def test_im2col3x3_nchw_exact(case):
    """clipmi_im2col3x3_nchw: every column of every row, border taps and padding columns included, bit for bit."""
    B, Cin, H, W, stride, kpad, dtype = case
    img = ref.im2col_nchw_input(*case)
    d = img.cuda()
    rows = B * ref.conv_out(H, stride) * ref.conv_out(W, stride)
    got = _twice(rows * kpad, torch.float16, "clipmi_im2col3x3_nchw",
                 lambda p: L.clipmi_im2col3x3_nchw(d.data_ptr(), DT[dtype], p, B, Cin, H, W, stride, kpad, _stream()))
    _assert_bits(got, ref.im2col3x3_nchw(img, stride, kpad), "clipmi_im2col3x3_nchw [row, column]")


@pytest.mark.parametrize("case", ref.IM2COL_NHWC_CASES, ids=str)
def test_im2col3x3_nhwc_exact(case):
    """clipmi_im2col3x3_nhwc at the sizes the tower sends to the implicit GEMM instead, and with taps that straddle 64-column groups."""
    B, H, W, C, kpad = case
    x = ref.im2col_nhwc_input(*case)
    d = x.cuda()
    got = _twice(B * H * W * kpad, torch.float16, "clipmi_im2col3x3_nhwc",
                 lambda p: L.clipmi_im2col3x3_nhwc(d.data_ptr(), p, B, H, W, C, kpad, _stream()))
    _assert_bits(got, ref.im2col3x3_nhwc(x, kpad), "clipmi_im2col3x3_nhwc [row, column]")


@pytest.mark.parametrize("case", ref.AVGPOOL_CASES, ids=str)
def test_avgpool_nhwc(case):
    """clipmi_avgpool_nhwc, vector path (C % 8 == 0) and scalar path (other C, or an input that is only 8-byte aligned):
    |got - ref| <= 2^-10 |ref| + 2^-24."""
    B, H, W, C, k, off = case
    x = ref.avgpool_input(*case)
    store = torch.empty(x.numel() + 8, dtype=torch.float16, device="cuda")
    d = store[off:off + x.numel()]
    d.copy_(x.reshape(-1))
    assert d.data_ptr() % 16 == 2 * off
    got = _twice(x.numel() // (k * k), torch.float16, "clipmi_avgpool_nhwc",
                 lambda p: L.clipmi_avgpool_nhwc(d.data_ptr(), p, B, H, W, C, k, _stream()))
    want = ref.avgpool_nhwc(x, k)
    _assert_within(got, want, ref.tol_avgpool(want), "clipmi_avgpool_nhwc [b, y, x, c]")


@pytest.mark.parametrize("case", ref.TOKENS_CASES, ids=str)
def test_attnpool_tokens(case):
    """clipmi_attnpool_tokens: rows 1..HW bit for bit (one fp32 add, one rounding), row 0 (the mean) within the avgpool bound plus
    HW 2^-24 mean|x| for the sequential fp32 sum."""
    B, HW, C = case
    x, pos = ref.tokens_input(*case)
    dx, dp = x.cuda(), pos.cuda()
    got = _twice(B * (HW + 1) * C, torch.float16, "clipmi_attnpool_tokens",
                 lambda p: L.clipmi_attnpool_tokens(dx.data_ptr(), dp.data_ptr(), p, B, HW, C, _stream())).reshape(B, HW + 1, C)
    rows, mean, tol = ref.attnpool_tokens(x, pos)
    _assert_bits(got[:, 1:], rows[:, 1:], "clipmi_attnpool_tokens rows 1.. [b, token - 1, c]")
    _assert_within(got[:, 0], mean, tol, "clipmi_attnpool_tokens row 0 [b, c]")


@pytest.mark.parametrize("case", ref.ATTNPOOL_CASES, ids=str)
def test_attnpool(case):
    """clipmi_attnpool: a convex combination of v rounded once, |got - ref| <= 2^-10 max_t |v|; random, peaked and flat score rows."""
    B, T, heads, kind = case
    q, kv = ref.attnpool_input(*case)
    dq, dkv = q.cuda(), kv.cuda()
    got = _twice(B * heads * 64, torch.float16, "clipmi_attnpool",
                 lambda p: L.clipmi_attnpool(dq.data_ptr(), dkv.data_ptr(), p, B, T, heads, _stream()))
    want, tol = ref.attnpool(q, kv, B, T, heads)
    _assert_within(got, want, tol, f"clipmi_attnpool ({kind}) [b, head * 64 + d]")


# ---- clipmi_gemm_f16: EPI_BIAS_RELU, EPI_BIAS_RESIDUAL16_RELU ----------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _gemm_case(shape):
    a, w, bias, res = ref.gemm_input(*shape)
    want = {"relu16": ref.gemm_relu(a, w, bias), "res16relu": ref.gemm_relu(a, w, bias, res)}
    want["relu32"] = want["relu16"]
    return tuple(t.cuda() for t in (a, w, bias, res)), want


@pytest.mark.parametrize("variant", [None, "0", "1", "a"])       # (the decorator nearest the function varies slowest: one reference per shape)
@pytest.mark.parametrize("epi", ref.GEMM_EPILOGUES)
@pytest.mark.parametrize("shape", ref.GEMM_SHAPES, ids=str)
def test_gemm_relu_epilogues(clipmi_option, shape, epi, variant):
    """clipmi_gemm_f16 with EPI_BIAS_RELU (fp16 and fp32 output) and EPI_BIAS_RESIDUAL16_RELU under each tile kernel (gemm_variant 0 =
    T128, 1 = T256w16, a = T320w8 ping-pong from K = 128 on: glue_ref.GEMM_SHAPES says which shapes that is) and under the cost model's choice, against relu(a w^T + bias [+ res16]) in
    float64; test_gemm's tolerance and scaling.  N % 8 == 0 takes the LDS-staged fp16 epilogue, N = 260 and N = 4 the direct one.  About
    half of the pre-activations are negative: the share of exact zeros in a large output must say so, which a ReLU applied before the
    residual add, or not at all, cannot."""
    M, N, K = shape
    (a, w, bias, res), want = _gemm_case(shape)
    clipmi_option("gemm_variant", _lib.gemm_variant_id(variant))
    code = _lib.EPI_BIAS_RESIDUAL16_RELU if epi == "res16relu" else _lib.EPI_BIAS_RELU
    pres = res.data_ptr() if epi == "res16relu" else None
    odt = torch.float32 if epi == "relu32" else torch.float16
    got = _twice(M * N, odt, "clipmi_gemm_f16", lambda p: L.clipmi_gemm_f16(a.data_ptr(), K, w.data_ptr(), K, bias.data_ptr(), pres, p, N, DT[odt],
                                                                            M, N, K, code, _stream())).reshape(M, N).double()
    r = want[epi]
    scale = r.abs().max().item() + 1e-6
    err = (got - r).abs()
    err[torch.isnan(err)] = float("inf")
    i = int(err.argmax())
    assert err.flatten()[i] <= ref.GEMM_TOL[epi] * scale, f"max err {err.flatten()[i].item()} at [{i // N}, {i % N}] vs scale {scale}"
    if M * N >= 10000:
        share = (got == 0).double().mean().item()
        assert 0.45 <= share <= 0.55, f"share of exact zeros {share}"


# ---- csrc/cocoop.hip, clipmi_group_mean, clipmi_l2_normalize_to --------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CTX_CASES, ids=str)
def test_cocoop_ctx(case):
    """clipmi_cocoop_ctx against float64 within 2 (E + H + 2) 2^-24 S."""
    B, E, H, D, n_ctx = case
    host = ref.ctx_input(*case)
    f, w1, b1, w2, b2, ctx = (t.cuda() for t in host)
    got = _twice(B * n_ctx * D, torch.float32, "clipmi_cocoop_ctx",
                 lambda p: L.clipmi_cocoop_ctx(f.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), ctx.data_ptr(), p,
                                               B, E, H, D, n_ctx, _stream()))
    want, tol = ref.cocoop_ctx(*host)
    _assert_within(got, want, tol, "clipmi_cocoop_ctx [b, t, d]")


@pytest.mark.parametrize("case", ref.PROMPTS_CASES, ids=str)
def test_cocoop_prompts_exact(case):
    """clipmi_cocoop_prompts bit for bit: rows 0, 1, n_ctx, n_ctx + 1 and L - 1 of every (image, class) pair sit on the boundaries."""
    nb, C, Lc, D, n_ctx, dtype = case
    base, ctxs = ref.prompts_input(*case)
    db, dc = base.cuda(), ctxs.cuda()
    got = _twice(nb * C * Lc * D, torch.float16, "clipmi_cocoop_prompts",
                 lambda p: L.clipmi_cocoop_prompts(db.data_ptr(), DT[dtype], dc.data_ptr(), p, nb, C, Lc, D, n_ctx, _stream()))
    _assert_bits(got, ref.cocoop_prompts(base, ctxs), "clipmi_cocoop_prompts [(b, c), l, d]")


def _logits_call(f, txt, dac, want_cp, want_last, B, C, E):
    lg, conf, pred, last = Guarded(B * C, torch.float32), Guarded(B, torch.float32), Guarded(B, torch.int32), Guarded(C * E, torch.float32)
    _check(L.clipmi_logits_per_image(f.data_ptr(), txt.data_ptr(), 100.0, None if dac is None else dac.data_ptr(), lg.ptr,
                                     conf.ptr if want_cp else None, pred.ptr if want_cp else None, last.ptr if want_last else None,
                                     B, C, E, _stream()), "clipmi_logits_per_image")
    out = [lg.result("logits").reshape(B, C)]
    if want_cp:
        out += [conf.result("conf"), pred.result("pred")]
    else:
        assert conf.untouched() and pred.untouched()
    if want_last:
        out.append(last.result("txt_n_last").reshape(C, E))
    else:
        assert last.untouched()
    return out


@pytest.mark.parametrize("case", ref.LOGITS_CASES, ids=str)
def test_logits_per_image(case):
    """clipmi_logits_per_image: logits against float64 within 2 (E + 2) 2^-24 S; txt_n_last = the LAST image's normalised text rows
    (every image has its own text matrix, so rows of any other image fail); the call with dac_conf / conf / pred = the call without
    followed by clipmi_calibrate_rows on its logits, bit for bit; DAC values against the oracle as test_l2_and_logits_dac_conf_pred."""
    B, C, E = case
    hf, htxt, hdac = ref.logits_input(*case)
    f, txt, dac = hf.cuda(), htxt.cuda(), hdac.cuda()
    lg, last = _logits_call(f, txt, None, False, True, B, C, E)
    lg_again, last_again = _logits_call(f, txt, None, False, True, B, C, E)
    assert torch.equal(_bits(lg), _bits(lg_again)) and torch.equal(_bits(last), _bits(last_again)), "two launches differ"
    want, tol, want_last = ref.logits_per_image(hf, htxt, 100.0)
    _assert_within(lg, want, tol, "clipmi_logits_per_image logits [b, c]")
    np.testing.assert_allclose(last.numpy(), want_last.numpy(), rtol=1e-6, atol=1e-7)
    (lg_nolast,) = _logits_call(f, txt, None, False, False, B, C, E)             # a null txt_n_last is allowed
    _assert_bits(lg_nolast, lg, "logits without txt_n_last")
    for d in (None, dac):
        lg2, conf2, pred2 = _logits_call(f, txt, d, True, False, B, C, E)
        sep, conf, pred = Guarded(B * C, torch.float32, lg), Guarded(B, torch.float32), Guarded(B, torch.int32)
        _check(L.clipmi_calibrate_rows(sep.ptr, None if d is None else d.data_ptr(), conf.ptr, pred.ptr, B, C, _stream()), "clipmi_calibrate_rows")
        _assert_bits(lg2, sep.result("calibrate_rows").reshape(B, C), "logits: fused row pass vs clipmi_calibrate_rows")
        _assert_bits(conf2, conf.result("conf"), "conf: fused row pass vs clipmi_calibrate_rows")
        _assert_bits(pred2, pred.result("pred"), "pred: fused row pass vs clipmi_calibrate_rows")
        scaled = lg.numpy() if d is None else orc.dac_predict(lg.numpy(), hdac.numpy())
        np.testing.assert_allclose(lg2.numpy(), scaled, rtol=1e-6, atol=1e-6)
        c_ref, p_ref = orc.conf_pred(orc.softmax_probs(scaled.astype(np.float64)))
        assert np.array_equal(pred2.numpy(), p_ref)
        np.testing.assert_allclose(conf2.numpy(), c_ref, rtol=2e-5)


@pytest.mark.parametrize("case", ref.ADAPTER_CASES, ids=str)
def test_adapter_blend(case):
    """clipmi_adapter_blend against float64 within 2 (E + H + 2) 2^-24 S."""
    B, E, H = case
    hf, hw1, hw2, ratio = ref.adapter_input(*case)
    f, w1, w2 = hf.cuda(), hw1.cuda(), hw2.cuda()
    got = _twice(B * E, torch.float32, "clipmi_adapter_blend",
                 lambda p: L.clipmi_adapter_blend(f.data_ptr(), w1.data_ptr(), w2.data_ptr(), ratio, p, B, E, H, _stream()))
    want, tol = ref.adapter_blend(hf, hw1, hw2, ratio)
    _assert_within(got, want, tol, "clipmi_adapter_blend [b, e]")


@pytest.mark.parametrize("n", ref.SCALE_ADD_CASES)
def test_scale_add_and_in_place(n):
    """clipmi_scale_add against float64 within 4 * 2^-24 S, and with out aliasing a (the header allows it): the same bits."""
    ha, hb, alpha = ref.scale_add_input(n)
    a, b = ha.cuda(), hb.cuda()
    got = _twice(n, torch.float32, "clipmi_scale_add", lambda p: L.clipmi_scale_add(a.data_ptr(), b.data_ptr(), alpha, p, n, _stream()))
    want, tol = ref.scale_add(ha, hb, alpha)
    _assert_within(got, want, tol, "clipmi_scale_add")
    in_place = _twice(n, torch.float32, "clipmi_scale_add (out = a)", lambda p: L.clipmi_scale_add(p, b.data_ptr(), alpha, p, n, _stream()), init=ha)
    _assert_bits(in_place, got, "clipmi_scale_add with out aliasing a")


@pytest.mark.parametrize("case", ref.GROUP_MEAN_CASES, ids=str)
def test_group_mean(case):
    """clipmi_group_mean against float64 within 2 P 2^-24 mean|x|."""
    G, P, E = case
    hx = ref.group_mean_input(*case)
    x = hx.cuda()
    got = _twice(G * E, torch.float32, "clipmi_group_mean", lambda p: L.clipmi_group_mean(x.data_ptr(), p, G, P, E, _stream()))
    want, tol = ref.group_mean(hx, P)
    _assert_within(got, want, tol, "clipmi_group_mean [g, e]")


@pytest.mark.parametrize("E", [16, 512, 1000, 1024, 20])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_l2_normalize_to_f16_is_the_f32_value_rounded_once(ops, E, dtype):
    """clipmi_l2_normalize_to with fp16 output = ops.l2_normalize(x).half() bit for bit (E = 20: the scalar path)."""
    rows = 37
    x = (torch.randn(rows, E, generator=torch.Generator().manual_seed(E)) * 3).to(dtype).cuda()
    want = ops.l2_normalize(x).half().cpu()
    _assert_bits(ops.l2_normalize(x, torch.float16).cpu(), want, "ops.l2_normalize(x, float16) [row, e]")
    got = _twice(rows * E, torch.float16, "clipmi_l2_normalize_to",
                 lambda p: L.clipmi_l2_normalize_to(x.data_ptr(), DT[dtype], p, F16, rows, E, _stream()))
    _assert_bits(got, want, "clipmi_l2_normalize_to [row, e]")


def test_empty_batch_is_ok_and_writes_nothing():
    """B == 0 (n == 0, G == 0, rows == 0, M == 0): every entry point returns OK and stores nothing."""
    g16, g32 = Guarded(256, torch.float16), Guarded(256, torch.float32)
    src = torch.zeros(4096, dtype=torch.float32, device="cuda")
    s, p, o16, o32, st = src.data_ptr(), src.data_ptr(), g16.ptr, g32.ptr, _stream()
    for what, rc in [("clipmi_im2col3x3_nchw", L.clipmi_im2col3x3_nchw(s, F32, o16, 0, 3, 8, 8, 2, 64, st)),
                     ("clipmi_im2col3x3_nhwc", L.clipmi_im2col3x3_nhwc(s, o16, 0, 4, 4, 8, 128, st)),
                     ("clipmi_avgpool_nhwc", L.clipmi_avgpool_nhwc(s, o16, 0, 4, 4, 8, 2, st)),
                     ("clipmi_attnpool_tokens", L.clipmi_attnpool_tokens(s, p, o16, 0, 4, 64, st)),
                     ("clipmi_attnpool", L.clipmi_attnpool(s, p, o16, 0, 5, 1, st)),
                     ("clipmi_gemm_f16 RELU", L.clipmi_gemm_f16(s, 64, p, 64, p, None, o16, 64, F16, 0, 64, 64, _lib.EPI_BIAS_RELU, st)),
                     ("clipmi_gemm_f16 RESIDUAL16_RELU", L.clipmi_gemm_f16(s, 64, p, 64, p, p, o16, 64, F16, 0, 64, 64, _lib.EPI_BIAS_RESIDUAL16_RELU, st)),
                     ("clipmi_cocoop_ctx", L.clipmi_cocoop_ctx(s, p, p, p, p, p, o32, 0, 16, 1, 8, 2, st)),
                     ("clipmi_cocoop_prompts nb", L.clipmi_cocoop_prompts(s, F32, p, o16, 0, 3, 6, 8, 2, st)),
                     ("clipmi_cocoop_prompts C", L.clipmi_cocoop_prompts(s, F32, p, o16, 3, 0, 6, 8, 2, st)),
                     ("clipmi_logits_per_image", L.clipmi_logits_per_image(s, p, 100.0, None, o32, o32, None, o32, 0, 3, 16, st)),
                     ("clipmi_adapter_blend", L.clipmi_adapter_blend(s, p, p, 0.2, o32, 0, 16, 1, st)),
                     ("clipmi_scale_add", L.clipmi_scale_add(s, p, 0.5, o32, 0, st)),
                     ("clipmi_group_mean", L.clipmi_group_mean(s, o32, 0, 4, 16, st)),
                     ("clipmi_l2_normalize_to", L.clipmi_l2_normalize_to(s, F32, o16, F16, 0, 16, st))]:
        assert rc == _lib.OK, what
    assert g16.untouched() and g32.untouched()
