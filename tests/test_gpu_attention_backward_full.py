"""clipmi_attention_backward_full at operator level, through the C ABI: attention's backward without a mask at the image tower's lengths."""
import pytest
import torch

import vptfit_ref as ref
from clip_calibration_amd import _lib, ops
from clip_calibration_amd._lib import lib

pytestmark = pytest.mark.gpu
N, H = 2, 2
D = 64 * H
FACTOR = 2.0      # the project's factor between a CPU emulation's error and the device's (fast exponential, other summation order)


def inputs(L, seed=0):
    g = torch.Generator().manual_seed(900 + 7 * L + seed)
    qkv = (torch.randn(N * L, 3 * D, generator=g) * 0.7).half()
    do = (torch.randn(N * L, D, generator=g) * 0.5).half()
    return qkv, do


def run(qkv, do, L, out):
    rc = lib.clipmi_attention_backward_full(qkv.data_ptr(), do.data_ptr(), out.data_ptr(), N, L, H, ops._stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("L", ref.ATTENTION_LENGTHS)
def test_against_float64_on_the_device_inputs(L):
    """The error against the float64 restatement on the same fp16 inputs, per output block (dq, dk, dv), within FACTOR x the error of a
    CPU emulation of the kernel's rounding points (fp32 arithmetic, P and dS rounded to fp16, fp16 outputs); element-wise, within FACTOR x
    the emulation's largest element error of the block plus one fp16 ulp of the value.  NaN-prefilled output fully overwritten, canaries
    around the exact buffer, two runs the same bits."""
    qkv, do = inputs(L)
    want = ref.attention_backward_full(qkv.double(), do.double(), N, L, H)
    emu = ref.attention_backward_full(qkv.float(), do.float(), N, L, H, lo=torch.float16).double()
    pad = 64
    buf = torch.full((pad + N * L * 3 * D + pad,), float("nan"), dtype=torch.float16)
    buf[:pad] = 3.0
    buf[-pad:] = 3.0
    dbuf = buf.cuda()
    out = dbuf[pad:pad + N * L * 3 * D]
    assert run(qkv.cuda(), do.cuda(), L, out) == _lib.OK
    back = dbuf.cpu()
    assert (back[:pad] == 3.0).all() and (back[-pad:] == 3.0).all(), "a write outside the buffer"
    got = back[pad:-pad].reshape(N * L, 3 * D)
    assert torch.isfinite(got.float()).all(), "an output element was not written"
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        w, e, g = want[:, sl], emu[:, sl], got[:, sl].double()
        r_dev, r_emu = float((g - w).norm()), float((e - w).norm())      # absolute: dq and dk are exactly zero at L = 1
        worst_dev, worst_emu = float((g - w).abs().max()), float((e - w).abs().max())
        print(f"\nattention-backward-full: L={L} {name} device |err| {r_dev:.3e} emulation |err| {r_emu:.3e} ratio {r_dev / max(r_emu, 1e-300):.2f}; "
              f"worst element {worst_dev:.3e} vs {worst_emu:.3e}")
        assert r_dev <= FACTOR * r_emu
        assert ((g - w).abs() <= FACTOR * worst_emu + 2.0 ** -10 * w.abs()).all()
    again = torch.empty(N * L * 3 * D, dtype=torch.float16, device="cuda")
    assert run(qkv.cuda(), do.cuda(), L, again) == _lib.OK
    assert torch.equal(again.cpu().reshape(N * L, 3 * D), got)


@pytest.mark.parametrize("L", [L for L in ref.ATTENTION_LENGTHS if L <= 80])
def test_short_lengths_carry_no_mask(L):
    """At the lengths the causal kernel also serves: the result is the UNMASKED restatement's -- the last key reaches the first query."""
    qkv, do = inputs(L, seed=1)
    out = torch.empty(N * L, 3 * D, dtype=torch.float16, device="cuda")
    assert run(qkv.cuda(), do.cuda(), L, out) == _lib.OK
    want = ref.attention_backward_full(qkv.double(), do.double(), N, L, H)
    assert ref.rel_fro(out.cpu(), want) <= 4e-3
    if L > 1:
        import coopfit_ref as cref
        masked = cref.attention_backward(qkv.double(), do.double(), N, L, H)
        assert ref.rel_fro(out.cpu(), masked) > 0.1


def test_padded_keys_and_queries_contribute_nothing():
    """L = 17 inside a 32-row pair of tiles: rows of another sequence behind the item (the next image's) must not reach it -- the result of
    sequence 0 keeps its bits when sequence 1 changes."""
    L = 17
    qkv, do = inputs(L)
    a = torch.empty(N * L, 3 * D, dtype=torch.float16, device="cuda")
    assert run(qkv.cuda(), do.cuda(), L, a) == _lib.OK
    qkv2, do2 = qkv.clone(), do.clone()
    qkv2[L:] = (qkv2[L:].float() * -1.5 + 0.25).half()
    do2[L:] = (do2[L:].float() * 2.0).half()
    b = torch.empty_like(a)
    assert run(qkv2.cuda(), do2.cuda(), L, b) == _lib.OK
    assert torch.equal(a[:L].cpu(), b[:L].cpu()) and not torch.equal(a[L:].cpu(), b[L:].cpu())


def test_refusals():
    x = torch.zeros(4096, dtype=torch.float16, device="cuda")
    p, s = x.data_ptr(), ops._stream()
    f = lib.clipmi_attention_backward_full
    assert f(p, p, p, 1, 225, 1, s) == _lib.ERR_SHAPE
    assert f(p, p, p, 1, 0, 1, s) == _lib.ERR_SHAPE
    assert f(p, p, p, -1, 8, 1, s) == _lib.ERR_SHAPE
    assert f(p, p, p, 1, 8, 0, s) == _lib.ERR_SHAPE
    assert f(None, p, p, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p, None, p, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p, p, None, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p + 2, p, p, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p, p + 8, p, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p, p, p + 4, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(None, None, None, 0, 8, 1, s) == _lib.OK
