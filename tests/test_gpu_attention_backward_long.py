"""clipmi_attention_backward_long at operator level, through the C ABI: attention's backward without a mask at ViT-L/14's lengths, in two
launches over blocks of 64 rows with the row statistics in a workspace."""
import functools

import pytest
import torch

import attention_ref as aref
import vptfit_ref as ref
from clip_calibration_amd import _lib, ops
from clip_calibration_amd._lib import lib

pytestmark = pytest.mark.gpu
N, H = 2, 2
D = 64 * H
FACTOR = 2.0      # the project's factor between a CPU emulation's error and the device's (fast exponential, other summation order)
QUERY_BLOCK = KEY_BLOCK = 64     # rows per workgroup and per LDS block, on the query-owned and on the key-owned side (attention.hip ABL_BLOCK)
LENGTHS = sorted({1, 15, 16, 17, 63, 64, 65, 224, 225, 256, 257, 259, 265, 577, 581, 585, 639, 640} |
                 {b + d for b in (QUERY_BLOCK, KEY_BLOCK) for d in (-1, 0, 1)} | {2 * QUERY_BLOCK + 1, 2 * KEY_BLOCK + 1})
PAD = 64


def inputs(L, seed=0):
    g = torch.Generator().manual_seed(900 + 7 * L + seed)
    qkv = (torch.randn(N * L, 3 * D, generator=g) * 0.7).half()
    do = (torch.randn(N * L, D, generator=g) * 0.5).half()
    return qkv, do


def ws_bytes(L, n=N, h=H):
    return lib.clipmi_attention_backward_long_bytes(n, L, h)


def run(qkv, do, L, out, ws=None, n=N, h=H):
    if ws is None:
        ws = torch.empty(max(ws_bytes(L, n, h), 16), dtype=torch.uint8, device="cuda")
    rc = lib.clipmi_attention_backward_long(qkv.data_ptr(), do.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), n, L, h, ops._stream())
    torch.cuda.synchronize()
    return rc


@functools.lru_cache(maxsize=None)
def references(L, seed=0):
    """(float64 result, CPU emulation with the kernel's rounding points) on the fp16 inputs of ``inputs(L, seed)``; computed once."""
    qkv, do = inputs(L, seed)
    want = ref.attention_backward_full(qkv.double(), do.double(), N, L, H)
    emu = ref.attention_backward_full(qkv.float(), do.float(), N, L, H, lo=torch.float16).double()
    return want, emu


def held(got, want, emu, what):
    """The sibling's criterion: per block the Frobenius error within FACTOR x the emulation's, every element within FACTOR x the emulation's
    worst element error of the block plus 2^-10 |w|.  -> the largest Frobenius ratio."""
    worst_ratio = 0.0
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        w, e, g = want[:, sl], emu[:, sl], got[:, sl].double()
        r_dev, r_emu = float((g - w).norm()), float((e - w).norm())      # absolute: dq and dk are exactly zero at L = 1
        worst_dev, worst_emu = float((g - w).abs().max()), float((e - w).abs().max())
        ratio = r_dev / max(r_emu, 1e-300)
        print(f"\n{what} {name} device |err| {r_dev:.3e} emulation |err| {r_emu:.3e} ratio {ratio:.2f}; worst element {worst_dev:.3e} vs {worst_emu:.3e}")
        assert r_dev <= FACTOR * r_emu
        assert ((g - w).abs() <= FACTOR * worst_emu + 2.0 ** -10 * w.abs()).all()
        worst_ratio = max(worst_ratio, ratio if r_emu > 0 else 0.0)
    return worst_ratio


@pytest.mark.parametrize("L", LENGTHS)
def test_against_float64_on_the_device_inputs(L):
    """The sibling's criterion against float64 on the same fp16 inputs, at ViT-L/14's lengths and at B - 1, B, B + 1, 2 B + 1 of the block
    size B = 64 of either launch.  NaN-prefilled output fully overwritten, canaries around the exact output and around the exact workspace,
    two runs the same bits."""
    qkv, do = inputs(L)
    want, emu = references(L)
    buf = torch.full((PAD + N * L * 3 * D + PAD,), float("nan"), dtype=torch.float16)
    buf[:PAD] = 3.0
    buf[-PAD:] = 3.0
    dbuf = buf.cuda()
    out = dbuf[PAD:PAD + N * L * 3 * D]
    need = ws_bytes(L)
    assert need == 12 * N * H * L
    wbuf = torch.full((PAD + need // 4 + PAD,), 5.0, dtype=torch.float32)
    wbuf[PAD:-PAD] = float("nan")
    dws = wbuf.cuda()
    ws = dws[PAD:PAD + need // 4].view(torch.uint8)
    assert ws.numel() == need
    assert run(qkv.cuda(), do.cuda(), L, out, ws) == _lib.OK
    back, wback = dbuf.cpu(), dws.cpu()
    assert (back[:PAD] == 3.0).all() and (back[-PAD:] == 3.0).all(), "a write outside the buffer"
    assert (wback[:PAD] == 5.0).all() and (wback[-PAD:] == 5.0).all(), "a write outside the workspace"
    assert torch.isfinite(wback[PAD:-PAD]).all(), "a statistic was not written"
    got = back[PAD:-PAD].reshape(N * L, 3 * D)
    assert torch.isfinite(got.float()).all(), "an output element was not written"
    held(got, want, emu, f"attention-backward-long: L={L}")
    again = torch.empty(N * L * 3 * D, dtype=torch.float16, device="cuda")
    assert run(qkv.cuda(), do.cuda(), L, again) == _lib.OK
    assert torch.equal(again.cpu().reshape(N * L, 3 * D), got)


@pytest.mark.parametrize("L", (17, 113, 197, 224))
def test_agrees_with_the_one_block_sibling(L):
    """Where clipmi_attention_backward_full also runs, both hold the same bound against float64 on the same inputs (not the same bits: the
    softmax sums are taken per key block here).  Largest Frobenius ratio against the emulation seen on an MI355X: 1.00 for either kernel
    at every length; largest element difference between the two 6.1e-5 (at L = 197; none at L = 17)."""
    qkv, do = inputs(L, seed=2)
    want, emu = references(L, 2)
    a = torch.empty(N * L, 3 * D, dtype=torch.float16, device="cuda")
    b = torch.empty_like(a)
    assert run(qkv.cuda(), do.cuda(), L, a) == _lib.OK
    assert lib.clipmi_attention_backward_full(qkv.cuda().data_ptr(), do.cuda().data_ptr(), b.data_ptr(), N, L, H, ops._stream()) == _lib.OK
    torch.cuda.synchronize()
    ra = held(a.cpu(), want, emu, f"long at L={L}")
    rb = held(b.cpu(), want, emu, f"full at L={L}")
    diff = (a.cpu().double() - b.cpu().double()).abs()
    print(f"\nlong vs full at L={L}: ratios {ra:.3f} / {rb:.3f}, largest difference {float(diff.max()):.3e}")


@pytest.mark.parametrize("L", (257, 577 + 4))
def test_padding_isolation(L):
    """Rows behind the item (the next image's) and the other head's columns never reach an item: sequence 0 keeps its bits when sequence 1
    changes, and head 0's output columns keep theirs when head 1's operand columns change."""
    qkv, do = inputs(L)
    a = torch.empty(N * L, 3 * D, dtype=torch.float16, device="cuda")
    assert run(qkv.cuda(), do.cuda(), L, a) == _lib.OK
    qkv2, do2 = qkv.clone(), do.clone()
    qkv2[L:] = (qkv2[L:].float() * -1.5 + 0.25).half()
    do2[L:] = (do2[L:].float() * 2.0).half()
    b = torch.empty_like(a)
    assert run(qkv2.cuda(), do2.cuda(), L, b) == _lib.OK
    assert torch.equal(a[:L].cpu(), b[:L].cpu()) and not torch.equal(a[L:].cpu(), b[L:].cpu())
    qkv3, do3 = qkv.clone().reshape(N * L, 3, H, 64), do.clone().reshape(N * L, H, 64)
    qkv3[:, :, 1] = (qkv3[:, :, 1].float() * 1.25 - 0.5).half()
    do3[:, 1] = (do3[:, 1].float() * -2.0).half()
    c = torch.empty_like(a)
    assert run(qkv3.reshape(N * L, 3 * D).cuda(), do3.reshape(N * L, D).cuda(), L, c) == _lib.OK
    a4, c4 = a.cpu().reshape(N * L, 3, H, 64), c.cpu().reshape(N * L, 3, H, 64)
    assert torch.equal(a4[:, :, 0], c4[:, :, 0]) and not torch.equal(a4[:, :, 1], c4[:, :, 1])


def test_permutation_softmax_is_exact_across_block_seams():
    """attention_ref.selection_backward_batch, kind "perm", at L = 257 (five blocks of 64 on either side, the last with one row): every
    query's softmax is one-hot in fp16 on the key pi(q) -- anywhere in the sequence, so in another block than the query for most rows --
    so dq == 0 and dk == 0 in every element and dv is a row permutation of d_out bit for bit.  The running maximum passes through blocks
    whose best key trails the target by 64 natural units: the rescaled sums must come out as exactly 1 and exactly dP of the target."""
    n, h, L = 2, 2, 257
    qkv, do, dv, _ = aref.selection_backward_batch(n, L, h, "perm")
    out = torch.full((n * L, 3 * 64 * h), float("nan"), dtype=torch.float16, device="cuda")
    assert run(qkv.cuda(), do.cuda(), L, out, n=n, h=h) == _lib.OK
    got = out.cpu()
    d = 64 * h
    assert (got[:, :2 * d] == 0).all()
    assert torch.equal(got[:, 2 * d:], dv)


def test_refusals():
    x = torch.zeros(8192, dtype=torch.float16, device="cuda")
    p, s = x.data_ptr(), ops._stream()
    f = lib.clipmi_attention_backward_long
    big = 1 << 20
    assert f(p, p, p, p, big, 1, 641, 1, s) == _lib.ERR_SHAPE
    assert f(p, p, p, p, big, 1, 0, 1, s) == _lib.ERR_SHAPE
    assert f(p, p, p, p, big, -1, 8, 1, s) == _lib.ERR_SHAPE
    assert f(p, p, p, p, big, 1, 8, 0, s) == _lib.ERR_SHAPE
    assert f(p, p, p, p, big, 1 << 30, 8, 2, s) == _lib.ERR_SHAPE          # N H beyond 31 bits
    assert f(p, p, p, p, big, 1 << 23, 640, 1, s) == _lib.ERR_SHAPE        # N L beyond 31 bits
    assert f(None, p, p, p, big, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p, None, p, p, big, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p, p, None, p, big, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p, p, p, None, big, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p + 2, p, p, p, big, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p, p + 8, p, p, big, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p, p, p + 4, p, big, 1, 8, 1, s) == _lib.ERR_ARG
    assert f(p, p, p, p + 4, big, 1, 8, 1, s) == _lib.ERR_ARG
    assert ws_bytes(8, 1, 1) == 96
    assert f(p, p, p, p, 95, 1, 8, 1, s) == _lib.ERR_ARG                   # a short workspace
    assert f(None, None, None, None, 0, 0, 8, 1, s) == _lib.OK
    assert ws_bytes(641, 1, 1) == 0 and ws_bytes(640, 1, 1) == 12 * 640 and ws_bytes(8, 0, 1) == 0
    # the sibling keeps its limit
    assert lib.clipmi_attention_backward_full(p, p, p, 1, 225, 1, s) == _lib.ERR_SHAPE
    torch.cuda.synchronize()


def test_ops_wrapper():
    L = 259
    qkv, do = inputs(L)
    want, emu = references(L)
    got = ops.attention_backward_long(qkv.cuda(), do.cuda(), N, H)
    torch.cuda.synchronize()
    held(got.cpu(), want, emu, f"ops.attention_backward_long: L={L}")
