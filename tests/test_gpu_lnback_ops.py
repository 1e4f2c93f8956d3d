"""ln_backward_kernel and quickgelu_backward_kernel (csrc/text_backward.hip) at operator level, through
``ops.layernorm_backward`` and ``ops.quickgelu_backward``: every width seam of the lane loop and every row kind of tests/lnback_ref.py
within the element-wise bound derived there, and QuickGELU's derivative over all of fp16.  tests/test_lnback_ref_cpu.py holds an
emulation of the kernel to half of the same bound and shows that eight defects exceed it; nothing here is taken from what the kernels
return."""
import pytest
import torch

import lnback_ref as ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import _lib, ops  # noqa: E402

SENTINEL = 7.0


def _fp(dt):
    return "fp32" if dt == torch.float32 else "fp16"


def _guarded(t, guard, value=SENTINEL):
    """``t`` on the device as the front of a longer buffer: (the view, the ``guard`` rows or elements behind it)."""
    buf = torch.full((t.shape[0] + guard,) + tuple(t.shape[1:]), value, dtype=t.dtype).cuda()
    buf[:t.shape[0]] = t.cuda()
    return buf[:t.shape[0]], buf[t.shape[0]:]


def _launch(c, g0=None, copy=True):
    g = (c["g0"] if g0 is None else g0).cuda()
    g16 = torch.full(g.shape, SENTINEL, dtype=torch.float16).cuda() if copy else None
    ops.layernorm_backward(c["x"].cuda(), c["gamma"].cuda(), c["dy"].cuda(), g, g16)
    return g.cpu(), None if g16 is None else g16.cpu()


# ---------------------------------------------------------------------------------------------------------------- LayerNorm backward
@pytest.mark.parametrize("dy_dtype", ref.DY_DTYPES, ids=_fp)
@pytest.mark.parametrize("D", ref.LN_WIDTHS)
def test_every_row_kind_within_the_bound(D, dy_dtype):
    worst = {k: 0.0 for k in ref.KINDS}
    for gi in (0, 1):                                                          # one launch per gamma
        c = ref.ln_case(D, dy_dtype, gi)
        got, g16 = _launch(c)
        assert torch.isfinite(got).all()
        for r, k in enumerate(c["kinds"]):
            worst[k] = max(worst[k], ref.ratio(got[r], c["want"][r], c["tol"][r]))
        err = (got.double() - c["want"]).abs()
        assert (err <= c["tol"]).all(), (gi, worst)
        assert torch.equal(g16, got.half())                                    # the fp16 operand copy is the rounded stream, bit for bit
    print(f"lnback-ops: D={D} dy={_fp(dy_dtype)} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("D", (8, 320, 1024))
def test_zero_g0_gives_dx_alone(D):
    """A zero stream: fl(0 + dX) = dX, so the bound has no accumulation term."""
    for gi in (0, 1):
        c = ref.ln_case(D, torch.float32, gi)
        got, g16 = _launch(c, g0=torch.zeros_like(c["g0"]))
        want, tol = ref.ln_backward(c["x"], c["gamma"], c["dy"]), ref.ln_backward_bound(c["x"], c["gamma"], c["dy"])
        assert torch.isfinite(got).all()
        assert ((got.double() - want).abs() <= tol).all(), ref.ratio(got, want, tol)
        assert torch.equal(g16, got.half())


@pytest.mark.parametrize("D", (260, 768))
def test_without_the_fp16_copy(D):
    for dt in ref.DY_DTYPES:
        c = ref.ln_case(D, dt, 0)
        with_copy, _ = _launch(c)
        alone, _ = _launch(c, copy=False)
        assert torch.equal(with_copy, alone)


@pytest.mark.parametrize("D", ref.SCATTER_WIDTHS)
def test_scatter_strided_and_guards(D):
    c = ref.ln_scatter(D)
    rows = c["idx"].long()
    wide = c["wide"].cuda()
    x = wide[:, :D]
    assert x.stride(0) > D
    g, g_guard = _guarded(c["g0"], 2)
    g16_0 = torch.full(c["g0"].shape, SENTINEL, dtype=torch.float16)
    g16, g16_guard = _guarded(g16_0, 2, value=-3.0)
    dy, dy_guard = _guarded(c["dy"], 1)
    ops.layernorm_backward(x, c["gamma"].cuda(), dy, g, g16, row_idx=c["idx"].cuda())
    got, got16 = g.cpu(), g16.cpu()
    untouched = torch.ones(got.shape[0], dtype=torch.bool)
    untouched[rows] = False
    assert torch.equal(got[untouched], c["g0"][untouched]) and (got16[untouched] == SENTINEL).all()
    assert (g_guard.cpu() == SENTINEL).all() and (g16_guard.cpu() == -3.0).all() and (dy_guard.cpu() == SENTINEL).all()
    assert torch.equal(wide.cpu(), c["wide"])
    assert torch.isfinite(got).all()
    err = (got.double() - c["want"]).abs()[rows]
    print(f"lnback-ops: scatter D={D} {float((err / c['tol'][rows]).max()):.3f}")
    assert (err <= c["tol"][rows]).all()
    assert torch.equal(got16[rows], got[rows].half())


def test_same_inputs_same_bits():
    c = ref.ln_case(1024, torch.float32, 0)
    first, second = _launch(c), _launch(c)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


def test_refusals_leave_g_untouched():
    rows = 3

    def attempt(exc, D, x=None, dy=None, g_dtype=torch.float32):
        g = torch.full((rows, D), 1.5, dtype=g_dtype).cuda()
        g16 = torch.full((rows, D), SENTINEL, dtype=torch.float16).cuda()
        x = torch.ones(rows, D).cuda() if x is None else x
        dy = torch.ones(rows, D).cuda() if dy is None else dy
        with pytest.raises(exc):
            ops.layernorm_backward(x, torch.ones(D).cuda(), dy, g, g16)
        torch.cuda.synchronize()
        assert (g.cpu() == 1.5).all() and (g16.cpu() == SENTINEL).all()

    attempt(_lib.ClipmiError, 6)                                               # not a multiple of 4
    attempt(_lib.ClipmiError, 4100)                                            # behind the cap of 4096
    attempt(_lib.ClipmiError, 64, x=torch.ones(rows * 64).cuda().as_strided((rows, 64), (60, 1)))      # rows that overlap: x_stride < D
    attempt(TypeError, 64, dy=torch.ones(rows, 64, dtype=torch.float64).cuda())
    attempt(TypeError, 64, x=torch.ones(rows, 64, dtype=torch.float16).cuda())
    attempt(TypeError, 64, g_dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.layernorm_backward(torch.ones(rows, 64).cuda(), torch.ones(64).cuda(), torch.ones(rows, 64), torch.zeros(rows, 64).cuda())


# ------------------------------------------------------------------------------------------------------------------------ QuickGELU
def test_quickgelu_backward_every_fp16_value():
    h, d_a = ref.gelu_sweep()
    want = ref.quickgelu_backward(h, d_a)
    tol = ref.quickgelu_backward_bound(h, d_a, want)
    got = ops.quickgelu_backward(h.cuda(), d_a.cuda()).cpu()
    assert torch.isfinite(got.float()).all()
    err = (got.double() - want).abs()
    exact = float((got == want.half()).float().mean())
    print(f"lnback-ops: quickgelu worst ratio {float((err / tol).max()):.3f}, correctly rounded {100 * exact:.3f} % of {h.numel()}")
    assert (err <= tol).all(), float((err / tol).max())
    hd = h.double()
    zero = hd == 0                                                             # both signs
    assert int(zero.sum()) == 2 * len(ref.GELU_D_A) and torch.equal(got[zero], (0.5 * d_a.double()[zero]).half())
    assert torch.equal(got[hd >= 20], d_a[hd >= 20])                           # 1 + exp(-34) is 1 in fp32
    assert (got[hd <= -60] == 0).all()                                         # exp(102) overflows: s is 0


@pytest.mark.parametrize("n", ref.GELU_LENGTHS)
def test_quickgelu_backward_lengths(n):
    """The vector body and the scalar tail on either side of a workgroup's 2048 elements.  ``ops.quickgelu_backward`` allocates its
    output, so the guard elements stand behind a buffer handed to the same C entry point; both give the same bits."""
    g = torch.Generator().manual_seed(n)
    h, d_a = (3.0 * torch.randn(n, generator=g)).half(), torch.randn(n, generator=g).half()
    want = ref.quickgelu_backward(h, d_a)
    tol = ref.quickgelu_backward_bound(h, d_a, want)
    hd, dd = h.cuda(), d_a.cuda()
    got = ops.quickgelu_backward(hd, dd).cpu()
    assert ((got.double() - want).abs() <= tol).all()
    out, guard = _guarded(torch.full((n,), -2.0, dtype=torch.float16), 19)
    _lib.check(_lib.lib.clipmi_quickgelu_backward(hd.data_ptr(), dd.data_ptr(), out.data_ptr(), n, None), "clipmi_quickgelu_backward")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), got) and (guard.cpu() == SENTINEL).all()
