"""clipmi_layernorm, clipmi_embed_ln, clipmi_patch_embed and clipmi_patchify through the C ABI, one entry point at a time, against the plain
references of tests/front_ref.py: per element within the derived tolerances (tests/test_front_ref_cpu.py holds an fp32 emulation of every
case to the same tolerances and shows that they tell wrong kernels apart), bit for bit where the operator only moves or casts data.  The call
forms are the towers': ln_post's in_stride = L D, ln_final's int32 gather of fp16 rows, padded output rows.  Every output lies inside a larger
buffer prefilled with a FINITE bit pattern, and everything the operator does not own -- the guards, the padding between strided rows, the rows
behind the last one, the class and prompt rows of patch_embed -- must keep those bits; input rows that must not be read hold a huge finite
value that would wreck the row.  The worst error / tolerance per operator is printed at the end of the module (pytest -s)."""
import functools

import pytest
import torch

import front_ref as ref
from clip_calibration_amd import _lib

pytestmark = pytest.mark.gpu

LIB = _lib.lib
DT = {torch.float16: _lib.F16, torch.float32: _lib.F32}
PAD = 64                                    # guard elements on either side of an output
MARK = {torch.float16: (torch.int16, 0x6B5A), torch.float32: (torch.int32, 0x4B5A5A5A)}   # finite: 3764.0 and 14309978.0
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    yield
    for k in sorted(WORST):
        print(f"\nMI355X, worst error / tolerance: {k}: {WORST[k]:.3f}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _name(dt):
    return "fp16" if dt == torch.float16 else "fp32"


class Out:
    """rows x stride elements between two guards, all prefilled with MARK; the operator owns [rows_owned, :width] of it."""

    def __init__(self, rows, stride, dtype):
        self.rows, self.stride, (self.idt, self.mark) = rows, stride, MARK[dtype]
        self.buf = torch.empty(2 * PAD + rows * stride, dtype=dtype, device="cuda")
        self.buf.view(self.idt).fill_(self.mark)
        self.ptr = self.buf.data_ptr() + PAD * self.buf.element_size()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf.view(self.idt) == self.mark).all())

    def owned(self, rows_owned, width, what):
        """-> [len(rows_owned), width] on the CPU, after asserting that nothing else changed."""
        torch.cuda.synchronize()
        host = self.buf.cpu()
        bits = host.view(self.idt)
        body = bits[PAD:PAD + self.rows * self.stride].reshape(self.rows, self.stride)
        free = torch.ones(self.rows, self.stride, dtype=torch.bool)
        free[torch.as_tensor(rows_owned).long(), :width] = False
        assert bool((bits[:PAD] == self.mark).all() and (bits[PAD + self.rows * self.stride:] == self.mark).all()), f"{what}: wrote outside its buffer"
        assert bool((body[free] == self.mark).all()), f"{what}: wrote {int((body[free] != self.mark).sum())} elements it does not own"
        return host[PAD:PAD + self.rows * self.stride].reshape(self.rows, self.stride)[torch.as_tensor(rows_owned).long(), :width].clone()


def _within(name, got, val, tol):
    err = (got.double() - val).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    worst = float(r.max()) if r.numel() else 0.0
    WORST[name] = max(WORST.get(name, 0.0), worst)
    assert worst <= 1.0, f"{name}: error / tolerance = {worst} at {int(r.argmax())} (got {got.reshape(-1)[int(r.argmax())]}, want {val.reshape(-1)[int(r.argmax())]})"


# ---------------------------------------------------------------------------------------------------------------------- clipmi_layernorm
@pytest.mark.parametrize("c", ref.LN_CASES, ids=ref.ln_case_id)
def test_layernorm(c):
    i = ref.ln_input(c)
    val, bound = ref.layer_norm_rows(i["x"], i["gamma"], i["beta"], i["eps"], rows=i["gather"], in_stride=i["in_stride"])
    x, gamma, beta = i["x"].cuda(), i["gamma"].cuda(), i["beta"].cuda()
    gather = None if i["gather"] is None else i["gather"].cuda()
    out = Out(c.rows + 2, i["out_stride"], c.dt_out)
    _lib.check(LIB.clipmi_layernorm(x.data_ptr(), DT[c.dt_in], i["in_stride"], _ptr(gather), gamma.data_ptr(), beta.data_ptr(), out.ptr, DT[c.dt_out],
                                    i["out_stride"], c.rows, c.D, i["eps"], _stream()), "clipmi_layernorm")
    got = out.owned(range(c.rows), c.D, "clipmi_layernorm")
    _within(f"layernorm -> {_name(c.dt_out)}", got, val, ref.tol_ln(val, bound, c.dt_out))


@pytest.mark.parametrize("D,stride,what", ref.LN_REJECTS)
@pytest.mark.parametrize("side", ["in", "out"])
def test_layernorm_rejects(D, stride, what, side):
    rows = 3
    x = torch.ones(rows * 4200, device="cuda")
    gamma, beta = torch.ones(4200, device="cuda"), torch.zeros(4200, device="cuda")
    out = Out(rows, 4200, torch.float32)
    good = max(D, stride) + (-max(D, stride)) % 4                   # the other stride is a legal one
    ins, outs = (stride, good) if side == "in" else (good, stride)
    rc = LIB.clipmi_layernorm(x.data_ptr(), _lib.F32, ins, None, gamma.data_ptr(), beta.data_ptr(), out.ptr, _lib.F32, outs, rows, D, 1e-5, _stream())
    assert rc == _lib.ERR_SHAPE, (what, rc)
    assert out.untouched(), f"{what}: a rejected call wrote"


# ---------------------------------------------------------------------------------------------------------------------- clipmi_embed_ln
@pytest.mark.parametrize("c", ref.EMBED_CASES, ids=ref.embed_case_id)
def test_embed_ln(c):
    i = ref.embed_input(c)
    L, n = i["L"], c.B * i["L"]
    dev = {k: i[k].cuda() for k in ("x0", "cls", "pos", "shallow", "gamma", "beta")}
    for add_pos in (0, 1):
        rows = ref.embed_rows(i["x0"], i["cls"], i["pos"], i["shallow"], L, i["tokens0"], add_pos)
        val, bound = ref.layer_norm_rows(rows, i["gamma"], i["beta"], 1e-5)
        for outs in ref.EMBED_OUTS:
            what = f"clipmi_embed_ln add_pos={add_pos} {outs}"
            y = Out(n + 2, c.D, torch.float32) if outs != "y16" else None
            y16 = Out(n + 2, c.D, torch.float16) if outs != "y" else None
            st = Out(n + 2, 2, torch.float32) if outs != "y" else None
            _lib.check(LIB.clipmi_embed_ln(dev["x0"].data_ptr(), DT[c.dt], add_pos, dev["cls"].data_ptr(), dev["pos"].data_ptr(),
                                           dev["shallow"].data_ptr() if c.n_ctx else None, dev["gamma"].data_ptr(), dev["beta"].data_ptr(),
                                           y.ptr if y else None, y16.ptr if y16 else None, st.ptr if st else None, c.B, L, i["tokens0"], c.D, 1e-5,
                                           _stream()), what)
            if y:
                gy = y.owned(range(n), c.D, what)
                _within("embed_ln y", gy, val, ref.tol_ln(val, bound, torch.float32))
            if y16:
                g16 = y16.owned(range(n), c.D, what)
                _within("embed_ln y16", g16, val, ref.tol_ln(val, bound, torch.float16))
                gst = st.owned(range(n), 2, what)
            if outs == "both":
                assert torch.equal(g16, gy.half()), f"{what}: y16 is not one fp16 rounding of y"
                s, q, bs, bq = ref.fold_row_sums(gy)                 # the sums of the kernel's own fp32 output
                _within("embed_ln stats of y", gst[:, 0], s, bs)
                _within("embed_ln stats of y", gst[:, 1], q, bq)
            if outs == "y16":
                s, q, _, _ = ref.fold_row_sums(val)
                ts, tq = ref.tol_fold_of_reference(val, bound)
                _within("embed_ln stats of the reference", gst[:, 0], s, ts)
                _within("embed_ln stats of the reference", gst[:, 1], q, tq)


# ---------------------------------------------------------------------------------------------------------------------- clipmi_patch_embed
def _patch_embed(image, w, pos, P, n_ctx, dt_out, what):
    """-> the patch rows of x0 [B * G^2, D] (CPU), after asserting that the class rows, the prompt rows and two rows behind the last kept their bits."""
    B, _, R, _ = image.shape
    G, D, K = R // P, w.shape[0], 3 * P * P
    tokens = 1 + G * G + n_ctx
    idt = DT[image.dtype]
    nbytes = LIB.clipmi_patch_embed_scratch_bytes(B, R, idt)
    assert (nbytes > 0) == (image.dtype == torch.float32)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda") if nbytes else None
    img_d, w_d, pos_d = image.cuda(), w.contiguous().cuda(), None if pos is None else pos.cuda()
    x0 = Out(B * tokens + 2, D, dt_out)
    _lib.check(LIB.clipmi_patch_embed(img_d.data_ptr(), idt, _ptr(scratch), w_d.data_ptr(), K, _ptr(pos_d), x0.ptr, DT[dt_out], B, R, P, D, tokens,
                                      _stream()), what)
    return x0.owned(ref.patch_x0_rows(B, G, tokens), D, what)


@functools.lru_cache(maxsize=None)
def _patch_reference(c, dt_in, with_pos, leak=False):
    """(image, w, pos or None, value, sum |a| |w|): computed once per input, shared by the output dtypes."""
    image, w, pos = ref.patch_input(c, dt_in, leak=leak)
    pos = pos if with_pos else None
    val, S, _ = ref.patch_rows(image, w, pos, c.P, 1 + (c.R // c.P) ** 2 + c.n_ctx)
    return image, w, pos, val, S


@pytest.mark.parametrize("B,R,P", ref.ADDRESS_CASES)
@pytest.mark.parametrize("dt_in", ref.DTYPES, ids=_name)
@pytest.mark.parametrize("dt_out", ref.DTYPES, ids=_name)
def test_patch_embed_address_map_is_exact(B, R, P, dt_in, dt_out):
    """One-hot weights, D = K = 3 P^2, pos = NULL: output column k of patch row (b, py, px) IS pixel (b, c, py P + ky, px P + kx), and the pixel
    code changes under the exchange of any two of the six coordinates."""
    K = 3 * P * P
    img = ref.coded_image(B, R, P, dt_in)
    got = _patch_embed(img, torch.eye(K).half(), None, P, 1, dt_out, "clipmi_patch_embed, one-hot")
    assert torch.equal(got.float(), ref.patchify(img, P, K).float())


@pytest.mark.parametrize("dt_out", ref.DTYPES, ids=_name)
def test_patch_embed_cast_rounds_to_nearest_even(dt_out):
    B, R, P = 2, 16, 8
    img = ref.tie_image(B, R)
    got = _patch_embed(img, torch.eye(3 * P * P).half(), None, P, 0, dt_out, "clipmi_patch_embed, ties")
    assert torch.equal(got.float(), ref.patchify(img.half(), P, 3 * P * P).float())


@pytest.mark.parametrize("c", ref.PATCH_CASES, ids=ref.patch_case_id)
@pytest.mark.parametrize("dt_in", ref.DTYPES, ids=_name)
@pytest.mark.parametrize("dt_out", ref.DTYPES, ids=_name)
def test_patch_embed(c, dt_in, dt_out):
    for with_pos in (True, False):
        image, w, p, val, S = _patch_reference(c, dt_in, with_pos)
        got = _patch_embed(image, w, p, c.P, c.n_ctx, dt_out, f"clipmi_patch_embed pos={with_pos}")
        _within(f"patch_embed -> {_name(dt_out)}", got, val, ref.tol_patch(val, S, p, c.B, 3 * c.P * c.P, dt_out))


@pytest.mark.parametrize("dt_in", ref.DTYPES, ids=_name)
@pytest.mark.parametrize("dt_out", ref.DTYPES, ids=_name)
def test_patch_embed_no_leak_between_images(dt_in, dt_out):
    """A zero image between two images of pixels near 6e4: its rows are pos, within the rounding of pos alone (its sum |a| |w| is zero) -- and
    exactly zero without pos."""
    c = ref.PATCH_LEAK_CASE
    G2 = (c.R // c.P) ** 2
    for with_pos in (True, False):
        image, w, p, val, S = _patch_reference(c, dt_in, with_pos, leak=True)
        assert bool((S[G2:2 * G2] == 0).all())
        got = _patch_embed(image, w, p, c.P, 0, dt_out, "clipmi_patch_embed, zero image")
        _within(f"patch_embed -> {_name(dt_out)}", got, val, ref.tol_patch(val, S, p, c.B, 3 * c.P * c.P, dt_out))
        if p is None:
            assert bool((got[G2:2 * G2] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------- clipmi_patchify
@pytest.mark.parametrize("B,R,P,kpad,dt", ref.PATCHIFY_CASES)
def test_patchify(B, R, P, kpad, dt):
    img = ref.patchify_input(B, R, P, kpad, dt)
    kp, rows = kpad or ref.default_kpad(P), B * (R // P) ** 2
    col, img_d = Out(rows + 2, kp, torch.float16), img.cuda()
    _lib.check(LIB.clipmi_patchify(img_d.data_ptr(), DT[dt], col.ptr, B, R, P, kp, _stream()), "clipmi_patchify")
    got = col.owned(range(rows), kp, "clipmi_patchify")
    assert torch.equal(got.view(torch.int16), ref.patchify(img, P, kp).view(torch.int16))
