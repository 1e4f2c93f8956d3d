"""The text tower's training entry points with MaPLe's deep prompts (clipmi_text_encoder_train_deep, clipmi_text_encoder_backward_deep),
stage by stage in the manner of tests/test_gpu_towertrain.py: the splice in the stash, the plain entry points' bits without deep
prompts, d_deep from the device's own stash against the float64 backward of that stash within FACTOR x a CPU emulation with the device's
rounding points, and the refusals."""
import ctypes as C
import functools

import pytest
import torch

import coopfit_ref as cref
import maplefit_ref as mref
import towertrain_ref as ref
from clip_calibration_amd import _lib, ops
from clip_calibration_amd.coopfit import _dgrad
from clip_calibration_amd.model import build_model

pytestmark = pytest.mark.gpu
LIB = _lib.lib
MARK = 0x5A
# (tower, depth, n_ctx, C, live-row cut)
CASES = [("tiny3", 3, 3, 3, True), ("tiny3", 2, 1, 5, False), ("tiny3", 3, 2, 5, True), ("tiny", 2, 2, 5, False)]


@functools.lru_cache(maxsize=None)
def _model(tower, n_ctx):
    m = build_model(dict(ref.state_dict(tower)), mref.design(n_ctx)).cuda()
    m._ensure_bound()
    return m


class Run:
    """One prompt set on the GPU: inputs, buffers prefilled with a mark, and the two entry points."""

    def __init__(self, tower, depth, n_ctx, Cn, cut, seed=0):
        g = ref.geometry(tower)
        self.tower, self.depth, self.n_ctx, self.C = tower, depth, n_ctx, Cn
        self.m = _model(tower, n_ctx)
        self.ids = cref.prompt_ids(tower, Cn, n_ctx, seed)
        self.rows = mref.live_rows(self.ids, cut)
        self.L, self.D, self.E, self.layers = self.rows or g.context_length, g.transformer_width, g.embed_dim, g.transformer_layers
        gen = torch.Generator().manual_seed(40 + seed)
        self.t = 0.02 * torch.randn(depth, n_ctx, self.D, generator=gen)          # ctx and the deep prompts: the front of a master block
        self.d_out = torch.randn(Cn, self.E, generator=gen) * 0.05
        self.base = ref.state_dict(tower)["token_embedding.weight"][self.ids].float().contiguous().cuda()
        self.eot = self.ids.argmax(dim=-1).to(torch.int32).cuda()
        wsb, stb = C.c_size_t(0), C.c_size_t(0)
        _lib.check(LIB.clipmi_text_train_bytes(self.m._handle, Cn, self.rows, C.byref(wsb), C.byref(stb)), "bytes")
        self.ws = torch.full((wsb.value,), MARK, dtype=torch.uint8, device="cuda")
        self.stash = torch.full((stb.value,), MARK, dtype=torch.uint8, device="cuda")
        self.out = torch.full((Cn, self.E), float("nan"), device="cuda")
        self.lay = ref.StashLayout(Cn, self.L, self.D, self.layers)
        assert self.lay.bytes == stb.value            # the stash size is the plain entry point's
        self.dgrad = _dgrad(self.m)

    def forward(self, n_deep=None, t=None, n_ctx=None, rows=None):
        t = (self.t if t is None else t).contiguous().cuda()
        n_deep = self.depth - 1 if n_deep is None else n_deep
        n_ctx = self.n_ctx if n_ctx is None else n_ctx
        deep = t.data_ptr() + 4 * self.n_ctx * self.D if n_deep else None
        self._keep = t
        return LIB.clipmi_text_encoder_train_deep(self.m._handle, self.base.data_ptr(), _lib.F32, t.data_ptr(), n_ctx, 0, self.eot.data_ptr(), self.C,
                                                  self.rows if rows is None else rows, deep, n_deep, self.out.data_ptr(), self.ws.data_ptr(),
                                                  self.ws.numel(), self.stash.data_ptr(), self.stash.numel(), _lib.CALL_DEFAULT, ops._stream())

    def plain_forward(self):
        t = self.t.contiguous().cuda()
        return LIB.clipmi_text_encoder_train(self.m._handle, self.base.data_ptr(), _lib.F32, t.data_ptr(), self.n_ctx, 0, self.eot.data_ptr(), self.C, self.rows,
                                             None, self.out.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self.stash.data_ptr(), self.stash.numel(),
                                             _lib.CALL_DEFAULT, ops._stream())

    def backward(self, d_embed, d_deep, n_deep=None):
        n_deep = self.depth - 1 if n_deep is None else n_deep
        d_out = self.d_out.cuda()
        return LIB.clipmi_text_encoder_backward_deep(self.m._handle, C.byref(self.dgrad[0]), d_out.data_ptr(), self.C, self.rows, self.n_ctx, n_deep,
                                                     d_embed.data_ptr(), None if d_deep is None else d_deep.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                                     self.stash.data_ptr(), self.stash.numel(), None, ops._stream())

    def buffers(self):
        d_embed = torch.full((self.C * self.L, self.D), float("nan"), device="cuda")
        d_deep = torch.full((max(self.depth - 1, 1), self.n_ctx, self.D), float("nan"), device="cuda")
        return d_embed, d_deep


def _ok(rc, what):
    _lib.check(rc, what)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", CASES)
def test_splice_rows_are_the_rounded_deep_prompts_and_nothing_else_moves(case):
    tower, depth, n_ctx, Cn, cut = case
    run = Run(*case)
    _ok(run.forward(), "train_deep")
    full, feats = run.stash.cpu(), run.out.cpu()
    assert torch.isfinite(feats).all()
    assert int(run.ids[0].argmax()) == 1 + n_ctx          # an EOT row directly behind the context rows
    x = lambda buf, k: run.lay.x(buf, k).reshape(Cn, run.L, run.D)  # noqa: E731
    for i in range(1, depth):
        want = run.t[i].half().float().expand(Cn, -1, -1)
        assert torch.equal(x(full, 2 * i)[:, 1:1 + n_ctx], want), f"x_in({i}): rows 1 .. n_ctx are not half(deep[{i - 1}])"
    # one deep prompt fewer: the towers agree up to the last splice, whose slab differs on the rows 1 .. n_ctx alone
    _ok(run.forward(n_deep=depth - 2), "train_deep, one prompt fewer")
    fewer = run.stash.cpu()
    i = depth - 1
    for k in range(2 * i):
        assert torch.equal(run.lay.x(fewer, k), run.lay.x(full, k)), k
    a, b = x(full, 2 * i), x(fewer, 2 * i)
    assert torch.equal(a[:, 0], b[:, 0]) and torch.equal(a[:, 1 + n_ctx:], b[:, 1 + n_ctx:])
    assert not torch.equal(a[:, 1:1 + n_ctx], b[:, 1:1 + n_ctx]) and not torch.equal(run.out.cpu(), feats)


@pytest.mark.parametrize("case", [CASES[0], CASES[3]])
def test_without_deep_prompts_the_deep_entry_points_are_the_plain_ones(case):
    run = Run(*case)
    _ok(run.plain_forward(), "train")
    stash, feats = run.stash.cpu(), run.out.cpu()
    g = torch.full((run.C * run.L, run.D), float("nan"), device="cuda")
    d_out = run.d_out.cuda()
    _ok(LIB.clipmi_text_encoder_backward(run.m._handle, C.byref(run.dgrad[0]), d_out.data_ptr(), run.C, run.rows, g.data_ptr(), run.ws.data_ptr(),
                                         run.ws.numel(), run.stash.data_ptr(), run.stash.numel(), None, ops._stream()), "backward")
    run.stash.fill_(MARK)
    run.out.fill_(float("nan"))
    _ok(run.forward(n_deep=0), "train_deep without deep prompts")
    assert torch.equal(run.stash.cpu(), stash) and torch.equal(run.out.cpu().view(torch.int32), feats.view(torch.int32))
    d_embed, _ = run.buffers()
    _ok(run.backward(d_embed, None, n_deep=0), "backward_deep without deep prompts")
    assert torch.equal(d_embed.cpu().view(torch.int32), g.cpu().view(torch.int32))


def _backward_with_splices(run, st, hi, lo):
    """(g [C L, D], [d_deep_i]) of dtype ``hi``: towertrain_ref.emulate_backward's steps -- a rounding to ``lo`` wherever the device writes
    fp16 -- with the splice reduction behind block i's ln_1 backward.  hi = lo = float64: the same steps without any rounding."""
    sd = ref.state_dict(run.tower)
    H = ref.geometry(run.tower).transformer_heads
    r = lambda t: t.to(lo).to(hi)  # noqa: E731
    idx = st.idx()
    dxf = r(run.d_out.to(hi)) @ r(sd["text_projection"].to(hi)).t()
    g = torch.zeros(st.M, st.D, dtype=hi)
    g[idx] = cref.ln_backward(st.x(2 * st.layers).to(hi)[idx], sd["ln_final.weight"].to(hi), dxf)
    d_deep = [None] * (run.depth - 1)
    for i in reversed(range(st.layers)):
        w = ref._w(sd, i, hi)
        d_a = r(r(g) @ w["mlp.c_proj.weight"])
        d_h = r(cref.quickgelu_backward(st.h(i).to(hi), d_a))
        g = g + cref.ln_backward(st.x(2 * i + 1).to(hi), w["ln_2.weight"], d_h @ w["mlp.c_fc.weight"])
        d_att = r(r(g) @ w["attn.out_proj.weight"])
        dqkv = ref._attention_backward_emu(st.qkv(i), d_att, st.C, st.L, H, hi, lo)
        g = g + cref.ln_backward(st.x(2 * i).to(hi), w["ln_1.weight"], dqkv @ w["attn.in_proj_weight"])
        if 1 <= i < run.depth:
            d_deep[i - 1], g = mref.splice_reduce(g, st.C, st.L, run.n_ctx)
    return g, d_deep


@pytest.mark.parametrize("case", CASES)
def test_d_deep_and_the_context_rows_from_the_device_stash(case):
    """The bound is towertrain's: FACTOR x the error of the CPU emulation (fp32 with the device's fp16 rounding points) against the float64
    backward of the SAME stash, per tensor; the device differs from the emulation by its fast exponential and its summation orders."""
    tower, depth, n_ctx, Cn, cut = case
    run = Run(*case)
    _ok(run.forward(), "train_deep")
    stash = run.stash.cpu()
    d_embed, d_deep = run.buffers()
    _ok(run.backward(d_embed, d_deep), "backward_deep")
    assert torch.equal(run.stash.cpu(), stash), "the backward wrote to the stash"
    d_embed, d_deep = d_embed.cpu(), d_deep.cpu()
    assert torch.isfinite(d_embed).all() and torch.isfinite(d_deep[:depth - 1]).all()
    st = ref.StashView(stash, run.lay)
    g64, deep64 = _backward_with_splices(run, st, torch.float64, torch.float64)
    g32, deep32 = _backward_with_splices(run, st, torch.float32, torch.float16)
    ctx = lambda g: cref.ctx_gradient(g.reshape(Cn * run.L, run.D), Cn, run.L, n_ctx, False)  # noqa: E731
    pairs = [("ctx rows", ctx(d_embed), ctx(g32), ctx(g64))] + [(f"d_deep[{i}]", d_deep[i], deep32[i], deep64[i]) for i in range(depth - 1)]
    for name, got, emu, want in pairs:
        err, yard = cref.rel_fro(got, want), cref.rel_fro(emu, want)
        print(f"\ntext-deep-parity: {tower} depth={depth} n_ctx={n_ctx} C={Cn} cut={cut} {name}: device {err:.3e} emulation {yard:.3e} "
              f"bound {ref.FACTOR * yard:.3e} ratio {err / (ref.FACTOR * yard):.2f}")
        assert err <= ref.FACTOR * yard, name
    # the splice rows left the stream: block i - 1 never sees them, so the rows of d_embed behind a prompt's EOT stay zero as well
    gp = d_embed.reshape(Cn, run.L, run.D)
    for p in range(Cn):
        assert (gp[p, int(run.ids[p].argmax()) + 1:] == 0).all()
    again_e, again_d = run.buffers()
    _ok(run.backward(again_e, again_d), "second backward")
    assert torch.equal(again_e.cpu().view(torch.int32), d_embed.view(torch.int32)) and torch.equal(again_d.cpu().view(torch.int32), d_deep.view(torch.int32))


def test_refusals_leave_every_buffer_untouched():
    run = Run("tiny3", 3, 2, 3, True)

    def untouched():
        torch.cuda.synchronize()
        return bool((run.stash == MARK).all()) and bool((run.ws == MARK).all()) and bool(torch.isnan(run.out).all())

    t4 = 0.02 * torch.randn(4, 2, run.D)
    assert run.forward(n_deep=3, t=t4) == _lib.ERR_SHAPE and "depth 4 for 3 text layers" in _lib.last_error() and untouched()
    assert run.forward(n_ctx=run.L) == _lib.ERR_SHAPE and "does not fit" in _lib.last_error() and untouched()      # 1 + n_ctx > live rows
    assert run.forward(n_deep=-1) == _lib.ERR_SHAPE and untouched()
    run._keep = None
    rc = LIB.clipmi_text_encoder_train_deep(run.m._handle, run.base.data_ptr(), _lib.F32, run.t.cuda().data_ptr(), 2, 0, run.eot.data_ptr(), run.C, run.rows,
                                            None, 2, run.out.data_ptr(), run.ws.data_ptr(), run.ws.numel(), run.stash.data_ptr(), run.stash.numel(),
                                            _lib.CALL_DEFAULT, ops._stream())
    assert rc == _lib.ERR_ARG and untouched()                                                                     # deep prompts missing
    assert LIB.clipmi_text_encoder_train_deep(run.m._handle, run.base.data_ptr(), _lib.F32, run.t.cuda().data_ptr(), 2, 0, run.eot.data_ptr(), run.C, run.rows,
                                              None, 0, run.out.data_ptr(), run.ws.data_ptr(), run.ws.numel(), run.stash.data_ptr(), run.stash.numel(),
                                              _lib.CALL_STREAM_F16, ops._stream()) == _lib.ERR_STATE and untouched()
    d_embed, d_deep = run.buffers()
    assert run.backward(d_embed, d_deep, n_deep=3) == _lib.ERR_SHAPE
    assert run.backward(d_embed, None, n_deep=2) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(d_embed).all() and torch.isnan(d_deep).all() and untouched()
    # the plain entry point still refuses a hook with deep prompts (tests/test_gpu_towertrain.py::test_train_refusals)
    hook = _lib.PromptHook(2, 1, None, run.t.cuda().data_ptr())
    rc = LIB.clipmi_text_encoder_train(run.m._handle, run.base.data_ptr(), _lib.F32, None, 0, 0, run.eot.data_ptr(), run.C, run.rows, C.byref(hook),
                                       run.out.data_ptr(), run.ws.data_ptr(), run.ws.numel(), run.stash.data_ptr(), run.stash.numel(), _lib.CALL_DEFAULT,
                                       ops._stream())
    assert rc == _lib.ERR_ARG and "deep prompts are not supported" in _lib.last_error() and untouched()
