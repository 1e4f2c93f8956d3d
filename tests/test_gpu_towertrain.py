"""The two drivers of the training text tower, clipmi_text_encoder_train and clipmi_text_encoder_backward (the bottom of
csrc/text_backward.hip), stage by stage against tests/towertrain_ref.py.  The entry points are called through ctypes with a workspace, a
stash and outputs of EXACTLY the sizes clipmi_text_train_bytes reports, each with canary bytes in front of it and behind it.  The stash is
read back and every stage is held against its float64 reference evaluated from the device's own stashed input of that stage, within a
bound derived from the formats (towertrain_ref's docstring; tests/test_towertrain_cpu.py keeps an fp32 emulation inside those bounds and
the mutants outside).  The whole backward is measured against the float64 backward from the device's stash; its yardstick is the CPU
emulation of the device's arithmetic on the same stash, never the device's own output.

Which test fails for which change of a driver (one line changed in a scratch build, the whole file run against it):
  x_in for x_mid as c_proj's residual (run_train_forward)       test_forward_stages, all 20 (x_in(i + 1) leaves its bound)
  b_out dropped (nullptr as the out-projection's bias)          every test that runs a forward: launch_gemm refuses the residual epilogue
                                                                without a bias ("gemm: bias missing"); a bias that is silently lost is
                                                                the CPU mutant no_b_out, which leaves x_mid(i)'s bound on all 20 cases
  L passed for src_L to coop_embed_kernel                       test_embedding_bit_for_bit on the 14 cut cases (prompt rows of the wrong
                                                                prompt), and with it test_forward_stages, test_tail_alone, test_whole_backward
  the hipMemsetAsync of g skipped                               test_tail_alone (10), test_whole_backward (10): the NaN prefill survives;
                                                                test_operand_statistics_exact (3)
  the hipMemsetAsync of g16 skipped                             test_whole_backward (10), test_cut_and_uncut_agree_on_the_live_rows (2)
  ln1_g for ln2_g in the backward                               test_whole_backward (10: accuracy, both row sets)
  0x0400 counted as a subnormal (a <= 0x0400u)                  test_operand_statistics_exact (3: the smallest normal in d_out)
"""
import ctypes as C
import functools

import pytest
import torch

import text_ref
import towertrain_ref as ref
from clip_calibration_amd import _lib, coopfit

pytestmark = pytest.mark.gpu

LIB = _lib.lib
DT = {torch.float16: _lib.F16, torch.float32: _lib.F32}
PLAIN = {"trainer": "CoOp", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0}
MARK, GUARD = 0xA5, 256
BOTH = [ref.on_tower(c, t) for c in ref.CASES for t in (c.tower, c.tower + "-pass")]
LIVE = list(ref.CASES)
PASS = [ref.on_tower(c, c.tower + "-pass") for c in ref.CASES]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _build(sd):
    from clip_calibration_amd.model import build_model
    model = build_model(dict(sd), dict(PLAIN)).cuda()
    model._ensure_bound()
    return model


@functools.lru_cache(maxsize=None)
def _model(tower):
    return _build(ref.state_dict(tower))


class _Bytes:
    """n bytes, 256-byte aligned, between two canaries."""

    def __init__(self, n, fill=MARK):
        self.n = n
        self.buf = torch.full((2 * GUARD + n,), MARK, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.mid = self.buf[GUARD:GUARD + n]
        self.mid.fill_(fill)
        self.ptr = self.buf.data_ptr() + GUARD

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.buf[:GUARD] == MARK).all()) and bool((self.buf[GUARD + self.n:] == MARK).all())

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == MARK).all())

    def cpu(self):
        torch.cuda.synchronize()
        return self.mid.cpu().clone()

    def f32(self):
        return self.mid.view(torch.float32)


class _Run:
    """One case on the device: buffers of exactly the reported sizes."""

    def __init__(self, c, model=None):
        self.c, self.inp = c, ref.case_input(c)
        g = ref.geometry(c.tower)
        self.model = model or _model(c.tower)
        self.L, self.D, self.E = ref.live_rows(c), g.transformer_width, g.embed_dim
        self.M = c.C * self.L
        wsb, stb = C.c_size_t(0), C.c_size_t(0)
        _lib.check(LIB.clipmi_text_train_bytes(self.model._handle, c.C, c.seq_rows, C.byref(wsb), C.byref(stb)), "clipmi_text_train_bytes")
        self.lay = ref.StashLayout(c.C, self.L, self.D, g.transformer_layers)
        assert stb.value == self.lay.bytes, "the stash is not the size include/clipmi.h's layout gives"
        self.ws, self.stash, self.out = _Bytes(wsb.value), _Bytes(stb.value), _Bytes(c.C * self.E * 4)
        self.prompts, self.eot = self.inp["prompts"].cuda(), self.inp["eot"].cuda()
        self.ctx = None if self.inp["ctx"] is None else self.inp["ctx"].cuda()
        self.dgrad = coopfit._dgrad(self.model)

    def forward(self, hook=None, flags=_lib.CALL_DEFAULT, n_ctx=None, ws_bytes=None, stash_bytes=None, ws_ptr=None, n_prompts=None):
        c = self.c
        return LIB.clipmi_text_encoder_train(self.model._handle, self.prompts.data_ptr(), DT[c.dtype], None if self.ctx is None else self.ctx.data_ptr(),
                                             c.n_ctx if n_ctx is None else n_ctx, int(c.ctx == "class"), self.eot.data_ptr(),
                                             c.C if n_prompts is None else n_prompts, c.seq_rows, hook, self.out.ptr, ws_ptr or self.ws.ptr,
                                             self.ws.n if ws_bytes is None else ws_bytes, self.stash.ptr, self.stash.n if stash_bytes is None else stash_bytes,
                                             flags, _stream())

    def backward(self, d_out, d_embed, stats=None, ws_bytes=None, stash_bytes=None, ws_ptr=None, n_prompts=None):
        return LIB.clipmi_text_encoder_backward(self.model._handle, C.byref(self.dgrad[0]), d_out.data_ptr(), self.c.C if n_prompts is None else n_prompts,
                                                self.c.seq_rows, d_embed.ptr, ws_ptr or self.ws.ptr, self.ws.n if ws_bytes is None else ws_bytes,
                                                self.stash.ptr, self.stash.n if stash_bytes is None else stash_bytes,
                                                None if stats is None else stats.data_ptr(), _stream())

    def d_embed(self, fill=MARK):
        return _Bytes(self.M * self.D * 4, fill)

    def intact(self, what):
        assert self.ws.intact() and self.stash.intact() and self.out.intact(), f"{what}: wrote outside a buffer of the reported size"


@functools.lru_cache(maxsize=None)
def _forward(c):
    """(run, stash bytes on the CPU, features [C, E]) of a case: one forward, shared by the tests, left unchanged."""
    run = _Run(c)
    what = f"clipmi_text_encoder_train {ref.case_id(c)}"
    _lib.check(run.forward(), what)
    run.intact(what)
    return run, run.stash.cpu(), run.out.cpu().view(torch.float32).reshape(c.C, run.E)


def _nan_d_embed(run):
    d = run.d_embed()
    d.f32().fill_(float("nan"))
    return d


def _backward(run, d_out, what, stats=None):
    """d_embed fp32 [M, D] (CPU) of one backward into a NaN-filled buffer; canaries checked."""
    d = _nan_d_embed(run)
    _lib.check(run.backward(d_out, d, stats), what)
    assert d.intact(), f"{what}: wrote outside d_embed"
    run.intact(what)
    return d.cpu().view(torch.float32).reshape(run.M, run.D)


# --------------------------------------------------------------------------------------------------------------- 4.1 the embedding, exact
@pytest.mark.parametrize("c", BOTH, ids=ref.case_id)
def test_embedding_bit_for_bit(c):
    run, stash, _ = _forward(c)
    want = ref.embed(c, run.inp)
    got = run.lay.x(stash, 0)
    bad = torch.nonzero(got.view(torch.int32) != want.view(torch.int32))
    assert bad.numel() == 0, f"x_in(0): {bad.shape[0]} of {want.numel()} elements differ, first at [row, column] {bad[0].tolist()}"
    assert torch.equal(run.lay.idx(stash), ref.eot_rows(c, run.inp))


def test_hook_without_deep_prompts_changes_nothing():
    c = ref.CASES[0]
    _, stash, feats = _forward(c)
    run = _Run(c)
    hook = _lib.PromptHook(c.n_ctx, 0, None, None)
    _lib.check(run.forward(hook=C.byref(hook)), "clipmi_text_encoder_train, hook with n_deep = 0")
    run.intact("hook with n_deep = 0")
    assert torch.equal(run.stash.cpu(), stash) and torch.equal(run.out.cpu().view(torch.float32).reshape(feats.shape).view(torch.int32), feats.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ 4.2 forward stages
def _text_encoder_features(run):
    """clipmi_text_encoder on the same prompts (the context written into fp32 prompt rows), ln_fold 0, fp32 stream."""
    c, m = run.c, run.model
    p = run.inp["prompts"].float().clone()
    p[:, run.L:] = 0.0
    if run.inp["ctx"] is not None:
        p[:, 1:1 + c.n_ctx] = run.inp["ctx"] if c.ctx == "class" else run.inp["ctx"][None]
    p = p.cuda()
    need = LIB.clipmi_text_workspace_bytes(m._handle, c.C, c.seq_rows)
    ws, out = _Bytes(need), _Bytes(c.C * run.E * 4)
    m.set_option("ln_fold", 0)
    try:
        _lib.check(LIB.clipmi_text_encoder(m._handle, p.data_ptr(), _lib.F32, run.eot.data_ptr(), c.C, c.seq_rows, None, out.ptr, ws.ptr, need,
                                           _lib.CALL_STREAM_F32, _stream()), "clipmi_text_encoder")
        torch.cuda.synchronize()
    finally:
        m.set_option("ln_fold", 1)
    assert ws.intact() and out.intact()
    return out.cpu().view(torch.float32).reshape(c.C, run.E)


@pytest.mark.parametrize("c", BOTH, ids=ref.case_id)
def test_forward_stages(c):
    """Every slab of the stash and the features within the derived bound of the float64 reference of that stage, evaluated from the
    device's own input of the stage; a second call gives the same bits; the inference encoder agrees."""
    run, stash, feats = _forward(c)
    assert torch.isfinite(feats).all()
    worst = {}
    for name, got, want, tol in ref.forward_stages(c.tower, c.C, run.L, stash, run.lay):
        worst[name] = ref.worst_ratio(feats if got is None else got, want, tol)
    print(f"\ntowertrain-parity: forward {ref.case_id(c)} worst error / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    again = _Run(c)
    _lib.check(again.forward(), "second call")
    again.intact("second call")
    assert torch.equal(again.stash.cpu(), stash), "two calls on the same input leave different stashes"
    assert torch.equal(again.out.cpu(), run.out.cpu())
    enc = _text_encoder_features(run).double().numpy()
    f = feats.double().numpy()
    gap = abs(text_ref.cos_table(f, enc) - text_ref.cos_table(enc, enc)).max()
    print(f"towertrain-parity: forward {ref.case_id(c)} against clipmi_text_encoder: cosine {gap:.2e} (tol {text_ref.LIVE_FOLD_TOL:g})")
    assert gap < text_ref.LIVE_FOLD_TOL


# ---------------------------------------------------------------------------------------------------------------------- 4.3 the tail alone
@pytest.mark.parametrize("c", PASS, ids=ref.case_id)
def test_tail_alone(c):
    """Pass-through blocks add exact zeros to the gradient: d_embed is zero off the EOT rows and ln_final's backward on them."""
    run, stash, _ = _forward(c)
    d_out = run.inp["d_out"]
    g = _backward(run, d_out.cuda(), f"clipmi_text_encoder_backward {ref.case_id(c)}")
    want, tol, idx = ref.tail_tolerance(c.tower, ref.StashView(stash, run.lay), d_out)
    off = torch.ones(run.M, dtype=torch.bool)
    off[idx] = False
    assert torch.isfinite(g).all() and (g[off] == 0).all(), "a row that is no EOT row carries a gradient"
    r = ref.worst_ratio(g[idx], want, tol)
    print(f"\ntowertrain-parity: tail {ref.case_id(c)} worst error / bound {r:.3f}")
    assert r <= 1.0
    assert torch.equal(run.stash.cpu(), stash), "the backward wrote to the stash"


# ------------------------------------------------------------------------------------------------------------------ 4.4 the whole backward
@functools.lru_cache(maxsize=None)
def _whole(c):
    """(device g, float64 g, {"live": bound, "plain": bound}) of a live case: the bound is FACTOR x the worst per-prompt error of the CPU
    emulation on the device's stash."""
    run, stash, _ = _forward(c)
    d_out = run.inp["d_out"]
    what = f"clipmi_text_encoder_backward {ref.case_id(c)}"
    g = _backward(run, d_out.cuda(), what)
    st = ref.StashView(stash, run.lay)
    want = ref.backward64(c.tower, st, d_out)
    emu = ref.prompt_errors(ref.emulate_backward(c.tower, st, d_out), want, c, run.inp)
    return g, want, {k: ref.FACTOR * max(v) for k, v in emu.items()}, {k: max(v) for k, v in emu.items()}


@pytest.mark.parametrize("c", LIVE, ids=ref.case_id)
def test_whole_backward(c):
    run, stash, _ = _forward(c)
    g, want, bound, emu = _whole(c)
    assert torch.isfinite(g).all(), "d_embed is accumulated into, or not written everywhere: the NaN prefill shows"
    gp = g.reshape(c.C, run.L, run.D)
    for p in range(c.C):
        assert (gp[p, int(run.inp["eot"][p]) + 1:] == 0).all(), f"prompt {p}: a row behind its EOT carries a gradient"
    assert torch.equal(run.stash.cpu(), stash), "the backward wrote to the stash"
    d_out = run.inp["d_out"].cuda()
    again = _backward(run, d_out, "second backward")                                  # the same buffers
    other = _backward(run, d_out, "backward into a second buffer")                    # as ProGrad makes it (a fresh d_embed either time)
    assert torch.equal(again.view(torch.int32), g.view(torch.int32)) and torch.equal(other.view(torch.int32), g.view(torch.int32))
    got = ref.prompt_errors(g, want, c, run.inp)
    for k in ("live", "plain"):
        print(f"\ntowertrain-parity: backward {ref.case_id(c)} rows={k} device worst {max(got[k]):.3e} emulation worst {emu[k]:.3e} "
              f"bound {bound[k]:.3e} ratio {max(got[k]) / bound[k]:.2f}")
    for k in ("live", "plain"):
        assert max(got[k]) <= bound[k], (k, got[k], bound[k])


@pytest.mark.parametrize("cut,whole", ref.UNCUT_PAIRS, ids=lambda c: ref.case_id(c))
def test_cut_and_uncut_agree_on_the_live_rows(cut, whole):
    run = _forward(cut)[0]
    g_cut, _, bound, _ = _whole(cut)
    g_all = _whole(whole)[0]
    L, Lw = ref.live_rows(cut), ref.live_rows(whole)
    a, b = g_cut.reshape(cut.C, L, -1).double(), g_all.reshape(cut.C, Lw, -1)[:, :L].double()
    assert (g_all.reshape(cut.C, Lw, -1)[:, L:] == 0).all()
    worst = max(float((a[p, :e + 1] - b[p, :e + 1]).norm() / b[p, :e + 1].norm()) for p, e in enumerate(run.inp["eot"].tolist()))
    print(f"\ntowertrain-parity: cut {ref.case_id(cut)} against uncut, live rows: worst {worst:.3e} bound {bound['live']:.3e}")
    assert worst <= bound["live"]


# --------------------------------------------------------------------------------------------------------------- 4.5 operand statistics
STATS_CASES = [ref.on_tower(c, c.tower + "-quiet") for c in (PASS[3], PASS[0], PASS[8])]      # towertrain_ref.QUIET


def _stats():
    return torch.zeros(4, dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("c", STATS_CASES, ids=ref.case_id)
def test_operand_statistics_exact(c):
    run, stash, _ = _forward(c)
    layers = run.lay.layers
    d_out = ref.special_d_out(c.C, run.E)
    plain = _backward(run, d_out.cuda(), "backward without statistics")
    stats = _stats()
    g = _backward(run, d_out.cuda(), "backward with statistics", stats)
    assert torch.equal(g.view(torch.int32), plain.view(torch.int32)), "the statistics change d_embed"
    assert torch.isfinite(g.half().float()).all(), "the gradient stream leaves fp16's range: inf times a zero weight is a NaN operand"
    want = ref.passthrough_stats(d_out, g, layers, run.M, run.D)
    assert want[3] == 0x7BFF and want[0] == c.C * run.E + 9 * layers * run.M * run.D
    got = stats.cpu().tolist()
    print(f"\ntowertrain-parity: statistics {ref.case_id(c)} elements {got[0]} zeros {got[1]} subnormals {got[2]} max 0x{got[3]:04x}")
    assert got == want, (got, want)
    assert ref.operand_counts(d_out.half())[2] >= 2 and ref.half_bits(d_out.half()[0, 4:5]).item() == 0x0400
    _backward(run, d_out.cuda(), "second backward into the same words", stats)
    assert stats.cpu().tolist() == [2 * want[0], 2 * want[1], 2 * want[2], want[3]]
    zero = _stats()
    gz = _backward(run, torch.zeros(c.C, run.E).cuda(), "zero d_out", zero)
    z = zero.cpu().tolist()
    assert (gz == 0).all() and z[0] == want[0] and z[1] == z[0] and z[2] == 0 and z[3] == 0
    nan = d_out.clone()
    nan[c.C - 1, 7] = float("nan")
    sn = _stats()
    _backward(run, nan.cuda(), "NaN in d_out", sn)
    assert sn.cpu().tolist()[0] == want[0] and sn.cpu().tolist()[3] == 0x7FFF
    assert torch.equal(run.stash.cpu(), stash)


def test_grid_stride_case_is_among_the_statistics_cases():
    assert any(c.C * ref.live_rows(c) * 4 * ref.geometry(c.tower).transformer_width > ref.STATS_GRID for c in STATS_CASES)


# ---------------------------------------------------------------------------------------------------------------------------- 4.6 refusals
def _refused(run, rc, code, who, d_embed=None):
    assert rc == code, (rc, code, _lib.last_error())
    assert who in _lib.last_error(), _lib.last_error()
    assert run.out.untouched() and run.stash.untouched() and run.ws.untouched(), f"{who}: a refused call wrote something"
    assert d_embed is None or d_embed.untouched()


def test_train_refusals():
    c = ref.CASES[0]
    run = _Run(c)
    who = "text_encoder_train"
    deep = torch.zeros(1, c.n_ctx, run.D, device="cuda")
    hook = _lib.PromptHook(c.n_ctx, 1, None, deep.data_ptr())
    _refused(run, run.forward(hook=C.byref(hook)), _lib.ERR_ARG, who)
    assert "deep prompts" in _lib.last_error()
    _refused(run, run.forward(flags=_lib.CALL_STREAM_F16), _lib.ERR_STATE, who)
    _refused(run, run.forward(flags=4), _lib.ERR_ARG, who)
    assert "flags" in _lib.last_error()
    _refused(run, run.forward(n_ctx=run.L), _lib.ERR_SHAPE, who)                      # 1 + n_ctx > the 16 live rows
    assert "n_ctx" in _lib.last_error()
    _refused(run, run.forward(ws_bytes=run.ws.n - 1), _lib.ERR_WORKSPACE, who)
    _refused(run, run.forward(stash_bytes=run.stash.n - 1), _lib.ERR_WORKSPACE, who)
    _refused(run, run.forward(ws_ptr=run.ws.ptr + 16), _lib.ERR_ARG, who)
    assert "aligned" in _lib.last_error()
    assert run.forward(n_prompts=0) == _lib.OK
    assert run.out.untouched() and run.stash.untouched() and run.ws.untouched()


def test_backward_refusals():
    c = ref.CASES[0]
    run = _Run(c)
    who = "text_encoder_backward"
    d_out, d = run.inp["d_out"].cuda(), run.d_embed()
    _refused(run, run.backward(d_out, d, ws_bytes=run.ws.n - 1), _lib.ERR_WORKSPACE, who, d)
    _refused(run, run.backward(d_out, d, stash_bytes=run.stash.n - 1), _lib.ERR_WORKSPACE, who, d)
    _refused(run, run.backward(d_out, d, ws_ptr=run.ws.ptr + 16), _lib.ERR_ARG, who, d)
    assert run.backward(d_out, d, n_prompts=0) == _lib.OK
    assert d.untouched() and run.stash.untouched() and run.ws.untouched()


def test_backward_refuses_more_than_80_live_rows():
    """A tower with an 88-row positional embedding: the forward runs, the backward (whose attention kernel holds at most 80 token rows)
    returns CLIPMI_ERR_SHAPE before it launches anything."""
    model = _build(ref.long_state_dict(88))
    assert model.geometry.context_length == 88
    c = ref.Case("tiny", 2, 4, 0, ref.F16, "shared", False)
    g = ref.geometry("tiny")
    wsb, stb = C.c_size_t(0), C.c_size_t(0)
    _lib.check(LIB.clipmi_text_train_bytes(model._handle, c.C, 0, C.byref(wsb), C.byref(stb)), "clipmi_text_train_bytes")
    assert stb.value == ref.StashLayout(c.C, 88, g.transformer_width, g.transformer_layers).bytes
    ws, stash, d = _Bytes(wsb.value), _Bytes(stb.value), _Bytes(c.C * 88 * g.transformer_width * 4)
    d_out = torch.zeros(c.C, g.embed_dim, device="cuda")
    dgrad = coopfit._dgrad(model)
    rc = LIB.clipmi_text_encoder_backward(model._handle, C.byref(dgrad[0]), d_out.data_ptr(), c.C, 0, d.ptr, ws.ptr, ws.n, stash.ptr, stash.n, None, _stream())
    assert rc == _lib.ERR_SHAPE and "text_encoder_backward" in _lib.last_error() and "88" in _lib.last_error(), _lib.last_error()
    assert d.untouched() and ws.untouched() and stash.untouched()
