"""The two kernels of csrc/prompt_position.hip at operator level, through ctypes: clipmi_prompt_place and clipmi_prompt_unplace against the
row formulas of tests/position_ref.py.  Both are copies (a base row is widened from fp16, which is exact), so every comparison is bit for
bit.  Outputs sit inside sentinel-filled buffers whose guards must survive, inputs end right in front of a NaN-patterned guard, every
launch is made twice and gives the same bits.  The last two tests hold the placed chain (place, the training tower with ctx = NULL,
backward, unplace, clipmi_ctx_step) to the existing ``end`` route's bits."""
import ctypes

import numpy as np
import pytest
import torch

import coopfit_ref as ref
import position_ref as pos
from test_gpu_glue_ops import PAD, SENTINEL, Guarded, _assert_bits, _stream, _twice  # noqa: F401

pytestmark = pytest.mark.gpu

from clip_calibration_amd import _lib, coopfit, ops  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

lib = _lib.lib
DT = {torch.float16: _lib.F16, torch.float32: _lib.F32}
LC, L_CUT = 24, 16
GRAD_SCALE = 256.0


def lengths(C, L, n_ctx):
    """Class c's name length: the longest that keeps '.' and EOT in the L rows (EOT on the last live row) first, then 1, 7, 0 and two values
    outside [0, L - 2 - n_ctx], which the kernels clamp and the restatement with them."""
    cycle = [L - 3 - n_ctx, 1, 7, 0, -2, 99]
    return np.array([cycle[c % len(cycle)] for c in range(C)], np.int32)


def guarded_input(t):
    """t on the device, its last element right in front of a NaN-patterned guard."""
    return Guarded(t.numel(), t.dtype, t.cuda())


@pytest.mark.parametrize("cut", [True, False], ids=["cut", "full"])
@pytest.mark.parametrize("per_class", [False, True], ids=["generic", "csc"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("C,D", [(2, 64), (2, 512), (3, 64), (3, 512), (37, 64), (37, 512)])
def test_place_and_unplace_are_the_row_formulas_bit_for_bit(C, D, dtype, per_class, cut):
    L = L_CUT if cut else LC
    mark = SENTINEL[torch.float32][1]
    for n_ctx in (4, 5):
        g = torch.Generator().manual_seed(C * 1000 + D + n_ctx)
        base = torch.randn(C, LC, D, generator=g).to(dtype)
        ctx = torch.randn(*((C, n_ctx, D) if per_class else (n_ctx, D)), generator=g)
        d_embed = torch.randn(C * L, D, generator=g)
        lens = lengths(C, L, n_ctx)
        gb, gc, gd, gl = guarded_input(base), guarded_input(ctx), guarded_input(d_embed), guarded_input(torch.from_numpy(lens))
        for code in (0, 1, 2):
            what = f"clipmi_prompt_place C={C} D={D} n_ctx={n_ctx} L={L} position={code}"
            got = _twice(C * LC * D, torch.float32, what,
                         lambda p: lib.clipmi_prompt_place(gb.ptr, DT[dtype], gc.ptr, int(per_class), code, gl.ptr, p, C, L, LC, D, n_ctx, _stream()))
            got = got.reshape(C, LC, D)
            _assert_bits(got[:, :L], pos.place(base, ctx, code, lens, L), what + " [class, row, column]")
            assert (got[:, L:].contiguous().view(torch.int32) == mark).all(), what + ": wrote behind the live rows"
            what = f"clipmi_prompt_unplace C={C} D={D} n_ctx={n_ctx} L={L} position={code}"
            back = _twice(C * (1 + n_ctx) * D, torch.float32, what,
                          lambda p: lib.clipmi_prompt_unplace(gd.ptr, code, gl.ptr, p, C, L, D, n_ctx, _stream()))
            _assert_bits(back.reshape(C, 1 + n_ctx, D), pos.unplace(d_embed.reshape(C, L, D), code, lens, n_ctx), what + " [class, row, column]")
        for gin, t in ((gb, base), (gc, ctx), (gd, d_embed)):                   # the inputs and their guards are as they were
            assert torch.equal(gin.result("an input").view(torch.int16), t.reshape(-1).view(torch.int16))
        # something moved: with a name in the prompt the positions differ
        assert not torch.equal(pos.place(base, ctx, 0, lens, L), pos.place(base, ctx, 2, lens, L))


def test_wrappers_are_the_entry_points():
    """ops.prompt_place / ops.prompt_unplace: names and codes, the caller's own output, the rows argument."""
    C, D, n_ctx = 3, 64, 5
    g = torch.Generator().manual_seed(5)
    base, ctx, d_embed = torch.randn(C, LC, D, generator=g).half(), torch.randn(n_ctx, D, generator=g), torch.randn(C * L_CUT, D, generator=g)
    lens = lengths(C, L_CUT, n_ctx)
    lens_d = torch.from_numpy(lens).cuda()
    for name, code in pos.CODES.items():
        full = ops.prompt_place(base.cuda(), ctx.cuda(), name, lens_d)
        assert torch.equal(full.cpu(), pos.place(base, ctx, code, lens)) and torch.equal(ops.prompt_place(base.cuda(), ctx.cuda(), code, lens_d), full)
        own = torch.zeros(C, LC, D, device="cuda")
        assert ops.prompt_place(base.cuda(), ctx.cuda(), name, lens_d, rows=L_CUT, prompts=own) is own
        assert torch.equal(own.cpu()[:, :L_CUT], pos.place(base, ctx, code, lens, L_CUT)) and not own[:, L_CUT:].any()
        back = ops.prompt_unplace(d_embed.cuda(), name, lens_d, n_ctx)
        assert torch.equal(back.cpu().reshape(C, 1 + n_ctx, D), pos.unplace(d_embed.reshape(C, L_CUT, D), code, lens, n_ctx))
    with pytest.raises(ValueError, match="position"):
        ops.prompt_place(base.cuda(), ctx.cuda(), "back", lens_d)
    with pytest.raises(ValueError, match="position"):
        ops.prompt_unplace(d_embed.cuda(), 3, lens_d, n_ctx)


# ------------------------------------------------------------------------------------------------------------------- the placed chain
def end_route(tower, c, method_args):
    """(text, grad) of the existing route: the tower splices ctx, clipmi_ctx_step reads rows 1 .. n_ctx of d_embed."""
    ctx = c["ctx"].cuda()
    text = tower.forward(ctx).clone()
    _, d_text, _ = ops.prompt_head(c["feats"].cuda(), c["labels"].cuda(), text, *method_args)
    d_embed = tower.backward(d_text)
    return text, ops.ctx_step(d_embed, tower.C, tower.n_ctx, tower.per_class, GRAD_SCALE)


def placed_chain(tower, c, code, lens, method_args):
    """The same through ctypes: place, clipmi_text_encoder_train with ctx = NULL, the head, the backward, unplace, clipmi_ctx_step."""
    m, t = tower.model, tower
    ctx, lens_d = c["ctx"].cuda(), torch.from_numpy(np.asarray(lens, np.int32)).cuda()
    prompts = torch.full((t.C, t.Lc, t.D), float("nan"), device="cuda")
    text = torch.empty(t.C, t.E, device="cuda")
    with m._launch_lock:
        _lib.check(lib.clipmi_prompt_place(t.base.data_ptr(), DT[t.base.dtype], ctx.data_ptr(), int(t.per_class), code, lens_d.data_ptr(), prompts.data_ptr(),
                                           t.C, t.L, t.Lc, t.D, t.n_ctx, _stream()), "clipmi_prompt_place")
        _lib.check(lib.clipmi_text_encoder_train(m._handle, prompts.data_ptr(), _lib.F32, None, 0, 0, t.eot.data_ptr(), t.C, t.rows, None, text.data_ptr(),
                                                 t.ws.data_ptr(), t.ws.numel(), t.stash.data_ptr(), t.stash.numel(), _lib.CALL_DEFAULT, _stream()),
                   "clipmi_text_encoder_train")
    _, d_text, _ = ops.prompt_head(c["feats"].cuda(), c["labels"].cuda(), text, *method_args)
    d_embed = torch.empty(t.C * t.L, t.D, device="cuda")
    compact = torch.empty(t.C * (1 + t.n_ctx), t.D, device="cuda")
    grad = torch.empty_like(ctx)
    with m._launch_lock:
        _lib.check(lib.clipmi_text_encoder_backward(m._handle, ctypes.byref(t.dgrad[0]), d_text.data_ptr(), t.C, t.rows, d_embed.data_ptr(), t.ws.data_ptr(),
                                                    t.ws.numel(), t.stash.data_ptr(), t.stash.numel(), None, _stream()), "clipmi_text_encoder_backward")
        _lib.check(lib.clipmi_prompt_unplace(d_embed.data_ptr(), code, lens_d.data_ptr(), compact.data_ptr(), t.C, t.L, t.D, t.n_ctx, _stream()),
                   "clipmi_prompt_unplace")
        _lib.check(lib.clipmi_ctx_step(compact.data_ptr(), None, None, grad.data_ptr(), t.C, 1 + t.n_ctx, t.D, t.n_ctx, int(t.per_class), GRAD_SCALE, None, 0,
                                       0.0, 0.0, 0.0, 0, _stream()), "clipmi_ctx_step")
    return text, grad


@pytest.mark.parametrize("seq_rows", [None, 0], ids=["cut", "full"])
@pytest.mark.parametrize("key", [("tiny", 3, 4, 8, False), ("tiny3", 37, 5, 8, True)], ids=lambda k: "-".join(str(v) for v in k))
def test_placed_chain_at_end_and_at_empty_names_is_the_end_route(key, seq_rows):
    c = pos.make_case(*key)
    m = build_model(dict(c["sd"]), {"trainer": "CoOp"}).cuda()
    Cn, n_ctx, per_class, last = coopfit._check_prompts("test", m, c["ids"], c["ctx"])
    tower = coopfit._Tower("test", m, c["ids"], Cn, n_ctx, per_class, last, seq_rows)
    head = (float(np.float32(np.exp(ref.LOGIT_SCALE))), GRAD_SCALE)
    text, grad = end_route(tower, c, head)
    assert torch.isfinite(grad).all() and bool(grad.any())
    assert (c["name_lens"] > 0).any()
    got_text, got_grad = placed_chain(tower, c, 2, c["name_lens"], head)          # position code 2: the names do not matter
    assert torch.equal(got_text, text) and torch.equal(got_grad, grad)
    for code in (0, 1, 2):                                                        # every name empty: the three positions coincide
        got_text, got_grad = placed_chain(tower, c, code, np.zeros(Cn, np.int32), head)
        assert torch.equal(got_text, text) and torch.equal(got_grad, grad), code
    moved_text, moved_grad = placed_chain(tower, c, 0, c["name_lens"], head)       # and with the names in front something else comes out
    assert not torch.equal(moved_text, text) and not torch.equal(moved_grad, grad)
