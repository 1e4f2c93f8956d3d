"""The plumbing kernels of the text tower (csrc/elementwise.hip) through clipmi_encode_text, clipmi_text_encoder and clipmi_text_blocks, against
the plain references of tests/text_ref.py.  The towers are built from pass-through state dicts (attn.out_proj and mlp.c_proj of every text
block are zero, so both residual GEMMs add exactly zero while every launch still runs): what clipmi_text_blocks returns is compared bit for
bit (as values: -0 == +0), a feature of the two encoders within the derived bound of ln_final's fp16 output and the fp32-accumulated projection
(tests/test_text_ref_cpu.py holds an fp32 emulation inside that bound on every case, and the mutants outside).  The entry points are called
through ctypes, so seq_rows, eot, dtype and flags are the test's own variables; every output is a slice out of the middle of a sentinel-filled
buffer, and every call is made twice: same input, same bits.

Which test guards which kernel (one line of the kernel changed -> the test fails):
  embed_kernel           test_encoder_features[ids-*]         (address map: every table row, every position; id clamp: the ties cases)
  eot_kernel             test_encoder_features[ids-*-ties]    (first maximum, lane wrap at 63 / 64, 64-bit ids), [ids-*-addr*] (positions)
  rows_from_eot_kernel   test_encoder_features[*-clamp], and every encoder case (rows[c] = c L + e)
  add_pos_kernel         test_encoder_features[prompts-*] (with pos, both input types, row bound), test_text_blocks_exact (without pos)
  rows_out_kernel        test_text_blocks_exact[*-r<bound>-*]  (all four instantiations; zeros behind the bound)
  cast_kernel            test_text_blocks_exact[*-r0-*-s32-*]  (fp32 stream, every row; both output types)
  cast16_kernel          test_text_blocks_exact[*-r0-*-s16-*]  (fp16 stream, every row; both output types)
  overwrite_kernel       test_text_blocks_exact[*-ctx*deep*], test_encoder_features[*-ctx*deep*] (layer offset, row offset, rows beside it)
  row_stats_kernel       test_text_blocks_exact[*-s16-*] (its fp16 copy is the fp16 stream), test_statistics_of_overwritten_rows (its sums and the
                         zeroed second partial, on a live tower)
cast_kernel's scalar tail (n % 4 != 0) cannot be reached through these entry points: n = n_prompts * L * D and the widths are multiples of 64.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import text_ref as ref
from clip_calibration_amd import _lib
from test_gpu_glue_ops import Guarded, _assert_within, _stream, _twice

pytestmark = pytest.mark.gpu

L = _lib.lib
DT = {torch.float16: _lib.F16, torch.float32: _lib.F32}
PLAIN = {"trainer": "CoOp", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0}
WS_MARK = 0xA5


def _build(sd):
    from clip_calibration_amd.model import build_model
    model = build_model(dict(sd), dict(PLAIN)).cuda()
    model._ensure_bound()
    return model


@functools.lru_cache(maxsize=None)
def _model(tower):
    return _build(ref.state_dict(tower))


class _Call:
    """Workspace of exactly the size the library asks for (bytes behind it must survive) and the hook structure of one call."""

    def __init__(self, model, n_prompts, seq_rows, hook=None, deep=None):
        self.model, self.keep = model, []
        self.need = L.clipmi_text_workspace_bytes(model._handle, n_prompts, seq_rows)
        self.ws = torch.empty(self.need + 256, dtype=torch.uint8, device="cuda")
        self.ws[self.need:] = WS_MARK
        self.hook = None
        if hook is not None:
            n_ctx, n_deep = hook
            d = deep.cuda().contiguous()
            self.keep.append(d)
            self.struct = _lib.PromptHook(n_ctx, n_deep, None, d.data_ptr() if n_deep else None)
            self.hook = C.byref(self.struct)

    def done(self, what):
        torch.cuda.synchronize()
        assert bool((self.ws[self.need:] == WS_MARK).all()), f"{what}: wrote behind its workspace"


def _set_fold(model, fold):
    model.set_option("ln_fold", int(fold))


def _values_equal(got, want, what):
    got, want = got.reshape(want.shape).float(), want.float()
    bad = torch.nonzero(~(got == want))
    assert bad.numel() == 0, (f"{what}: {bad.shape[0]} of {want.numel()} elements differ, first at [prompt, token, column] {bad[0].tolist()}: got "
                              f"{got[tuple(bad[0].tolist())].item()!r}, want {want[tuple(bad[0].tolist())].item()!r}")


# ------------------------------------------------------------------------------------------------------------------ clipmi_text_blocks
@pytest.mark.parametrize("case", ref.BLOCKS_CASES, ids=ref.blocks_case_id)
def test_text_blocks_exact(case):
    """y = cast(x) (fp32 stream) or cast(fp16(x)) (fp16 stream) on the live rows, the last applied deep prompt on rows 1..n_ctx, zeros behind the
    bound; the sentinel rows of x behind the bound are never read; guards of y and of the workspace intact; two launches, the same bits."""
    t = ref.TOWERS[case.tower]
    model = _model(case.tower)
    _set_fold(model, case.fold)
    inp = ref.blocks_input(case)
    x = inp["x"].cuda()
    call = _Call(model, case.C, case.seq_rows, case.hook, inp["deep"])
    what = f"clipmi_text_blocks {ref.blocks_case_id(case)}"
    got = _twice(x.numel(), case.dtype, what,
                 lambda p: L.clipmi_text_blocks(model._handle, x.data_ptr(), p, DT[case.dtype], case.C, case.seq_rows, call.hook, call.ws.data_ptr(),
                                                call.need, case.stream, _stream()))
    call.done(what)
    assert torch.equal(x.cpu(), inp["x"]), f"{what}: wrote to its input"
    _values_equal(got.reshape(case.C, t.ctx, t.width), ref.blocks_expected(case, inp), what)


# ------------------------------------------------------------------------------------------- clipmi_encode_text / clipmi_text_encoder
@functools.lru_cache(maxsize=None)
def _enc_reference(case):
    """(input, value, tol) of a case: computed once, shared by the tests that need it."""
    inp = ref.enc_input(case)
    rows, _ = ref.enc_rows(case, inp)
    return (inp,) + ref.enc_features(case, rows)


def _encode(case, inp, what):
    t = ref.TOWERS[case.tower]
    model = _model(case.tower)
    _set_fold(model, case.fold)
    call = _Call(model, case.C, case.seq_rows, case.hook, inp["deep"])
    if case.entry == "ids":
        ids = inp["ids"].cuda()
        fn = lambda p: L.clipmi_encode_text(model._handle, ids.data_ptr(), case.C, case.seq_rows, p, call.ws.data_ptr(), call.need, case.stream,  # noqa: E731
                                            _stream())
    else:
        prompts, eot = inp["prompts"].cuda(), inp["eot"].cuda()
        fn = lambda p: L.clipmi_text_encoder(model._handle, prompts.data_ptr(), DT[case.dtype], eot.data_ptr(), case.C, case.seq_rows, call.hook, p,  # noqa: E731
                                             call.ws.data_ptr(), call.need, case.stream, _stream())
    got = _twice(case.C * t.embed, torch.float32, what, fn)
    call.done(what)
    return got.reshape(case.C, t.embed)


@pytest.mark.parametrize("case", ref.ENC_CASES, ids=ref.enc_case_id)
def test_encoder_features(case):
    """The feature of prompt c is ln_final(row) @ text_projection of ONE row: the token (or prompt, or deep prompt) row and the positional row
    the references pick -- first maximum of the raw ids, clamps, the row bound, the hook's layer -- each within the derived bound."""
    what = f"{'clipmi_encode_text' if case.entry == 'ids' else 'clipmi_text_encoder'} {ref.enc_case_id(case)}"
    inp, val, tol = _enc_reference(case)
    got = _encode(case, inp, what)
    assert torch.isfinite(got).all(), what
    print(f"\n{what}: worst error / tolerance {float(((got.double() - val).abs() / tol).max()):.3f}")
    _assert_within(got, val, tol, what + " [prompt, feature]")


def test_ids_behind_the_bound_do_not_matter():
    """The ids behind seq_rows cannot be the maximum of their prompt (ID_SENTINEL): zeros in their place give the same bits."""
    case = next(c for c in ref.ENC_CASES if c.entry == "ids" and c.seq_rows == 30)
    inp, _, _ = _enc_reference(case)
    other = dict(inp, ids=inp["ids"].clone())
    other["ids"][:, 30:] = 0
    assert (inp["ids"][:, 30:] == ref.ID_SENTINEL).all()
    a, b = _encode(case, inp, "encode_text, sentinel ids behind the bound"), _encode(case, other, "encode_text, zeros behind the bound")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------- case 6
def test_statistics_of_overwritten_rows():
    """A live two-layer tower of width 512 (two statistics partials per row and more), deep prompts of mean 2 on rows 1..2 against token rows of
    0.02, seq_rows 16, fold on: row_stats_kernel's sums of the overwritten rows -- and the partials it has to zero -- feed ln_1 of block 1.
    Against the CPU oracle with the tolerance of test_gpu_model.py's hooked towers, and against ln_fold = 0 (test_layernorm_fold_path's bound).
    tests/test_text_ref_cpu.py: a stale second partial misses the oracle by 72 tolerances."""
    inp = ref.live_input()
    model = _build(inp["sd"])
    prompts, eot = inp["prompts"].cuda(), inp["eot"].cuda()
    want = ref.live_reference().double().numpy()
    feats = {}
    for fold in (1, 0):
        _set_fold(model, fold)
        call = _Call(model, ref.LIVE_C, ref.LIVE_ROWS, (ref.LIVE_N_CTX, 1), inp["deep"])
        what = f"clipmi_text_encoder, live tower, ln_fold {fold}"
        got = _twice(ref.LIVE_C * ref.LIVE_TOWER.embed, torch.float32, what,
                     lambda p: L.clipmi_text_encoder(model._handle, prompts.data_ptr(), _lib.F32, eot.data_ptr(), ref.LIVE_C, ref.LIVE_ROWS, call.hook, p,
                                                     call.ws.data_ptr(), call.need, _lib.CALL_DEFAULT, _stream()))
        call.done(what)
        got = got.reshape(ref.LIVE_C, -1).double().numpy()
        feats[fold] = got
        mag = np.abs(got - want).max() / np.abs(want).max()
        cos = np.abs(ref.cos_table(got, want) - ref.cos_table(want, want)).max()
        print(f"\n{what}: max |d| / max |ref| {mag:.2e} (tol {ref.LIVE_MAG_TOL:g}), cosine {cos:.2e} (tol {ref.LIVE_COS_TOL:g})")
        assert np.isfinite(got).all() and cos < ref.LIVE_COS_TOL and mag <= ref.LIVE_MAG_TOL, what
    gap = np.abs(ref.cos_table(feats[1], feats[0]) - ref.cos_table(feats[0], feats[0])).max()
    print(f"fold against no fold: cosine {gap:.2e} (tol {ref.LIVE_FOLD_TOL:g})")
    assert gap < ref.LIVE_FOLD_TOL


# ------------------------------------------------------------------------------------------------------------------ empty and refusals
def test_no_prompts_writes_nothing():
    model = _model("w64")
    _set_fold(model, 1)
    t = ref.TOWERS["w64"]
    x = torch.zeros(1, t.ctx, t.width, device="cuda")
    ids, eot = torch.zeros(1, t.ctx, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    call = _Call(model, 0, 0)
    y, out = Guarded(x.numel(), torch.float32), Guarded(t.embed, torch.float32)
    args = (call.ws.data_ptr(), call.need, 0, _stream())
    assert L.clipmi_text_blocks(model._handle, x.data_ptr(), y.ptr, _lib.F32, 0, 0, None, *args) == _lib.OK
    assert L.clipmi_text_encoder(model._handle, x.data_ptr(), _lib.F32, eot.data_ptr(), 0, 0, None, out.ptr, *args) == _lib.OK
    assert L.clipmi_encode_text(model._handle, ids.data_ptr(), 0, 0, out.ptr, *args) == _lib.OK
    call.done("n_prompts = 0")
    assert y.untouched() and out.untouched()


@pytest.mark.parametrize("code", [2, -1, 7])
def test_bad_dtype_code_is_refused(code):
    model = _model("w64")
    _set_fold(model, 1)
    t = ref.TOWERS["w64"]
    x = torch.zeros(3, t.ctx, t.width, device="cuda")
    eot = torch.zeros(3, dtype=torch.int32, device="cuda")
    call = _Call(model, 3, 0)
    y, out = Guarded(x.numel(), torch.float32), Guarded(3 * t.embed, torch.float32)
    args = (call.ws.data_ptr(), call.need, 0, _stream())
    assert L.clipmi_text_blocks(model._handle, x.data_ptr(), y.ptr, code, 3, 0, None, *args) == _lib.ERR_ARG and "dtype" in _lib.last_error()
    assert L.clipmi_text_encoder(model._handle, x.data_ptr(), code, eot.data_ptr(), 3, 0, None, out.ptr, *args) == _lib.ERR_ARG and "dtype" in _lib.last_error()
    call.done("bad dtype")
    assert y.untouched() and out.untouched()
