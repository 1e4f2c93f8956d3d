"""CPU checks of the class-token positions of CoOp, KgCoOp and ProGrad (csrc/prompt_position.hip, clip_calibration_amd/coopfit.py and
trainers/coop.py with ``class_token_position=``): the row formulas against the reference's torch.cat forward (tests/position_ref.py), the
gather of the gradient stream against autograd, the host-side refusals and the C ABI's own without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import coopfit_ref as ref
import position_ref as pos
from oracle import clip_oracle as orc

from clip_calibration_amd import _lib, coopfit, ops  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
from clip_calibration_amd.trainers import CoOpCLIP, KgCoOpCLIP, ProGradFitCLIP, PromptLearner  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_ROWS = 32


# ------------------------------------------------------------------------------------------------------------------- 1. the two statements
@pytest.mark.parametrize("per_class", [False, True], ids=["generic", "csc"])
@pytest.mark.parametrize("n_ctx", pos.N_CTX)
def test_row_formulas_equal_the_cat_form(n_ctx, per_class):
    """Name lengths 0, 1, 7 and the longest that leaves '.' and EOT in the rows; odd n_ctx for the half split; n_ctx = 1 has h = 0."""
    lens = pos.name_lengths(L_ROWS, n_ctx)
    assert lens[:3] == [0, 1, 7] and lens[-1] == L_ROWS - 3 - n_ctx and 1 + n_ctx + lens[-1] + 2 == L_ROWS
    emb, ctx, name_lens = pos.layout_case(len(lens) + 1, L_ROWS, 8, n_ctx, per_class, seed=n_ctx)
    got = {}
    for name, code in pos.CODES.items():
        cat = pos.cat_prompts(emb, ctx, name, name_lens)
        got[name] = pos.place(emb, ctx, code, name_lens)
        assert cat.shape == emb.shape and torch.equal(got[name], cat), name
        # the inverse reads every context vector back from its row, and only those
        back = pos.unplace(cat, code, name_lens, n_ctx)
        want = ctx if per_class else ctx.unsqueeze(0).expand(emb.shape[0], -1, -1)
        assert torch.equal(back[:, 1:], want) and not back[:, 0].any()
    named = np.nonzero(name_lens > 0)[0]
    assert named.size >= 3                                                    # nothing below passes for want of a name
    for c in range(emb.shape[0]):
        differs = name_lens[c] > 0
        assert torch.equal(got["front"][c], got["end"][c]) != differs
        # middle moves n_ctx - h vectors: at n_ctx = 1 (h = 0) it is front
        assert torch.equal(got["middle"][c], got["end"][c]) != differs
        if n_ctx == 1:
            assert torch.equal(got["middle"][c], got["front"][c])
        elif differs:
            assert not torch.equal(got["middle"][c], got["front"][c])
    # SOS and the rows from 1 + n_ctx + nl on are the base's, whatever the position
    for name in pos.CODES:
        for c in range(emb.shape[0]):
            assert torch.equal(got[name][c, 0], emb[c, 0]) and torch.equal(got[name][c, 1 + n_ctx + name_lens[c]:], emb[c, 1 + n_ctx + name_lens[c]:])


def test_the_restatement_clamps_a_name_length_as_the_kernels_do():
    emb, ctx, _ = pos.layout_case(3, 16, 8, 4, False)
    for code in (0, 1, 2):
        assert torch.equal(pos.place(emb, ctx, code, [-3, 99, 10]), pos.place(emb, ctx, code, [0, 10, 10]))   # [0, L - 2 - n_ctx] = [0, 10]
        assert torch.equal(pos.unplace(emb, code, [-3, 99, 10], 4), pos.unplace(emb, code, [0, 10, 10], 4))
    assert torch.equal(pos.place(emb, ctx, 2, [0, 1, 2], L=8), pos.place(emb, ctx, 2, [0, 1, 2])[:, :8])


@pytest.mark.parametrize("position", ["middle", "front"])
@pytest.mark.parametrize("key", [("tiny", 3, 4, 8, False), ("tiny", 3, 5, 8, True)], ids=lambda k: "-".join(str(v) for v in k))
def test_gather_of_d_embed_equals_autograd_of_the_cat_form(key, position):
    """float64: the gradient with respect to the prompts' rows, gathered by the unplace restatement (and added over the classes for a
    generic context), is autograd's gradient of the cat form with respect to ctx."""
    c = pos.make_case(*key)
    assert (c["name_lens"] > 0).any()
    sd, ids = ref.cut(c["sd"], c["ids"])
    n_ctx, per_class = key[2], key[4]
    w = torch.randn(ids.shape[0], c["feats"].shape[1], generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    emb = pos.embeddings(sd, ids, torch.float64)
    ctx = c["ctx"].double().requires_grad_(True)
    (orc.text_encoder(sd, pos.cat_prompts(emb, ctx, position, c["name_lens"]), ids, torch.float64) * w).sum().backward()
    prompts = pos.place(emb, c["ctx"].double(), pos.CODES[position], c["name_lens"]).requires_grad_(True)
    (orc.text_encoder(sd, prompts, ids, torch.float64) * w).sum().backward()
    rows = pos.unplace(prompts.grad, pos.CODES[position], c["name_lens"], n_ctx)[:, 1:]
    assert float(ctx.grad.abs().max()) > 0
    if per_class:
        assert torch.equal(rows, ctx.grad)
    else:   # autograd adds the classes in its own order
        assert float((rows.sum(0) - ctx.grad).abs().max()) <= 1e-12 * float(ctx.grad.abs().max())
    end = c["ctx"].double().requires_grad_(True)
    (orc.text_encoder(sd, pos.cat_prompts(emb, end, "end", c["name_lens"]), ids, torch.float64) * w).sum().backward()
    assert not torch.allclose(end.grad, ctx.grad, rtol=1e-6, atol=0)          # the position matters to the gradient


# ------------------------------------------------------------------------------------------------------------------- 2. the host checks
@pytest.fixture(scope="module")
def cpu_model():
    return build_model(dict(ref.state_dict("tiny")), {"trainer": "CoOp"})


def test_python_argument_checks(cpu_model):
    c = pos.make_case("tiny", 3, 4, 8, False)
    ids, ctx, f, y = c["ids"], c["ctx"], c["feats"], c["labels"]
    tea = torch.zeros(3, int(cpu_model.geometry.embed_dim))
    eot = ids.argmax(dim=-1).numpy()

    def gradient(**kw):
        return coopfit.context_gradient(cpu_model, ids, ctx, f, y, **kw)

    def state(**kw):
        return coopfit.CoOpFitState(cpu_model, ids, ctx, **kw)

    def fit(**kw):
        return coopfit.fit_context(f, y, cpu_model, ids, ctx, epochs=1, **kw)

    def learner(**kw):
        return PromptLearner(cpu_model, ids, n_ctx=4, **kw)

    for make in (gradient, state, fit, learner):
        for bad in ("begin", "END", 2, None):
            with pytest.raises(ValueError, match="'end', 'middle', 'front'"):
                make(class_token_position=bad)
        for position in ("end", "middle", "front"):
            with pytest.raises(ValueError, match="one per class"):
                make(class_token_position=position, name_lens=[0, 1])
            with pytest.raises(ValueError, match="one per class"):
                make(class_token_position=position, name_lens=[0.0, 1.0, 2.0])
            with pytest.raises(ValueError, match=r"name_lens\[1\]=-1"):
                make(class_token_position=position, name_lens=[0, -1, 0])
            over = [0, int(eot[1]) - 4, 0]                                    # 1 + n_ctx + nl = eot + 1: the name would cover the EOT
            with pytest.raises(ValueError, match=r"name_lens\[1\]"):
                make(class_token_position=position, name_lens=over)
    for make in (gradient, state, fit):
        for position in ("middle", "front"):                                 # everything checks out: the call needs the device
            with pytest.raises(RuntimeError, match="GPU"):
                make(class_token_position=position)
            with pytest.raises(RuntimeError, match="GPU"):
                make(class_token_position=position, name_lens=[int(e) - 5 for e in eot], method="kgcoop", teacher=tea)
    for make in (state, fit):
        for position in ("end", "middle", "front"):                          # ProGrad keeps its static scale at every position
            with pytest.raises(ValueError, match="ProGrad"):
                make(grad_scale="dynamic", method="prograd", teacher=tea, class_token_position=position)
    assert coopfit.POSITIONS == ("end", "middle", "front") and ops.PROMPT_POSITIONS == {"front": 0, "middle": 1, "end": 2}
    # name_lens=None is the reference's layout [SOT, X * n_ctx, name, '.', EOT]
    code, lens = coopfit._placement("t", ids, 4, "front", None)
    assert code == 0 and lens.dtype == np.int32 and np.array_equal(lens, eot - 4 - 2) and np.array_equal(lens, c["name_lens"])
    assert coopfit._placement("t", ids, 4, "end", None) is None and coopfit._placement("t", ids, 4, "end", list(lens)) is None


@pytest.mark.parametrize("per_class", [False, True], ids=["generic", "csc"])
def test_prompt_learner_on_the_cpu_is_the_cat_form(cpu_model, per_class):
    c = pos.make_case("tiny", 3, 5, 8, per_class)
    dtype = cpu_model.dtype                                                   # the learner holds ctx and the embeddings in the model's dtype
    emb, ctx = pos.embeddings(c["sd"], c["ids"], dtype).float(), c["ctx"].to(dtype).float()
    for position in ("end", "middle", "front"):
        for lens in (None, [int(n) for n in c["name_lens"]]):
            pl = PromptLearner(cpu_model, c["ids"], n_ctx=5, csc=per_class, class_token_position=position, name_lens=lens)
            with torch.no_grad():
                pl.ctx.copy_(c["ctx"])
            assert pl.class_token_position == position and pl.name_lens == lens
            assert torch.equal(pl().detach().float(), pos.cat_prompts(emb, ctx, position, c["name_lens"]))
            assert sorted(pl.state_dict()) == ["ctx", "token_prefix", "token_suffix"]


def test_trainers_pass_the_position_to_the_learner(cpu_model):
    c = pos.make_case("tiny", 3, 4, 8, False)
    lens = [int(n) for n in c["name_lens"]]
    for cls in (CoOpCLIP, KgCoOpCLIP, ProGradFitCLIP):
        clip = cls(cpu_model, c["ids"], n_ctx=4, class_token_position="middle", name_lens=lens)
        assert clip.prompt_learner.class_token_position == "middle" and clip.prompt_learner.name_lens == lens
        assert cls(cpu_model, c["ids"], n_ctx=4).prompt_learner.class_token_position == "end"
        with pytest.raises(ValueError, match="class_token_position"):
            cls(cpu_model, c["ids"], n_ctx=4, class_token_position="back")


# ------------------------------------------------------------------------------------------------------------------------- 3. the C ABI
NEW = ("clipmi_prompt_place", "clipmi_prompt_unplace", "clipmi_prompt_train_step_placed_bytes", "clipmi_prompt_train_step_placed",
       "clipmi_prompt_train_step_scaled_placed_bytes", "clipmi_prompt_train_step_scaled_placed")


def test_header_declares_the_entries_with_the_abi_at_16():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clipmi.h")).read(), flags=re.S)
    assert re.search(r"#define CLIPMI_ABI_VERSION 16\b", text) and _lib.ABI_VERSION == 16 and _lib.lib.clipmi_abi_version() == 16
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols(), name
    assert "CLIPMI_POS" not in text                                           # the positions are plain ints


def test_library_refuses_bad_calls_without_a_device():
    """Argument checks that return before anything is launched: with no device a launch would answer CLIPMI_ERR_HIP."""
    lib = _lib.lib
    p = ctypes.c_void_p(4096)

    def place(base=p, dtype=_lib.F32, ctx=p, position=1, lens=p, out=p, C=3, L=16, Lc=20, D=64, n_ctx=4):
        return lib.clipmi_prompt_place(base, dtype, ctx, 0, position, lens, out, C, L, Lc, D, n_ctx, None)

    def unplace(d_embed=p, position=1, lens=p, out=p, C=3, L=16, D=64, n_ctx=4):
        return lib.clipmi_prompt_unplace(d_embed, position, lens, out, C, L, D, n_ctx, None)

    for null in ("base", "ctx", "lens", "out"):
        assert place(**{null: None}) == _lib.ERR_ARG, null
    for null in ("d_embed", "lens", "out"):
        assert unplace(**{null: None}) == _lib.ERR_ARG, null
    for call in (place, unplace):
        for bad in (-1, 3, 77):
            assert call(position=bad) == _lib.ERR_ARG and "position" in _lib.last_error()
        assert call(C=0) == _lib.ERR_SHAPE and call(n_ctx=0) == _lib.ERR_SHAPE and call(D=62) == _lib.ERR_SHAPE
        assert call(n_ctx=15) == _lib.ERR_SHAPE                               # 2 + n_ctx > L
    assert place(L=21) == _lib.ERR_SHAPE                                      # L > Lc
    assert place(dtype=7) == _lib.ERR_ARG
    assert place(base=ctypes.c_void_p(4096 + 8)) == _lib.ERR_ARG and "aligned" in _lib.last_error()
    assert unplace(out=ctypes.c_void_p(4096 + 4)) == _lib.ERR_ARG and "aligned" in _lib.last_error()
    for sizer in (lib.clipmi_prompt_train_step_placed_bytes, lib.clipmi_prompt_train_step_scaled_placed_bytes):
        assert sizer(None, 3, 0, 8, 0, 4, 0) == 0


@pytest.mark.parametrize("geom", ["tiny"])
def test_one_call_refusals_and_sizes_with_a_model(geom):
    """With a model handle (no device needed for one): the position, name_lens and every stage's arguments are refused before any
    launch, and the sizers are the unplaced steps' plus the prompts [C, Lc, D] and one compact gradient per backward."""
    lib = _lib.lib
    m = build_model(dict(ref.state_dict(geom)), {"trainer": "CoOp"})
    m._ensure_handle()
    h, g = m._handle, m.geometry
    D, Lc, Cn, B, n_ctx = int(g.transformer_width), int(g.context_length), 3, 8, 4
    p = ctypes.c_void_p(4096)

    def a256(n):
        return (n + 255) // 256 * 256

    for mode in (_lib.PROMPT_COOP, _lib.PROMPT_KGCOOP, _lib.PROMPT_PROGRAD):
        for rows in (0, 16):
            extra = a256(Cn * Lc * D * 4) + (2 if mode == _lib.PROMPT_PROGRAD else 1) * a256(Cn * (1 + n_ctx) * D * 4)
            assert lib.clipmi_prompt_train_step_placed_bytes(h, Cn, rows, B, mode, n_ctx, 0) == lib.clipmi_prompt_train_step_bytes(h, Cn, rows, B, mode, n_ctx, 0) + extra
            scaled = lib.clipmi_prompt_train_step_scaled_bytes(h, Cn, rows, B, mode, n_ctx, 0)
            assert lib.clipmi_prompt_train_step_scaled_placed_bytes(h, Cn, rows, B, mode, n_ctx, 0) == (scaled + extra if scaled else 0)
    assert lib.clipmi_prompt_train_step_placed_bytes(h, 1, 0, B, 0, n_ctx, 0) == 0 and lib.clipmi_prompt_train_step_placed_bytes(h, Cn, 0, 0, 0, n_ctx, 0) == 0

    def static(position=1, lens=p, mode=_lib.PROMPT_COOP, ctx=p, feats=p, teacher=None, grad_scale=256.0, B=B, ws_bytes=1 << 40, momentum=0.0, lam=1.0):
        return lib.clipmi_prompt_train_step_placed(h, None, p, _lib.F16, ctx, None, n_ctx, 0, position, lens, p, Cn, 16, feats, 128, p, B, 100.0, grad_scale,
                                                   mode, teacher, 8.0, 1.0, lam, p, 1, momentum, 0.0, 5e-4, 0, p, None, None, None, p, ws_bytes, p, 1 << 40, None)

    def scaled(position=1, lens=p, mode=_lib.PROMPT_COOP, state=p, feats=p, teacher=None, growth=2.0, B=B, ws_bytes=1 << 40):
        return lib.clipmi_prompt_train_step_scaled_placed(h, None, p, _lib.F16, p, None, n_ctx, 0, position, lens, p, Cn, 16, feats, 128, p, B, 100.0, state,
                                                          growth, 0.5, 2000, mode, teacher, 8.0, p, 0.0, 0.0, 5e-4, 0, p, None, p, ws_bytes, p, 1 << 40, None)

    for call in (static, scaled):
        for bad in (-1, 3):
            assert call(position=bad) == _lib.ERR_ARG and "position" in _lib.last_error()
        assert call(lens=None) == _lib.ERR_ARG and call(feats=None) == _lib.ERR_ARG
        assert call(mode=_lib.PROMPT_KGCOOP, teacher=None) == _lib.ERR_ARG
        assert call(B=0) == _lib.ERR_SHAPE and call(ws_bytes=64) == _lib.ERR_WORKSPACE
        assert call(mode=5) == _lib.ERR_ARG and "mode" in _lib.last_error()
    assert static(ctx=None) == _lib.ERR_ARG and static(grad_scale=0.0) == _lib.ERR_ARG and static(momentum=0.9) == _lib.ERR_ARG
    assert static(mode=_lib.PROMPT_PROGRAD, teacher=p, lam=float("nan")) == _lib.ERR_ARG
    assert scaled(mode=_lib.PROMPT_PROGRAD, teacher=p) == _lib.ERR_ARG and "ProGrad" in _lib.last_error()
    assert scaled(state=None) == _lib.ERR_ARG and scaled(growth=0.0) == _lib.ERR_ARG
    # everything above was refused before the text weights were looked at: a call that passes those checks is told they are not bound
    assert static() == _lib.ERR_STATE and scaled() == _lib.ERR_STATE
