"""CPU checks of ProDA's training path (clip_calibration_amd/prodafit.py, csrc/proda_train.hip): the restatement (tests/prodafit_ref.py) equals
float64 autograd through the oracle on the reference's own assembly and loss, the mean of the class features equals the oracle's
classifier, the selection schedule, the host-side refusals, the library's refusals without a device, the header."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import coopfit_ref as ref
import prodafit_ref as dref

from clip_calibration_amd import _lib, prodafit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
from oracle import clip_oracle as orc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-9


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("key,sel", dref.CASE_LIST, ids=ident)
def test_restatement_equals_autograd(key, sel):
    """Loss parts, gradient and text features of the restatement against float64 autograd through oracle.clip_oracle.text_encoder at
    rtol 1e-9.  The oracle's LayerNorm and softmax work in fp32 whatever the activation dtype, so its float64 run carries fp32
    rounding that no float64 formula reproduces (the plain float64 restatement is 2.5e-7 .. 1.0e-6 away on the gradient).  The
    restatement is therefore taken with those two islands restated as well (prodafit_ref.island_tower): the same fp32
    operations forward, their derivatives in fp32 backward, by hand.  The test below holds the plain float64 formulas, through a tower
    that is float64 throughout."""
    c = dref.make_case(*key)
    args = (c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"], sel)
    want, got = dref.oracle_parts(*args), dref.restated(*args, islands=True)
    figures = {k: abs(got[k] - want[k]) / max(1.0, abs(want[k])) for k in ("loss", "upper", "m")}
    figures.update({k: ref.rel_fro(got[k], want[k]) for k in ("grad", "text")})
    print(f"prodafit-restatement: {key} sel={sel} " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    assert got["grad"].shape == c["ctx"].shape and float(want["grad"].norm()) > 0.0
    assert all(v <= RTOL for v in figures.values()), figures
    if key[4] == 1:
        z = dref.head(c["feats"].double(), c["labels"], want["text"], key[1], 1, math.exp(dref.LOGIT_SCALE), dref.ALPHA)[4]
        x, u = dref.unit(c["feats"].double()), dref.unit(want["text"][:key[1]])
        assert torch.equal(z, math.exp(dref.LOGIT_SCALE) * x @ u.t() + 0.0)          # Pb = 1: sigma is exactly zero
    used = set(range(key[3])) if sel is None else set(sel)
    for p in range(key[3]):                 # a context outside the selection receives the no-class term alone
        if p not in used:
            only_m = dref.oracle_parts(*args[:5], sel, alpha=0.0)["grad"][p]
            assert float(only_m.abs().max()) == 0.0 and float(want["grad"][p].abs().max()) > 0.0


@pytest.mark.parametrize("key,sel", dref.CASE_LIST, ids=ident)
def test_restatement_equals_autograd_through_a_float64_tower(key, sel):
    """The same comparison with autograd running through coopfit_ref's forward formulas instead of the oracle's encoder: float64
    throughout, so the assembly by row formulas, the difference form of sigma, the head's backward, the tower's backward and the context
    reduce are held against the reference's slicing and its three-term sigma at rtol 1e-9."""
    c = dref.make_case(*key)
    args = (c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"], sel)
    want, got = dref.oracle_parts(*args, encoder=dref.restated_encoder), dref.restated(*args)
    for k in ("loss", "upper", "m"):
        assert abs(got[k] - want[k]) <= RTOL * max(1.0, abs(want[k])), k
    assert ref.rel_fro(got["grad"], want["grad"]) <= RTOL and ref.rel_fro(got["text"], want["text"]) <= RTOL


def test_restatement_equals_autograd_with_shorter_name_lens():
    """name_lens below the prompts' own: the row formulas against the truth's own assembly, the EOT rows staying the prompts'."""
    key, sel = ("tiny", 3, 5, 8, 2, 8), (0, 3)
    c = dref.make_case(*key)
    nl = dref.name_lens_of(c["ids"], key[2]) // 2
    args = (c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"], sel)
    for want, got in ((dref.oracle_parts(*args, name_lens=nl), dref.restated(*args, islands=True, name_lens=nl)),
                      (dref.oracle_parts(*args, encoder=dref.restated_encoder, name_lens=nl), dref.restated(*args, name_lens=nl))):
        assert abs(got["loss"] - want["loss"]) <= RTOL * max(1.0, abs(want["loss"]))
        assert ref.rel_fro(got["grad"], want["grad"]) <= RTOL and ref.rel_fro(got["text"], want["text"]) <= RTOL
    assert ref.rel_fro(dref.oracle_parts(*args)["grad"], want["grad"]) > 1e-3       # the lengths matter


@pytest.mark.parametrize("key,sel", dref.CASE_LIST, ids=ident)
def test_yardstick_is_finite(key, sel):
    c = dref.make_case(*key)
    yard, how = dref.yardstick_parts(c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"], sel)
    assert how in ("fp16", "fp32-rounded") and torch.isfinite(yard["grad"]).all() and math.isfinite(yard["loss"])


@pytest.mark.parametrize("key", [k for k in dref.CASES if k[3] == k[4]], ids=ident)
def test_mean_of_all_contexts_is_the_oracles_classifier(key):
    c = dref.make_case(*key)
    sd_c, ids_c = ref.cut(c["sd"], c["ids"])
    text = dref.restated(c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"], islands=True)["text"]     # the oracle's fp32 islands restated
    C, P = key[1], key[3]
    m = dref.unit(text[:C * P]).reshape(C, P, -1).mean(1)
    assert torch.allclose(m, orc.proda_classifier(sd_c, ids_c, c["ctx"].double(), torch.float64), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("B,C,E,Pb,P", dref.HEAD_CASES)
def test_head_cases_are_not_saturated(B, C, E, Pb, P):
    """The condition of the GPU head test: the float64 softmax of at least half the rows has its largest probability below 0.99."""
    wide, text, y = dref.head_case(B, C, E, Pb, P)
    z = dref.head(wide[:, 8:8 + E].double(), y, text.double(), C, Pb, dref.HEAD_SCALE, dref.ALPHA)[4]
    top = torch.softmax(z, dim=-1).max(dim=-1).values
    assert int((top < 0.99).sum()) * 2 >= B, top


def test_head_formulas_equal_autograd():
    g = torch.Generator().manual_seed(5)
    C, Pb, P, E = 4, 3, 4, 64
    f = torch.randn(6, E, generator=g, dtype=torch.float64)
    t = torch.randn(C * Pb + P, E, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.tensor([0, 3, 1, 1, 2, 0])
    total, upper, lm = dref.truth_loss(dref.unit(f), t[:C * Pb], t[C * Pb:], y, C, 20.0, 0.3)
    (d,) = torch.autograd.grad(total, t)
    got = dref.head(f, y, t.detach(), C, Pb, 20.0, 0.3)
    assert abs(float(got[0]) - float(total)) < 1e-11 and abs(float(got[1]) - float(upper)) < 1e-11 and abs(float(got[2]) - float(lm)) < 1e-13
    assert torch.allclose(got[3], d, rtol=1e-9, atol=1e-12)


# --------------------------------------------------------------------------------------------------------------------- the schedule
@pytest.mark.parametrize("P,Pb", [(8, 2), (32, 4), (4, 1), (8, 8)])
def test_drawn_schedule(P, Pb):
    n_iter, pos = P // Pb, prodafit.positions(P)
    assert np.array_equal(pos, dref.positions(P))
    sels = prodafit.draw_selections(P, Pb, 3 * n_iter, torch.Generator().manual_seed(11))
    again = prodafit.draw_selections(P, Pb, 3 * n_iter, torch.Generator().manual_seed(11))
    assert sels.shape == (3 * n_iter, Pb) and sels.dtype == np.int32 and np.array_equal(sels, again)
    g = torch.Generator().manual_seed(11)
    for r in range(3):
        block = sels[r * n_iter:(r + 1) * n_iter]
        assert sorted(block.reshape(-1).tolist()) == list(range(P))            # every context exactly once per P / Pb steps
        perm = np.arange(P) if n_iter == 1 else torch.randperm(P, generator=g).numpy()
        for k, row in enumerate(block):
            drawn = perm[k * Pb:(k + 1) * Pb]
            assert np.array_equal(row, dref.ordered(drawn, pos))               # the slice, end | middle | front, the draw order inside a group
            assert list(pos[row]) == sorted(pos[row], reverse=True)
    if n_iter > 1:
        assert not np.array_equal(sels, prodafit.draw_selections(P, Pb, 3 * n_iter, torch.Generator().manual_seed(12)))


def test_state_draws_the_same_schedule():
    """ProDAFitState.next_selection, step by step, is draw_selections (no device needed for the draw itself)."""
    st = types.SimpleNamespace(P=8, Pb=2, steps=0, _perm=None, generator=torch.Generator().manual_seed(3), pos_host=prodafit.positions(8))
    want = prodafit.draw_selections(8, 2, 9, torch.Generator().manual_seed(3))
    for k in range(9):
        st.steps = k
        assert np.array_equal(prodafit.ProDAFitState.next_selection(st), want[k])


# ------------------------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def cpu_model():
    return build_model(dict(ref.state_dict("tiny")), {"trainer": "CoOp"})


def test_argument_checks(cpu_model):
    c = dref.make_case("tiny", 3, 5, 8, 2, 8)
    ids, ctx, f, y = c["ids"], c["ctx"], c["feats"], c["labels"]
    cg, fit = prodafit.context_gradient, prodafit.fit_context
    with pytest.raises(ValueError, match="n_prompt.*mean of nothing"):
        cg(cpu_model, ids, ctx[:6], f, y)
    with pytest.raises(ValueError, match="n_prompt.*mean of nothing"):
        fit(f, y, cpu_model, ids, n_ctx=5, n_prompt=1, prompt_bs=1, epochs=1)
    with pytest.raises(ValueError, match="n_prompt"):
        prodafit.ProDAFitState(cpu_model, ids, ctx[:2], prompt_bs=2)
    with pytest.raises(ValueError, match="prompt_bs"):
        fit(f, y, cpu_model, ids, ctx, prompt_bs=3, epochs=1)
    with pytest.raises(ValueError, match="prompt_bs"):
        prodafit.ProDAFitState(cpu_model, ids, ctx, prompt_bs=3)
    with pytest.raises(ValueError, match="sel"):
        cg(cpu_model, ids, ctx, f, y, sel=[1, 1])
    with pytest.raises(ValueError, match="sel"):
        cg(cpu_model, ids, ctx, f, y, sel=[0, 8])
    with pytest.raises(ValueError, match="sel"):
        cg(cpu_model, ids, ctx, f, y, sel=[-1, 2])
    with pytest.raises(ValueError, match="sel"):
        cg(cpu_model, ids, ctx, f, y, sel=[0, 1, 2])                      # 3 does not divide 8
    with pytest.raises(ValueError, match="selections"):
        fit(f, y, cpu_model, ids, ctx, prompt_bs=2, epochs=1, batch_size=8, selections=[[3, 3]])
    with pytest.raises(ValueError, match="selections"):
        fit(f, y, cpu_model, ids, ctx, prompt_bs=2, epochs=2, batch_size=8, selections=[[3, 4]])     # two steps need two rows
    nl = dref.name_lens_of(ids, 5)
    for bad, what in ((-1, "negative"), (int(nl[1]) + 1, "past the live rows")):
        lens = nl.copy()
        lens[1] = bad
        with pytest.raises(ValueError, match="name_lens.*" + what):
            cg(cpu_model, ids, ctx, f, y, name_lens=lens)
    with pytest.raises(ValueError, match="name_lens"):
        cg(cpu_model, ids, ctx, f, y, name_lens=nl[:2])
    for alpha in (-0.1, math.inf, math.nan):
        with pytest.raises(ValueError, match="alpha"):
            cg(cpu_model, ids, ctx, f, y, alpha=alpha)
        with pytest.raises(ValueError, match="alpha"):
            fit(f, y, cpu_model, ids, ctx, prompt_bs=2, epochs=1, alpha=alpha)
    with pytest.raises(ValueError, match="grad_scale"):
        cg(cpu_model, ids, ctx, f, y, grad_scale=3.0)
    with pytest.raises(ValueError, match="momentum"):
        fit(f, y, cpu_model, ids, ctx, prompt_bs=2, epochs=1, momentum=1.0)
    with pytest.raises(ValueError, match="labels"):
        cg(cpu_model, ids, ctx, f, torch.full((8,), 3))
    with pytest.raises(ValueError, match="ctx"):
        cg(cpu_model, ids, ctx[0], f, y)
    with pytest.raises(ValueError, match="n_ctx"):
        cg(cpu_model, ids, torch.zeros(8, 30, 128), f, y)
    deep = types.SimpleNamespace(context_length=77, ln_final=cpu_model.ln_final, ivlp_text_prompts=lambda: (True,))
    with pytest.raises(ValueError, match="deep prompts"):
        cg(deep, ids, ctx, f, y)
    # more than 80 live rows: a stand-in with a longer context (the checks run before anything touches the model's weights)
    long_model = types.SimpleNamespace(context_length=96, ln_final=cpu_model.ln_final, text_dead_row_elimination=True)
    long_ids = torch.zeros(3, 96, dtype=torch.int64)
    long_ids[:, :77] = ids
    with pytest.raises(ValueError, match="80"):
        cg(long_model, long_ids, ctx, f, y, seq_rows=0)
    with pytest.raises(ValueError, match="80"):
        cg(long_model, long_ids, ctx, f, y, seq_rows=88)
    with pytest.raises(RuntimeError, match="GPU"):
        cg(cpu_model, ids, ctx, f, y)                                     # everything checks out: the call needs the device
    with pytest.raises(RuntimeError, match="GPU"):
        cg(cpu_model, ids, ctx, f, y, sel=[3, 6], name_lens=nl, alpha=0.0, seq_rows=0)
    with pytest.raises(RuntimeError, match="GPU"):
        cg(cpu_model, ids, ctx, f, y, name_lens=nl // 2)                  # shorter names than the prompts' own are the caller's to give
    with pytest.raises(ValueError, match="seq_rows"):
        cg(cpu_model, ids, ctx, f, y, seq_rows=8)                         # cuts an EOT row
    with pytest.raises(RuntimeError, match="GPU"):
        fit(f, y, cpu_model, ids, ctx, prompt_bs=2, epochs=1)
    out = fit(f, y, cpu_model, ids, ctx, prompt_bs=2, epochs=0)
    assert torch.equal(out, ctx)


def test_header_declares_the_entries_with_the_abi_at_16():
    text = open(os.path.join(ROOT, "include", "clipmi.h")).read()
    assert re.search(r"#define CLIPMI_ABI_VERSION 16\b", text) and _lib.ABI_VERSION == 16
    for n in ("clipmi_proda_embed", "clipmi_proda_head_workspace_bytes", "clipmi_proda_head", "clipmi_proda_ctx_step", "clipmi_proda_train_step_bytes",
              "clipmi_proda_train_step"):
        assert re.search(r"\b(int|size_t) " + n + r"\(", text), n
        assert n in _lib.exported_symbols() and hasattr(_lib.lib, n)


def test_library_refuses_bad_calls_without_a_device():
    """Argument checks that return before anything is launched."""
    lib = _lib.lib
    p = ctypes.c_void_p(4096)

    def embed(base=p, sel=p, eot=p, dtype=0, C=3, Pb=2, P=8, L=24, Lc=77, D=128, n_ctx=4):
        return lib.clipmi_proda_embed(base, p, dtype, p, sel, p, p, eot, p, p, C, Pb, P, L, Lc, D, n_ctx, None)
    assert embed(base=None) == _lib.ERR_ARG and embed(sel=None) == _lib.ERR_ARG and embed(eot=None) == _lib.ERR_ARG and embed(dtype=2) == _lib.ERR_ARG
    assert embed(Pb=9) == _lib.ERR_SHAPE and embed(P=1, Pb=1) == _lib.ERR_SHAPE and embed(C=1) == _lib.ERR_SHAPE
    assert embed(D=126) == _lib.ERR_SHAPE and embed(L=6) == _lib.ERR_SHAPE and embed(L=78) == _lib.ERR_SHAPE
    assert embed(base=ctypes.c_void_p(4100)) == _lib.ERR_ARG

    def head(feats=p, losses=p, alpha=0.1, ws_bytes=1 << 20, B=8, Pb=2, P=8):
        return lib.clipmi_proda_head(feats, 64, p, p, B, 64, 3, Pb, P, 100.0, 256.0, alpha, losses, p, p, ws_bytes, None)
    assert head(feats=None) == _lib.ERR_ARG and head(losses=None) == _lib.ERR_ARG
    assert head(alpha=-1.0) == _lib.ERR_ARG and "alpha" in _lib.last_error()
    assert head(alpha=math.nan) == _lib.ERR_ARG and head(alpha=math.inf) == _lib.ERR_ARG
    assert head(B=0) == _lib.ERR_SHAPE and head(Pb=0) == _lib.ERR_SHAPE and head(Pb=9) == _lib.ERR_SHAPE and head(P=1, Pb=1) == _lib.ERR_SHAPE
    assert head(ws_bytes=64) == _lib.ERR_WORKSPACE
    by = lib.clipmi_proda_head_workspace_bytes
    assert by(8, 64, 3, 2, 8) >= (2 * 8 + 3 * 2 + 8 + 3 * 64 + 2 * 8 * 3 + 64) * 4
    assert by(0, 64, 3, 2, 8) == 0 and by(8, 64, 1, 2, 8) == 0 and by(8, 64, 3, 9, 8) == 0 and by(8, 64, 3, 1, 1) == 0

    def step(d=p, sel=p, ctx=p, lr=p, grad=None, n_ctx=4, momentum=0.0, gs=256.0):
        return lib.clipmi_proda_ctx_step(d, ctx, None, grad, sel, p, p, 3, 2, 8, 24, 128, n_ctx, gs, lr, 1, momentum, 0.0, 0.0, 0, None)
    assert step(d=None) == _lib.ERR_ARG and step(sel=None) == _lib.ERR_ARG and step(ctx=None) == _lib.ERR_ARG      # nothing to write
    assert step(lr=None) == _lib.ERR_ARG and step(momentum=0.9) == _lib.ERR_ARG and step(gs=0.0) == _lib.ERR_ARG
    assert step(n_ctx=22) == _lib.ERR_SHAPE                     # SOS, 22 vectors, '.' and EOT do not fit 24 rows
    assert lib.clipmi_proda_train_step_bytes(None, 3, 2, 8, 0, 8) == 0
    assert lib.clipmi_proda_train_step(None, None, p, p, 0, p, None, 4, p, p, p, p, 3, 2, 8, 0, p, 64, p, 8, 100.0, 256.0, 0.1, p, 1, 0.0, 0.0, 0.0, 0, p, None,
                                       p, 1 << 20, p, 1 << 20, None) == _lib.ERR_ARG
