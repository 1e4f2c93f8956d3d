"""CPU checks of KgCoOp's and ProGrad's training path (clip_calibration_amd/coopfit.py with ``method=``, csrc/prompt_train.hip): the
restatement of both heads and of the projection rule (tests/promptfit_ref.py) equals float64 autograd through the oracle and the
reference's own arithmetic, the host-side argument checks, the library's refusals without a device, the header."""
import ctypes
import math
import os
import re

import pytest
import torch

import coopfit_ref as ref
import promptfit_ref as pref
from test_coopfit_cpu import RESTATEMENT_RTOL

from clip_calibration_amd import _lib, coopfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("geom,C,n_ctx,B,csc", ref.GRADIENT_CASES)
def test_restatement_equals_autograd(geom, C, n_ctx, B, csc):
    c = pref.case((geom, C, n_ctx, B, csc))
    want = pref.oracle_parts(c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"], c["teacher"], w=8.0, T=2.0)
    sd_c, ids_c = ref.cut(c["sd"], c["ids"])
    got = pref.restated(sd_c, ids_c, c["ctx"], c["feats"], c["labels"], c["teacher"], w=8.0, T=2.0)
    for k in ("kgcoop", "ce", "score", "xe", "kl"):
        assert abs(got[k] - want[k]) <= 1e-5 * max(1.0, abs(want[k])), k
    for k in ("grad_kgcoop", "grad_xe", "grad_kl"):
        assert got[k].shape == c["ctx"].shape
        assert ref.rel_fro(got[k], want[k]) <= RESTATEMENT_RTOL, k


@pytest.mark.parametrize("T,w", [(1.0, 8.0), (2.0, 0.0), (0.5, 64.0)])
def test_head_formulas_equal_autograd(T, w):
    g = torch.Generator().manual_seed(5)
    f = torch.randn(6, 64, generator=g, dtype=torch.float64)
    t = torch.randn(4, 64, generator=g, dtype=torch.float64, requires_grad=True)
    o = torch.randn(4, 64, generator=g, dtype=torch.float64) * 3.0          # not normalised: the head normalises
    y = torch.tensor([0, 3, 1, 1, 2, 0])
    x = pref.unit(f)
    z = 100.0 * x @ pref.unit(t).t()
    total, ce, score = pref.kgcoop_loss(z, y, t, o, w)
    (d_kg,) = torch.autograd.grad(total, t, retain_graph=True)
    xe, kl = pref.prograd_losses(z, (100.0 * x @ pref.unit(o).t()).detach(), y, T)
    (d_xe,) = torch.autograd.grad(xe, t, retain_graph=True)
    (d_kl,) = torch.autograd.grad(kl, t)
    got = pref.kgcoop_head(f, y, t.detach(), o, 100.0, w)
    assert abs(float(got[0]) - float(total)) < 1e-12 and abs(float(got[1]) - float(ce)) < 1e-12 and abs(float(got[2]) - float(score)) < 1e-12
    assert torch.allclose(got[3], d_kg, rtol=1e-9, atol=1e-13)
    got = pref.prograd_head(f, y, t.detach(), o, 100.0, T)
    assert abs(float(got[0]) - float(xe)) < 1e-12 and abs(float(got[1]) - float(kl)) <= 1e-12 * max(1.0, float(kl))
    assert torch.allclose(got[2], d_xe, rtol=1e-9, atol=1e-13) and torch.allclose(got[3], d_kl, rtol=1e-9, atol=1e-13)
    if w == 0.0:
        assert torch.equal(pref.kgcoop_head(f, y, t.detach(), o, 100.0, 0.0)[3], ref.head(f, y, t.detach(), 100.0)[1])


def reference_update(a, b, lam):
    """The arithmetic of the reference's prograd_backward_and_update (prograd.py:396-405) on one parameter: both gradients normalised,
    their dot product compared with zero, the component of a along the normalised b taken out."""
    b_unit = b / torch.linalg.norm(b)
    a_unit = a / torch.linalg.norm(a)
    if torch.dot(a_unit.flatten(), b_unit.flatten()) < 0:
        return a - lam * torch.dot(a.flatten(), b_unit.flatten()) * b_unit
    return a


@pytest.mark.parametrize("lam", [1.0, 0.5])
def test_projection_rule_is_the_references(lam):
    g = torch.Generator().manual_seed(6)
    seen = set()
    for _ in range(40):
        a = torch.randn(4, 16, generator=g, dtype=torch.float64)
        b = torch.randn(4, 16, generator=g, dtype=torch.float64)
        got, projected = pref.project(a, b, lam)
        assert projected == (pref.cosine(a, b) < 0)
        assert torch.allclose(got, reference_update(a, b, lam), rtol=1e-12, atol=1e-14)
        if projected:
            assert abs(pref.cosine(got, b) - (1.0 - lam) * pref.cosine(a, b) * float(a.norm() / got.norm())) < 1e-12
        seen.add(projected)
    assert seen == {True, False}
    a = torch.randn(4, 16, generator=g, dtype=torch.float64)
    zero = torch.zeros_like(a)
    got, projected = pref.project(a, zero, lam)                 # b = 0: the reference's comparison is NaN < 0, false
    assert not projected and torch.equal(got, a) and torch.equal(reference_update(a, zero, lam), a)
    assert not pref.project(zero, a, lam)[1] and not pref.project(a, a * float("nan"), lam)[1]


@pytest.fixture(scope="module")
def cpu_model():
    return build_model(dict(ref.state_dict("tiny")), {"trainer": "CoOp"})


def test_argument_checks(cpu_model):
    c = pref.case(("tiny", 3, 4, 8, False))
    ids, ctx, f, y, t = c["ids"], c["ctx"], c["feats"], c["labels"], c["teacher"]
    cg = coopfit.context_gradient
    with pytest.raises(ValueError, match="method"):
        cg(cpu_model, ids, ctx, f, y, method="proda", teacher=t)
    for method in ("kgcoop", "prograd"):
        with pytest.raises(ValueError, match="teacher"):
            cg(cpu_model, ids, ctx, f, y, method=method)
        with pytest.raises(ValueError, match="teacher"):
            cg(cpu_model, ids, ctx, f, y, method=method, teacher=t[:2])
        with pytest.raises(ValueError, match="teacher"):
            cg(cpu_model, ids, ctx, f, y, method=method, teacher=t.double())
        with pytest.raises(ValueError, match="w="):
            cg(cpu_model, ids, ctx, f, y, method=method, teacher=t, w=-1.0)
        with pytest.raises(ValueError, match="w="):
            cg(cpu_model, ids, ctx, f, y, method=method, teacher=t, w=math.inf)
        with pytest.raises(ValueError, match="T="):
            cg(cpu_model, ids, ctx, f, y, method=method, teacher=t, T=0.0)
        with pytest.raises(ValueError, match="T="):
            cg(cpu_model, ids, ctx, f, y, method=method, teacher=t, T=math.nan)
        with pytest.raises(ValueError, match="lam="):
            cg(cpu_model, ids, ctx, f, y, method=method, teacher=t, lam=math.inf)
        with pytest.raises(RuntimeError, match="GPU"):
            cg(cpu_model, ids, ctx, f, y, method=method, teacher=t)              # everything checks out: the call needs the device
        with pytest.raises(ValueError, match="T="):
            coopfit.fit_context(f, y, cpu_model, ids, ctx, epochs=1, method=method, teacher=t, T=-1.0)
        with pytest.raises(ValueError, match="teacher"):
            coopfit.CoOpFitState(cpu_model, ids, ctx, method=method)
    with pytest.raises(ValueError, match="method"):
        coopfit.fit_context(f, y, cpu_model, ids, ctx, epochs=1, method="KgCoOp", teacher=t)
    out = coopfit.fit_context(f, y, cpu_model, ids, ctx, epochs=0, method="prograd", teacher=t)
    assert torch.equal(out, ctx)


def test_trainers_need_their_teacher(cpu_model):
    from clip_calibration_amd.trainers import kgcoop, prograd
    from clip_calibration_amd.trainers.coop import CustomCLIP as CoOp
    ids = ref.prompt_ids("tiny", 3, 4)
    with pytest.raises(ValueError, match="zeroshot_tokenized_prompts"):
        kgcoop.CustomCLIP(cpu_model, ids, n_ctx=4).fit_context([])
    with pytest.raises(ValueError, match="zeroshot_tokenized_prompts"):
        prograd.CustomCLIP(cpu_model, ids, n_ctx=4).fit_context([])
    assert issubclass(prograd.CustomCLIP, CoOp) and prograd.CustomCLIP is not CoOp and prograd.CLIP is not None
    assert prograd.CustomCLIP.forward is CoOp.forward


def test_header_declares_the_entries_with_the_abi_at_16():
    text = open(os.path.join(ROOT, "include", "clipmi.h")).read()
    assert re.search(r"#define CLIPMI_ABI_VERSION 16\b", text) and _lib.ABI_VERSION == 16
    for n in ("clipmi_prompt_head_workspace_bytes", "clipmi_prompt_head", "clipmi_prograd_step_workspace_bytes", "clipmi_prograd_step",
              "clipmi_prompt_train_step_bytes", "clipmi_prompt_train_step"):
        assert re.search(r"\b(int|size_t) " + n + r"\(", text), n
        assert n in _lib.exported_symbols() and hasattr(_lib.lib, n)
    assert re.search(r"`mode` is a plain integer: 0 CoOp, 1 KgCoOp, 2 ProGrad", text)
    assert (_lib.PROMPT_COOP, _lib.PROMPT_KGCOOP, _lib.PROMPT_PROGRAD) == (0, 1, 2)


def test_library_refuses_bad_calls_without_a_device():
    """Argument checks that return before anything is launched."""
    lib = _lib.lib
    p = ctypes.c_void_p(4096)

    def head(mode=_lib.PROMPT_PROGRAD, feats=p, teacher=p, w=8.0, T=1.0, losses=p, d_kl=p, ws_bytes=1 << 20, B=8):
        return lib.clipmi_prompt_head(feats, 64, p, p, B, 64, 3, 100.0, 256.0, mode, teacher, w, T, losses, p, None, d_kl, p, ws_bytes, None)
    assert head(mode=3) == _lib.ERR_ARG and "mode" in _lib.last_error()
    assert head(mode=-1) == _lib.ERR_ARG
    assert head(feats=None) == _lib.ERR_ARG and head(losses=None) == _lib.ERR_ARG
    assert head(teacher=None) == _lib.ERR_ARG and head(mode=_lib.PROMPT_KGCOOP, teacher=None) == _lib.ERR_ARG
    assert head(d_kl=None) == _lib.ERR_ARG
    assert head(T=0.0) == _lib.ERR_ARG and "T=" in _lib.last_error()
    assert head(T=-1.0) == _lib.ERR_ARG and head(T=math.inf) == _lib.ERR_ARG and head(T=math.nan) == _lib.ERR_ARG
    assert head(mode=_lib.PROMPT_KGCOOP, w=-1.0) == _lib.ERR_ARG and head(mode=_lib.PROMPT_KGCOOP, w=math.nan) == _lib.ERR_ARG
    assert head(B=0) == _lib.ERR_SHAPE
    assert head(ws_bytes=64) == _lib.ERR_WORKSPACE
    by = lib.clipmi_prompt_head_workspace_bytes
    assert by(8, 64, 3, 3) == 0 and by(8, 64, 1, 0) == 0
    assert by(8, 64, 3, 0) == lib.clipmi_coop_head_workspace_bytes(8, 64, 3)
    assert by(8, 64, 3, 1) >= (2 * 8 * 3 + 16 + 3 + 2 * 3) * 4 and by(8, 64, 3, 2) >= (4 * 8 * 3 + 24 + 3 + 2 * 3) * 4

    def step(a=p, b=p, ws=p, ws_bytes=1 << 20, lam=1.0, ctx=p, lr=p, n_ctx=4, momentum=0.0):
        return lib.clipmi_prograd_step(a, b, ctx, None, None, None, None, 3, 8, 64, n_ctx, 0, 256.0, lam, lr, 1, momentum, 0.0, 0.0, 0, ws, ws_bytes, None)
    assert step(a=None) == _lib.ERR_ARG and step(b=None) == _lib.ERR_ARG and step(ws=None) == _lib.ERR_ARG
    assert step(ctx=None) == _lib.ERR_ARG                       # nothing to write
    assert step(lr=None) == _lib.ERR_ARG and step(lam=math.nan) == _lib.ERR_ARG
    assert step(momentum=0.9) == _lib.ERR_ARG                  # a momentum needs the buffer
    assert step(n_ctx=8) == _lib.ERR_SHAPE                     # 1 + n_ctx > L
    assert step(ws_bytes=64) == _lib.ERR_WORKSPACE
    assert lib.clipmi_prograd_step_workspace_bytes(3, 64, 4, 0) >= 3 * 8 + 2 * 4 * 64 * 4 and lib.clipmi_prograd_step_workspace_bytes(3, 64, 0, 0) == 0
    assert lib.clipmi_prompt_train_step_bytes(None, 3, 0, 8, 2, 4, 0) == 0
    assert lib.clipmi_prompt_train_step(None, None, p, 0, p, None, 4, 0, p, 3, 0, p, 64, p, 8, 100.0, 256.0, 2, p, 8.0, 1.0, 1.0, p, 1, 0.0, 0.0, 0.0, 0,
                                        p, None, None, None, p, 1 << 20, p, 1 << 20, None) == _lib.ERR_ARG
