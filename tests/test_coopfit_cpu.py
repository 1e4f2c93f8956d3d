"""CPU checks of CoOp's training path (clip_calibration_amd/coopfit.py, csrc/text_backward.hip, csrc/prompt_train.hip): the hand-written restatement of every
backward formula (tests/coopfit_ref.py) equals float64 autograd through the oracle, the host-side argument checks, the header."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import coopfit_ref as ref

from clip_calibration_amd import _lib, coopfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def case(*key):
    return ref.make_case(*key)


# The oracle's LayerNorm and softmax work in fp32 whatever the activation dtype (oracle.clip_oracle.layer_norm), so its "float64" run
# carries fp32 rounding inside: 2^-24 per operation, amplified by the blocks.  1e-4 relative on the whole gradient is three orders
# above that and two below the fp16 yardstick of the GPU tests.
RESTATEMENT_RTOL = 1e-4


@pytest.mark.parametrize("geom,C,n_ctx,B,csc", ref.GRADIENT_CASES)
def test_restatement_equals_autograd(geom, C, n_ctx, B, csc):
    c = case(geom, C, n_ctx, B, csc)
    loss_o, grad_o = ref.oracle_loss_grad(c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"])
    sd_c, ids_c = ref.cut(c["sd"], c["ids"])
    loss_r, grad_r = ref.loss_and_grad(sd_c, ids_c, c["ctx"], c["feats"], c["labels"])
    assert grad_r.shape == c["ctx"].shape
    assert abs(float(loss_r) - float(loss_o)) <= 1e-5 * max(1.0, abs(float(loss_o)))
    assert ref.rel_fro(grad_r, grad_o) <= RESTATEMENT_RTOL


def test_restatement_live_row_cut_is_exact_in_exact_arithmetic():
    """Rows behind the last EOT influence nothing: the gradient on 24 live rows equals the one on the whole context."""
    c = case("tiny", 3, 4, 8, False)
    _, g_full = ref.loss_and_grad(c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"])
    _, g_cut = ref.loss_and_grad(c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"], rows=16)
    assert ref.rel_fro(g_cut, g_full) <= 1e-12


def test_operator_formulas_equal_autograd():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 64, generator=g, dtype=torch.float64, requires_grad=True)
    gamma, beta = torch.randn(64, generator=g, dtype=torch.float64), torch.randn(64, generator=g, dtype=torch.float64)
    dy = torch.randn(5, 64, generator=g, dtype=torch.float64)
    torch.nn.functional.layer_norm(x, (64,), gamma, beta, 1e-5).backward(dy)
    assert torch.allclose(ref.ln_backward(x.detach(), gamma, dy), x.grad, rtol=1e-10, atol=1e-12)
    h = torch.randn(300, generator=g, dtype=torch.float64, requires_grad=True)
    da = torch.randn(300, generator=g, dtype=torch.float64)
    ref.quickgelu(h).backward(da)
    assert torch.allclose(ref.quickgelu_backward(h.detach(), da), h.grad, rtol=1e-10, atol=1e-12)
    qkv = torch.randn(2 * 7, 3 * 128, generator=g, dtype=torch.float64, requires_grad=True)
    do = torch.randn(2 * 7, 128, generator=g, dtype=torch.float64)
    ref.attention_forward(qkv, 2, 7, 2).backward(do)
    assert torch.allclose(ref.attention_backward(qkv.detach(), do, 2, 7, 2), qkv.grad, rtol=1e-9, atol=1e-12)
    f = torch.randn(6, 64, generator=g, dtype=torch.float64)
    t = torch.randn(4, 64, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.tensor([0, 3, 1, 1, 2, 0])
    z = 100.0 * torch.nn.functional.normalize(f, dim=-1) @ torch.nn.functional.normalize(t, dim=-1).t()
    loss = torch.nn.functional.cross_entropy(z, y)
    loss.backward()
    loss_r, d_text, _ = ref.head(f, y, t.detach(), 100.0)
    assert abs(float(loss_r) - float(loss.detach())) < 1e-12 and torch.allclose(d_text, t.grad, rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize("momentum,dampening,wd,nesterov", [(0.0, 0.0, 0.0, False), (0.9, 0.0, 5e-4, False), (0.9, 0.0, 0.0, True), (0.5, 0.1, 1e-2, False)])
def test_sgd_rule_equals_torch(momentum, dampening, wd, nesterov):
    g = torch.Generator().manual_seed(4)
    w0 = torch.randn(4, 8, generator=g, dtype=torch.float64)
    p = torch.nn.Parameter(w0.clone())
    opt = torch.optim.SGD([p], lr=0.1, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    w, buf = w0.clone(), None
    for k in range(3):
        grad = torch.randn(4, 8, generator=g, dtype=torch.float64)
        p.grad = grad.clone()
        opt.step()
        w, buf = ref.sgd_step(w, buf, grad, 0.1, momentum, dampening, wd, nesterov, k == 0)
        assert torch.allclose(w, p.detach(), rtol=1e-13, atol=0)


@pytest.fixture(scope="module")
def cpu_model():
    return build_model(dict(ref.state_dict("tiny")), {"trainer": "CoOp"})


def test_argument_checks(cpu_model):
    c = case("tiny", 3, 4, 8, False)
    ids, ctx, f, y = c["ids"], c["ctx"], c["feats"], c["labels"]
    cg = coopfit.context_gradient
    with pytest.raises(ValueError, match="power of two"):
        cg(cpu_model, ids, ctx, f, y, grad_scale=3.0)
    with pytest.raises(ValueError, match="power of two"):
        cg(cpu_model, ids, ctx, f, y, grad_scale=0.0)
    with pytest.raises(ValueError, match="ctx"):
        cg(cpu_model, ids, ctx[:, :64], f, y)                      # wrong width
    with pytest.raises(ValueError, match="one context per prompt"):
        cg(cpu_model, ids, ctx.unsqueeze(0).repeat(2, 1, 1), f, y)  # class-specific with the wrong C
    with pytest.raises(ValueError, match="n_ctx"):
        cg(cpu_model, ids, torch.zeros(5, 128), f, y)               # prompt 0's EOT sits at 1 + 4: five context rows overwrite it
    with pytest.raises(ValueError, match="tokenized_prompts"):
        cg(cpu_model, ids[:, :40], ctx, f, y)
    with pytest.raises(ValueError, match="features"):
        cg(cpu_model, ids, ctx, f[:, :64], y)
    with pytest.raises(ValueError, match="labels"):
        cg(cpu_model, ids, ctx, f, torch.full_like(y, 3))           # label == C
    with pytest.raises(ValueError, match="labels"):
        cg(cpu_model, ids, ctx, f, y[:5])
    with pytest.raises(RuntimeError, match="GPU"):
        cg(cpu_model, ids, ctx, f, y)                               # everything checks out: the call needs the device
    with pytest.raises(ValueError, match="Nesterov"):
        coopfit.fit_context(f, y, cpu_model, ids, ctx, epochs=1, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError, match="order"):
        coopfit.fit_context(f, y, cpu_model, ids, ctx, epochs=1, order=np.zeros((2, 8), np.int64))
    with pytest.raises(ValueError, match="learning rates"):
        coopfit.fit_context(f, y, cpu_model, ids, ctx, epochs=2, lr_per_epoch=[0.1])


def test_deep_prompts_are_refused():
    sd = dict(ref.state_dict("tiny"))
    model = build_model(sd, {"trainer": "CoOp"})
    model.ivlp_text_prompts = lambda: ([torch.zeros(4, 128)], 4)    # what an IVLP model reports
    c = case("tiny", 3, 4, 8, False)
    with pytest.raises(ValueError, match="deep prompts"):
        coopfit.context_gradient(model, c["ids"], c["ctx"], c["feats"], c["labels"])


def test_zero_epoch_fit_returns_the_context(cpu_model):
    c = case("tiny", 3, 4, 8, False)
    out, hist = coopfit.fit_context(c["feats"], c["labels"], cpu_model, c["ids"], c["ctx"], epochs=0, return_history=True)
    assert torch.equal(out, c["ctx"]) and out.data_ptr() != c["ctx"].data_ptr() and hist.shape == (0,)
    out = coopfit.fit_context(c["feats"], c["labels"], cpu_model, c["ids"], c["ctx"], epochs=3, batch_size=16, drop_last=True)
    assert torch.equal(out, c["ctx"])                               # 8 samples, batches of 16, the short one dropped: no step


def test_header_declares_the_entries_with_the_abi_at_16():
    text = open(os.path.join(ROOT, "include", "clipmi.h")).read()
    assert re.search(r"#define CLIPMI_ABI_VERSION 16\b", text) and _lib.ABI_VERSION == 16
    names = ["clipmi_text_train_bytes", "clipmi_text_encoder_train", "clipmi_text_encoder_backward", "clipmi_coop_head", "clipmi_ctx_step",
             "clipmi_layernorm_backward", "clipmi_attention_backward", "clipmi_quickgelu_backward", "clipmi_coop_train_step"]
    for n in names:
        assert re.search(r"\b(int|size_t) " + n + r"\(", text), n
        assert n in _lib.exported_symbols() and hasattr(_lib.lib, n)


@pytest.mark.parametrize("geom", ["tiny", "tiny3"])
def test_coop_sizes_are_mode_0_of_the_prompt_sizes(geom):
    """clipmi_coop_head_workspace_bytes and clipmi_coop_train_step_bytes wrap the prompt learners' sizing functions at mode 0, whose size
    depends on neither n_ctx nor ctx_per_class; shapes either refuses keep their zero."""
    lib = _lib.lib
    m = build_model(dict(ref.state_dict(geom)), {"trainer": "CoOp"})
    m._ensure_handle()
    h, E = m._handle, int(m.geometry.embed_dim)
    for Cn in (2, 3, 37, 257):
        for B in (1, 4):
            head = lib.clipmi_coop_head_workspace_bytes(B, E, Cn)
            assert head >= (2 * B * Cn + 2 * B + Cn) * 4 and head == lib.clipmi_prompt_head_workspace_bytes(B, E, Cn, _lib.PROMPT_COOP)
            for rows in (0, 16):
                step = lib.clipmi_coop_train_step_bytes(h, Cn, rows, B)
                assert step > head
                for n_ctx, per_class in ((1, 0), (4, 0), (16, 1)):
                    assert step == lib.clipmi_prompt_train_step_bytes(h, Cn, rows, B, _lib.PROMPT_COOP, n_ctx, per_class)
    assert lib.clipmi_coop_head_workspace_bytes(0, E, 3) == 0 and lib.clipmi_coop_head_workspace_bytes(4, 0, 3) == 0
    assert lib.clipmi_coop_head_workspace_bytes(4, E, 1) == 0
    assert lib.clipmi_coop_train_step_bytes(None, 3, 0, 4) == 0 and lib.clipmi_coop_train_step_bytes(h, 1, 0, 4) == 0
    assert lib.clipmi_coop_train_step_bytes(h, 3, 0, 0) == 0 and lib.clipmi_coop_train_step_bytes(h, -1, 0, 4) == 0


def test_library_refuses_bad_calls_without_a_device():
    """Argument checks that return before anything is launched."""
    lib = _lib.lib
    assert lib.clipmi_attention_backward(None, None, None, 1, 81, 1, None) == _lib.ERR_SHAPE          # more than 80 token rows
    assert lib.clipmi_attention_backward(None, None, None, 1, 8, 1, None) == _lib.ERR_ARG            # null pointers
    assert lib.clipmi_attention_backward(None, None, None, 0, 8, 1, None) == _lib.OK                 # nothing to do
    assert lib.clipmi_layernorm_backward(None, 64, None, None, None, _lib.F32, None, None, 0, 64, 1e-5, None) == _lib.OK
    assert lib.clipmi_layernorm_backward(None, 64, None, None, None, _lib.F32, None, None, 1, 66, 1e-5, None) == _lib.ERR_SHAPE
    assert lib.clipmi_quickgelu_backward(None, None, None, 8, None) == _lib.ERR_ARG
    assert lib.clipmi_coop_head_workspace_bytes(8, 64, 1) == 0 and lib.clipmi_coop_head_workspace_bytes(8, 64, 3) >= (2 * 8 * 3 + 16 + 3) * 4
    assert lib.clipmi_ctx_step(None, None, None, None, 3, 8, 64, 4, 0, 1.0, None, 0, 0.0, 0.0, 0.0, 0, None) == _lib.ERR_ARG
