"""VPT's training path without a GPU: the hand-written restatement of tests/vptfit_ref.py against torch autograd through the oracle's
image tower in float64, and the package's new surface."""
import pytest
import torch

import vptfit_ref as ref

# The restatement is float64 throughout; the oracle keeps fp32 inside its float64 run (softmax and LayerNorm are evaluated in fp32 as the
# reference evaluates them), so the distance between the two is fp32 round-off amplified by the blocks, not float64 round-off.  Measured on
# these cases (printed below): loss 1e-7 .. 1.2e-6 absolute on losses of 5 .. 15, gradient 1.3e-7 .. 3.2e-7 relative.  Both bounds are about
# 10 x the largest measured (the loss's is relative to the loss); a formula error is of order 1.
BOUND, LOSS_BOUND = 3e-6, 1e-5


@pytest.mark.parametrize("geom,n_ctx,depth,B,C", ref.GRADIENT_CASES)
def test_restatement_equals_autograd_in_float64(geom, n_ctx, depth, B, C):
    c = ref.make_case(geom, n_ctx, depth, B, C)
    loss, grad = ref.loss_and_grad(c["sd"], c["images"], c["prompts"], c["text"], c["labels"])
    loss_t, grad_t = ref.oracle_loss_grad(c["sd"], c["images"], c["prompts"], c["text"], c["labels"])
    err = ref.rel_fro(grad, grad_t)
    print(f"\nvptfit-cpu: {geom} n_ctx={n_ctx} depth={depth} B={B} C={C}: loss {abs(float(loss - loss_t)):.2e}, grad rel {err:.2e} (bound {BOUND:.0e})")
    assert grad.shape == (depth, n_ctx, ref.geometry(geom).vision_width)
    assert abs(float(loss - loss_t)) <= LOSS_BOUND * max(1.0, abs(float(loss_t)))
    assert err <= BOUND
    for i in range(depth):
        assert float(grad_t[i].norm()) > 0, f"slot {i} carries no gradient: the case tests nothing there"


def test_attention_backward_full_restatement_equals_autograd():
    gen = torch.Generator().manual_seed(3)
    for L in (1, 17, 33):
        N, H = 2, 2
        qkv = torch.randn(N * L, 3 * 64 * H, generator=gen, dtype=torch.float64, requires_grad=True)
        d_out = torch.randn(N * L, 64 * H, generator=gen, dtype=torch.float64)
        (ref.attention_forward_full(qkv, N, L, H) * d_out).sum().backward()
        assert ref.rel_fro(ref.attention_backward_full(qkv.detach(), d_out, N, L, H), qkv.grad) <= 1e-13


def test_head_image_equals_autograd():
    gen = torch.Generator().manual_seed(4)
    f = torch.randn(5, 64, generator=gen, dtype=torch.float64, requires_grad=True)
    t = torch.randn(7, 64, generator=gen, dtype=torch.float64)
    y = torch.randint(0, 7, (5,), generator=gen)
    z = 100.0 * torch.nn.functional.normalize(f, dim=-1) @ torch.nn.functional.normalize(t, dim=-1).t()
    loss_t = torch.nn.functional.cross_entropy(z, y)
    loss_t.backward()
    loss, d, _ = ref.head_image(f.detach(), y, t, 100.0)
    assert abs(float(loss - loss_t)) <= 1e-13 and ref.rel_fro(d, f.grad) <= 1e-13


def test_package_surface():
    """The symbols this feature adds: the C entry points, the Python module and the trainer's method."""
    from clip_calibration_amd import _lib, vptfit
    from clip_calibration_amd.trainers import vpt
    for name in ("clipmi_attention_backward_full", "clipmi_vision_train_bytes", "clipmi_vision_encoder_train", "clipmi_vision_encoder_backward",
                 "clipmi_vpt_head", "clipmi_vpt_head_workspace_bytes", "clipmi_vpt_step", "clipmi_vpt_train_step", "clipmi_vpt_train_step_bytes"):
        assert hasattr(_lib.lib, name), name
    assert _lib.ABI_VERSION == 16
    for name in ("VPTFitState", "prompt_gradient", "fit_prompts"):
        assert callable(getattr(vptfit, name))
    assert callable(vpt.CustomCLIP.fit_prompts)


def test_refusals_need_no_gpu():
    from clip_calibration_amd import _lib, synthetic as syn, vptfit
    from clip_calibration_amd.model import build_model
    lib = _lib.lib
    assert lib.clipmi_attention_backward_full(None, None, None, 1, 225, 1, None) == _lib.ERR_SHAPE
    assert lib.clipmi_attention_backward_full(None, None, None, 1, 0, 1, None) == _lib.ERR_SHAPE
    assert lib.clipmi_attention_backward_full(None, None, None, 1, 224, 1, None) == _lib.ERR_ARG
    assert lib.clipmi_attention_backward_full(16, 16, 8, 1, 224, 1, None) == _lib.ERR_ARG
    sd = syn.synthetic_state_dict("tiny", seed=0)
    text = torch.zeros(3, 128)
    with pytest.raises(ValueError, match="trainer='VPT'"):
        vptfit.model_prompts(build_model(dict(sd), {"trainer": "CoOp"}))
    m = build_model(dict(sd), {"trainer": "VPT", "vision_depth": 2, "vision_ctx": 4, "language_depth": 0, "language_ctx": 0})
    assert tuple(vptfit.model_prompts(m).shape) == (2, 4, 128)
    with pytest.raises(ValueError, match="n_ctx"):
        vptfit._check_prompts("t", m, torch.zeros(2, 5, 128))
    big = build_model(dict(syn.synthetic_state_dict(ref.CUSTOM, seed=0)),
                      {"trainer": "VPT", "vision_depth": 1, "vision_ctx": 28, "language_depth": 0, "language_ctx": 0})
    with pytest.raises(ValueError, match="at most 224"):
        vptfit._check_prompts("t", big, vptfit.model_prompts(big))
    del text
