"""The image tower's training path beyond 224 token rows per image (library option vision_train_long): VPT, MaPLe and PromptSRC / IVLP on a
toy tower with ViT-L/14's 257 tokens, end to end against float64 autograd through the oracle.

The toy tower: 128 px images in patches of 8 (16 x 16 + 1 = 257 tokens), width 128 (two heads), two layers -- the smallest tower that
reaches clipmi_attention_backward_long through run_vision_backward (the training forward serves patches of 8, 16 and 32)."""
import ctypes

import numpy as np
import pytest
import torch

import maplefit_ref as mref
import promptsrcfit_ref as sref
import vptfit_ref as ref
from clip_calibration_amd import _lib, maplefit, promptsrcfit, synthetic as syn, vptfit
from clip_calibration_amd.model import build_model

pytestmark = pytest.mark.gpu
FACTOR = 2.0      # the project's bound: within 2 x the oracle's own fp16-autograd error on the same case
TOY = "toy257"
TOY_GEOMETRY = syn.ClipGeometry(128, 128, 2, 128, 8, 77, 256, 128, 2, 2)
TOKENS = 257
_CACHE = {}


@pytest.fixture(autouse=True)
def toy_geometry_and_option():
    """The reference modules look geometries up by name: the toy one is registered for the test and taken out again; the option is put
    back to what it was."""
    before = _lib.get_option("vision_train_long")
    syn.GEOMETRIES[TOY] = TOY_GEOMETRY
    try:
        yield
    finally:
        syn.GEOMETRIES.pop(TOY, None)
        _lib.set_option("vision_train_long", before)


def long_on():
    _lib.set_option("vision_train_long", 1)


def vpt_case(geom, n_ctx, depth, B, C, separable=False):
    key = ("vpt", geom, n_ctx, depth, B, C, separable)
    if key not in _CACHE:
        c = ref.make_case(geom, n_ctx, depth, B, C, separable=separable)
        c["model"] = build_model(dict(c["sd"]), {"trainer": "VPT", "vision_depth": depth, "vision_ctx": n_ctx, "language_depth": 0, "language_ctx": 0}).cuda()
        _CACHE[key] = c
    return _CACHE[key]


def test_geometry():
    assert TOY_GEOMETRY.grid ** 2 + 1 == TOKENS and TOKENS > vptfit.MAX_ROWS


def test_option_off_refuses_and_option_on_accepts():
    c = vpt_case(TOY, 8, 2, 2, 5)
    m, text = c["model"], c["text"].cuda()
    m._ensure_bound()
    ws, st = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert _lib.get_option("vision_train_long") == 0 and vptfit.max_rows() == 224
    with pytest.raises(ValueError, match="at most 224"):
        vptfit.VPTFitState(m, text)
    assert _lib.lib.clipmi_vision_train_bytes(m._handle, 2, 8, ctypes.byref(ws), ctypes.byref(st)) == _lib.ERR_SHAPE and ws.value == 0 and st.value == 0
    long_on()
    assert vptfit.max_rows() == 640
    vptfit.VPTFitState(m, text)
    assert _lib.lib.clipmi_vision_train_bytes(m._handle, 2, 8, ctypes.byref(ws), ctypes.byref(st)) == _lib.OK
    B, L, D, E, H, layers = 2, TOKENS + 8, 128, 128, 2, 2
    M = B * L
    a = lambda n: (n + 255) // 256 * 256
    abl = _lib.lib.clipmi_attention_backward_long_bytes(B, L, H)
    assert abl == 12 * B * H * L
    # the documented layout: the tower's pieces, the gradient stream, the fp16 image copy, the fp16 prompts, slot 0's sum, the long kernel's statistics
    want = (2 * a(M * D * 2) + a(M * D * 8) + a(M * D * 6) + a(M * D * 4) + a(B * D * 2) + a(B * E * 2) + a(B * D * 4) + a(M * D * 4)
            + a(B * 3 * 128 * 128 * 2) + a(layers * 8 * D * 2) + a(8 * D * 4) + a(abl))
    assert ws.value == want, (ws.value, want)
    assert st.value == (2 * layers + 1) * a(M * D * 4) + layers * (a(M * D * 6) + a(M * D * 8)) + a(B * 8) + a(layers * 8 * D * 4)
    assert vptfit.stash_bytes(m, 2, 8) == (ws.value, st.value)
    with pytest.raises(ValueError, match="at most 640"):
        vptfit.check_rows("x", 577, 64)


def test_vpt_gradient_within_the_fp16_yardstick():
    """vptfit.prompt_gradient at 257 + 8 = 265 rows, depth 2, against float64 autograd through the oracle: within 2 x the fp16 reference's
    own error on the same inputs (tests/test_gpu_vptfit.py's bound)."""
    long_on()
    n_ctx, depth, B, C = 8, 2, 2, 5
    c = vpt_case(TOY, n_ctx, depth, B, C)
    loss64, grad64 = ref.oracle_loss_grad(c["sd"], c["images"], c["prompts"], c["text"], c["labels"])
    loss16, grad16, how = ref.yardstick(c["sd"], c["images"], c["prompts"], c["text"], c["labels"])
    loss, grad = vptfit.prompt_gradient(c["model"], c["prompts"], c["images"].cuda(), c["labels"], c["text"].cuda(), ref.LOGIT_SCALE)
    torch.cuda.synchronize()
    loss, grad = float(loss.cpu()), grad.cpu().double()
    yard, err = ref.rel_fro(grad16, grad64), ref.rel_fro(grad, grad64)
    lyard, lerr = abs(float(loss16 - loss64)), abs(loss - float(loss64))
    print(f"\nvitlfit-parity: VPT {TOKENS}+{n_ctx} rows depth={depth} B={B} C={C} grad device {err:.3e} yardstick({how}) {yard:.3e} ratio {err / yard:.2f}; "
          f"loss device {lerr:.3e} yardstick {lyard:.3e}")
    assert torch.isfinite(grad).all()
    assert err <= FACTOR * yard
    # The loss, as tests/test_gpu_maplefit.py holds it (one scalar's own fp16 draw is no bound: it is small or large by cancellation, and
    # is printed above): the device's logits -- its raw features through the float64 head -- within 2 x the fp16 reference's largest logit
    # error; cross-entropy moves by at most 2 max|dz| when a row of logits moves by dz, and the fp32 head is within 1e-5 of the float64
    # head on the features it is given (test_gpu_vptfit.py).
    feats = vptfit.image_features(c["model"], c["prompts"], c["images"].cuda())
    torch.cuda.synchronize()
    z64 = mref.logits_of(ref.forward(c["sd"], c["images"], c["prompts"])[0], c["text"])
    z16 = mref.logits_of(reference_features16(c, how), c["text"].half())
    zerr, zyard = float((mref.logits_of(feats.cpu(), c["text"]) - z64).abs().max()), float((z16 - z64).abs().max())
    print(f"vitlfit-parity: VPT logits: device max error {zerr:.3e} yardstick {zyard:.3e} ratio {zerr / zyard:.2f}; "
          f"loss bound {2 * FACTOR * zyard + 1e-5 * abs(float(loss64)):.3e}")
    assert zerr <= FACTOR * zyard
    assert lerr <= 2 * FACTOR * zyard + 1e-5 * abs(float(loss64))


def reference_features16(c, how):
    """The oracle's image features at the yardstick's precision (vptfit_ref.yardstick: float16, or fp32 on fp16-rounded weights and inputs)."""
    from oracle import clip_oracle as orc
    p = c["prompts"].half()
    with torch.no_grad():
        if how == "fp16":
            return orc.encode_image(c["sd"], c["images"].half(), torch.float16, p[0], [p[i] for i in range(1, p.shape[0])])
        sd16 = {k: (v.half().float() if v.is_floating_point() else v) for k, v in c["sd"].items()}
        p = p.float()
        return orc.encode_image(sd16, c["images"].half().float(), torch.float32, p[0], [p[i] for i in range(1, p.shape[0])])


def maple_case():
    if "maple" not in _CACHE:
        depth, n_ctx, C, B = 2, 2, 3, 2
        c = mref.make_case(TOY, depth, n_ctx, C, B)
        c["model"] = build_model(dict(c["sd"]), mref.design(n_ctx)).cuda()
        c["rows"] = mref.live_rows(c["ids"], True)
        c["depth"], c["n_ctx"] = depth, n_ctx
        _CACHE["maple"] = c
    return _CACHE["maple"]


def test_maple_gradients_within_the_fp16_yardstick():
    """maplefit.gradients at n_ctx 2 (259 rows per image), depth 2: every parameter tensor within 2 x the fp16 reference's own error."""
    long_on()
    c = maple_case()
    _, grad64 = mref.oracle_loss_grads(c["sd"], c["ids"], c["pl"], c["images"], c["labels"])
    _, grad16, how, _ = mref.yardstick(c["sd"], c["ids"], c["pl"], c["images"], c["labels"])
    loss, grads = maplefit.gradients(c["model"], c["pl"], c["images"].cuda(), c["labels"], c["ids"], mref.LOGIT_SCALE, seq_rows=c["rows"])
    torch.cuda.synchronize()
    fails = []
    for name in mref.param_names(c["depth"]):
        got, want = grads[name].cpu().double(), grad64[name]
        assert torch.isfinite(got).all() and float(want.norm()) > 0, name
        yard, err = mref.rel_fro(grad16[name], want), mref.rel_fro(got, want)
        print(f"\nvitlfit-parity: MaPLe {TOKENS}+{c['n_ctx']} rows {name}: device {err:.3e} yardstick({how}) {yard:.3e} ratio {err / yard:.2f}")
        if err > FACTOR * yard:
            fails.append((name, err, yard))
    assert not fails, fails


def test_ivlp_gradients_within_the_fp16_yardstick():
    """promptsrcfit.gradients with the IVLP weights at nt = 2, nv = 4 (261 rows per image), depths (2, 2): every parameter tensor within
    2 x the fp16 reference's own error."""
    long_on()
    dt, dv, nt, nv, C, B = 2, 2, 2, 4, 3, 2
    c = sref.e2e_case(TOY, dt, dv, nt, nv, C, B, sref.E2E_WEIGHTS["ivlp"], 0)
    m = build_model(dict(c["sd"]), sref.design(nt, dt, nv, dv)).cuda()
    rows = sref.live_rows(c["ids"], True)
    _, grads = promptsrcfit.gradients(m, c["p"], c["images"].cuda(), c["labels"], c["ids"], c["teacher"].cuda(), sref.LOGIT_SCALE, *c["weights"], seq_rows=rows)
    torch.cuda.synchronize()
    fails = []
    for name in sref.param_names(dt, dv):
        got, want = grads[name].cpu().double(), c["grad64"][name]
        assert torch.isfinite(got).all() and float(want.norm()) > 0, name
        yard, err = sref.rel_fro(c["grad16"][name], want), sref.rel_fro(got, want)
        print(f"\nvitlfit-parity: IVLP {TOKENS}+{nv} rows {name}: device {err:.3e} yardstick({c['how']}) {yard:.3e} ratio {err / yard:.2f}")
        if err > FACTOR * yard:
            fails.append((name, err, yard))
    assert not fails, fails


def vpt_steps(c, one_call, rates=(0.01, 0.02, 0.005)):
    st = vptfit.VPTFitState(c["model"], c["text"].cuda(), ref.LOGIT_SCALE, c["prompts"], momentum=0.9, weight_decay=5e-4)
    for r in rates:
        st.step(c["images"].cuda(), c["labels"], r, one_call=one_call)
    torch.cuda.synchronize()
    return st.prompts.cpu()


def test_vpt_one_call_equals_separate_calls_and_runs_repeat():
    long_on()
    c = vpt_case(TOY, 8, 2, 2, 5)
    base = vpt_steps(c, False)
    assert torch.isfinite(base).all() and not torch.equal(base, c["prompts"])
    for one_call in (True, False, True):
        assert torch.equal(vpt_steps(c, one_call).view(torch.int32), base.view(torch.int32)), one_call


def test_maple_one_call_equals_separate_calls_and_runs_repeat():
    long_on()
    c = maple_case()

    def steps(one_call):
        st = maplefit.MaPLeFitState(c["model"], c["ids"], c["pl"], mref.LOGIT_SCALE, seq_rows=c["rows"], momentum=0.9, weight_decay=5e-4, nesterov=True)
        for r in (0.01, 0.02, 0.005):
            st.step(c["images"].cuda(), c["labels"], r, one_call=one_call)
        torch.cuda.synchronize()
        return st.block.cpu()
    base = steps(False)
    assert torch.isfinite(base).all() and not torch.equal(base, mref.pack(c["pl"]))
    for one_call in (True, False, True):
        assert torch.equal(steps(one_call).view(torch.int32), base.view(torch.int32)), one_call


def test_step_is_torch_sgd_on_the_returned_gradient():
    """Two steps of VPTFitState at 265 rows against torch.optim.SGD on the GPU fed with vptfit.prompt_gradient's gradient at the same
    prompts: the same bits (tests/test_gpu_vptfit.py's check of the step, on the long path's own gradient)."""
    long_on()
    c = vpt_case(TOY, 8, 2, 2, 5)
    images, text = c["images"].cuda(), c["text"].cuda()
    lr, momentum, wd = 0.0025, 0.9, 5e-4
    p = torch.nn.Parameter(c["prompts"].clone().cuda())
    opt = torch.optim.SGD([p], lr=lr, momentum=momentum, weight_decay=wd)
    st = vptfit.VPTFitState(c["model"], text, ref.LOGIT_SCALE, c["prompts"], momentum=momentum, weight_decay=wd)
    for k in range(2):
        _, grad = vptfit.prompt_gradient(c["model"], p.detach().clone(), images, c["labels"], text, ref.LOGIT_SCALE)
        p.grad = grad.clone()
        opt.step()
        st.step(images, c["labels"], lr)
        torch.cuda.synchronize()
        assert torch.equal(st.prompts, p.detach()), k


def test_short_fit_lowers_the_loss():
    long_on()
    c = vpt_case(TOY, 8, 2, 4, 4, separable=True)
    st = vptfit.VPTFitState(c["model"], c["text"].cuda(), ref.LOGIT_SCALE, c["prompts"])
    losses = [st.step(c["images"].cuda(), c["labels"], 0.05, want_loss=True) for _ in range(4)]
    torch.cuda.synchronize()
    losses = torch.cat(losses).cpu().numpy()
    print(f"\nvitlfit: losses over 4 steps at 265 rows {np.array2string(losses, precision=4)}")
    assert losses.shape == (4,) and np.isfinite(losses).all() and losses[-1] < losses[0]
    assert torch.isfinite(st.prompts).all()


def test_short_geometries_keep_their_bits_and_sizes():
    """205 rows per image (vptfit_ref.CUSTOM with 8 prompt rows): the option changes neither the workspace nor a bit of three steps."""
    c = vpt_case("custom", 8, 2, 2, 5)
    off = vpt_steps(c, False)
    sizes_off = vptfit.stash_bytes(c["model"], 2, 8)
    long_on()
    assert vptfit.stash_bytes(c["model"], 2, 8) == sizes_off
    assert torch.equal(vpt_steps(c, False).view(torch.int32), off.view(torch.int32))
    assert torch.equal(vpt_steps(c, True).view(torch.int32), off.view(torch.int32))
