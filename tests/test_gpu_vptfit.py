"""VPT's training path end to end on the GPU: the prompt gradient against float64 autograd through the oracle's image tower, the step
against torch.optim.SGD, the four ways through three steps, the trainer's fit and the refusals."""
import math

import numpy as np
import pytest
import torch

import vptfit_ref as ref
from clip_calibration_amd import _lib, synthetic as syn, vptfit
from clip_calibration_amd.model import build_model
from clip_calibration_amd.trainers import VPTCLIP

pytestmark = pytest.mark.gpu
FACTOR = 2.0      # the project's bound: within 2 x the oracle's own fp16-autograd error on the same case
_CACHE = {}


def design(n_ctx, depth):
    return {"trainer": "VPT", "vision_depth": depth, "vision_ctx": n_ctx, "language_depth": 0, "language_ctx": 0}


def case(geom, n_ctx, depth, B, C, separable=False):
    """The case, its model on the GPU, and the truth and the yardstick computed once."""
    key = (geom, n_ctx, depth, B, C, separable)
    if key not in _CACHE:
        c = ref.make_case(geom, n_ctx, depth, B, C, separable=separable)
        c["model"] = build_model(dict(c["sd"]), design(n_ctx, depth)).cuda()
        c["loss64"], c["grad64"] = ref.oracle_loss_grad(c["sd"], c["images"], c["prompts"], c["text"], c["labels"])
        c["loss16"], c["grad16"], c["how"] = ref.yardstick(c["sd"], c["images"], c["prompts"], c["text"], c["labels"])
        _CACHE[key] = c
    return _CACHE[key]


def device_grad(c, grad_scale=vptfit.DEFAULT_GRAD_SCALE):
    loss, grad = vptfit.prompt_gradient(c["model"], c["prompts"], c["images"].cuda(), c["labels"], c["text"].cuda(), ref.LOGIT_SCALE, grad_scale)
    torch.cuda.synchronize()
    return float(loss.cpu()), grad.cpu().double()


@pytest.mark.parametrize("geom,n_ctx,depth,B,C", ref.GPU_CASES)
def test_prompt_gradient_within_the_fp16_yardstick(geom, n_ctx, depth, B, C):
    c = case(geom, n_ctx, depth, B, C)
    loss, grad = device_grad(c)
    yard = ref.rel_fro(c["grad16"], c["grad64"])
    err = ref.rel_fro(grad, c["grad64"])
    lyard, lerr = abs(float(c["loss16"] - c["loss64"])), abs(loss - float(c["loss64"]))
    print(f"\nvptfit-parity: {geom} n_ctx={n_ctx} depth={depth} B={B} C={C} grad device {err:.3e} yardstick({c['how']}) {yard:.3e} ratio {err / yard:.2f}; "
          f"loss device {lerr:.3e} yardstick {lyard:.3e}")
    assert torch.isfinite(grad).all()
    assert err <= FACTOR * yard
    assert lerr <= FACTOR * lyard + 2.0 ** -22 * abs(float(c["loss64"]))      # + two fp32 ulps of the loss the device returns in fp32


@pytest.mark.parametrize("geom,n_ctx,depth,B,C", [ref.GPU_CASES[1], ref.GPU_CASES[4]])
def test_grad_scale_is_exact_scaling(geom, n_ctx, depth, B, C):
    c = case(geom, n_ctx, depth, B, C)
    yard = ref.rel_fro(c["grad16"], c["grad64"])
    _, g1 = device_grad(c, 1.0)
    _, g8 = device_grad(c, 256.0)
    d = ref.rel_fro(g1, g8)
    print(f"\nvptfit-parity: grad_scale 1 vs 2^8 {geom}: {d:.3e} (yardstick {yard:.3e})")
    assert d <= FACTOR * yard


def sgd_args():
    return dict(momentum=0.9, weight_decay=5e-4)


def three_steps(c, way):
    m, text = c["model"], c["text"].cuda()
    images, labels = c["images"].cuda(), c["labels"]
    rates = [0.01, 0.02, 0.005]
    if way == "fit":
        out = vptfit.fit_prompts([(images, labels)], None, m, text, c["prompts"], ref.LOGIT_SCALE, epochs=3, lr_per_epoch=rates, **sgd_args())
        return out.cpu()
    st = vptfit.VPTFitState(m, text, ref.LOGIT_SCALE, c["prompts"], **sgd_args())
    for r in rates:
        st.step(images, labels, r, one_call=(way == "one_call"))
    torch.cuda.synchronize()
    return st.prompts.cpu()


@pytest.mark.parametrize("geom,n_ctx,depth,B,C", [ref.GPU_CASES[1], ref.GPU_CASES[4], ref.GPU_CASES[5]])
def test_three_steps_four_ways_identical_bits(geom, n_ctx, depth, B, C):
    c = case(geom, n_ctx, depth, B, C)
    base = three_steps(c, "step")
    assert torch.isfinite(base).all() and not torch.equal(base, c["prompts"])
    for way in ("fit", "one_call", "step"):
        assert torch.equal(three_steps(c, way), base), way


@pytest.mark.parametrize("momentum,dampening,wd,nesterov", [(0.0, 0.0, 0.0, False), (0.9, 0.0, 5e-4, False), (0.9, 0.0, 5e-4, True), (0.5, 0.1, 1e-2, False)])
def test_step_equals_torch_sgd_on_the_gpu(momentum, dampening, wd, nesterov):
    """The device's own gradient fed to torch.optim.SGD on the GPU gives clipmi_vpt_step's bits, over three steps."""
    g = torch.Generator().manual_seed(11)
    w0 = torch.randn(2, 8, 128, generator=g) * 0.02
    grads = [torch.randn(2, 8, 128, generator=g) * 3.0 for _ in range(3)]
    gs, lr = 4096.0, 0.0025
    p = torch.nn.Parameter(w0.clone().cuda())
    opt = torch.optim.SGD([p], lr=lr, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    mine, buf = w0.clone().cuda(), (torch.zeros(2, 8, 128, device="cuda") if momentum else None)
    lr_d = torch.tensor([lr], dtype=torch.float32, device="cuda")
    for k, d in enumerate(grads):
        d = d.cuda()
        grad = vptfit.vpt_step(d, gs, mine, buf, lr_d, k == 0, momentum, dampening, wd, nesterov)
        p.grad = grad.clone()
        opt.step()
        assert torch.equal(mine, p.detach()), k


def test_head_matches_float64_and_bad_labels_are_nan():
    g = torch.Generator().manual_seed(5)
    f, t = torch.randn(9, 128, generator=g), torch.randn(37, 128, generator=g)
    y = torch.randint(0, 37, (9,), generator=g)
    loss, d = vptfit.vpt_head(f.cuda(), y.cuda(), t.cuda(), 100.0, 1.0)
    want_loss, want_d, _ = ref.head_image(f.double(), y, t.double(), 100.0)
    assert abs(float(loss.cpu()) - float(want_loss)) <= 1e-5 * float(want_loss) and ref.rel_fro(d.cpu(), want_d) <= 1e-5
    y[3] = 37
    loss, d = vptfit.vpt_head(f.cuda(), y.cuda(), t.cuda(), 100.0, 1.0)
    d = d.cpu()
    assert math.isnan(float(loss.cpu())) and torch.isnan(d[3]).all() and torch.isfinite(d[[0, 1, 2, 4, 5, 6, 7, 8]]).all()


def test_training_forward_equals_inference_forward():
    """The training forward is the inference forward in fp32-stream mode up to QuickGELU's rounding point."""
    c = case(*ref.GPU_CASES[1])
    m = c["model"]
    shallow, deep = m.ivlp_vision_prompts()
    with torch.no_grad():
        for p, v in zip([shallow] + list(deep), c["prompts"]):
            p.copy_(v)
    want = m.image_features_f32(c["images"].cuda(), flags=_lib.CALL_STREAM_F32).cpu()
    got = vptfit.image_features(m, c["prompts"], c["images"].cuda()).cpu()
    assert ref.rel_fro(got, want) <= 2e-3
    truth, _ = ref.forward(c["sd"], c["images"], c["prompts"])
    assert ref.rel_fro(got, truth) <= 2 * max(ref.rel_fro(want, truth), 1e-4)


def test_fit_prompts_updates_the_model_and_lowers_the_loss():
    geom, n_ctx, depth, B, C = "tiny", 8, 2, 8, 4
    c = ref.make_case(geom, n_ctx, depth, B, C, seed=1, separable=True)
    m = build_model(dict(c["sd"]), design(n_ctx, depth)).cuda()
    ids = syn.synthetic_token_ids(C, geom, seed=0)
    tr = VPTCLIP(m, ids)
    tr.text_features = torch.nn.functional.normalize(c["text"], dim=-1).cuda()
    images = c["images"].cuda()
    before = m.encode_image(images).float().cpu()
    fitted, losses = tr.fit_prompts([(images, c["labels"])], epochs=8, lr=0.05, lr_per_epoch=[0.05] * 8, return_history=True)
    torch.cuda.synchronize()
    print(f"\nvptfit: losses over 8 steps {np.array2string(losses, precision=4)}")
    assert losses.shape == (8,) and np.isfinite(losses).all() and losses[-1] < losses[0]
    shallow, deep = m.ivlp_vision_prompts()
    assert torch.equal(shallow.detach().cpu().float(), fitted[0].cpu().to(shallow.dtype).float())
    assert torch.equal(deep[0].detach().cpu().float(), fitted[1].cpu().to(shallow.dtype).float())
    after = m.encode_image(images).float().cpu()
    assert not torch.equal(after, before)
    want = vptfit.image_features(m, fitted, images).cpu()
    assert ref.rel_fro(after, want) <= 5e-3       # the inference forward uses the fitted prompts


def test_refusals():
    sd = syn.synthetic_state_dict("tiny", seed=0)
    text = torch.randn(3, 128).cuda()
    m = build_model(dict(sd), design(4, 2)).cuda()
    images = torch.randn(2, 3, 64, 64).cuda()
    with pytest.raises(ValueError, match="trainer='VPT'"):
        vptfit.VPTFitState(build_model(dict(sd), {"trainer": "CoOp"}).cuda(), text)
    with pytest.raises(ValueError, match="n_ctx"):
        vptfit.prompt_gradient(m, torch.zeros(2, 5, 128), images, [0, 1], text)
    with pytest.raises(_lib.ClipmiError) as e:
        vptfit.prompt_gradient(m, torch.zeros(2, 4, 128), images, [0, 1], text, flags=_lib.CALL_STREAM_F16)
    assert e.value.code == _lib.ERR_STATE
    rn = build_model(dict(syn.synthetic_resnet_state_dict()), {"trainer": "VPT", "vision_depth": 1, "vision_ctx": 4}).cuda()
    with pytest.raises(ValueError, match="ViT towers only"):
        vptfit.VPTFitState(rn, text)
    big = build_model(dict(syn.synthetic_state_dict(ref.CUSTOM, seed=0)), design(28, 1)).cuda()
    with pytest.raises(ValueError, match="at most 224"):
        vptfit.VPTFitState(big, text)
    import ctypes
    big._ensure_bound()
    ws, st = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert _lib.lib.clipmi_vision_train_bytes(big._handle, 2, 28, ctypes.byref(ws), ctypes.byref(st)) == _lib.ERR_SHAPE and ws.value == 0 and st.value == 0


def test_fit_prompts_with_a_transform_equals_the_hand_written_loop():
    """``transform=TrainPreprocess.for_model(model)``: decoded uint8 batches go transform -> VPTFitState.step (augment.fit_with_transform
    with a state whose step takes images); the fitted prompts are those of a hand-written loop over the same views, bit for bit, and land
    in the model's parameters."""
    import augment_ref as aref
    from clip_calibration_amd.augment import TrainPreprocess
    from clip_calibration_amd.preprocess import pack_images
    n_ctx, depth, C = 4, 2, 5
    m = build_model(dict(syn.synthetic_state_dict("tiny", seed=0)), design(n_ctx, depth)).cuda()
    sizes = [(80, 100), (64, 64), (70, 51), (120, 90), (66, 97), (100, 100), (45, 80), (90, 64)]
    imgs = [aref.synthetic_image(h, w, 70 + i) for i, (h, w) in enumerate(sizes)]
    labels = torch.arange(8) % C
    loader = [(pack_images(imgs[i:i + 4]).pin_memory(), labels[i:i + 4]) for i in (0, 4)]
    tr = VPTCLIP(m, syn.synthetic_token_ids(C, "tiny", seed=0))
    start = vptfit.model_prompts(m).clone()
    rates = [0.02, 0.01]
    tp = TrainPreprocess.for_model(m, generator=torch.Generator().manual_seed(23))
    st = vptfit.VPTFitState(m, tr.text_features.float(), math.log(tr.scale))
    want_losses = []
    for e in range(2):
        for images, y in loader:
            want_losses.append(st.step(tp(images), y, rates[e], want_loss=True))
    torch.cuda.synchronize()
    tp2 = TrainPreprocess.for_model(m, generator=torch.Generator().manual_seed(23))
    fitted, losses = tr.fit_prompts(loader, transform=tp2, epochs=2, lr_per_epoch=rates, return_history=True)
    assert torch.equal(fitted, st.prompts) and np.array_equal(losses, torch.cat(want_losses).cpu().numpy())
    assert losses.shape == (4,) and np.isfinite(losses).all() and not torch.equal(fitted.cpu(), start.cpu())
    shallow, deep = m.ivlp_vision_prompts()
    assert torch.equal(shallow.detach(), fitted[0].to(shallow.dtype)) and torch.equal(deep[0].detach(), fitted[1].to(shallow.dtype))
