"""MaPLe's training path end to end on the GPU: the coupling functions, the joint head against the two existing heads, the step against
torch.optim.SGD, the ways through three steps, every parameter's gradient against float64 autograd through the oracle, the trainer's fit
and the refusals."""
import math

import numpy as np
import pytest
import torch

import maplefit_ref as ref
from clip_calibration_amd import _lib, maplefit, ops, synthetic as syn, vptfit
from clip_calibration_amd.model import build_model
from clip_calibration_amd.trainers import MaPLeCLIP

pytestmark = pytest.mark.gpu
FACTOR = 2.0      # the project's bound: within 2 x the oracle's own fp16-autograd error on the same case
_CACHE = {}


def case(geom, depth, n_ctx, C, B, cut):
    """The case, its model on the GPU, and the truth and the yardstick computed once."""
    key = (geom, depth, n_ctx, C, B, cut)
    if key not in _CACHE:
        c = ref.make_case(geom, depth, n_ctx, C, B)
        c["model"] = build_model(dict(c["sd"]), ref.design(n_ctx)).cuda()
        c["rows"] = ref.live_rows(c["ids"], cut)
        c["loss64"], c["grad64"], c["z64"] = ref.oracle_loss_grads(c["sd"], c["ids"], c["pl"], c["images"], c["labels"], return_logits=True)
        c["loss16"], c["grad16"], c["how"], c["z16"] = ref.yardstick(c["sd"], c["ids"], c["pl"], c["images"], c["labels"])
        _CACHE[key] = c
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------------- coupling
@pytest.mark.parametrize("depth,n_ctx", [(1, 2), (2, 1), (3, 3)])
def test_couple_forward_is_the_mirrors_prompt_learner(depth, n_ctx):
    """clipmi_maple_couple against MultiModalPromptLearner.forward on the GPU.  Slot 0: the mirror's half Linear returns fp16, the kernel
    the unrounded fp32 sum of the same fp16 products -- its rounding to fp16 is within one fp16 ulp of the mirror's (another summation
    order in front of one rounding).  Slots >= 1: fp32 Linears of inner length Dt; two fp32 summation orders differ by at most
    2 gamma_Dt |t|.|w| <= 2 Dt 2^-24 sum_k |t_k w_k| per element."""
    geom, Cn = "tiny3", 3
    g = syn.GEOMETRIES[geom]
    Dt, Dv = g.transformer_width, g.vision_width
    m = build_model(dict(syn.synthetic_state_dict(geom, seed=0)), ref.design(n_ctx)).cuda()
    mc = MaPLeCLIP(m, ref.cref.prompt_ids(geom, Cn, n_ctx), n_ctx=n_ctx, prompt_depth=depth, seed=3)
    with torch.no_grad():
        _, shared, deep_t, deep_v = mc.prompt_learner()
    block = maplefit.pack_block(mc.learner_params(), depth, "cuda")
    assert block.numel() == _lib.lib.clipmi_maple_block_floats(n_ctx, depth, Dt, Dv)
    vis = maplefit.couple(block, n_ctx, depth, Dt, Dv)
    torch.cuda.synchronize()
    assert shared.dtype == torch.float16
    ulp = torch.maximum(shared.float().abs(), torch.tensor(2.0 ** -14, device="cuda")) * 2.0 ** -10
    assert ((vis[0].half().float() - shared.float()).abs() <= ulp).all()
    pl = {k: v.detach().float() for k, v in mc.learner_params().items()}
    for i in range(depth - 1):
        t, w = pl[f"compound_prompts_text.{i}"], pl[f"compound_prompt_projections.{i}.weight"]
        bound = 2 * Dt * 2.0 ** -24 * (t.abs() @ w.abs().t()) + 2.0 ** -23 * deep_v[i].float().abs()
        assert ((vis[1 + i] - deep_v[i].float()).abs() <= bound).all(), i
    want = ref.couple_forward({k: v.cpu() for k, v in pl.items()})
    assert ref.rel_fro(vis.cpu(), want) <= Dt * 2.0 ** -24


@pytest.mark.parametrize("depth,n_ctx,C", [(1, 2, 3), (3, 3, 5)])
def test_couple_backward_against_float64(depth, n_ctx, C):
    """clipmi_maple_step's gradient with a random d_vis, d_embed and d_deep against the float64 restatement.  Every element is an fp32 sum
    of exact-operand products: of n_ctx terms (dW, db), of Dv + C terms (the text-side prompts: Dv coupling products and C class rows, or
    one d_deep row).  fp32 accumulation of n terms is within gamma_n = n 2^-24 / (1 - n 2^-24) of the sum of absolute values; relative to
    the tensor's norm that is at most sqrt(n) gamma_n for random signs -- the bound below takes the plain n 2^-23 per tensor."""
    g = syn.GEOMETRIES["tiny3"]
    Dt, Dv, L = g.transformer_width, g.vision_width, 16
    pl = ref.make_params("tiny3", n_ctx, depth, seed=7)
    gen = torch.Generator().manual_seed(8)
    d_vis = torch.randn(depth, n_ctx, Dv, generator=gen)
    d_embed = torch.randn(C * L, Dt, generator=gen)
    d_deep = torch.randn(max(depth - 1, 1), n_ctx, Dt, generator=gen)
    gs = 256.0
    block = ref.pack(pl).cuda()
    before = block.clone()
    grad = maplefit.maple_step(d_embed.cuda(), d_deep.cuda() if depth > 1 else None, d_vis.cuda(), block, C, L, n_ctx, depth, Dt, Dv, gs, apply=False)
    torch.cuda.synchronize()
    assert torch.equal(block, before)             # apply=False writes the gradient alone
    got = ref.unpack(grad.cpu(), n_ctx, depth, Dt, Dv)
    want = ref.couple_backward(pl, d_vis.double())
    want["ctx"] = want["ctx"] + d_embed.double().reshape(C, L, Dt)[:, 1:1 + n_ctx].sum(0)
    for i in range(1, depth):
        want[ref.text_name(i)] = want[ref.text_name(i)] + d_deep[i - 1].double()
    for name in ref.param_names(depth):
        n = n_ctx if name.startswith(("proj", "compound_prompt_projections")) else Dv + C
        err = ref.rel_fro(got[name] * gs, want[name])
        assert err <= n * 2.0 ** -23, (name, err)


# -------------------------------------------------------------------------------------------------------------------------- joint head
@pytest.mark.parametrize("B,C,E", [(1, 3, 64), (3, 5, 128), (9, 37, 128)])
def test_joint_head_equals_both_heads_bit_for_bit(B, C, E):
    g = torch.Generator().manual_seed(5)
    f, t = torch.randn(B, E, generator=g).cuda(), torch.randn(C, E, generator=g).cuda()
    y = torch.randint(0, C, (B,), generator=g).cuda()
    loss, d_feats, d_text, d16 = maplefit.maple_head(f, y, t, 100.0, 4096.0, want_f16=True)
    losses, want_text, _ = ops.prompt_head(f, y, t, 100.0, 4096.0, "coop", None, 8.0, 1.0, torch.zeros(3, device="cuda"))
    want_loss, want_feats = vptfit.vpt_head(f, y, t, 100.0, 4096.0)
    torch.cuda.synchronize()
    bits = lambda x: x.view(torch.int32)  # noqa: E731
    assert torch.equal(bits(d_text), bits(want_text)) and torch.equal(bits(d_feats), bits(want_feats))
    assert torch.equal(bits(loss), bits(want_loss)) and torch.equal(bits(loss), bits(losses[0:1]))
    assert torch.equal(d16, d_text.half())


# -------------------------------------------------------------------------------------------------------------------------------- step
@pytest.mark.parametrize("momentum,dampening,wd,nesterov", [(0.0, 0.0, 0.0, False), (0.9, 0.0, 5e-4, False), (0.9, 0.0, 5e-4, True), (0.5, 0.1, 1e-2, False)])
def test_step_equals_torch_sgd_on_the_gpu(momentum, dampening, wd, nesterov):
    """Given grad_out, the update is torch.optim.SGD's over the parameter list bit for bit, over three steps."""
    geom, depth, n_ctx, C, L = "tiny3", 3, 2, 5, 16
    g = syn.GEOMETRIES[geom]
    Dt, Dv = g.transformer_width, g.vision_width
    pl = ref.make_params(geom, n_ctx, depth, seed=11)
    gen = torch.Generator().manual_seed(12)
    mine = ref.pack(pl).cuda()
    params = [torch.nn.Parameter(pl[n].clone().cuda()) for n in ref.param_names(depth)]
    opt = torch.optim.SGD(params, lr=0.0035, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    buf = torch.zeros_like(mine) if momentum else None
    lr_d = torch.tensor([0.0035], dtype=torch.float32, device="cuda")
    for k in range(3):
        d_vis = (torch.randn(depth, n_ctx, Dv, generator=gen) * 300).cuda()
        d_embed = (torch.randn(C * L, Dt, generator=gen) * 300).cuda()
        d_deep = (torch.randn(depth - 1, n_ctx, Dt, generator=gen) * 300).cuda()
        grad = maplefit.maple_step(d_embed, d_deep, d_vis, mine, C, L, n_ctx, depth, Dt, Dv, 4096.0, buf, lr_d, k == 0, momentum, dampening, wd, nesterov)
        for p, gr in zip(params, maplefit.unpack_block(grad, n_ctx, depth, Dt, Dv).values()):
            p.grad = gr.clone()
        opt.step()
        torch.cuda.synchronize()
        for p, v in zip(params, maplefit.unpack_block(mine, n_ctx, depth, Dt, Dv).values()):
            assert torch.equal(v, p.detach()), k


def three_steps(c, way):
    m, images, labels = c["model"], c["images"].cuda(), c["labels"]
    rates = [0.01, 0.02, 0.005]
    sgd = dict(momentum=0.9, weight_decay=5e-4, nesterov=True)
    if way == "fit":
        out = maplefit.fit_prompt_learner([(images, labels)], None, m, c["ids"], c["pl"], logit_scale=ref.LOGIT_SCALE, epochs=3, lr_per_epoch=rates,
                                          seq_rows=c["rows"], **sgd)
        return maplefit.pack_block(out, ref.depth_of(c["pl"]), "cuda").cpu()
    st = maplefit.MaPLeFitState(m, c["ids"], c["pl"], ref.LOGIT_SCALE, seq_rows=c["rows"], **sgd)
    for r in rates:
        st.step(images, labels, r, one_call=(way == "one_call"))
    torch.cuda.synchronize()
    return st.block.cpu()


@pytest.mark.parametrize("key", [ref.CASES[0], ref.CASES[2], ref.CASES[4]])
def test_three_steps_every_way_identical_bits(key):
    """Separate calls, the one-call step and fit_prompt_learner (run twice) give the same bits over three steps with momentum, weight
    decay and Nesterov."""
    c = case(*key)
    base = three_steps(c, "step")
    assert torch.isfinite(base).all() and not torch.equal(base, ref.pack(c["pl"]))
    for way in ("one_call", "fit", "fit", "step"):
        assert torch.equal(three_steps(c, way).view(torch.int32), base.view(torch.int32)), way


# ---------------------------------------------------------------------------------------------------------------------- gradient parity
@pytest.mark.parametrize("key", ref.CASES)
def test_every_gradient_within_the_fp16_yardstick(key):
    """Every parameter tensor's gradient against float64 autograd through the oracle, within 2 x the fp16 reference's own error on the
    same inputs.  A tensor whose float64 gradient is identically zero would be compared in absolute terms and listed; these cases have
    none (tests/test_maplefit_cpu.py asserts every norm positive).

    The loss.  The device's own logits (its raw features through the float64 head) are held to the project's rule on the same inputs: their
    largest error is within 2 x the largest error of the reference's fp16 logits, a matrix of B C numbers, not one.  Cross-entropy moves
    by at most 2 max|dz| when a row of logits moves by dz (|d logsumexp| <= max|dz|, and so is the label's own logit), and the fp32
    head itself is within test_gpu_vptfit.py's 1e-5 of the float64 head on the features it is given; so the loss is held to
    2 x (2 x the reference's largest fp16 logit error) + 1e-5 |loss|.  One scalar's own fp16 draw (printed: the reference's loss error is
    2.7e-3 .. 2.5e-2 over these cases, by cancellation) is reported, not asserted."""
    geom, depth, n_ctx, C, B, cut = key
    c = case(*key)
    loss, grads = maplefit.gradients(c["model"], c["pl"], c["images"].cuda(), c["labels"], c["ids"], ref.LOGIT_SCALE, seq_rows=c["rows"])
    torch.cuda.synchronize()
    loss = float(loss.cpu())
    lyard, lerr = abs(float(c["loss16"] - c["loss64"])), abs(loss - float(c["loss64"]))
    print(f"\nmaplefit-parity: {geom} depth={depth} n_ctx={n_ctx} C={C} B={B} cut={cut} loss device {lerr:.3e} yardstick({c['how']}) {lyard:.3e}")
    zero, fails = [], []
    for name in ref.param_names(depth):
        got, want, yard16 = grads[name].cpu().double(), c["grad64"][name], c["grad16"][name]
        assert torch.isfinite(got).all(), name
        if float(want.norm()) == 0.0:
            zero.append(name)
            print(f"maplefit-parity:   {name}: float64 gradient identically zero; device max |g| {float(got.abs().max()):.3e}")
            assert float(got.abs().max()) == 0.0, name
            continue
        yard, err = ref.rel_fro(yard16, want), ref.rel_fro(got, want)
        print(f"maplefit-parity:   {name}: device {err:.3e} yardstick {yard:.3e} ratio {err / yard:.2f}")
        if err > FACTOR * yard:
            fails.append((name, err, yard))
    assert not fails, fails
    text, feats = maplefit.features(c["model"], c["pl"], c["images"].cuda(), c["ids"], seq_rows=c["rows"])
    torch.cuda.synchronize()
    zerr = float((ref.logits_of(feats.cpu(), text.cpu()) - c["z64"]).abs().max())
    zyard = float((c["z16"] - c["z64"]).abs().max())
    print(f"maplefit-parity:   logits: device max error {zerr:.3e} yardstick {zyard:.3e} ratio {zerr / zyard:.2f}; "
          f"loss bound {2 * FACTOR * zyard + 1e-5 * abs(float(c['loss64'])):.3e}, own fp16 draw {lyard:.3e}")
    assert zerr <= FACTOR * zyard
    assert lerr <= 2 * FACTOR * zyard + 1e-5 * abs(float(c["loss64"]))
    assert zero == []


# ------------------------------------------------------------------------------------------------------------------------------ trainer
def test_trainer_fit_lowers_the_loss_and_the_inference_forward_uses_it():
    geom, n_ctx, depth, C = "tiny", 2, 2, 3
    sd = syn.synthetic_state_dict(geom, seed=1)
    m = build_model(dict(sd), ref.design(n_ctx)).cuda()
    ids = ref.cref.prompt_ids(geom, C, n_ctx)
    mc = MaPLeCLIP(m, ids, n_ctx=n_ctx, prompt_depth=depth, seed=2)
    images = syn.synthetic_images(6, geom, seed=3).cuda()
    before, _, _ = mc(images)
    before = before.clone()
    labels = before.argmax(dim=1).cpu()          # the untrained model's own predictions: a loss that can go down from the first step
    loader = [(images[:3], labels[:3]), (images[3:], labels[3:])]
    key0 = mc._cache_key
    assert key0 is not None
    fitted, losses = mc.fit_prompt_learner(loader, epochs=2, lr_per_epoch=[0.005, 0.005], return_history=True)
    torch.cuda.synchronize()
    print(f"\nmaplefit: losses over 4 steps {np.array2string(losses, precision=4)}")
    assert losses.shape == (4,) and np.isfinite(losses).all()
    assert losses[2] < losses[0] and losses[3] < losses[1]          # each batch's loss is lower one epoch later
    assert mc._cache_key is None and mc._cache is None
    for name, p in mc.learner_params().items():
        assert torch.equal(p.detach(), fitted[name].to(p.dtype)), name
    assert mc.prompt_learner.proj.weight.dtype == torch.float16 and mc.prompt_learner.compound_prompts_text[0].dtype == torch.float32
    after, _, _ = mc(images)
    assert not torch.equal(after, before)


def test_fit_with_a_transform_equals_the_hand_written_loop():
    """``transform=TrainPreprocess.for_model(model)``: decoded uint8 batches go transform -> MaPLeFitState.step (augment.fit_with_transform
    with a state whose step takes images); the fitted block is that of a hand-written loop over the same views, bit for bit, and lands in
    the prompt learner's parameters."""
    import augment_ref as aref
    from clip_calibration_amd.augment import TrainPreprocess
    from clip_calibration_amd.preprocess import pack_images
    geom, n_ctx, depth, C = "tiny", 2, 2, 5
    m = build_model(dict(syn.synthetic_state_dict(geom, seed=0)), ref.design(n_ctx)).cuda()
    mc = MaPLeCLIP(m, ref.cref.prompt_ids(geom, C, n_ctx), n_ctx=n_ctx, prompt_depth=depth, seed=4)
    sizes = [(80, 100), (64, 64), (70, 51), (120, 90), (66, 97), (100, 100), (45, 80), (90, 64)]
    imgs = [aref.synthetic_image(h, w, 70 + i) for i, (h, w) in enumerate(sizes)]
    labels = torch.arange(8) % C
    loader = [(pack_images(imgs[i:i + 4]).pin_memory(), labels[i:i + 4]) for i in (0, 4)]
    start = maplefit.pack_block(mc.learner_params(), depth, "cuda").clone()
    rates = [0.004, 0.002]
    tp = TrainPreprocess.for_model(m, generator=torch.Generator().manual_seed(23))
    st = maplefit.MaPLeFitState(m, mc.prompt_learner.tokenized_prompts, mc.learner_params(), math.log(mc.scale))
    want_losses = []
    for e in range(2):
        for images, y in loader:
            want_losses.append(st.step(tp(images), y, rates[e], want_loss=True))
    torch.cuda.synchronize()
    tp2 = TrainPreprocess.for_model(m, generator=torch.Generator().manual_seed(23))
    fitted, losses = mc.fit_prompt_learner(loader, transform=tp2, epochs=2, lr_per_epoch=rates, return_history=True)
    block = maplefit.pack_block(fitted, depth, "cuda")
    assert torch.equal(block.view(torch.int32), st.block.view(torch.int32)) and np.array_equal(losses, torch.cat(want_losses).cpu().numpy())
    assert losses.shape == (4,) and np.isfinite(losses).all() and not torch.equal(block, start)
    for name, p in mc.learner_params().items():
        assert torch.equal(p.detach(), fitted[name].to(p.dtype)), name
    assert mc._cache_key is None


def test_one_call_refuses_bad_optimiser_arguments_before_it_launches():
    """clipmi_maple_train_step checks the optimiser's arguments before the towers are enqueued: the block and the stashes stay as they were."""
    c = case(*ref.CASES[0])
    st = maplefit.MaPLeFitState(c["model"], c["ids"], c["pl"], ref.LOGIT_SCALE, seq_rows=c["rows"])
    images = c["images"].cuda()
    st.step(images, c["labels"], 0.001, one_call=True)
    torch.cuda.synchronize()
    block, ts, vs = st.block.clone(), st.towers.text.stash.clone(), st.towers.vision.stash.clone()
    st.momentum = 1.5
    with pytest.raises(_lib.ClipmiError) as e:
        st.step(images, c["labels"], 0.001, one_call=True)
    torch.cuda.synchronize()
    assert e.value.code == _lib.ERR_ARG
    assert torch.equal(st.block, block) and torch.equal(st.towers.text.stash, ts) and torch.equal(st.towers.vision.stash, vs)


def test_refusals():
    geom, n_ctx = "tiny", 2
    sd = syn.synthetic_state_dict(geom, seed=0)
    ids = ref.cref.prompt_ids(geom, 3, n_ctx)
    images = torch.randn(2, 3, 64, 64).cuda()
    pl = ref.make_params(geom, n_ctx, 2)
    m = build_model(dict(sd), ref.design(n_ctx)).cuda()
    with pytest.raises(ValueError, match="trainer='MaPLe'"):
        maplefit.MaPLeFitState(build_model(dict(sd), {"trainer": "CoOp"}).cuda(), ids, pl)
    with pytest.raises(ValueError, match="depth=3 for 2 text and 2 image layers"):
        maplefit.MaPLeFitState(m, ids, ref.make_params(geom, n_ctx, 3))
    with pytest.raises(ValueError, match="class_token_position"):
        maplefit.gradients(m, pl, images, [0, 1], ids, class_token_position="middle")
    rn = build_model(dict(syn.synthetic_resnet_state_dict()), ref.design(n_ctx)).cuda()
    with pytest.raises(ValueError, match="ViT towers only"):
        maplefit.MaPLeFitState(rn, ids, pl)
    big = build_model(dict(syn.synthetic_state_dict(ref.vref.CUSTOM, seed=0)), ref.design(28)).cuda()
    pl_big = {"ctx": torch.zeros(28, 128), "proj.weight": torch.zeros(128, 128), "proj.bias": torch.zeros(128)}
    with pytest.raises(ValueError, match="at most 224"):
        maplefit.MaPLeFitState(big, syn.synthetic_token_ids(3, ref.vref.CUSTOM), pl_big)
    with pytest.raises(ValueError, match="power of two"):
        maplefit.gradients(m, pl, images, [0, 1], ids, grad_scale=3.0)
    with pytest.raises(ValueError, match="must be a floating-point tensor"):
        maplefit.gradients(m, dict(pl, **{"proj.bias": torch.zeros(5)}), images, [0, 1], ids)
    assert math.isfinite(maplefit.DEFAULT_GRAD_SCALE)
