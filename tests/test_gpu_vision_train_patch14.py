"""The image tower's training path on towers with patches of 14 pixels (ViT-L/14's), which the im2col-free loader does not serve: the
training forward takes the inference pass's route -- patchify into the [B G^2, kpad] fp16 matrix (kpad 640 against K = 588), the dense GEMM
whose epilogue adds the positional rows, ln_pre without a second positional add.  VPT, MaPLe and IVLP end to end against float64 autograd
through the oracle, the steps and the monitored fit bit for bit, the front end's address map read back from the stash, and the geometries
the loader serves held to their bits and sizes.

The toy towers have width 128 (two heads), two layers and embed 128:
  toy14      42 px,  3 x 3 patches,   10 tokens: the short backward; a grid that is no power of two; 9 B ragged GEMM rows; kpad padding
  toy14_257  224 px, 16 x 16 patches, 257 tokens: ViT-L/14's own resolution and patch, through the long backward (option on)
  toy14_577  336 px, 24 x 24 patches, 577 tokens: ViT-L/14@336px's, one image
Bounds are the project's: a gradient within FACTOR = 2 x the fp16 reference's own error against float64 autograd on the same case, logits
within 2 x the fp16 reference's largest logit error, the loss as tests/test_gpu_vision_train_long.py holds it."""
import ctypes
import math

import numpy as np
import pytest
import torch

import front_ref as fref
import maplefit_ref as mref
import promptsrcfit_ref as sref
import vptfit_ref as ref
from test_gpu_vision_train import Stash
from clip_calibration_amd import _lib, maplefit, ops, promptsrcfit, synthetic as syn, vptfit
from clip_calibration_amd.model import build_model

pytestmark = pytest.mark.gpu
FACTOR = 2.0      # the project's bound: within 2 x the oracle's own fp16-autograd error on the same case


def toy(R, width=128):
    return syn.ClipGeometry(128, R, 2, width, 14, 77, 256, 128, 2, 2)


TOYS = {"toy14": toy(42), "toy14_257": toy(224), "toy14_577": toy(336)}
_CACHE = {}


@pytest.fixture(autouse=True)
def toy_geometries_and_option():
    """The reference modules look geometries up by name: the toy ones are registered for the test and taken out again; the option is put
    back to what it was."""
    before = _lib.get_option("vision_train_long")
    syn.GEOMETRIES.update(TOYS)
    try:
        yield
    finally:
        for name in TOYS:
            syn.GEOMETRIES.pop(name, None)
        _lib.set_option("vision_train_long", before)


def long_on():
    _lib.set_option("vision_train_long", 1)


def a256(n):
    return (n + 255) // 256 * 256


def vpt_design(depth, n_ctx):
    return {"trainer": "VPT", "vision_depth": depth, "vision_ctx": n_ctx, "language_depth": 0, "language_ctx": 0}


def vpt_case(geom, n_ctx, depth, B, C):
    key = ("vpt", geom, n_ctx, depth, B, C)
    if key not in _CACHE:
        c = ref.make_case(geom, n_ctx, depth, B, C)
        c["model"] = build_model(dict(c["sd"]), vpt_design(depth, n_ctx)).cuda()
        c["truth"] = ref.oracle_loss_grad(c["sd"], c["images"], c["prompts"], c["text"], c["labels"])
        c["yard"] = ref.yardstick(c["sd"], c["images"], c["prompts"], c["text"], c["labels"])
        _CACHE[key] = c
    return _CACHE[key]


def test_geometries():
    assert [g.vision_tokens for g in TOYS.values()] == [10, 257, 577] and [g.grid for g in TOYS.values()] == [3, 16, 24]
    assert fref.default_kpad(14) == 640 > 3 * 14 * 14


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


def hold_vpt_gradient(c, images, what):
    """(loss, grad) of vptfit.prompt_gradient on ``images`` held to the gradient bound; the device tensors are returned."""
    loss64, grad64 = c["truth"]
    loss16, grad16, how = c["yard"]
    loss_d, grad_d = vptfit.prompt_gradient(c["model"], c["prompts"], images.cuda(), c["labels"], c["text"].cuda(), ref.LOGIT_SCALE)
    torch.cuda.synchronize()
    grad = grad_d.cpu().double()
    yard, err = ref.rel_fro(grad16, grad64), ref.rel_fro(grad, grad64)
    print(f"\nvitl14-parity: VPT {what} grad norm {float(grad64.norm()):.3g} device {err:.3e} yardstick({how}) {yard:.3e} ratio {err / yard:.2f}")
    assert float(grad64.norm()) > 0 and torch.isfinite(grad).all()
    assert err <= FACTOR * yard
    return loss_d, grad_d


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_vpt_on_toy14_gradient_logits_and_loss(dtype):
    """10 + 4 rows per image, depth 2, B 3, C 5, from an fp32 and from an fp16 image batch."""
    n_ctx, depth, B, C = 4, 2, 3, 5
    c = vpt_case("toy14", n_ctx, depth, B, C)
    images = c["images"].to(dtype)
    loss64, _ = c["truth"]
    loss16, _, how = c["yard"]
    loss, _ = hold_vpt_gradient(c, images, f"toy14 10+{n_ctx} rows {str(dtype)[6:]} images")
    loss = float(loss.cpu())
    # the loss, as tests/test_gpu_vision_train_long.py holds it: the device's logits within 2 x the fp16 reference's largest logit error;
    # cross-entropy moves by at most 2 max|dz|, and the fp32 head is within 1e-5 of the float64 head on the features it is given
    feats = vptfit.image_features(c["model"], c["prompts"], images.cuda())
    torch.cuda.synchronize()
    z64 = mref.logits_of(ref.forward(c["sd"], c["images"], c["prompts"])[0], c["text"])
    z16 = mref.logits_of(reference_features16(c, how), c["text"].half())
    zerr, zyard = float((mref.logits_of(feats.cpu(), c["text"]) - z64).abs().max()), float((z16 - z64).abs().max())
    lerr, lyard = abs(loss - float(loss64)), abs(float(loss16 - loss64))
    print(f"vitl14-parity: VPT toy14 {str(dtype)[6:]} images logits: device max error {zerr:.3e} yardstick {zyard:.3e} ratio {zerr / zyard:.2f}; "
          f"loss device {lerr:.3e} yardstick {lyard:.3e} bound {2 * FACTOR * zyard + 1e-5 * abs(float(loss64)):.3e}")
    assert zerr <= FACTOR * zyard
    assert lerr <= 2 * FACTOR * zyard + 1e-5 * abs(float(loss64))


def test_fp16_images_give_the_bits_of_fp32_images_rounded_through_fp16():
    """patchify rounds the pixel to fp16 first on both paths: an fp16 batch and the fp32 batch ``images.half().float()`` give the same loss,
    gradient and features bit for bit, and so does the unrounded fp32 batch, whose pixels the device rounds itself (the case's pixels are
    not fp16 numbers: the rounding is not vacuous)."""
    c = vpt_case("toy14", 4, 2, 3, 5)
    run = lambda im: vptfit.prompt_gradient(c["model"], c["prompts"], im.cuda(), c["labels"], c["text"].cuda(), ref.LOGIT_SCALE)
    l16, g16 = run(c["images"].half())
    l32, g32 = run(c["images"].half().float())
    f16 = vptfit.image_features(c["model"], c["prompts"], c["images"].half().cuda())
    f32 = vptfit.image_features(c["model"], c["prompts"], c["images"].half().float().cuda())
    lraw, graw = run(c["images"])
    torch.cuda.synchronize()
    assert torch.equal(g16.view(torch.int32), g32.view(torch.int32)) and torch.equal(l16.view(torch.int32), l32.view(torch.int32))
    assert torch.equal(f16.view(torch.int32), f32.view(torch.int32))
    assert not torch.equal(c["images"].half().float(), c["images"])
    assert torch.equal(graw.view(torch.int32), g32.view(torch.int32)) and torch.equal(lraw.view(torch.int32), l32.view(torch.int32))


def test_vpt_on_toy14_257_needs_the_option_by_length_and_holds_the_bound():
    """257 + 8 = 265 rows, depth 2, B 2, C 5: refused by length with the option off, within the bound with it on."""
    n_ctx, depth, B, C = 8, 2, 2, 5
    c = vpt_case("toy14_257", n_ctx, depth, B, C)
    m = c["model"]
    m._ensure_bound()
    ws, st = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert _lib.get_option("vision_train_long") == 0
    with pytest.raises(ValueError, match="at most 224"):
        vptfit.prompt_gradient(m, c["prompts"], c["images"].cuda(), c["labels"], c["text"].cuda(), ref.LOGIT_SCALE)
    assert _lib.lib.clipmi_vision_train_bytes(m._handle, B, n_ctx, ctypes.byref(ws), ctypes.byref(st)) == _lib.ERR_SHAPE
    assert "at most 224" in _lib.last_error() and "patch" not in _lib.last_error()
    long_on()
    hold_vpt_gradient(c, c["images"], f"toy14_257 257+{n_ctx} rows")
    # the documented layout with the im2col matrix in the front end's slot and the long kernel's statistics at the end
    L, D, E, H, layers = 257 + n_ctx, 128, 128, 2, 2
    M = B * L
    want = (2 * a256(M * D * 2) + a256(M * D * 8) + a256(M * D * 6) + a256(M * D * 4) + a256(B * D * 2) + a256(B * E * 2) + a256(B * D * 4)
            + a256(M * D * 4) + a256(B * 256 * 640 * 2) + a256(layers * n_ctx * D * 2) + a256(n_ctx * D * 4) + a256(12 * B * H * L))
    assert vptfit.stash_bytes(m, B, n_ctx)[0] == want


def test_vpt_on_toy14_577_one_image():
    """ViT-L/14@336px's 577 tokens + 4 prompt rows = 581 rows, depth 2, B 1, C 3."""
    long_on()
    n_ctx = 4
    c = vpt_case("toy14_577", n_ctx, 2, 1, 3)
    hold_vpt_gradient(c, c["images"], f"toy14_577 577+{n_ctx} rows")


def maple_case(geom):
    key = ("maple", geom)
    if key not in _CACHE:
        depth, n_ctx, C, B = 2, 2, 3, 2
        c = mref.make_case(geom, depth, n_ctx, C, B)
        c["model"] = build_model(dict(c["sd"]), mref.design(n_ctx)).cuda()
        c["rows"] = mref.live_rows(c["ids"], True)
        c["depth"], c["n_ctx"] = depth, n_ctx
        _CACHE[key] = c
    return _CACHE[key]


def test_maple_on_toy14_257_every_tensor_within_the_fp16_yardstick():
    """maplefit.gradients at n_ctx 2 (259 rows per image), depth 2, C 3, B 2."""
    long_on()
    c = maple_case("toy14_257")
    _, grad64 = mref.oracle_loss_grads(c["sd"], c["ids"], c["pl"], c["images"], c["labels"])
    _, grad16, how, _ = mref.yardstick(c["sd"], c["ids"], c["pl"], c["images"], c["labels"])
    _, grads = maplefit.gradients(c["model"], c["pl"], c["images"].cuda(), c["labels"], c["ids"], mref.LOGIT_SCALE, seq_rows=c["rows"])
    torch.cuda.synchronize()
    fails = []
    for name in mref.param_names(c["depth"]):
        got, want = grads[name].cpu().double(), grad64[name]
        assert torch.isfinite(got).all() and float(want.norm()) > 0, name
        yard, err = mref.rel_fro(grad16[name], want), mref.rel_fro(got, want)
        print(f"\nvitl14-parity: MaPLe toy14_257 257+{c['n_ctx']} rows {name}: device {err:.3e} yardstick({how}) {yard:.3e} ratio {err / yard:.2f}")
        if err > FACTOR * yard:
            fails.append((name, err, yard))
    assert not fails, fails


def test_ivlp_on_toy14_257_every_tensor_within_the_fp16_yardstick():
    """promptsrcfit.gradients with the IVLP weights at nt 2, nv 4 (261 rows per image), depths (2, 2); the teacher's features come from the
    frozen plain tower on the same patch-14 handle."""
    long_on()
    dt, dv, nt, nv, C, B = 2, 2, 2, 4, 3, 2
    c = sref.e2e_case("toy14_257", dt, dv, nt, nv, C, B, sref.E2E_WEIGHTS["ivlp"], 0)
    m = build_model(dict(c["sd"]), sref.design(nt, dt, nv, dv)).cuda()
    rows = sref.live_rows(c["ids"], True)
    _, grads = promptsrcfit.gradients(m, c["p"], c["images"].cuda(), c["labels"], c["ids"], c["teacher"].cuda(), sref.LOGIT_SCALE, *c["weights"], seq_rows=rows)
    torch.cuda.synchronize()
    fails = []
    for name in sref.param_names(dt, dv):
        got, want = grads[name].cpu().double(), c["grad64"][name]
        assert torch.isfinite(got).all() and float(want.norm()) > 0, name
        yard, err = sref.rel_fro(c["grad16"][name], want), sref.rel_fro(got, want)
        print(f"\nvitl14-parity: IVLP toy14_257 257+{nv} rows {name}: device {err:.3e} yardstick({c['how']}) {yard:.3e} ratio {err / yard:.2f}")
        if err > FACTOR * yard:
            fails.append((name, err, yard))
    assert not fails, fails


def vpt_steps(c, one_call, rates=(0.01, 0.02, 0.005)):
    st = vptfit.VPTFitState(c["model"], c["text"].cuda(), ref.LOGIT_SCALE, c["prompts"], momentum=0.9, weight_decay=5e-4)
    for r in rates:
        st.step(c["images"].cuda(), c["labels"], r, one_call=one_call)
    torch.cuda.synchronize()
    return st.prompts.cpu()


def test_vpt_steps_on_toy14_one_call_equals_separate_calls_and_runs_repeat():
    c = vpt_case("toy14", 4, 2, 3, 5)
    base = vpt_steps(c, False)
    assert torch.isfinite(base).all() and not torch.equal(base, c["prompts"])
    for one_call in (True, False, True):
        assert torch.equal(vpt_steps(c, one_call).view(torch.int32), base.view(torch.int32)), one_call


def test_maple_steps_on_toy14_one_call_equals_separate_calls_and_runs_repeat():
    c = maple_case("toy14")

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


def test_vpt_step_on_toy14_is_torch_sgd_on_the_returned_gradient():
    c = vpt_case("toy14", 4, 2, 3, 5)
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


def test_monitored_vpt_fit_on_toy14():
    """vptfit.fit_prompts with ``val`` over two epochs and a val_batch_size that does not divide the validation set (clipmi_vision_val_chunk
    on the patchify route): the prompts of the fit without ``val`` bit for bit, and every epoch's record is, byte for byte, clipmi_val_score's
    on the logits of the validation images recomputed chunk by chunk at that epoch's prompts, as tests/test_gpu_blockmonitor.py holds the
    image-tower fits."""
    n_ctx, depth, B, C, N, bs, E = 4, 2, 3, 5, 7, 3, 2
    c = vpt_case("toy14", n_ctx, depth, B, C)
    m, text = c["model"], c["text"].cuda()
    images = c["images"].cuda()
    gen = torch.Generator().manual_seed(47)
    vi, vl = torch.randn(N, 3, 42, 42, generator=gen).cuda(), torch.randint(0, C, (N,), generator=gen)
    loader = [(images[:2], c["labels"][:2]), (images[2:], c["labels"][2:])]
    rates = [0.02, 0.03]
    sgd = dict(momentum=0.9, weight_decay=5e-4)

    def fit(epochs, **kw):
        out = vptfit.fit_prompts(loader, None, m, text, c["prompts"], ref.LOGIT_SCALE, epochs=epochs, lr_per_epoch=rates[:epochs], **sgd, **kw)
        torch.cuda.synchronize()
        return out
    plain = fit(E)
    assert torch.isfinite(plain).all() and not torch.equal(plain.cpu(), c["prompts"])
    watched, mon = fit(E, val=(vi, vl), val_batch_size=bs, return_monitor=True)
    assert torch.equal(watched.view(torch.int32), plain.view(torch.int32)), "the fit with val differs from the fit without"
    assert len(mon["records"]) == E and all(r["n"] == N for r in mon["records"])
    got = ops.encode_val_records(mon["records"], 10)
    scale = float(np.float32(math.exp(ref.LOGIT_SCALE)))
    tn = ops.l2_normalize(text)
    for e in range(E):
        block = plain if e == E - 1 else fit(e + 1)
        z = []
        for lo in range(0, N, bs):
            fn = ops.l2_normalize(vptfit.image_features(m, block, vi[lo:lo + bs]))
            zc = torch.empty(fn.shape[0], C, dtype=torch.float32, device="cuda")
            _lib.check(_lib.lib.clipmi_logits(fn.data_ptr(), tn.data_ptr(), scale, None, zc.data_ptr(), None, None, fn.shape[0], C, fn.shape[1],
                                              torch.cuda.current_stream().cuda_stream), "clipmi_logits")
            z.append(zc)
        want = ops.val_score(torch.cat(z), vl.cuda(), 10).cpu().numpy()
        assert np.array_equal(want, got[e]), f"record {e} is not val_score's on the recomputed logits"


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_front_end_address_map_through_the_training_entry_point(dtype):
    """R = 42, P = 14, B = 3 at width 640 = kpad: conv1 is the identity on the 588 patch columns (and zero on the 52 rows behind them), the
    positional rows are small integers, ln_pre has gamma 1 and beta 0, and the pixels are front_ref.coded_image's integer codes.  The front
    end is then exact: x0[b, 1 + p, k] = front_ref.patchify(image)[b G^2 + p, k] + pos[1 + p, k], pad columns included.  Slot 0 of the stash
    (the stash's first fp32 slab: ln_pre's output, DESIGN.md "VPT fit") is held to front_ref.layer_norm_rows of those rows within its fp32
    bound, and, ln_pre undone with the reference's own row statistics, rounds to those integers exactly.  The workspace is filled with the
    fp16 NaN pattern first: a pad column that patchify left unwritten would poison its row.  A transposed (ky, kx) or a wrong image stride
    moves codes by whole integers, hundreds of tolerances."""
    B, R, P, n_ctx, depth = 3, 42, 14, 4, 1
    G, K, kpad = R // P, 3 * P * P, fref.default_kpad(P)
    g = toy(R, width=kpad)
    D, L0 = g.vision_width, G * G + 1
    L = L0 + n_ctx
    sd = dict(syn.synthetic_state_dict(g, seed=0))
    w = torch.zeros(D, K)
    w[torch.arange(K), torch.arange(K)] = 1.0
    sd["visual.conv1.weight"] = w.reshape(D, 3, P, P).to(sd["visual.conv1.weight"].dtype)
    l, d = torch.meshgrid(torch.arange(L0), torch.arange(D), indexing="ij")
    pos = ((3 * l + 5 * d) % 7 - 3).float()
    sd["visual.positional_embedding"] = pos.to(sd["visual.positional_embedding"].dtype)
    sd["visual.ln_pre.weight"] = torch.ones_like(sd["visual.ln_pre.weight"])
    sd["visual.ln_pre.bias"] = torch.zeros_like(sd["visual.ln_pre.bias"])
    m = build_model(sd, vpt_design(depth, n_ctx)).cuda()
    image = fref.coded_image(B, R, P, dtype)
    prompts = 0.02 * torch.randn(depth, n_ctx, D, generator=torch.Generator().manual_seed(3))
    t = vptfit._Tower("test", m, depth, n_ctx)
    t.size(B)
    t.ws.fill_(0xFF)
    t.forward(image.cuda(), prompts.cuda().contiguous())
    torch.cuda.synchronize()
    x0 = Stash(t.stash, B, L, D, g.vision_layers, n_ctx).x(0).reshape(B, L, D)
    col = fref.patchify(image, P, kpad)
    assert (col[:, K:] == 0).all() and col.shape == (B * G * G, kpad)
    rows = col.double() + pos.double()[1:].repeat(B, 1)
    one, zero = torch.ones(D), torch.zeros(D)
    val, bound = fref.layer_norm_rows(rows.float(), one, zero, 1e-5)
    got = x0[:, 1:L0].reshape(B * G * G, D)
    assert torch.isfinite(x0).all()
    worst = float(((got.double() - val).abs() / fref.tol_ln(val, bound, torch.float32)).max())
    print(f"\nvitl14-parity: front end {str(dtype)[6:]} images, slot 0 patch rows: worst error / tolerance {worst:.3f}")
    assert worst <= 1.0
    mean = rows.mean(dim=1, keepdim=True)
    std = torch.sqrt(((rows - mean) ** 2).mean(dim=1, keepdim=True) + 1e-5)
    assert torch.equal(torch.round(got.double() * std + mean), rows), "a patch or a pad column is not where front_ref.patchify places it"
    # the check can fail: the reference of the image transposed inside every patch, and of the images in another order, is far outside
    for other in (image.reshape(B, 3, G, P, G, P).transpose(3, 5).reshape(B, 3, R, R), image.flip(0)):
        wrong = fref.patchify(other, P, kpad).double() + pos.double()[1:].repeat(B, 1)
        assert float(((fref.layer_norm_rows(wrong.float(), one, zero, 1e-5)[0] - val).abs() / fref.tol_ln(val, bound, torch.float32)).max()) > 100.0
    # the class row and the prompt rows, as they were
    cls = sd["visual.class_embedding"].float() + pos[0]
    v, b = fref.layer_norm_rows(torch.cat([cls[None], prompts[0].half().float()]), one, zero, 1e-5)
    for i in range(B):
        assert bool(((torch.cat([x0[i, :1], x0[i, L0:]]).double() - v).abs() <= fref.tol_ln(v, b, torch.float32)).all()), i


def loader_slot0(c, B, n_ctx):
    """Slot 0 through the two operators of the unchanged route, called on their own: clipmi_patch_embed (the im2col-free loader; pos left
    to ln_pre) and clipmi_embed_ln with add_pos = 1, on the model's weights."""
    g, sd = ref.geometry(c["geom"]), c["sd"]
    R, P, D = g.image_resolution, g.vision_patch_size, g.vision_width
    L0 = g.vision_tokens
    L, K = L0 + n_ctx, 3 * P * P
    dev = lambda t, dt: t.detach().to(dt).contiguous().cuda()
    img = dev(c["images"], torch.float32)
    w = dev(sd["visual.conv1.weight"].reshape(D, K), torch.float16)
    names = ("visual.class_embedding", "visual.positional_embedding", "visual.ln_pre.weight", "visual.ln_pre.bias")
    cls, pos, gam, bet = (dev(sd[n], torch.float32) for n in names)
    shallow = dev(c["prompts"][0].half(), torch.float32)
    scratch = torch.empty(_lib.lib.clipmi_patch_embed_scratch_bytes(B, R, _lib.F32), dtype=torch.uint8, device="cuda")
    x0 = torch.zeros(B * L, D, dtype=torch.float32, device="cuda")
    y = torch.empty_like(x0)
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib.clipmi_patch_embed(img.data_ptr(), _lib.F32, scratch.data_ptr(), w.data_ptr(), K, None, x0.data_ptr(), _lib.F32, B, R, P, D, L, s),
               "clipmi_patch_embed")
    _lib.check(_lib.lib.clipmi_embed_ln(x0.data_ptr(), _lib.F32, 1, cls.data_ptr(), pos.data_ptr(), shallow.data_ptr(), gam.data_ptr(), bet.data_ptr(),
                                        y.data_ptr(), None, None, B, L, L0, D, 1e-5, s), "clipmi_embed_ln")
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("geom,B,n_ctx", [("custom", 2, 8), ("tiny", 3, 8)])
def test_loader_geometries_keep_their_route_bits_and_sizes(geom, B, n_ctx):
    """Patches of 8 (vptfit_ref.CUSTOM, 205 rows) and 16 (tiny): the sizes are the layout with the fp16 image copy in the slot, slot 0 of the
    stash has the bits of the loader's two operators called on their own, and three steps give the same bits through the separate calls
    and the one-call step, with the option off and on."""
    c = vpt_case(geom, n_ctx, 2, B, 5)
    g = ref.geometry(geom)
    L, D, E, layers = g.vision_tokens + n_ctx, g.vision_width, g.embed_dim, g.vision_layers
    M = B * L
    want_ws = (2 * a256(M * D * 2) + a256(M * D * 8) + a256(M * D * 6) + a256(M * D * 4) + a256(B * D * 2) + a256(B * E * 2) + a256(B * D * 4)
               + a256(M * D * 4) + a256(B * 3 * g.image_resolution ** 2 * 2) + a256(layers * n_ctx * D * 2) + a256(n_ctx * D * 4))
    want_st = (2 * layers + 1) * a256(M * D * 4) + layers * (a256(M * D * 6) + a256(M * D * 8)) + a256(B * 8) + a256(layers * n_ctx * D * 4)
    assert vptfit.stash_bytes(c["model"], B, n_ctx) == (want_ws, want_st)
    t = vptfit._Tower("test", c["model"], 2, n_ctx)
    t.forward(c["images"].cuda(), c["prompts"].cuda().contiguous())
    torch.cuda.synchronize()
    slot0 = Stash(t.stash, B, L, D, layers, n_ctx).x(0)
    assert torch.equal(slot0.view(torch.int32), loader_slot0(c, B, n_ctx).view(torch.int32)), "slot 0 is not the loader route's"
    off = vpt_steps(c, False)
    assert torch.isfinite(off).all() and not torch.equal(off, c["prompts"])
    assert torch.equal(vpt_steps(c, True).view(torch.int32), off.view(torch.int32))
    long_on()
    assert vptfit.stash_bytes(c["model"], B, n_ctx) == (want_ws, want_st)
    assert torch.equal(vpt_steps(c, False).view(torch.int32), off.view(torch.int32))
    assert torch.equal(vpt_steps(c, True).view(torch.int32), off.view(torch.int32))
