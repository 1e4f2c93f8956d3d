"""CoCoOp's training on the GPU (clip_calibration_amd/cocoopfit.py, csrc/cocoop_train.hip) on the `tiny` and `tiny3` geometries against the
restatement and float64 autograd through the oracle (tests/cocoopfit_ref.py).

Operator level: the assembly, the reduce with the meta-net's backward (on small integers) and the step bit for bit; the meta-net and the
head within 4 x the distance of torch's own fp32 evaluation of the same formulas from float64, with a floor derived where it is used.
End to end: the relative Frobenius error of each of the five gradients against float64 autograd within FACTOR = 2 x the same error of
the oracle's autograd at float16 (the reference's own precision, the meta-net in half as well), the rule of tests/test_gpu_promptfit.py.
Every test prints its figures on lines that start with "cocoopfit-parity:"; profiles/cocoopfit_parity.txt holds one run's lines."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import cocoopfit_ref as cref
import coopfit_ref as ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import _lib, ops  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

FACTOR = 2.0
GRAD_SCALE = 256.0          # as tests/test_gpu_coopfit.py: the synthetic weights give gradients far larger than ViT-B/16's
U32 = 2.0 ** -24
RATES = [2e-3, 1e-3, 5e-4]
SGD = dict(momentum=0.9, dampening=0.0, nesterov=False, weight_decay=5e-4)
NAMES = cref.NAMES


def say(line):
    print("cocoopfit-parity: " + line)


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def model(geom):
    return build_model(dict(ref.state_dict(geom)), {"trainer": "CoOp"}).cuda()


@functools.lru_cache(maxsize=None)
def oracle(key):
    """(case, float64 parts, float16 parts, how the float16 ones were made), computed once per case."""
    c = cref.make_case(*key)
    args = (c["sd"], c["ids"], c["params"], c["feats"], c["labels"])
    yard, how = cref.yardstick_parts(*args)
    return c, cref.oracle_parts(*args), yard, how


def live_rows(ids):
    return (int(ids.argmax(dim=-1).max()) + 1 + 7) // 8 * 8


def dev_params(p):
    return {k: v.cuda() for k, v in p.items()}


# ------------------------------------------------------------------------------------------------------------------ a. meta and embed
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("key", cref.CASES, ids=ident)
def test_meta(key, strided):
    c = cref.make_case(*key)
    p = c["params"]
    E = c["feats"].shape[1]
    wide = torch.cat([torch.zeros(len(c["feats"]), 8), c["feats"], torch.ones(len(c["feats"]), 16)], dim=1)
    fd = wide.cuda()[:, 8:8 + E] if strided else c["feats"].cuda()
    x64, _, h64, pi64 = cref.meta(c["feats"].double(), {k: v.double() for k, v in p.items()})
    x32, _, h32, pi32 = cref.meta(c["feats"], p)
    x, hid, pi = ops.cocoop_meta(fd, *(p[k].cuda() for k in NAMES[1:]))
    # 4 x the distance of torch's fp32 evaluation from float64, with floors in test_coop_head's style.  x = f / |f| carries the sum's
    # tree, the root, the quotient and the product: 8 u of the largest entry.  A hidden unit is a dot product of E terms on that x plus
    # the bias: 8 u of sum_e |W1 x| + |b1| (the terms' own rounding and x's).  pi is a dot product of H terms on hid: 8 u of
    # sum_h |W2 hid| + |b2|, plus hid's floor carried through |W2|.
    w1, w2 = p[NAMES[1]].double().abs(), p[NAMES[3]].double().abs()
    floor_x = 8 * U32 * float(x64.abs().max())
    floor_h = 8 * U32 * float((x64.abs() @ w1.t() + p[NAMES[2]].double().abs()).max())
    floor_pi = 8 * U32 * float((h64 @ w2.t() + p[NAMES[4]].double().abs()).max()) + floor_h * float(w2.sum(1).max())
    for name, got, v32, v64, floor in (("x_n", x, x32, x64, floor_x), ("hid", hid, h32, h64, floor_h), ("pi", pi, pi32, pi64, floor_pi)):
        tol = max(4 * float((v32.double() - v64).abs().max()), floor)
        err = float((got.cpu().double() - v64).abs().max())
        say(f"meta {key} strided={strided} {name}: {err:.2e} (tol {tol:.2e})")
        assert err <= tol, name
    assert torch.equal((hid.cpu() > 0), (h64 > 0)) and bool((hid == 0).any()) and bool((hid > 0).any())       # the mask as float64 has it
    again = ops.cocoop_meta(fd, *(p[k].cuda() for k in NAMES[1:]))
    assert all(torch.equal(a, b) for a, b in zip(again, (x, hid, pi)))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("key", cref.CASES, ids=ident)
def test_embed_bit_for_bit(key, dtype):
    """Prompt buffer and EOT vector: context rows fp32(ctx + pi) of the device's own pi, every other row the widened base.  NaN prefill:
    rows behind the live ones stay untouched; canaries on both sides."""
    c = cref.make_case(*key)
    Cn, n_ctx, B = key[1], key[2], key[3]
    emb = c["sd"]["token_embedding.weight"][c["ids"]].to(dtype)
    Lc, D = emb.shape[1], emb.shape[2]
    L = live_rows(c["ids"])
    N = B * Cn
    pi = (0.02 * torch.randn(B, D, generator=torch.Generator().manual_seed(N))).cuda()
    ctx = c["params"]["ctx"].cuda()
    want = cref.assemble(emb.float(), ctx.cpu(), pi.cpu())
    want_eot = c["ids"].argmax(dim=-1).to(torch.int32).repeat(B)
    assert torch.equal(want.view(B, Cn, Lc, D)[B - 1, 1, 1:1 + n_ctx], (ctx + pi[B - 1]).cpu())          # one fp32 addition
    pad = 1024
    store = torch.full((N * Lc * D + 2 * pad,), float("nan"), device="cuda")
    eot_store = torch.full((N + 16,), -7, dtype=torch.int32, device="cuda")
    prompts, eot = store[pad:pad + N * Lc * D].view(N, Lc, D), eot_store[8:8 + N]
    cls_eot = c["ids"].argmax(dim=-1).to(torch.int32).cuda()
    ops.cocoop_embed(emb.cuda(), ctx, pi, cls_eot, L, prompts, eot)
    got = prompts.cpu()
    assert L < Lc and torch.equal(got[:, :L], want[:, :L]) and torch.isnan(got[:, L:]).all()
    assert torch.isnan(store[:pad]).all() and torch.isnan(store[-pad:]).all()
    assert torch.equal(eot.cpu(), want_eot) and bool((eot_store[:8] == -7).all()) and bool((eot_store[-8:] == -7).all())
    full, _ = ops.cocoop_embed(emb.cuda(), ctx, pi, cls_eot)
    assert torch.equal(full.cpu(), want)


# -------------------------------------------------------------------------------------------------------------------- b. tower tie-in
@pytest.mark.parametrize("geom", ["tiny", "tiny3"])
def test_zero_shift_gives_coops_text_features(geom):
    """W2 = 0 and b2 = 0 at B = 1: pi is exactly zero, the prompts are CoOp's, and the tower gives coopfit.text_features' bits."""
    from clip_calibration_amd import cocoopfit, coopfit
    c = cref.make_case(geom, 5, 4, 1)
    p = dict(c["params"])
    p[NAMES[3]], p[NAMES[4]] = torch.zeros_like(p[NAMES[3]]), torch.zeros_like(p[NAMES[4]])
    _, _, parts = cocoopfit.gradients(model(geom), c["ids"], p, c["feats"].cuda(), c["labels"], grad_scale=GRAD_SCALE, return_parts=True)
    assert float(parts["pi"].abs().max()) == 0.0
    assert torch.equal(parts["text"], coopfit.text_features(model(geom), c["ids"], p["ctx"]))


# ------------------------------------------------------------------------------------------------------------------------- c. head
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("B,Cn,E", ref.HEAD_CASES)
def test_head(B, Cn, E, strided):
    wide, text, y = cref.head_case(B, Cn, E)
    f = wide[:, 8:8 + E]
    scale, gs = cref.HEAD_SCALE, 4.0
    l64, d64, r64, _ = cref.head(f.double(), y, text.double(), scale)
    l32, d32, r32, _ = cref.head(f.float().contiguous(), y, text, scale)
    fd = wide.cuda()[:, 8:8 + E] if strided else f.contiguous().cuda()
    # tests/test_gpu_prodafit.py::test_head's floors without the sigma term: a logit z = scale * cosine carries about eight fp32
    # roundings, dz <= 8 u scale; a cross-entropy moves by at most 2 dz and every gradient entry by at most 2 dz of the largest entry.
    dz = 8 * U32 * scale
    loss, d_text, rows = ops.cocoop_head(fd, y.cuda(), text.cuda(), scale, gs, want_rows=True)
    tol_l = max(4 * abs(float(l32) - float(l64)), 2 * dz)
    tol_r = max(4 * float((r32.double() - r64).abs().max()), 2 * dz)
    tol_d = max(4 * float((d32.double() - d64).abs().max()), 2 * dz * float(d64.abs().max()))
    err_l, err_r = abs(float(loss.cpu()) - float(l64)), float((rows.cpu().double() - r64).abs().max())
    err_d = float((d_text.cpu().double() / gs - d64).abs().max())
    say(f"head B={B} C={Cn} E={E} strided={strided}: dloss {err_l:.2e} (tol {tol_l:.2e}), drows {err_r:.2e} (tol {tol_r:.2e}), dgrad {err_d:.2e} (tol {tol_d:.2e})")
    assert err_l <= tol_l and err_r <= tol_r and err_d <= tol_d
    again = ops.cocoop_head(fd, y.cuda(), text.cuda(), scale, gs)
    assert torch.equal(again[0], loss) and torch.equal(again[1], d_text)                      # the same inputs, the same bits


def test_head_bad_label_poisons_its_image_only():
    B, Cn, E = 8, 3, 64
    wide, text, y = cref.head_case(B, Cn, E)
    f = wide[:, :E].contiguous().cuda()
    good = ops.cocoop_head(f, y.cuda(), text.cuda(), cref.HEAD_SCALE, 1.0, want_rows=True)
    for bad_values in ((5, -1), (1 << 40, -(1 << 40))):
        bad = y.clone()
        bad[1], bad[5] = bad_values
        loss, d_text, rows = ops.cocoop_head(f, bad.cuda(), text.cuda(), cref.HEAD_SCALE, 1.0, want_rows=True)
        d, r = d_text.cpu().view(B, Cn, E), rows.cpu()
        poisoned = torch.tensor([False, True, False, False, False, True, False, False])
        assert torch.isnan(loss.cpu()).all() and torch.isnan(d[poisoned]).all() and torch.isnan(r[poisoned]).all()
        assert torch.equal(d[~poisoned], good[1].cpu().view(B, Cn, E)[~poisoned]) and torch.equal(r[~poisoned], good[2].cpu()[~poisoned])


# ------------------------------------------------------------------------------------------------- d. reduce and meta-net backward
@pytest.mark.parametrize("B,Cn,L,D,E,H", [(1, 3, 8, 64, 64, 4), (3, 5, 16, 128, 128, 8), (2, 4, 9, 132, 72, 5)])
def test_reduce_is_exact_on_small_integers(B, Cn, L, D, E, H):
    """d_embed, hid, x_n and W2 hold small integers (|v| <= 8) and grad_scale is a power of two: every partial sum is exact in fp32, so
    the five gradients equal the float64 restatement bit for bit -- a wrong row, class or image index shows exactly.  hid holds zeros:
    the mask convention is seen."""
    n_ctx, gs = 4, 4.0
    g = torch.Generator().manual_seed(B * 100 + Cn)
    d_embed = torch.randint(-8, 9, (B * Cn, L, D), generator=g).float()
    x = torch.randint(-8, 9, (B, E), generator=g).float()
    hid = torch.randint(-3, 9, (B, H), generator=g).clamp(min=0).float()
    w2 = torch.randint(-8, 9, (D, H), generator=g).float()
    assert bool((hid == 0).any()) and bool((hid > 0).any())
    want = cref.reduce(d_embed.double() / gs, x.double(), hid.double(), w2.double(), B, Cn, n_ctx)
    block = ops.cocoop_reduce(d_embed.view(-1, D).cuda(), x.cuda(), hid.cuda(), w2.cuda(), Cn, n_ctx, gs)
    got = ops.cocoop_block_views(block, n_ctx, D, E, H)
    for k in NAMES:
        assert float(want[k].abs().max()) < 2 ** 24 and torch.equal(got[k].cpu().double(), want[k]), k
    again = ops.cocoop_reduce(d_embed.view(-1, D).cuda(), x.cuda(), hid.cuda(), w2.cuda(), Cn, n_ctx, gs)
    assert torch.equal(again, block)


# ------------------------------------------------------------------------------------------------------------------------- e. step
@pytest.mark.parametrize("momentum,dampening,wd,nesterov", [(0.0, 0.0, 0.0, False), (0.9, 0.0, 5e-4, False), (0.9, 0.0, 0.0, True), (0.5, 0.25, 1e-2, False)])
def test_step_is_torch_sgd_bit_for_bit(momentum, dampening, wd, nesterov):
    """Three steps at three rates on the five tensors against torch.optim.SGD on the GPU over five nn.Parameters fed the same gradients."""
    n_ctx, D, E, H = 4, 128, 64, 5
    layout, total = ops.cocoop_block_layout(n_ctx, D, E, H)
    g = torch.Generator().manual_seed(11)
    block = torch.randn(total, generator=g).cuda()
    buf = torch.zeros_like(block) if momentum else None
    pars = [torch.nn.Parameter(v.clone()) for v in ops.cocoop_block_views(block, n_ctx, D, E, H).values()]
    opt = torch.optim.SGD(pars, lr=RATES[0], momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    lr = torch.tensor(RATES, dtype=torch.float32).cuda()
    for k in range(3):
        grad = torch.randn(total, generator=g).cuda()
        ops.cocoop_step(grad, block, buf, lr[k:k + 1], n_ctx, D, E, H, k == 0, momentum, dampening, wd, nesterov)
        for par, gv in zip(pars, ops.cocoop_block_views(grad, n_ctx, D, E, H).values()):
            par.grad = gv.clone()
        opt.param_groups[0]["lr"] = RATES[k]
        opt.step()
        for par, (name, v) in zip(pars, ops.cocoop_block_views(block, n_ctx, D, E, H).items()):
            assert torch.equal(v, par.detach()), (k, name)


# -------------------------------------------------------------------------------------------------------------------- f. end to end
def device_parts(c, geom, **kw):
    from clip_calibration_amd import cocoopfit
    kw.setdefault("grad_scale", GRAD_SCALE)
    loss, grads = cocoopfit.gradients(model(geom), c["ids"], c["params"], c["feats"].cuda(), c["labels"], logit_scale=ref.LOGIT_SCALE, **kw)
    return float(loss.cpu()[0]), {k: v.cpu() for k, v in grads.items()}


@pytest.mark.parametrize("seq_rows", [None, 0], ids=["cut", "whole"])
@pytest.mark.parametrize("key", cref.CASES, ids=ident)
def test_gradients_against_float64(key, seq_rows):
    """Each of the five gradients within FACTOR x its own float16 yardstick; the loss within FACTOR x the context gradient's yardstick,
    relative to max(1, |loss|), as the CoOp tests hold theirs."""
    c, want, yard, how = oracle(key)
    loss, grads = device_parts(c, key[0], seq_rows=seq_rows)
    ys = {k: ref.rel_fro(yard["grads"][k], want["grads"][k]) for k in NAMES}
    es = {k: ref.rel_fro(grads[k], want["grads"][k]) for k in NAMES}
    say(f"gradient {key} seq_rows={seq_rows} loss {loss:.6f} vs {want['loss']:.6f} (float16 oracle {yard['loss']:.6f}, {how}); rel. Frobenius error / yardstick: " +
        ", ".join(f"{k} {es[k]:.3e} / {ys[k]:.3e} = {es[k] / ys[k]:.2f}" for k in NAMES))
    for k in NAMES:
        assert grads[k].shape == c["params"][k].shape and torch.isfinite(grads[k]).all() and float(want["grads"][k].norm()) > 0.0, k
        assert es[k] <= FACTOR * ys[k], k
    assert abs(loss - want["loss"]) <= FACTOR * ys["ctx"] * max(1.0, abs(want["loss"]))


# ---------------------------------------------------------------------------------------------------------------- g. reproducibility
def raw_loop(c, geom):
    """clipmi_cocoop_train_step called directly, three times, on buffers made here."""
    from clip_calibration_amd import cocoopfit
    m = model(geom)
    st = cocoopfit.CoCoOpFitState(m, c["ids"], c["params"], logit_scale=ref.LOGIT_SCALE, grad_scale=GRAD_SCALE, **SGD)
    f, y = c["feats"].cuda(), c["labels"].cuda()
    t = st.tower(f.shape[0])
    lr = torch.tensor(RATES, dtype=torch.float32).cuda()
    block, buf = st.block.clone(), torch.zeros_like(st.block)
    ws = torch.empty(_lib.lib.clipmi_cocoop_train_step_bytes(m._handle, t.n_cls, t.rows, f.shape[0], t.H, t.n_ctx), dtype=torch.uint8, device="cuda")
    losses = torch.zeros(3, device="cuda")
    for k in range(3):
        with m._launch_lock:
            _lib.check(_lib.lib.clipmi_cocoop_train_step(m._handle, C.byref(t.dgrad[0]), t.base.data_ptr(), _lib.F16 if t.base.dtype == torch.float16 else
                                                         _lib.F32, block.data_ptr(), buf.data_ptr(), t.n_ctx, t.H, t.cls_eot.data_ptr(), t.n_cls, t.rows,
                                                         f.data_ptr(), f.stride(0), y.data_ptr(), f.shape[0], st.scale, GRAD_SCALE, lr[k:k + 1].data_ptr(),
                                                         int(k == 0), 0.9, 0.0, 5e-4, 0, losses[k:k + 1].data_ptr(), None, ws.data_ptr(), ws.numel(),
                                                         t.stash.data_ptr(), t.stash.numel(), ops._stream()), "clipmi_cocoop_train_step")
        torch.cuda.synchronize()
    return block.cpu(), losses.cpu().numpy()


def three_steps(c, geom, how):
    from clip_calibration_amd import cocoopfit
    m = model(geom)
    f, y = c["feats"].cuda(), c["labels"].cuda()
    if how == "raw":
        return raw_loop(c, geom)
    if how == "fit":
        out, hist = cocoopfit.fit_prompt_learner(f, c["labels"], m, c["ids"], c["params"], logit_scale=ref.LOGIT_SCALE, epochs=3, batch_size=f.shape[0],
                                                 lr_per_epoch=RATES, grad_scale=GRAD_SCALE, return_history=True, **SGD)
        return torch.cat([out[k].reshape(-1) for k in NAMES]).cpu(), hist
    st = cocoopfit.CoCoOpFitState(m, c["ids"], c["params"], logit_scale=ref.LOGIT_SCALE, grad_scale=GRAD_SCALE, **SGD)
    lr = torch.tensor(RATES, dtype=torch.float32).cuda()
    losses = [st.step(f, y, lr[k:k + 1], want_loss=True, one_call=(how == "one_call")) for k in range(3)]
    assert all(v.data_ptr() == st.block.data_ptr() + 4 * off for v, (off, _) in zip(st.params().values(), ops.cocoop_block_layout(st.n_ctx, st.D, st.E, st.H)[0].values()))
    return st.block.cpu(), torch.cat(losses).cpu().numpy()


@pytest.mark.parametrize("key", [("tiny", 5, 4, 3), ("tiny3", 3, 4, 3), ("tiny3", 5, 4, 1)], ids=ident)
def test_three_steps_same_bits_every_way(key):
    c = cref.make_case(*key)
    a, la = three_steps(c, key[0], "step")
    start = torch.cat([c["params"][k].reshape(-1) for k in NAMES])
    assert torch.isfinite(a).all() and np.isfinite(la).all()
    layout, _ = ops.cocoop_block_layout(key[2], c["params"]["ctx"].shape[1], c["feats"].shape[1], c["params"][NAMES[2]].shape[0])
    for k, (off, shape) in layout.items():                          # every one of the five tensors has moved
        n = int(np.prod(shape))
        assert not torch.equal(a[off:off + n], start[off:off + n]), k
    for how in ("fit", "one_call", "raw", "step"):                  # the last: two runs, the same bits
        b, lb = three_steps(c, key[0], how)
        assert torch.equal(a, b) and np.array_equal(la, lb), how


def test_three_steps_against_float64_sgd():
    """Three SGD steps with momentum and weight decay follow float64 SGD on the oracle within 3 x the single-gradient bound, relative to
    the distance each tensor travels (the CoOp test's rule)."""
    key = ("tiny", 5, 4, 3)
    c, want, yard, _ = oracle(key)
    got, _ = three_steps(c, key[0], "step")
    w, grads = {k: v.double() for k, v in c["params"].items()}, []
    bufs = {k: None for k in NAMES}
    for step, lr in enumerate(RATES):
        g = cref.oracle_parts(c["sd"], c["ids"], w, c["feats"], c["labels"])["grads"]
        for k in NAMES:
            w[k], bufs[k] = ref.sgd_step(w[k], bufs[k], g[k], lr, SGD["momentum"], SGD["dampening"], SGD["weight_decay"], SGD["nesterov"], step == 0)
    layout, _ = ops.cocoop_block_layout(key[2], w["ctx"].shape[1], c["feats"].shape[1], w[NAMES[2]].shape[0])
    for k, (off, shape) in layout.items():
        y = ref.rel_fro(yard["grads"][k], want["grads"][k])
        moved = float((w[k] - c["params"][k].double()).norm())
        e = float((got[off:off + w[k].numel()].view(shape).double() - w[k]).norm()) / moved
        say(f"three steps {key} {k}: error {e:.3e} of the distance travelled, yardstick {y:.3e}")
        assert e <= 3 * FACTOR * y, k


# --------------------------------------------------------------------------------------------------------------------------- h. fit
def test_five_steps_lower_the_loss():
    from clip_calibration_amd import cocoopfit
    c = cref.make_case("tiny", 3, 4, 3, 0, True)
    f = c["feats"].cuda()
    _, hist = cocoopfit.fit_prompt_learner(f, c["labels"], model("tiny"), c["ids"], c["params"], logit_scale=ref.LOGIT_SCALE, epochs=5, batch_size=3,
                                           lr_per_epoch=[0.002] * 5, grad_scale=GRAD_SCALE, return_history=True, **SGD)
    say(f"fit: loss {hist[0]:.5f} -> {hist[-1]:.5f} over {len(hist)} steps")
    assert len(hist) == 5 and np.isfinite(hist).all() and hist[-1] < hist[0]


# ------------------------------------------------------------------------------------------------------------------- i. integration
def test_trainer_fit_prompt_learner_updates_the_module():
    from clip_calibration_amd.trainers import cocoop
    m = model("tiny")
    ids = ref.prompt_ids("tiny", 3, 4)
    clip = cocoop.CustomCLIP(m, ids, n_ctx=4)
    pl = clip.prompt_learner
    before = {k: v.detach().clone() for k, v in pl.state_dict().items() if k in NAMES}
    g = torch.Generator().manual_seed(0)
    centres = torch.randn(3, 128, generator=g)
    labels = torch.arange(3).repeat_interleave(2)
    feats = centres[labels] + 0.1 * torch.randn(6, 128, generator=g)
    image = torch.randn(2, 128, generator=g).cuda()
    try:
        m.image_features_f32 = lambda x: x              # the loader's "images" are the features (tests/test_gpu_coopfit.py)
        fitted, hist = clip.fit_prompt_learner([(feats.cuda(), labels)], epochs=4, lr_per_epoch=[0.01] * 4, batch_size=2, grad_scale=GRAD_SCALE,
                                               return_history=True, **SGD)
        say(f"cocoop.CustomCLIP.fit_prompt_learner: loss {hist[0]:.5f} -> {hist[-1]:.5f} over {len(hist)} steps")
        assert len(hist) == 12 and np.isfinite(hist).all()
        after = {k: v.detach() for k, v in pl.state_dict().items() if k in NAMES}
        for k in NAMES:
            assert after[k].dtype == before[k].dtype and torch.equal(after[k], fitted[k].to(after[k].dtype)) and not torch.equal(after[k], before[k]), k
        mirror = cocoop.CustomCLIP(m, ids, n_ctx=4)
        mirror.prompt_learner.load_state_dict({k: v for k, v in pl.state_dict().items() if k in NAMES}, strict=False)
        got, want = clip(image), mirror(image)
        assert all(torch.equal(a, b) for a, b in zip(got, want)) and torch.isfinite(got[0]).all()
    finally:
        del m.image_features_f32


def test_trainer_transform_route_gives_the_cached_routes_bits():
    """With explicit, deterministic views the per-step route (transform -> image tower -> CoCoOpFitState.step) gives the bits of the
    cached route on the features of the same views."""
    import augment_ref
    from clip_calibration_amd.augment import TrainPreprocess
    from clip_calibration_amd.preprocess import pack_images
    from clip_calibration_amd.trainers import cocoop
    m = model("tiny")
    sizes = [(80, 100), (64, 64), (70, 51), (120, 90)]
    imgs = [augment_ref.synthetic_image(h, w, 70 + i) for i, (h, w) in enumerate(sizes)]
    labels = torch.arange(4) % 3
    loader = [(pack_images(imgs[i:i + 2]).pin_memory(), labels[i:i + 2]) for i in (0, 2)]
    ids = ref.prompt_ids("tiny", 3, 4)
    rates = [0.002, 0.001]
    opt = dict(grad_scale=GRAD_SCALE, **SGD)

    def views(e, k, shapes):       # the whole image, unflipped: one deterministic view per image
        return np.array([[i, 0, 0, int(h), int(w), 0] for i, (h, w) in enumerate(shapes)], np.int32)

    tp = TrainPreprocess.for_model(m)
    a = cocoop.CustomCLIP(m, ids, n_ctx=4)
    start = {k: v.detach().clone() for k, v in a.prompt_learner.state_dict().items() if k in NAMES}
    fitted_a, losses_a = a.fit_prompt_learner(loader, transform=tp, epochs=2, lr_per_epoch=rates, views=views, return_history=True, **opt)
    b = cocoop.CustomCLIP(m, ids, n_ctx=4)
    b.prompt_learner.load_state_dict(start, strict=False)          # nn.Linear draws the meta-net from the global generator
    cached = []
    with torch.no_grad():
        for images, y in loader:
            buf, descs, B = tp._gather(images, torch.device("cuda", torch.cuda.current_device()))
            from clip_calibration_amd.augment import _view_table
            x = tp._run_views(buf, descs, B, _view_table(views(0, 0, descs.view(np.int32)[:, 2:4].copy())), torch.device("cuda", torch.cuda.current_device()))
            cached.append((m.image_features_f32(x).clone(), y))
    try:
        m.image_features_f32 = lambda x: x
        fitted_b, losses_b = b.fit_prompt_learner(cached, epochs=2, lr_per_epoch=rates, batch_size=2, return_history=True, **opt)
    finally:
        del m.image_features_f32
    assert np.isfinite(losses_a).all() and np.array_equal(losses_a, losses_b)
    assert all(torch.equal(fitted_a[k], fitted_b[k]) for k in NAMES)
    sa, sb = a.prompt_learner.state_dict(), b.prompt_learner.state_dict()
    assert all(torch.equal(sa[k], sb[k]) and not torch.equal(sa[k], start[k]) for k in NAMES)
