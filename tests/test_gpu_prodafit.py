"""ProDA's training on the GPU (clip_calibration_amd/prodafit.py, csrc/proda_train.hip) on the `tiny` and `tiny3` geometries against the
restatement and float64 autograd through the oracle (tests/prodafit_ref.py).

Operator level: the assembly and the context reduce bit for bit; the head within 4 x the distance of torch's own fp32 evaluation of the
same formulas from float64, with a floor derived where it is used.  End to end: the relative Frobenius error against float64 autograd
within FACTOR = 2 x the same error of the oracle's autograd at float16 (the reference's own precision), the rule of
tests/test_gpu_promptfit.py.  Every test prints its figures on lines that start with "prodafit-parity:"; profiles/prodafit_parity.txt is
one run's lines."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import coopfit_ref as ref
import prodafit_ref as dref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import _lib, ops  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

FACTOR = 2.0
GRAD_SCALE = 256.0          # as tests/test_gpu_coopfit.py: the synthetic weights give gradients far larger than ViT-B/16's
U32 = 2.0 ** -24
RATES = [2e-3, 1e-3, 5e-4]
SGD = dict(momentum=0.9, dampening=0.0, nesterov=False, weight_decay=5e-4)


def say(line):
    print("prodafit-parity: " + line)


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def model(geom):
    return build_model(dict(ref.state_dict(geom)), {"trainer": "CoOp"}).cuda()


@functools.lru_cache(maxsize=None)
def oracle(key, sel):
    """(case, float64 parts, float16 parts, how the float16 ones were made), computed once per case."""
    c = dref.make_case(*key)
    args = (c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"], sel)
    yard, how = dref.yardstick_parts(*args)
    return c, dref.oracle_parts(*args), yard, how


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def pieces(key, sel):
    """The case's host-side pieces: ordered selection, positions, name lengths."""
    c = dref.make_case(*key)
    P, n_ctx = key[3], key[2]
    pos = dref.positions(P)
    s = dref.ordered(np.arange(P) if sel is None else sel, pos)
    return c, s, pos, dref.name_lens_of(c["ids"], n_ctx)


def eot_of(c):
    return c["ids"].argmax(dim=-1).numpy()


# ------------------------------------------------------------------------------------------------------------------------ a. embed
@pytest.mark.parametrize("short", [False, True], ids=["own", "short"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("key,sel", dref.CASE_LIST, ids=ident)
def test_embed_bit_for_bit(key, sel, dtype, short):
    """Prompt buffer and EOT vector against the restated assembly: class 0 has an empty name (front, middle and end coincide), the last
    class has its EOT on the last live row.  NaN prefill: rows behind the live ones stay untouched; canaries on both sides.  ``short``:
    name lengths of half the prompts' own (fewer tokens move, the EOT rows stay)."""
    c, s, pos, nl = pieces(key, sel)
    own = nl
    nl = nl // 2 if short else nl
    Cn, n_ctx, P = key[1], key[2], key[3]
    emb = c["sd"]["token_embedding.weight"][c["ids"]].to(dtype)
    Lc, D = emb.shape[1], emb.shape[2]
    L = (int(c["ids"].argmax(dim=-1).max()) + 1 + 7) // 8 * 8
    assert int(c["ids"][-1].argmax()) == L - 1 and nl[0] == 0
    N = Cn * len(s) + P
    want, want_eot = dref.assemble(emb.float(), emb[:1].float(), c["ctx"], s, pos, nl, eot_of(c))
    assert short or np.array_equal(want_eot[:Cn * len(s)], np.repeat(n_ctx + 2 + own, len(s)))
    pad = 1024
    store = torch.full((N * Lc * D + 2 * pad,), float("nan"), device="cuda")
    eot_store = torch.full((N + 16,), -7, dtype=torch.int32, device="cuda")
    prompts, eot = store[pad:pad + N * Lc * D].view(N, Lc, D), eot_store[8:8 + N]
    ops.proda_embed(emb[:Cn].cuda(), emb[:1].cuda(), c["ctx"].cuda(), i32(s), i32(pos), i32(nl), i32(eot_of(c)), L, prompts, eot)
    got = prompts.cpu()
    assert torch.equal(got[:, :L], want[:, :L]) and torch.isnan(got[:, L:]).all()
    assert torch.isnan(store[:pad]).all() and torch.isnan(store[-pad:]).all()
    assert np.array_equal(eot.cpu().numpy(), want_eot) and bool((eot_store[:8] == -7).all()) and bool((eot_store[-8:] == -7).all())
    full, _ = ops.proda_embed(emb[:Cn].cuda(), emb[:1].cuda(), c["ctx"].cuda(), i32(s), i32(pos), i32(nl), i32(eot_of(c)))
    assert torch.equal(full.cpu(), want)


def test_embed_bad_selection_poisons_and_never_addresses():
    key, sel = ("tiny", 3, 5, 8, 2, 8), (3, 6)
    c, s, pos, nl = pieces(key, sel)
    emb = c["sd"]["token_embedding.weight"][c["ids"]].float()
    for bad in (8, -1, 1 << 30):
        prompts, _ = ops.proda_embed(emb.cuda(), emb[:1].cuda(), c["ctx"].cuda(), i32([bad, 3]), i32(pos), i32(nl), i32(eot_of(c)))
        got = prompts[:6].cpu().view(3, 2, 77, -1)
        assert torch.isnan(got[:, 0]).all() and torch.isfinite(got[:, 1]).all() and torch.isfinite(prompts[6:].cpu()).all()


# ------------------------------------------------------------------------------------------------------------------------- b. head
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("B,Cn,E,Pb,P", dref.HEAD_CASES)
def test_head(B, Cn, E, Pb, P, strided):
    wide, text, y = dref.head_case(B, Cn, E, Pb, P)
    f = wide[:, 8:8 + E]
    scale, gs, alpha = dref.HEAD_SCALE, 4.0, dref.ALPHA
    h64 = dref.head(f.double(), y, text.double(), Cn, Pb, scale, alpha)
    h32 = dref.head(f.float().contiguous(), y, text, Cn, Pb, scale, alpha)
    fd = wide.cuda()[:, 8:8 + E] if strided else f.contiguous().cuda()
    # 4 x the distance of torch's fp32 evaluation from float64, with test_coop_head's floors.  The cosine term of a logit carries about
    # eight fp32 roundings: 8 u scale.  sigma is built from the same normalised rows and carries the factor 0.5 scale^2 in their place:
    # 0.5 scale^2 8 u.  A cross-entropy moves by at most 2 dz and every gradient entry by at most 2 dz of the largest entry.  m is a mean of
    # cosines without the scale: 8 u; the total's floor is upper's plus alpha times m's.
    dz = 8 * U32 * scale + 0.5 * scale * scale * 8 * U32

    def tol(v32, v64, floor):
        return max(4 * float((torch.as_tensor(v32).double() - v64).abs().max()), floor)

    def err(got, v64):
        return float((got.double() - v64).abs().max())

    losses, d_text = ops.proda_head(fd, y.cuda(), text.cuda(), Cn, Pb, scale, gs, alpha)
    lo = losses.cpu()
    tols = [tol(h32[0], h64[0], 2 * dz + alpha * 8 * U32), tol(h32[1], h64[1], 2 * dz), tol(h32[2], h64[2], 8 * U32)]
    tol_d = tol(h32[3], h64[3], 2 * dz * float(h64[3].abs().max()))
    errs = [err(lo[i], h64[i]) for i in range(3)]
    err_d = err(d_text.cpu() / gs, h64[3])
    say(f"head B={B} C={Cn} E={E} Pb={Pb} P={P} strided={strided}: d(total, upper, m) " + ", ".join(f"{e:.2e} (tol {t:.2e})" for e, t in zip(errs, tols)) +
        f"; dgrad {err_d:.2e} (tol {tol_d:.2e})")
    assert all(e <= t for e, t in zip(errs, tols)) and err_d <= tol_d
    again = ops.proda_head(fd, y.cuda(), text.cuda(), Cn, Pb, scale, gs, alpha)
    assert torch.equal(again[0].cpu(), lo) and torch.equal(again[1], d_text)                 # the same inputs, the same bits
    zero = ops.proda_head(fd, y.cuda(), text.cuda(), Cn, Pb, scale, gs, 0.0)
    assert float(zero[1][Cn * Pb:].abs().max()) == 0.0                                        # alpha = 0: exact zeros in the no-class rows
    assert torch.equal(zero[1][:Cn * Pb], d_text[:Cn * Pb]) and torch.equal(zero[0].cpu()[1:], lo[1:]) and torch.equal(zero[0].cpu()[0], lo[1])
    if Pb == 1:       # v = 0, sigma = 0: upper is CoOp's cross-entropy on the class rows, two logit roundings apart at most
        coop_loss, _ = ops.coop_head(fd, y.cuda(), text[:Cn].cuda(), scale, gs)
        assert abs(float(coop_loss.cpu()) - float(lo[1])) <= 2 * 8 * U32 * scale


def test_head_bad_label_poisons_and_never_addresses():
    wide, text, y = dref.head_case(8, 3, 64, 2, 4)
    f = wide[:, :64].contiguous().cuda()
    bad = y.clone()
    bad[1], bad[5] = 5, -1
    losses, d_text = ops.proda_head(f, bad.cuda(), text.cuda(), 3, 2, dref.HEAD_SCALE, 1.0, dref.ALPHA)
    lo, d = losses.cpu(), d_text.cpu()
    assert torch.isnan(lo[:2]).all() and torch.isnan(d[:6]).all()                            # every class row, every element
    assert torch.isfinite(lo[2]) and torch.isfinite(d[6:]).all()                             # the labels do not reach the no-class term
    bad[1], bad[5] = 1 << 40, -(1 << 40)
    losses, _ = ops.proda_head(f, bad.cuda(), text.cuda(), 3, 2, dref.HEAD_SCALE, 1.0, dref.ALPHA)
    assert torch.isnan(losses.cpu()[:2]).all()


# ------------------------------------------------------------------------------------------------------------------ c. context step
@pytest.mark.parametrize("key,sel", dref.CASE_LIST, ids=ident)
def test_ctx_step_gather_reduce_and_sgd(key, sel):
    c, s, pos, nl = pieces(key, sel)
    Cn, n_ctx, P = key[1], key[2], key[3]
    D, L = c["ctx"].shape[-1], (int(c["ids"].argmax(dim=-1).max()) + 1 + 7) // 8 * 8
    N = Cn * len(s) + P
    g = torch.Generator().manual_seed(N)
    d_embed = torch.randint(-8, 9, (N, L, D), generator=g).float()                          # small integers: every sum is exact in fp32
    want = dref.ctx_reduce(d_embed, s, pos, nl, Cn, P, n_ctx) / 4.0
    dev = d_embed.view(N * L, D).cuda()
    grad = ops.proda_ctx_step(dev, i32(s), i32(pos), i32(nl), n_ctx, 4.0)
    assert torch.equal(grad.cpu(), want)
    for p in set(range(P)) - set(int(v) for v in s):                                         # unselected: the no-class rows only
        assert torch.equal(grad[p].cpu(), d_embed[Cn * len(s) + p, 1:1 + n_ctx] / 4.0)
    # the step: torch.optim.SGD on the GPU applied to the reported gradient, bit for bit, three steps
    ctx = c["ctx"].cuda().clone()
    buf = torch.zeros_like(ctx)
    par = torch.nn.Parameter(ctx.clone())
    opt = torch.optim.SGD([par], lr=0.05, momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=False)
    lr = torch.tensor([0.05]).cuda()
    for k in range(3):
        got = ops.proda_ctx_step(dev, i32(s), i32(pos), i32(nl), n_ctx, 4.0, ctx, buf, lr, k == 0, 0.9, 0.0, 5e-4, False)
        assert torch.equal(got, grad)
        par.grad = grad.clone()
        opt.step()
        assert torch.equal(ctx, par.detach()), k


# -------------------------------------------------------------------------------------------------------------------- d. end to end
def device_parts(c, geom, sel, **kw):
    from clip_calibration_amd import prodafit
    kw.setdefault("grad_scale", GRAD_SCALE)
    loss, grad, parts = prodafit.context_gradient(model(geom), c["ids"], c["ctx"], c["feats"].cuda(), c["labels"], sel=sel, logit_scale=ref.LOGIT_SCALE,
                                                  return_parts=True, **kw)
    return float(loss.cpu()[0]), grad.cpu(), {k: v.cpu() for k, v in parts.items()}


END_TO_END = [(k, s, None) for k, s in dref.CASE_LIST] + [(k, s, 0) for k, s in dref.SEQ_ROWS_CASES]


@pytest.mark.parametrize("key,sel,seq_rows", END_TO_END, ids=ident)
def test_context_gradient_against_float64(key, sel, seq_rows):
    c, want, yard, how = oracle(key, sel)
    assert torch.isfinite(yard["grad"]).all() and float(want["grad"].norm()) > 0.0
    loss, grad, parts = device_parts(c, key[0], sel, seq_rows=seq_rows)
    y = ref.rel_fro(yard["grad"], want["grad"])
    e = ref.rel_fro(grad, want["grad"])
    ratios = {k: abs(v - want[k]) / (y * max(1.0, abs(want[k]))) for k, v in (("loss", loss), ("upper", float(parts["upper"])), ("m", float(parts["m"])))}
    say(f"gradient {key} sel={sel} seq_rows={seq_rows} loss {loss:.6f} vs {want['loss']:.6f} (upper {float(parts['upper']):.6f} vs {want['upper']:.6f}, "
        f"m {float(parts['m']):.6f} vs {want['m']:.6f}; float16 oracle loss {yard['loss']:.6f}); rel. Frobenius error {e:.3e}, yardstick ({how}) {y:.3e}, "
        f"ratio {e / y:.2f}; loss ratios " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    assert grad.shape == c["ctx"].shape and torch.isfinite(grad).all()
    assert all(v <= FACTOR for v in ratios.values())
    assert e <= FACTOR * y
    if key[4] == 1:   # Pb = 1: upper is CoOp's loss on the class prompts' own features
        coop_loss, _ = ops.coop_head(c["feats"].cuda(), c["labels"].cuda(), parts["text"][:key[1]].cuda(), float(np.float32(np.exp(ref.LOGIT_SCALE))))
        assert abs(float(coop_loss.cpu()) - float(parts["upper"])) <= 2 * 8 * U32 * float(np.exp(ref.LOGIT_SCALE))


def test_context_gradient_with_shorter_name_lens():
    """name_lens below the prompts' own: fewer tokens move in front of or between the context vectors, the EOT rows stay; the truth takes
    the same lengths through its own assembly."""
    from clip_calibration_amd import prodafit
    key, sel = ("tiny", 3, 5, 8, 2, 8), (0, 3)
    c = dref.make_case(*key)
    nl = dref.name_lens_of(c["ids"], key[2]) // 2
    assert (nl < dref.name_lens_of(c["ids"], key[2])).any()
    args = (c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"], sel)
    want, (yard, how) = dref.oracle_parts(*args, name_lens=nl), dref.yardstick_parts(*args, name_lens=nl)
    loss, grad = prodafit.context_gradient(model("tiny"), c["ids"], c["ctx"], c["feats"].cuda(), c["labels"], sel=sel, name_lens=nl,
                                           logit_scale=ref.LOGIT_SCALE, grad_scale=GRAD_SCALE)
    y, e = ref.rel_fro(yard["grad"], want["grad"]), ref.rel_fro(grad.cpu(), want["grad"])
    own = dref.oracle_parts(*args)["grad"]
    say(f"gradient {key} sel={sel} name_lens={nl.tolist()} loss {float(loss.cpu()):.6f} vs {want['loss']:.6f}; rel. Frobenius error {e:.3e}, yardstick ({how}) "
        f"{y:.3e}, ratio {e / y:.2f}; distance of the full-name gradient {ref.rel_fro(own, want['grad']):.3e}")
    assert e <= FACTOR * y and abs(float(loss.cpu()) - want["loss"]) <= FACTOR * y * max(1.0, abs(want["loss"]))
    assert ref.rel_fro(own, want["grad"]) > 10 * FACTOR * y          # the lengths matter: the full-name gradient is far outside the bound


# -------------------------------------------------------------------------------------------------------------------- e. three steps
def selections_of(key, sel):
    """Three explicit selections: the case's own and two rotations of it inside the collection."""
    P = key[3]
    base = np.arange(P) if sel is None else np.asarray(sel)
    return np.stack([(base + k) % P for k in range(3)]).astype(np.int32)


def raw_loop(c, geom, key, sels):
    """clipmi_proda_train_step called directly, three times, on buffers made here."""
    from clip_calibration_amd import prodafit
    m = model(geom)
    st = prodafit.ProDAFitState(m, c["ids"], c["ctx"], prompt_bs=key[4], logit_scale=ref.LOGIT_SCALE, grad_scale=GRAD_SCALE, **SGD)
    t = st.tower
    f, y = c["feats"].cuda(), c["labels"].cuda()
    lr = torch.tensor(RATES, dtype=torch.float32).cuda()
    ctx, buf = c["ctx"].cuda().clone(), torch.zeros_like(c["ctx"]).cuda()
    ws = torch.empty(_lib.lib.clipmi_proda_train_step_bytes(m._handle, t.n_cls, t.Pb, t.P, t.rows, f.shape[0]), dtype=torch.uint8, device="cuda")
    losses = torch.zeros(3, 3, device="cuda")
    pos = dref.positions(key[3])
    for k in range(3):
        sel_d = i32(dref.ordered(sels[k], pos))
        with m._launch_lock:
            _lib.check(_lib.lib.clipmi_proda_train_step(m._handle, C.byref(t.dgrad[0]), t.cls_base.data_ptr(), t.nc_base.data_ptr(), _lib.F16 if
                                                        t.base.dtype == torch.float16 else _lib.F32, ctx.data_ptr(), buf.data_ptr(), t.n_ctx, sel_d.data_ptr(),
                                                        t.pos.data_ptr(), t.name_lens.data_ptr(), t.cls_eot.data_ptr(), t.n_cls, t.Pb, t.P, t.rows, f.data_ptr(),
                                                        f.stride(0),
                                                        y.data_ptr(), f.shape[0], st.scale, GRAD_SCALE, dref.ALPHA, lr[k:k + 1].data_ptr(), int(k == 0), 0.9, 0.0,
                                                        5e-4, 0, losses[k].data_ptr(), None, ws.data_ptr(), ws.numel(), t.stash.data_ptr(), t.stash.numel(),
                                                        ops._stream()), "clipmi_proda_train_step")
        torch.cuda.synchronize()
    return ctx.cpu(), losses[:, 0].cpu().numpy()


def three_steps(c, geom, key, sels, how):
    from clip_calibration_amd import prodafit
    m = model(geom)
    f, y = c["feats"].cuda(), c["labels"].cuda()
    if how == "raw":
        return raw_loop(c, geom, key, sels)
    if how == "fit":
        ctx, hist = prodafit.fit_context(f, c["labels"], m, c["ids"], c["ctx"], prompt_bs=key[4], logit_scale=ref.LOGIT_SCALE, epochs=3, batch_size=f.shape[0],
                                         lr_per_epoch=RATES, selections=sels, grad_scale=GRAD_SCALE, return_history=True, **SGD)
        return ctx.cpu(), hist
    st = prodafit.ProDAFitState(m, c["ids"], c["ctx"], prompt_bs=key[4], logit_scale=ref.LOGIT_SCALE, grad_scale=GRAD_SCALE, **SGD)
    lr = torch.tensor(RATES, dtype=torch.float32).cuda()
    losses = []
    for k in range(3):
        losses.append(st.step(f, y, lr[k:k + 1], sel=sels[k], want_loss=True, one_call=(how == "one_call")))
        if how == "step" and k == 1:       # the backward leaves the stash as the forward wrote it
            before = st.tower.stash.clone()
            st.tower.backward(torch.ones_like(st.tower.text))
            assert torch.equal(st.tower.stash, before)
    return st.ctx.cpu(), torch.cat(losses).cpu().numpy()


@pytest.mark.parametrize("key,sel", [(("tiny", 3, 5, 8, 2, 8), (3, 6)), (("tiny3", 37, 4, 8, 4, 1), (7, 0, 3, 4)), (("tiny", 2, 4, 4, 4, 1), None)], ids=ident)
def test_three_steps_same_bits_every_way(key, sel):
    c = dref.make_case(*key)
    sels = selections_of(key, sel)
    a, la = three_steps(c, key[0], key, sels, "step")
    assert torch.isfinite(a).all() and not torch.equal(a, c["ctx"]) and np.isfinite(la).all()
    for how in ("fit", "one_call", "raw", "step"):                 # the last: two runs, the same bits
        b, lb = three_steps(c, key[0], key, sels, how)
        assert torch.equal(a, b) and np.array_equal(la, lb), how


def test_three_steps_against_float64_sgd():
    """Three SGD steps with momentum and weight decay follow float64 SGD on the oracle within 3 x the single-gradient bound, relative to
    the distance the context travels (the CoOp test's rule)."""
    key, sel = ("tiny", 3, 5, 8, 2, 8), (3, 6)
    c, want, yard, _ = oracle(key, sel)
    y = ref.rel_fro(yard["grad"], want["grad"])
    sels = selections_of(key, sel)
    got, _ = three_steps(c, key[0], key, sels, "step")
    w, buf = c["ctx"].double(), None
    for k, lr in enumerate(RATES):
        grad = dref.oracle_parts(c["sd"], c["ids"], w, c["feats"], c["labels"], tuple(int(v) for v in sels[k]))["grad"]
        w, buf = ref.sgd_step(w, buf, grad, lr, SGD["momentum"], SGD["dampening"], SGD["weight_decay"], SGD["nesterov"], k == 0)
    moved = float((w - c["ctx"].double()).norm())
    e = float((got.double() - w).norm()) / moved
    say(f"three steps {key} sel={sel}: error {e:.3e} of the distance travelled, yardstick {y:.3e}")
    assert e <= 3 * FACTOR * y


def test_state_draws_its_schedule():
    """sel=None: the state's own draw is draw_selections from the same seed, and gives the bits of the explicit schedule."""
    from clip_calibration_amd import prodafit
    key = ("tiny", 3, 5, 8, 2, 8)
    c, m = dref.make_case(*key), model("tiny")
    f, y = c["feats"].cuda(), c["labels"].cuda()
    sels = prodafit.draw_selections(8, 2, 5, torch.Generator().manual_seed(9))
    out = []
    for explicit in (False, True):
        st = prodafit.ProDAFitState(m, c["ids"], c["ctx"], prompt_bs=2, grad_scale=GRAD_SCALE, generator=torch.Generator().manual_seed(9), **SGD)
        for k in range(5):
            st.step(f, y, 1e-3, sel=sels[k] if explicit else None)
        out.append(st.ctx.cpu())
    assert torch.equal(out[0], out[1])


# ------------------------------------------------------------------------------------------------------------------------ f. trainer
def test_trainer_fit_context_lowers_the_loss():
    from clip_calibration_amd.trainers import proda
    m = model("tiny")
    ids = dref.prompt_ids("tiny", 3, 4)
    clip = proda.CustomCLIP(m, ids, n_ctx=4, n_prompt=4)
    clip.set_classifier()
    before_ctx, before_text = clip.prompt_learner.ctx.detach().clone(), clip.text_features.clone()
    g = torch.Generator().manual_seed(0)
    centres = torch.randn(3, 128, generator=g)
    labels = torch.arange(3).repeat_interleave(8)
    feats = centres[labels] + 0.1 * torch.randn(24, 128, generator=g)
    try:
        m.image_features_f32 = lambda image: image          # the loader's "images" are the features (tests/test_gpu_coopfit.py)
        fitted, hist = clip.fit_context([(feats.cuda(), labels)], epochs=20, lr_per_epoch=[0.002] * 20, batch_size=24, prompt_bs=4, momentum=0.9,
                                        weight_decay=5e-4, grad_scale=GRAD_SCALE, return_history=True)
    finally:
        del m.image_features_f32
    say(f"proda.CustomCLIP.fit_context: loss {hist[0]:.5f} -> {hist[-1]:.5f} over {len(hist)} steps")
    assert len(hist) == 20 and np.isfinite(hist).all() and hist[-1] < hist[0]
    assert clip.text_features is None
    assert torch.equal(clip.prompt_learner.ctx.detach().float().cpu(), fitted.to(clip.prompt_learner.ctx.dtype).float().cpu())
    assert not torch.equal(clip.prompt_learner.ctx.detach(), before_ctx)
    clip.set_classifier()
    assert not torch.equal(clip.text_features, before_text)
    mirror = proda.CustomCLIP(m, ids, n_ctx=4, n_prompt=4)
    with torch.no_grad():
        mirror.prompt_learner.ctx.copy_(clip.prompt_learner.ctx)
    mirror.set_classifier()
    assert torch.equal(mirror.text_features, clip.text_features)


def test_trainer_fit_context_with_a_transform_equals_the_hand_written_loop():
    """The per-step route: TrainPreprocess -> image tower -> ProDAFitState.step, the state drawing its own selection schedule."""
    import augment_ref
    from clip_calibration_amd import prodafit
    from clip_calibration_amd.augment import TrainPreprocess
    from clip_calibration_amd.preprocess import pack_images
    from clip_calibration_amd.trainers import proda
    m = model("tiny")
    sizes = [(80, 100), (64, 64), (70, 51), (120, 90), (66, 97), (100, 100), (45, 80), (90, 64)]
    imgs = [augment_ref.synthetic_image(h, w, 70 + i) for i, (h, w) in enumerate(sizes)]
    labels = torch.arange(8) % 3
    loader = [(pack_images(imgs[i:i + 4]).pin_memory(), labels[i:i + 4]) for i in (0, 4)]
    clip = proda.CustomCLIP(m, dref.prompt_ids("tiny", 3, 4), n_ctx=4, n_prompt=8)
    start = clip.prompt_learner.ctx.detach().clone()
    rates = [0.002, 0.001]
    opt = dict(prompt_bs=2, grad_scale=GRAD_SCALE, **SGD)
    tp = TrainPreprocess.for_model(m, generator=torch.Generator().manual_seed(21))
    with torch.no_grad():
        st = prodafit.ProDAFitState(m, clip.prompt_learner.tokenized_prompts, start, logit_scale=math.log(clip.scale),
                                    generator=torch.Generator().manual_seed(5), **opt)
        want = [st.step(m.image_features_f32(tp(images)), y, rates[e], want_loss=True) for e in range(2) for images, y in loader]
    tp2 = TrainPreprocess.for_model(m, generator=torch.Generator().manual_seed(21))
    fitted, losses = clip.fit_context(loader, transform=tp2, epochs=2, lr_per_epoch=rates, return_history=True,
                                      generator=torch.Generator().manual_seed(5), **opt)
    assert st.steps == 4 and torch.equal(fitted, st.ctx) and np.array_equal(losses, torch.cat(want).cpu().numpy())
    assert np.isfinite(losses).all() and not torch.equal(fitted.cpu(), start.float().cpu())
    assert clip.text_features is None and torch.equal(clip.prompt_learner.ctx.detach(), fitted.to(clip.prompt_learner.ctx.dtype))


# ------------------------------------------------------------------------------------------------------------------ g. CoOp unchanged
def test_coop_is_unchanged_by_prodafit():
    """coopfit.context_gradient(method="coop") before and after ProDA's module is imported and used: the same bits, and ProDA stays
    refused there.  (Other tests of this file may have imported the module already; the run in between uses it in any case.)"""
    from clip_calibration_amd import coopfit
    key = ("tiny", 3, 4, 8, False)
    c, m = ref.make_case(*key), model("tiny")
    f = c["feats"].cuda()
    loss0, grad0 = coopfit.context_gradient(m, c["ids"], c["ctx"], f, c["labels"], ref.LOGIT_SCALE, grad_scale=GRAD_SCALE, method="coop")
    loss0, grad0 = loss0.clone(), grad0.clone()
    from clip_calibration_amd import prodafit
    d = dref.make_case("tiny", 2, 4, 4, 4, 1)
    prodafit.context_gradient(m, d["ids"], d["ctx"], d["feats"].cuda(), d["labels"], grad_scale=GRAD_SCALE)
    loss1, grad1 = coopfit.context_gradient(m, c["ids"], c["ctx"], f, c["labels"], ref.LOGIT_SCALE, grad_scale=GRAD_SCALE, method="coop")
    assert torch.equal(loss0, loss1) and torch.equal(grad0, grad1)
    with pytest.raises(ValueError, match="method"):
        coopfit.context_gradient(m, c["ids"], c["ctx"], f, c["labels"], method="proda")
