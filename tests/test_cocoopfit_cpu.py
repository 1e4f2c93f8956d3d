"""CPU checks of CoCoOp's training path (clip_calibration_amd/cocoopfit.py, csrc/cocoop_train.hip): the restatement (tests/cocoopfit_ref.py)
equals float64 autograd through the oracle's pieces, its logits equal the inference oracle's, the five-tensor SGD restatement equals
torch.optim.SGD, the ReLU-at-zero convention, the host-side refusals, the library's refusals without a device, the header."""
import ctypes
import math
import os
import re
import types

import pytest
import torch

import cocoopfit_ref as cref
import coopfit_ref as ref

from clip_calibration_amd import _lib, cocoopfit  # noqa: E402
from clip_calibration_amd import synthetic as syn  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
from oracle import clip_oracle as orc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-9          # tests/test_prodafit_cpu.py's bound: the restatement runs on prodafit_ref.island_tower
NAMES = cref.NAMES


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("key", cref.CASES, ids=ident)
def test_case_keeps_the_relu_margin(key):
    """The condition of every gradient comparison: no float64 pre-activation within 1e-2 of the largest one's size from zero, and both
    signs present, so the mask is seen and never flips between precisions."""
    c = cref.make_case(*key)
    a = cref.meta(c["feats"].double(), {k: v.double() for k, v in c["params"].items()})[1]
    assert float(a.abs().min()) >= cref.MARGIN * float(a.abs().max())
    assert bool((a > 0).any()) and bool((a < 0).any())


@pytest.mark.parametrize("key", cref.CASES, ids=ident)
def test_restatement_equals_autograd(key):
    """Loss, logits and the five gradients of the hand-written backward against float64 autograd through oracle.clip_oracle.coop_prompts
    and text_encoder at rtol 1e-9, the restatement on the tower that restates the oracle's two fp32 islands."""
    c = cref.make_case(*key)
    args = (c["sd"], c["ids"], c["params"], c["feats"], c["labels"])
    want, got = cref.oracle_parts(*args), cref.restated(*args, islands=True)
    figures = {"loss": abs(got["loss"] - want["loss"]) / max(1.0, abs(want["loss"])), "logits": ref.rel_fro(got["logits"], want["logits"])}
    figures.update({k: ref.rel_fro(got["grads"][k], want["grads"][k]) for k in NAMES})
    print(f"cocoopfit-restatement: {key} " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    for k in NAMES:
        assert got["grads"][k].shape == c["params"][k].shape and float(want["grads"][k].norm()) > 0.0, k
    assert all(v <= RTOL for v in figures.values()), figures


@pytest.mark.parametrize("key", cref.CASES[:2], ids=ident)
def test_restatement_on_a_float64_tower_is_close(key):
    """The plain float64 formulas (no islands) stay within test_coopfit_cpu.py's 1e-4 of the oracle's float64 run."""
    c = cref.make_case(*key)
    args = (c["sd"], c["ids"], c["params"], c["feats"], c["labels"])
    want, got = cref.oracle_parts(*args), cref.restated(*args)
    assert abs(got["loss"] - want["loss"]) <= 1e-4 * max(1.0, abs(want["loss"]))
    assert all(ref.rel_fro(got["grads"][k], want["grads"][k]) <= 1e-4 for k in NAMES)


@pytest.mark.parametrize("geom", ["tiny", "tiny3"])
def test_logits_equal_the_inference_oracle(geom):
    """The training function's logits are oracle.clip_oracle.cocoop_forward's on a tiny image batch."""
    c = cref.make_case(geom, 3, 4, 1)
    g = syn.GEOMETRIES[geom]
    image = torch.randn(2, 3, g.image_resolution, g.image_resolution, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    sd_c, ids_c = ref.cut(c["sd"], c["ids"])
    pl = {k: v.double() for k, v in c["params"].items()}
    logits, f_n, _ = orc.cocoop_forward(sd_c, pl, image, ids_c, torch.float64)
    feats = orc.encode_image(c["sd"], image, torch.float64) * 3.0            # raw features: the head normalises them itself
    got = cref.restated(c["sd"], c["ids"], c["params"], feats, torch.zeros(2, dtype=torch.int64), islands=True,
                        logit_scale=math.log(float(c["sd"]["logit_scale"].exp())))      # the oracle exponentiates the fp32 parameter in fp32
    assert ref.rel_fro(got["x"], f_n) <= RTOL and ref.rel_fro(got["logits"], logits) <= RTOL


@pytest.mark.parametrize("momentum,dampening,wd,nesterov", [(0.0, 0.0, 0.0, False), (0.9, 0.0, 5e-4, False), (0.9, 0.0, 0.0, True), (0.5, 0.25, 1e-2, False)])
def test_five_tensor_sgd_equals_torch(momentum, dampening, wd, nesterov):
    c = cref.make_case("tiny", 3, 4, 1)
    start = {k: v.double() for k, v in c["params"].items()}
    g = torch.Generator().manual_seed(4)
    grads = [{k: torch.randn(v.shape, generator=g, dtype=torch.float64) for k, v in start.items()} for _ in range(3)]
    rates = [2e-3, 1e-3, 5e-4]
    got = cref.sgd_steps(start, grads, rates, momentum, dampening, wd, nesterov)
    pars = {k: torch.nn.Parameter(v.clone()) for k, v in start.items()}
    opt = torch.optim.SGD(list(pars.values()), lr=rates[0], momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    for step in range(3):
        for k in NAMES:
            pars[k].grad = grads[step][k].clone()
        opt.param_groups[0]["lr"] = rates[step]
        opt.step()
    for k in NAMES:
        assert torch.allclose(got[k], pars[k].detach(), rtol=1e-13, atol=1e-15), k


def test_relu_at_zero_follows_autograd():
    """A hidden unit whose pre-activation is exactly zero: autograd's relu backward gives it no gradient, and so does the mask hid > 0."""
    c = cref.make_case("tiny", 3, 4, 1)
    p = {k: v.clone() for k, v in c["params"].items()}
    p[NAMES[1]][2] = 0.0
    p[NAMES[2]][2] = 0.0
    args = (c["sd"], c["ids"], p, c["feats"], c["labels"])
    want, got = cref.oracle_parts(*args), cref.restated(*args, islands=True)
    assert float(got["a"][0, 2]) == 0.0 and float(got["hid"][0, 2]) == 0.0
    assert float(want["grads"][NAMES[1]][2].abs().max()) == 0.0 and float(want["grads"][NAMES[2]][2]) == 0.0
    assert float(got["grads"][NAMES[1]][2].abs().max()) == 0.0 and float(got["grads"][NAMES[2]][2]) == 0.0
    assert all(ref.rel_fro(got["grads"][k], want["grads"][k]) <= RTOL for k in NAMES)


@pytest.mark.parametrize("key", cref.CASES, ids=ident)
def test_yardstick_is_finite(key):
    c = cref.make_case(*key)
    yard, how = cref.yardstick_parts(c["sd"], c["ids"], c["params"], c["feats"], c["labels"])
    assert how in ("fp16", "fp32-rounded") and math.isfinite(yard["loss"]) and all(torch.isfinite(g).all() for g in yard["grads"].values())


@pytest.mark.parametrize("B,C,E", ref.HEAD_CASES)
def test_head_cases_are_not_saturated_and_equal_autograd(B, C, E):
    wide, text, y = cref.head_case(B, C, E)
    f = wide[:, 8:8 + E].double()
    t = text.double().requires_grad_(True)
    z = cref.HEAD_SCALE * (cref.unit(f)[:, None] * cref.unit(t.reshape(B, C, E))).sum(-1)
    (d,) = torch.autograd.grad(torch.nn.functional.cross_entropy(z, y), t)
    loss, d_text, rows, z2 = cref.head(f, y, text.double(), cref.HEAD_SCALE)
    assert torch.allclose(d_text, d, rtol=1e-9, atol=1e-13) and torch.allclose(z2, z.detach())
    top = torch.softmax(z2, dim=-1).max(dim=-1).values
    assert int((top < 0.99).sum()) * 2 >= B, top


# ------------------------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def cpu_model():
    return build_model(dict(ref.state_dict("tiny")), {"trainer": "CoOp"})


def test_argument_checks(cpu_model):
    c = cref.make_case("tiny", 3, 4, 3)
    ids, p, f, y = c["ids"], c["params"], c["feats"], c["labels"]
    cg, fit = cocoopfit.gradients, cocoopfit.fit_prompt_learner

    def without(**kw):
        return {**p, **kw}
    with pytest.raises(ValueError, match="keys"):
        cg(cpu_model, ids, {"ctx": p["ctx"]}, f, y)
    with pytest.raises(ValueError, match="class-specific"):
        cg(cpu_model, ids, without(ctx=p["ctx"][None].repeat(3, 1, 1)), f, y)
    with pytest.raises(ValueError, match="meta_net shapes"):
        cg(cpu_model, ids, without(**{NAMES[2]: torch.zeros(9)}), f, y)
    with pytest.raises(ValueError, match="meta_net shapes"):
        cg(cpu_model, ids, without(**{NAMES[3]: torch.zeros(128, 9)}), f, y)
    with pytest.raises(ValueError, match="n_ctx"):
        cg(cpu_model, ids, without(ctx=torch.zeros(30, 128)), f, y)
    with pytest.raises(ValueError, match="grad_scale"):
        cg(cpu_model, ids, p, f, y, grad_scale=3.0)
    with pytest.raises(ValueError, match="grad_scale"):
        cocoopfit.CoCoOpFitState(cpu_model, ids, p, grad_scale=-4.0)
    with pytest.raises(ValueError, match="momentum"):
        fit(f, y, cpu_model, ids, p, epochs=1, momentum=1.0)
    with pytest.raises(ValueError, match="Nesterov"):
        cocoopfit.CoCoOpFitState(cpu_model, ids, p, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError, match="labels"):
        cg(cpu_model, ids, p, f, torch.full((3,), 3))
    with pytest.raises(ValueError, match="features"):
        cg(cpu_model, ids, p, f[:, :64], y)
    with pytest.raises(ValueError, match="seq_rows"):
        cg(cpu_model, ids, p, f, y, seq_rows=4)                            # cuts an EOT row
    with pytest.raises(ValueError, match="learning rates"):
        fit(f, y, cpu_model, ids, p, epochs=2, lr_per_epoch=[1e-3])
    geometry = cpu_model.geometry
    deep = types.SimpleNamespace(context_length=77, ln_final=cpu_model.ln_final, geometry=geometry, ivlp_text_prompts=lambda: (True,))
    with pytest.raises(ValueError, match="deep prompts"):
        cg(deep, ids, p, f, y)
    # more than 80 live rows: a stand-in with a longer context (the checks run before anything touches the model's weights)
    long_model = types.SimpleNamespace(context_length=96, ln_final=cpu_model.ln_final, geometry=geometry, text_dead_row_elimination=True)
    long_ids = torch.zeros(3, 96, dtype=torch.int64)
    long_ids[:, :77] = ids
    with pytest.raises(ValueError, match="80"):
        cg(long_model, long_ids, p, f, y, seq_rows=0)
    with pytest.raises(ValueError, match="80"):
        cg(long_model, long_ids, p, f, y, seq_rows=88)
    with pytest.raises(RuntimeError, match="GPU"):
        cg(cpu_model, ids, p, f, y)                                        # everything checks out: the call needs the device
    with pytest.raises(RuntimeError, match="GPU"):
        fit(f, y, cpu_model, ids, p, epochs=1)
    with pytest.raises(RuntimeError, match="GPU"):
        cocoopfit.CoCoOpFitState(cpu_model, ids, p)
    out = fit(f, y, cpu_model, ids, p, epochs=0)
    assert list(out) == list(NAMES) and all(torch.equal(out[k], p[k]) for k in NAMES)


def test_init_params(cpu_model):
    p = cocoopfit.init_params(cpu_model, n_ctx=4, seed=1)
    assert list(p) == list(NAMES) and [tuple(v.shape) for v in p.values()] == [(4, 128), (8, 128), (8,), (128, 8), (128,)]
    again = cocoopfit.init_params(cpu_model, n_ctx=4, seed=1)
    assert all(torch.equal(p[k], again[k]) for k in NAMES) and not torch.equal(p["ctx"], cocoopfit.init_params(cpu_model, seed=2)["ctx"])
    init_ids = torch.zeros(1, 77, dtype=torch.int64)
    init_ids[0, :5] = torch.tensor([254, 7, 8, 9, 255])
    q = cocoopfit.init_params(cpu_model, ctx_init_ids=init_ids)
    assert torch.equal(q["ctx"], cpu_model.token_embedding.weight.detach().float()[[7, 8, 9]])


def test_header_declares_the_entries_with_the_abi_at_16():
    text = open(os.path.join(ROOT, "include", "clipmi.h")).read()
    assert re.search(r"#define CLIPMI_ABI_VERSION 16\b", text) and _lib.ABI_VERSION == 16 and _lib.lib.clipmi_abi_version() == 16
    for n in ("clipmi_cocoop_block_floats", "clipmi_cocoop_meta", "clipmi_cocoop_embed", "clipmi_cocoop_head_workspace_bytes", "clipmi_cocoop_head",
              "clipmi_cocoop_reduce_workspace_bytes", "clipmi_cocoop_reduce", "clipmi_cocoop_step", "clipmi_cocoop_train_step_bytes",
              "clipmi_cocoop_train_step"):
        assert re.search(r"\b(int|size_t) " + n + r"\(", text), n
        assert n in _lib.exported_symbols() and hasattr(_lib.lib, n)


def test_block_layout():
    from clip_calibration_amd import ops
    layout, total = ops.cocoop_block_layout(4, 128, 64, 5)
    assert list(layout) == list(NAMES) and total == 4 * 128 + 5 * 64 + 5 + 128 * 5 + 128 == _lib.lib.clipmi_cocoop_block_floats(4, 128, 64, 5)
    assert [layout[k][0] for k in NAMES] == [0, 512, 832, 837, 1477]
    views = ops.cocoop_block_views(torch.arange(total, dtype=torch.float32), 4, 128, 64, 5)
    assert [tuple(v.shape) for v in views.values()] == [(4, 128), (5, 64), (5,), (128, 5), (128,)] and float(views[NAMES[4]][0]) == 1477.0
    by = _lib.lib.clipmi_cocoop_block_floats
    assert by(0, 128, 64, 5) == 0 and by(4, 128, 64, 0) == 0 and by(4, 128, 64, 4097) == 0 and by(4, 128, 64, 4096) > 0


def test_library_refuses_bad_calls_without_a_device():
    """Argument checks that return before anything is launched."""
    lib = _lib.lib
    p = ctypes.c_void_p(4096)
    odd = ctypes.c_void_p(4100)

    def meta(feats=p, pi=p, B=2, E=64, ld=64, H=4, D=128):
        return lib.clipmi_cocoop_meta(feats, ld, p, p, p, p, p, p, pi, B, E, H, D, None)
    assert meta(feats=None) == _lib.ERR_ARG and meta(pi=None) == _lib.ERR_ARG
    assert meta(B=0) == _lib.ERR_SHAPE and meta(ld=63) == _lib.ERR_SHAPE and meta(H=0) == _lib.ERR_SHAPE and meta(H=4097) == _lib.ERR_SHAPE
    assert "H=4097" in _lib.last_error()

    def embed(base=p, ctx=p, pi=p, eot=p, dtype=0, B=2, C=3, L=24, Lc=77, D=128, n_ctx=4):
        return lib.clipmi_cocoop_embed(base, dtype, ctx, pi, p, p, eot, B, C, L, Lc, D, n_ctx, None)
    assert embed(base=None) == _lib.ERR_ARG and embed(pi=None) == _lib.ERR_ARG and embed(eot=None) == _lib.ERR_ARG and embed(dtype=2) == _lib.ERR_ARG
    assert embed(base=odd) == _lib.ERR_ARG and embed(ctx=odd) == _lib.ERR_ARG and embed(pi=odd) == _lib.ERR_ARG
    assert embed(D=126) == _lib.ERR_SHAPE and embed(n_ctx=0) == _lib.ERR_SHAPE and embed(n_ctx=24) == _lib.ERR_SHAPE
    assert embed(L=78) == _lib.ERR_SHAPE and embed(C=1) == _lib.ERR_SHAPE and embed(B=0) == _lib.ERR_SHAPE
    assert embed(B=1 << 14, C=1 << 11) == _lib.ERR_SHAPE and "tokens" in _lib.last_error()

    def head(feats=p, loss=p, ws=p, ws_bytes=1 << 20, B=2, C=3, scale=100.0, gs=256.0):
        return lib.clipmi_cocoop_head(feats, 64, p, p, B, 64, C, scale, gs, loss, None, p, ws, ws_bytes, None)
    assert head(feats=None) == _lib.ERR_ARG and head(loss=None) == _lib.ERR_ARG and head(ws=odd) == _lib.ERR_ARG
    assert head(gs=0.0) == _lib.ERR_ARG and head(gs=-1.0) == _lib.ERR_ARG and head(gs=math.inf) == _lib.ERR_ARG and head(gs=math.nan) == _lib.ERR_ARG
    assert "grad_scale" in _lib.last_error() and head(scale=math.nan) == _lib.ERR_ARG
    assert head(B=0) == _lib.ERR_SHAPE and head(C=1) == _lib.ERR_SHAPE and head(ws_bytes=16) == _lib.ERR_WORKSPACE
    by = lib.clipmi_cocoop_head_workspace_bytes
    assert by(2, 3) >= (2 * 2 + 3 * 6) * 4 and by(0, 3) == 0 and by(2, 1) == 0

    def reduce(d=p, grad=p, ws_bytes=1 << 20, B=2, C=3, L=24, H=4, n_ctx=4, gs=256.0):
        return lib.clipmi_cocoop_reduce(d, p, p, p, grad, B, C, L, 128, 64, H, n_ctx, gs, p, ws_bytes, None)
    assert reduce(d=None) == _lib.ERR_ARG and reduce(grad=None) == _lib.ERR_ARG and reduce(gs=0.0) == _lib.ERR_ARG and reduce(gs=math.nan) == _lib.ERR_ARG
    assert reduce(H=0) == _lib.ERR_SHAPE and reduce(H=4097) == _lib.ERR_SHAPE and reduce(n_ctx=0) == _lib.ERR_SHAPE and reduce(n_ctx=24) == _lib.ERR_SHAPE
    assert reduce(ws_bytes=16) == _lib.ERR_WORKSPACE
    rb = lib.clipmi_cocoop_reduce_workspace_bytes
    assert rb(2, 4, 128, 4) >= (2 * 4 * 128 + 2 * 128 + 2 * 4) * 4 and rb(0, 4, 128, 4) == 0 and rb(2, 4, 128, 4097) == 0

    def step(grad=p, params=p, buf=None, lr=p, momentum=0.0, dampening=0.0, wd=0.0, nesterov=0, H=4):
        return lib.clipmi_cocoop_step(grad, params, buf, 4, 128, 64, H, lr, 1, momentum, dampening, wd, nesterov, None)
    assert step(grad=None) == _lib.ERR_ARG and step(params=None) == _lib.ERR_ARG and step(lr=None) == _lib.ERR_ARG
    assert step(momentum=0.9) == _lib.ERR_ARG and "buffer" in _lib.last_error()                       # a momentum needs the buffer
    assert step(momentum=1.0, buf=p) == _lib.ERR_ARG and step(dampening=1.0) == _lib.ERR_ARG and step(wd=-1.0) == _lib.ERR_ARG
    assert step(wd=math.inf) == _lib.ERR_ARG and step(nesterov=1) == _lib.ERR_ARG and step(momentum=0.9, dampening=0.1, nesterov=1, buf=p) == _lib.ERR_ARG
    assert step(H=0) == _lib.ERR_SHAPE
    assert lib.clipmi_cocoop_train_step_bytes(None, 3, 0, 2, 4, 4) == 0
    assert lib.clipmi_cocoop_train_step(None, None, p, 0, p, None, 4, 4, p, 3, 0, p, 64, p, 2, 100.0, 256.0, p, 1, 0.0, 0.0, 0.0, 0, p, None, p, 1 << 20, p,
                                        1 << 20, None) == _lib.ERR_ARG


def fake_model(context_length=77):
    """A handle of the tiny text geometry whose weights are bound to pointers nobody reads: enough for every host-side check."""
    lib = _lib.lib
    geo = _lib.Geometry(128, 64, 16, 128, 2, context_length, 256, 128, 2, 2)
    h = ctypes.c_void_p()
    assert lib.clipmi_create(ctypes.byref(geo), ctypes.byref(h)) == _lib.OK
    blocks = (_lib.BlockWeights * 2)(*[_lib.BlockWeights(*([4096] * 18)) for _ in range(2)])
    tw = _lib.TextWeights(4096, 4096, 4096, 4096, 4096, blocks)
    assert lib.clipmi_set_text_weights(h, ctypes.byref(tw)) == _lib.OK, _lib.last_error()
    dg = (_lib.BlockDgrad * 2)(*[_lib.BlockDgrad(4096, 4096, 4096, 4096) for _ in range(2)])
    return h, _lib.TextDgrad(4096, dg), (blocks, tw, dg)


def test_one_call_step_refuses_before_any_launch():
    """clipmi_cocoop_train_step without a device: every stage's refusal comes back as an error code.  No call here may reach a launch --
    there is no GPU, and a launch would come back as CLIPMI_ERR_HIP, which none of them returns."""
    lib = _lib.lib
    m, wt, keep = fake_model()
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    big = 1 << 40

    def call(m=m, wtp=ctypes.byref(wt), base=p, dtype=0, params=p, buf=None, n_ctx=4, H=8, C=3, rows=24, feats=p, ld=128, B=2, gs=256.0, lr=p, momentum=0.0,
             dampening=0.0, wd=0.0, nesterov=0, loss=p, ws=big, stash=big, wsp=p):
        return lib.clipmi_cocoop_train_step(m, wtp, base, dtype, params, buf, n_ctx, H, p, C, rows, feats, ld, p, B, 100.0, gs, lr, 1, momentum, dampening, wd,
                                            nesterov, loss, None, wsp, ws, p, stash, None)
    assert call(params=None) == _lib.ERR_ARG and call(lr=None) == _lib.ERR_ARG and call(loss=None) == _lib.ERR_ARG and call(wtp=None) == _lib.ERR_ARG
    assert call(base=None) == _lib.ERR_ARG and call(feats=None) == _lib.ERR_ARG and call(dtype=2) == _lib.ERR_ARG
    assert call(base=odd) == _lib.ERR_ARG and "aligned" in _lib.last_error()
    assert call(params=odd) == _lib.ERR_ARG and call(wsp=odd) == _lib.ERR_ARG
    assert call(H=0) == _lib.ERR_SHAPE and call(H=4097) == _lib.ERR_SHAPE and "H=4097" in _lib.last_error()
    assert call(n_ctx=0) == _lib.ERR_SHAPE and call(n_ctx=24) == _lib.ERR_SHAPE and "live rows" in _lib.last_error()     # rows 1 .. 24 of 24
    assert call(C=1) == _lib.ERR_SHAPE and call(B=0) == _lib.ERR_SHAPE and call(ld=127) == _lib.ERR_SHAPE
    assert call(B=1 << 15, C=1 << 11) == _lib.ERR_SHAPE and "tokens" in _lib.last_error()
    assert call(ws=1024) == _lib.ERR_WORKSPACE and call(stash=1024) == _lib.ERR_WORKSPACE
    for gs in (0.0, -256.0, math.inf, math.nan):
        assert call(gs=gs) == _lib.ERR_ARG and "grad_scale" in _lib.last_error()
    assert call(momentum=1.0, buf=p) == _lib.ERR_ARG and call(dampening=-0.1) == _lib.ERR_ARG and call(wd=math.nan) == _lib.ERR_ARG
    assert call(nesterov=1) == _lib.ERR_ARG and call(momentum=0.9) == _lib.ERR_ARG and "buffer" in _lib.last_error()
    long_m, long_wt, keep2 = fake_model(96)
    assert call(m=long_m, wtp=ctypes.byref(long_wt), rows=0) == _lib.ERR_SHAPE and "at most 80" in _lib.last_error()
    assert call(m=long_m, wtp=ctypes.byref(long_wt), rows=88) == _lib.ERR_SHAPE
    by = lib.clipmi_cocoop_train_step_bytes
    assert by(m, 3, 24, 2, 8, 4) > by(m, 3, 24, 1, 8, 4) > 0 and by(m, 1, 24, 2, 8, 4) == 0 and by(m, 3, 24, 2, 0, 4) == 0 and by(m, 3, 24, 2, 8, 0) == 0
    lib.clipmi_destroy(m)
    lib.clipmi_destroy(long_m)
